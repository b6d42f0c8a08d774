// smg_emd_device.hip -- the kernels of the earth mover's distance on a mesh (smg_emd_*, include/smg.h; host side in smg_emd.cpp; the arithmetic
// in smg_emd_inl.hpp).
//
// Layout: positions are xyz rows; W2 is 6 and Af 1 double per face; the state is 4 doubles per (face, column), Z then U, column c at c * 4 nF, so
// that a lane of the update kernel owns 32 contiguous bytes; a field in the faces' frames is 2 doubles per (face, column).  Masses, potentials and
// right-hand sides are column-major blocks with a leading dimension, one column per pair of distributions.
//
// Determinism: no atomics.  A vertex's right-hand side is one lane's sequential loop over its corners in corner-list order (faces ascending); the
// bounds are launch_fixed_sum / launch_fixed_max of per-lane terms.  Expressions are written operation by operation (-ffp-contract=off):
// tests/emd_np.py restates them in numpy in the same order.  Only +, -, *, /, sqrt and max occur.
//
// Grid order of the (vertex, column) and (face, column) kernels: the k blocks of one vertex (face) block are adjacent (blockIdx.x = block * k + c),
// so a block's geometry -- corner lists, faces, W2, areas -- is read for all columns while it is still in cache, as in k_hodge_rhs.
#include <hip/hip_runtime.h>

#include "smg_device.hpp"
#include "smg_emd_inl.hpp"

namespace smg {

namespace {

constexpr int EMD_THREADS = 256;

inline int emd_grid(long long n) { return (int)((n + EMD_THREADS - 1) / EMD_THREADS); }

// the grid of a (row block, column) kernel; false: it does not fit a grid dimension
bool emd_column_grid(int rows, int k, unsigned* blocks)
{
    const long long b = (long long)emd_grid(rows) * k;
    *blocks = (unsigned)b;
    return b <= 0x7fffffffLL;
}

}  // namespace

// One lane per face: W2 (6), Af = A
__global__ __launch_bounds__(EMD_THREADS) void k_emd_geometry(const double* __restrict__ V, const int* __restrict__ F, int nF, double* __restrict__ W2,
                                                              double* __restrict__ Af)
{
    const int f = blockIdx.x * EMD_THREADS + threadIdx.x;
    if (f >= nF) return;
    double w[6], A;
    emd_geometry(V + 3 * (size_t)F[3 * (size_t)f], V + 3 * (size_t)F[3 * (size_t)f + 1], V + 3 * (size_t)F[3 * (size_t)f + 2], w, &A);
#pragma unroll
    for (int e = 0; e < 6; e++) W2[6 * (size_t)f + e] = w[e];
    Af[f] = A;
}

// One lane per (vertex v, column c): over v's corners (f, i) in list order, acc += A_f (W2_fi . X_f); R[c * ldr + v] = acc - b[c * ldb + v].
// STATE: X is the state and X_f = Z_f - U_f; else X is a field in the frames.  dsq (nullptr ok): dsq[c * n + v] = the square, 0 for vertex 0.
template <bool STATE>
__global__ __launch_bounds__(EMD_THREADS) void k_emd_rhs(int n, int k, int nF, const int* __restrict__ m_ptr, const int* __restrict__ m_idx,
                                                         const double* __restrict__ W2, const double* __restrict__ Af, const double* __restrict__ X,
                                                         const double* __restrict__ b, int ldb, double* __restrict__ R, int ldr, double* __restrict__ dsq)
{
    const int c = (int)(blockIdx.x % (unsigned)k);
    const int v = (int)(blockIdx.x / (unsigned)k) * EMD_THREADS + (int)threadIdx.x;
    if (v >= n) return;
    constexpr int STRIDE = STATE ? 4 : 2;
    const double* Xc = X + (size_t)c * nF * STRIDE;
    double acc = 0.0;
    const int p1 = m_ptr[v + 1];
    for (int p = m_ptr[v]; p < p1; p++) {
        const int q = m_idx[p];
        const int f = q / 3, i = q - 3 * f;
        const double* x = Xc + (size_t)f * STRIDE;
        double x0, x1;
        if (STATE) {
            const double2 z = *reinterpret_cast<const double2*>(x), u = *reinterpret_cast<const double2*>(x + 2);
            x0 = z.x - u.x; x1 = z.y - u.y;
        } else {
            const double2 j = *reinterpret_cast<const double2*>(x);
            x0 = j.x; x1 = j.y;
        }
        const double2 w = *reinterpret_cast<const double2*>(W2 + 6 * (size_t)f + 2 * i);
        const double w2[2] = {w.x, w.y};
        acc += emd_corner(Af[f], w2, x0, x1);
    }
    const double r = acc - b[(size_t)c * ldb + v];
    R[(size_t)c * ldr + v] = r;
    if (dsq) dsq[(size_t)c * n + v] = v == 0 ? 0.0 : r * r;
}

// One lane per (face f, column c), the hot kernel: gathers phi at the three corners, reads the lane's Z and U, writes them back in place, and
// up[c * nF + f] = A_f |J_f|, gq[c * nF + f] = rho_c^2 |grad phi_f|^2; J2 (nullptr ok): J in the frame, 2 doubles per lane.
__global__ __launch_bounds__(EMD_THREADS) void k_emd_update(int nF, int k, const int* __restrict__ F, const double* __restrict__ W2,
                                                            const double* __restrict__ Af, const double* __restrict__ phi, int ldp, double* __restrict__ ZU,
                                                            const double* __restrict__ rho, double alpha, double* __restrict__ J2, double* __restrict__ up,
                                                            double* __restrict__ gq)
{
    const int c = (int)(blockIdx.x % (unsigned)k);
    const int f = (int)(blockIdx.x / (unsigned)k) * EMD_THREADS + (int)threadIdx.x;
    if (f >= nF) return;
    double w[6];
#pragma unroll
    for (int e = 0; e < 3; e++) {
        const double2 t = *reinterpret_cast<const double2*>(W2 + 6 * (size_t)f + 2 * e);
        w[2 * e] = t.x; w[2 * e + 1] = t.y;
    }
    const double* pc = phi + (size_t)c * ldp;
    const double p0 = pc[F[3 * (size_t)f]], p1 = pc[F[3 * (size_t)f + 1]], p2 = pc[F[3 * (size_t)f + 2]];
    double* s = ZU + ((size_t)c * nF + f) * 4;
    const double2 z = *reinterpret_cast<const double2*>(s), u = *reinterpret_cast<const double2*>(s + 2);
    double zu[4] = {z.x, z.y, u.x, u.y}, J[2], upv, gqv;
    emd_update(w, Af[f], p0, p1, p2, rho[c], alpha, zu, J, &upv, &gqv);
    *reinterpret_cast<double2*>(s) = make_double2(zu[0], zu[1]);
    *reinterpret_cast<double2*>(s + 2) = make_double2(zu[2], zu[3]);
    if (J2) *reinterpret_cast<double2*>(J2 + ((size_t)c * nF + f) * 2) = make_double2(J[0], J[1]);
    up[(size_t)c * nF + f] = upv;
    gq[(size_t)c * nF + f] = gqv;
}

// One lane per (vertex v, column c): pot[c * ldq + v] = (-rho_c / max(1, sqrt(gmax2_c))) phi[c * ldp + v]; terms[c * n + v] = b pot
__global__ __launch_bounds__(EMD_THREADS) void k_emd_dual(int n, int k, const double* __restrict__ b, int ldb, const double* __restrict__ phi, int ldp,
                                                          const double* __restrict__ rho, const double* __restrict__ gmax2, double* __restrict__ pot, int ldq,
                                                          double* __restrict__ terms)
{
    const int c = (int)(blockIdx.x % (unsigned)k);
    const int v = (int)(blockIdx.x / (unsigned)k) * EMD_THREADS + (int)threadIdx.x;
    if (v >= n) return;
    const double q = emd_dual_scale(rho[c], gmax2[c]) * phi[(size_t)c * ldp + v];
    pot[(size_t)c * ldq + v] = q;
    terms[(size_t)c * n + v] = b[(size_t)c * ldb + v] * q;
}

// One lane per (face f, column c): out = J[0] t1 + J[1] t2, 3 doubles per lane, column c at c * 3 nF; the frame is recomputed from the positions
__global__ __launch_bounds__(EMD_THREADS) void k_emd_flow(int nF, int k, const double* __restrict__ V, const int* __restrict__ F,
                                                          const double* __restrict__ J2, double* __restrict__ out)
{
    const int c = (int)(blockIdx.x % (unsigned)k);
    const int f = (int)(blockIdx.x / (unsigned)k) * EMD_THREADS + (int)threadIdx.x;
    if (f >= nF) return;
    double t1[3], t2[3], W[9], dA;
    emd_frame(V + 3 * (size_t)F[3 * (size_t)f], V + 3 * (size_t)F[3 * (size_t)f + 1], V + 3 * (size_t)F[3 * (size_t)f + 2], t1, t2, W, &dA);
    const double2 j = *reinterpret_cast<const double2*>(J2 + ((size_t)c * nF + f) * 2);
    double* o = out + ((size_t)c * nF + f) * 3;
#pragma unroll
    for (int d = 0; d < 3; d++) o[d] = j.x * t1[d] + j.y * t2[d];
}

hipError_t launch_emd_geometry(const double* V, const int* F, int nF, double* W2, double* Af, hipStream_t st)
{
    if (nF <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_emd_geometry, dim3(emd_grid(nF)), dim3(EMD_THREADS), 0, st, V, F, nF, W2, Af);
    return hipGetLastError();
}

hipError_t launch_emd_rhs(int n, int k, int nF, const int* m_ptr, const int* m_idx, const double* W2, const double* Af, const double* X, bool state,
                          const double* b, int ldb, double* R, int ldr, double* dsq, hipStream_t st)
{
    if (n <= 0 || k <= 0) return hipSuccess;
    unsigned blocks = 0;
    if (!emd_column_grid(n, k, &blocks)) return hipErrorInvalidConfiguration;
    if (state)
        hipLaunchKernelGGL(k_emd_rhs<true>, dim3(blocks), dim3(EMD_THREADS), 0, st, n, k, nF, m_ptr, m_idx, W2, Af, X, b, ldb, R, ldr, dsq);
    else
        hipLaunchKernelGGL(k_emd_rhs<false>, dim3(blocks), dim3(EMD_THREADS), 0, st, n, k, nF, m_ptr, m_idx, W2, Af, X, b, ldb, R, ldr, dsq);
    return hipGetLastError();
}

hipError_t launch_emd_update(int nF, int k, const int* F, const double* W2, const double* Af, const double* phi, int ldp, double* ZU, const double* rho,
                             double alpha, double* J2, double* up, double* gq, hipStream_t st)
{
    if (nF <= 0 || k <= 0) return hipSuccess;
    unsigned blocks = 0;
    if (!emd_column_grid(nF, k, &blocks)) return hipErrorInvalidConfiguration;
    hipLaunchKernelGGL(k_emd_update, dim3(blocks), dim3(EMD_THREADS), 0, st, nF, k, F, W2, Af, phi, ldp, ZU, rho, alpha, J2, up, gq);
    return hipGetLastError();
}

hipError_t launch_emd_dual(int n, int k, const double* b, int ldb, const double* phi, int ldp, const double* rho, const double* gmax2, double* pot, int ldq,
                           double* terms, hipStream_t st)
{
    if (n <= 0 || k <= 0) return hipSuccess;
    unsigned blocks = 0;
    if (!emd_column_grid(n, k, &blocks)) return hipErrorInvalidConfiguration;
    hipLaunchKernelGGL(k_emd_dual, dim3(blocks), dim3(EMD_THREADS), 0, st, n, k, b, ldb, phi, ldp, rho, gmax2, pot, ldq, terms);
    return hipGetLastError();
}

hipError_t launch_emd_flow(int nF, int k, const double* V, const int* F, const double* J2, double* out, hipStream_t st)
{
    if (nF <= 0 || k <= 0) return hipSuccess;
    unsigned blocks = 0;
    if (!emd_column_grid(nF, k, &blocks)) return hipErrorInvalidConfiguration;
    hipLaunchKernelGGL(k_emd_flow, dim3(blocks), dim3(EMD_THREADS), 0, st, nF, k, V, F, J2, out);
    return hipGetLastError();
}

}  // namespace smg
