// smg_hodge_device.hip -- the kernels of the Helmholtz-Hodge decomposition (smg_hodge_*, include/smg.h; host side in smg_hodge.cpp; the
// arithmetic in smg_hodge_inl.hpp).
//
// Layout: positions are xyz rows; per-face arrays are face rows (W: 9, nrm: 3, Af: 1, a field: 3, the parts: 9 contiguous doubles per face), so
// a corner costs one gather per array; a set's field follows the previous set's (set c at c * 3 nF).  Potentials and right-hand sides are
// column-major blocks with a leading dimension, one column per set.
//
// Determinism: no atomics.  A vertex's two right-hand sides are one lane's sequential loop over its corners in corner-list order (faces
// ascending); the energies and |rhs|_F^2 are launch_fixed_sum of per-lane terms.  Expressions are written operation by operation
// (-ffp-contract=off): tests/hodge_np.py restates them in numpy in the same order.  Only +, -, *, / and sqrt occur.
//
// Grid order of the (vertex, set) and (face, set) kernels: the k blocks of one vertex (face) block are adjacent (blockIdx.x = block * k + c), so a
// block's geometry -- corner lists, faces, normals, positions, basis -- is read for all sets while it is still in cache, as in k_geo_divergence.
#include <hip/hip_runtime.h>

#include "smg_device.hpp"
#include "smg_hodge_inl.hpp"

namespace smg {

namespace {

constexpr int HODGE_THREADS = 256;

inline int hodge_grid(long long n) { return (int)((n + HODGE_THREADS - 1) / HODGE_THREADS); }

// the grid of a (row block, set) kernel; false: it does not fit a grid dimension
bool hodge_set_grid(int rows, int k, unsigned* blocks)
{
    const long long b = (long long)hodge_grid(rows) * k;
    *blocks = (unsigned)b;
    return b <= 0x7fffffffLL;
}

// the face's basis, normal and area from the stored rows; its three vertices
__device__ __forceinline__ void hodge_load_face(const int* __restrict__ F, const double* __restrict__ W, const double* __restrict__ nrm, int f, double* w,
                                                double* nn, size_t* i)
{
#pragma unroll
    for (int e = 0; e < 9; e++) w[e] = W[9 * (size_t)f + e];
#pragma unroll
    for (int e = 0; e < 3; e++) nn[e] = nrm[3 * (size_t)f + e];
#pragma unroll
    for (int e = 0; e < 3; e++) i[e] = (size_t)F[3 * (size_t)f + e];
}

}  // namespace

// One lane per face: W (9), nrm (3), Af = A
__global__ __launch_bounds__(HODGE_THREADS) void k_hodge_geometry(const double* __restrict__ V, const int* __restrict__ F, int nF, double* __restrict__ W,
                                                                  double* __restrict__ nrm, double* __restrict__ Af)
{
    const int f = blockIdx.x * HODGE_THREADS + threadIdx.x;
    if (f >= nF) return;
    double w[9], nn[3], dA;
    morph_basis(V + 3 * (size_t)F[3 * (size_t)f], V + 3 * (size_t)F[3 * (size_t)f + 1], V + 3 * (size_t)F[3 * (size_t)f + 2], w, nn, &dA);
#pragma unroll
    for (int e = 0; e < 9; e++) W[9 * (size_t)f + e] = w[e];
#pragma unroll
    for (int e = 0; e < 3; e++) nrm[3 * (size_t)f + e] = nn[e];
    Af[f] = dA * 0.5;
}

// One lane per (vertex v, set c): over v's corners (f, j) in list order, accb += (n_f x e_fj) . X_f and accc += e_fj . X_f with X of set c;
// Bb[c * ldb + v] = accb / 2, Bc[c * ldb + v] = -accc / 2; bsq[c * n + v] and bsq[(k + c) * n + v] = their squares.
__global__ __launch_bounds__(HODGE_THREADS) void k_hodge_rhs(int n, int k, int nF, const int* __restrict__ m_ptr, const int* __restrict__ m_idx,
                                                             const int* __restrict__ F, const double* __restrict__ V, const double* __restrict__ nrm,
                                                             const double* __restrict__ X, double* __restrict__ Bb, double* __restrict__ Bc, int ldb,
                                                             double* __restrict__ bsq)
{
    const int c = (int)(blockIdx.x % (unsigned)k);
    const int v = (int)(blockIdx.x / (unsigned)k) * HODGE_THREADS + (int)threadIdx.x;
    if (v >= n) return;
    const double* Xc = X + (size_t)c * nF * 3;
    double accb = 0.0, accc = 0.0;
    const int p1 = m_ptr[v + 1];
    for (int p = m_ptr[v]; p < p1; p++) {
        const int q = m_idx[p];
        const int f = q / 3, j = q - 3 * f;
        const int ja = j == 0 ? 2 : j - 1, jb = j == 2 ? 0 : j + 1;          // (j + 2) % 3, (j + 1) % 3
        const double* a = V + 3 * (size_t)F[3 * (size_t)f + ja];
        const double* b = V + 3 * (size_t)F[3 * (size_t)f + jb];
        const double pa[3] = {a[0], a[1], a[2]}, pb[3] = {b[0], b[1], b[2]};
        const double nn[3] = {nrm[3 * (size_t)f], nrm[3 * (size_t)f + 1], nrm[3 * (size_t)f + 2]};
        const double xf[3] = {Xc[3 * (size_t)f], Xc[3 * (size_t)f + 1], Xc[3 * (size_t)f + 2]};
        double e[3], tb, tc;
        hodge_edge(pa, pb, e);
        hodge_corner(nn, e, xf, &tb, &tc);
        accb += tb;
        accc += tc;
    }
    const double bv = 0.5 * accb, cv = -0.5 * accc;
    Bb[(size_t)c * ldb + v] = bv;
    Bc[(size_t)c * ldb + v] = cv;
    bsq[(size_t)c * n + v] = bv * bv;
    bsq[((size_t)k + c) * n + v] = cv * cv;
}

// One lane per (face f, set c): Xt, G = grad u, R = n x grad v, H of set c's field and potentials (columns c of u and v).  parts (nullptr ok):
// 9 doubles per face, set c at c * 9 nF; terms[(4 c + e) * nF + f] = A_f |.|^2 of Xt, G, R, H.
__global__ __launch_bounds__(HODGE_THREADS) void k_hodge_parts(int nF, int k, const int* __restrict__ F, const double* __restrict__ W,
                                                               const double* __restrict__ nrm, const double* __restrict__ Af, const double* __restrict__ X,
                                                               const double* __restrict__ u, int ldu, const double* __restrict__ v, int ldv,
                                                               double* __restrict__ parts, double* __restrict__ terms)
{
    const int c = (int)(blockIdx.x % (unsigned)k);
    const int f = (int)(blockIdx.x / (unsigned)k) * HODGE_THREADS + (int)threadIdx.x;
    if (f >= nF) return;
    double w[9], nn[3], Xt[3], P[9];
    size_t i[3];
    hodge_load_face(F, W, nrm, f, w, nn, i);
    const double* uc = u + (size_t)c * ldu;
    const double* vc = v + (size_t)c * ldv;
    const double* x = X + ((size_t)c * nF + f) * 3;
    const double uf[3] = {uc[i[0]], uc[i[1]], uc[i[2]]}, vf[3] = {vc[i[0]], vc[i[1]], vc[i[2]]}, xf[3] = {x[0], x[1], x[2]};
    hodge_parts(w, nn, xf, uf, vf, Xt, P);
    if (parts) {
        double* out = parts + ((size_t)c * nF + f) * 9;
#pragma unroll
        for (int e = 0; e < 9; e++) out[e] = P[e];
    }
    const double A = Af[f];
    double* t = terms + (size_t)(4 * c) * nF + f;
    t[0] = hodge_term(A, Xt);
    t[(size_t)nF] = hodge_term(A, P);
    t[2 * (size_t)nF] = hodge_term(A, P + 3);
    t[3 * (size_t)nF] = hodge_term(A, P + 6);
}

// One lane per (face f, set c): X = grad u + n x grad v, set c at c * 3 nF
__global__ __launch_bounds__(HODGE_THREADS) void k_hodge_field(int nF, int k, const int* __restrict__ F, const double* __restrict__ W,
                                                               const double* __restrict__ nrm, const double* __restrict__ u, int ldu,
                                                               const double* __restrict__ v, int ldv, double* __restrict__ X)
{
    const int c = (int)(blockIdx.x % (unsigned)k);
    const int f = (int)(blockIdx.x / (unsigned)k) * HODGE_THREADS + (int)threadIdx.x;
    if (f >= nF) return;
    double w[9], nn[3], xf[3];
    size_t i[3];
    hodge_load_face(F, W, nrm, f, w, nn, i);
    const double* uc = u + (size_t)c * ldu;
    const double* vc = v + (size_t)c * ldv;
    const double uf[3] = {uc[i[0]], uc[i[1]], uc[i[2]]}, vf[3] = {vc[i[0]], vc[i[1]], vc[i[2]]};
    hodge_field(w, nn, uf, vf, xf);
    double* out = X + ((size_t)c * nF + f) * 3;
    out[0] = xf[0]; out[1] = xf[1]; out[2] = xf[2];
}

hipError_t launch_hodge_geometry(const double* V, const int* F, int nF, double* W, double* nrm, double* Af, hipStream_t st)
{
    if (nF <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_hodge_geometry, dim3(hodge_grid(nF)), dim3(HODGE_THREADS), 0, st, V, F, nF, W, nrm, Af);
    return hipGetLastError();
}

hipError_t launch_hodge_rhs(int n, int k, int nF, const int* m_ptr, const int* m_idx, const int* F, const double* V, const double* nrm, const double* X,
                            double* Bb, double* Bc, int ldb, double* bsq, hipStream_t st)
{
    if (n <= 0 || k <= 0) return hipSuccess;
    unsigned blocks = 0;
    if (!hodge_set_grid(n, k, &blocks)) return hipErrorInvalidConfiguration;
    hipLaunchKernelGGL(k_hodge_rhs, dim3(blocks), dim3(HODGE_THREADS), 0, st, n, k, nF, m_ptr, m_idx, F, V, nrm, X, Bb, Bc, ldb, bsq);
    return hipGetLastError();
}

hipError_t launch_hodge_parts(int nF, int k, const int* F, const double* W, const double* nrm, const double* Af, const double* X, const double* u, int ldu,
                              const double* v, int ldv, double* parts, double* terms, hipStream_t st)
{
    if (nF <= 0 || k <= 0) return hipSuccess;
    unsigned blocks = 0;
    if (!hodge_set_grid(nF, k, &blocks)) return hipErrorInvalidConfiguration;
    hipLaunchKernelGGL(k_hodge_parts, dim3(blocks), dim3(HODGE_THREADS), 0, st, nF, k, F, W, nrm, Af, X, u, ldu, v, ldv, parts, terms);
    return hipGetLastError();
}

hipError_t launch_hodge_field(int nF, int k, const int* F, const double* W, const double* nrm, const double* u, int ldu, const double* v, int ldv,
                              double* X, hipStream_t st)
{
    if (nF <= 0 || k <= 0) return hipSuccess;
    unsigned blocks = 0;
    if (!hodge_set_grid(nF, k, &blocks)) return hipErrorInvalidConfiguration;
    hipLaunchKernelGGL(k_hodge_field, dim3(blocks), dim3(HODGE_THREADS), 0, st, nF, k, F, W, nrm, u, ldu, v, ldv, X);
    return hipGetLastError();
}

}  // namespace smg
