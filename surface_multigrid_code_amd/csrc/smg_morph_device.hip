// smg_morph_device.hip -- the kernels of gradient-domain morphing (smg_morph_*, include/smg.h; host side in smg_morph.cpp; the per-face
// arithmetic in smg_morph_inl.hpp).
//
// Layout: poses are xyz rows (3 doubles per vertex); per-face arrays are face rows (W: 9, nrm: 3, omega: 3, S: 6, J and R: 9 contiguous doubles
// per face), so a corner costs one gather per array; a set's gradients follow the previous set's (set c at c * 9 nF).  The solver's blocks are
// column-major with a leading dimension: column 3c + d is coordinate d of set c.
//
// Determinism: no atomics.  A vertex's right-hand side is one lane's sequential loop over its corners in corner-list order (faces ascending), and
// |b|_F^2 is the fixed-order sum of the lanes' |b_v|^2 (launch_fixed_sum).  The interpolated gradient J_f(t_c) is never stored: every corner
// recomputes it from the face's omega and S (9 doubles) and the set's t.  Expressions are written operation by operation (-ffp-contract=off):
// tests/morph_np.py restates them in numpy in the same order.  sin, cos and atan2 are called by k_morph_face_polar and k_morph_rhs<true> alone.
//
// Grid order of the (vertex, set) and (face, set) kernels: the k blocks of one vertex (face) block are adjacent (blockIdx.x = block * k + c), so a
// block's geometry -- corner lists, basis, areas, omega, S -- is read for all sets while it is still in cache, as in k_geo_divergence.
#include <hip/hip_runtime.h>

#include "smg_device.hpp"
#include "smg_morph_inl.hpp"

namespace smg {

namespace {

constexpr int MORPH_THREADS = 256;

inline int morph_grid(long long n) { return (int)((n + MORPH_THREADS - 1) / MORPH_THREADS); }

// (1 - t) v + t x, the blend of the rest pose and the pose that starts an interpolation and places its pins
__device__ __forceinline__ double morph_blend(double v, double x, double t) { return (1.0 - t) * v + t * x; }

}  // namespace

// the rest faces: W (9), nrm (3), Af = A
__global__ __launch_bounds__(MORPH_THREADS) void k_morph_basis(const double* __restrict__ V, const int* __restrict__ F, int nF, double* __restrict__ W,
                                                               double* __restrict__ nrm, double* __restrict__ Af)
{
    const int f = blockIdx.x * MORPH_THREADS + threadIdx.x;
    if (f >= nF) return;
    double w[9], nn[3], dA;
    morph_basis(V + 3 * (size_t)F[3 * (size_t)f], V + 3 * (size_t)F[3 * (size_t)f + 1], V + 3 * (size_t)F[3 * (size_t)f + 2], w, nn, &dA);
#pragma unroll
    for (int e = 0; e < 9; e++) W[9 * (size_t)f + e] = w[e];
#pragma unroll
    for (int e = 0; e < 3; e++) nrm[3 * (size_t)f + e] = nn[e];
    Af[f] = dA * 0.5;
}

// One lane per (face f, set c): J[c][f] = the gradient of pose c (X + c * 3 nVs) on the rest face f of (S0, Fs); the rest basis is formed here.
__global__ __launch_bounds__(MORPH_THREADS) void k_morph_face_gradient(int nF, int k, const int* __restrict__ Fs, const double* __restrict__ S0,
                                                                       const double* __restrict__ X, size_t set_stride, double* __restrict__ J)
{
    const int c = (int)(blockIdx.x % (unsigned)k);
    const int f = (int)(blockIdx.x / (unsigned)k) * MORPH_THREADS + (int)threadIdx.x;
    if (f >= nF) return;
    const size_t i0 = (size_t)Fs[3 * (size_t)f], i1 = (size_t)Fs[3 * (size_t)f + 1], i2 = (size_t)Fs[3 * (size_t)f + 2];
    double W[9], nn[3], dA, Jf[9];
    morph_basis(S0 + 3 * i0, S0 + 3 * i1, S0 + 3 * i2, W, nn, &dA);
    const double* x = X + (size_t)c * set_stride;
    morph_gradient(x + 3 * i0, x + 3 * i1, x + 3 * i2, W, nn, Jf);
    double* out = J + ((size_t)c * nF + f) * 9;
#pragma unroll
    for (int e = 0; e < 9; e++) out[e] = Jf[e];
}

// One lane per face: the gradient of the pose X on the stored rest basis, its polar factors and the rotation vector.  R (9 per face) may be nullptr.
__global__ __launch_bounds__(MORPH_THREADS) void k_morph_face_polar(int nF, const int* __restrict__ F, const double* __restrict__ W,
                                                                    const double* __restrict__ nrm, const double* __restrict__ X,
                                                                    double* __restrict__ R, double* __restrict__ omega, double* __restrict__ S)
{
    const int f = blockIdx.x * MORPH_THREADS + threadIdx.x;
    if (f >= nF) return;
    const size_t i0 = (size_t)F[3 * (size_t)f], i1 = (size_t)F[3 * (size_t)f + 1], i2 = (size_t)F[3 * (size_t)f + 2];
    double w[9], nn[3], J[9], Rf[9], S6[6], om[3];
#pragma unroll
    for (int e = 0; e < 9; e++) w[e] = W[9 * (size_t)f + e];
#pragma unroll
    for (int e = 0; e < 3; e++) nn[e] = nrm[3 * (size_t)f + e];
    morph_gradient(X + 3 * i0, X + 3 * i1, X + 3 * i2, w, nn, J);
    morph_polar(J, Rf, S6);
    morph_log(Rf, om);
    if (R) {
#pragma unroll
        for (int e = 0; e < 9; e++) R[9 * (size_t)f + e] = Rf[e];
    }
#pragma unroll
    for (int e = 0; e < 3; e++) omega[3 * (size_t)f + e] = om[e];
#pragma unroll
    for (int e = 0; e < 6; e++) S[6 * (size_t)f + e] = S6[e];
}

// One lane per (vertex v, set c): b_v = sum over v's corners (f, j), in list order, of A_f J_f W_fj, with J_f read from J (set c at c * 9 nF)
// or, INTERP, recomputed from omega_f, S_f and t[c].  B[(3c + d) * ldb + v] = b_v,d; bsq[c * n + v] = |b_v|^2.
template <bool INTERP>
__global__ __launch_bounds__(MORPH_THREADS) void k_morph_rhs(int n, int k, int nF, const int* __restrict__ m_ptr, const int* __restrict__ m_idx,
                                                             const double* __restrict__ W, const double* __restrict__ Af, const double* __restrict__ J,
                                                             const double* __restrict__ omega, const double* __restrict__ S, const double* __restrict__ t,
                                                             double* __restrict__ B, int ldb, double* __restrict__ bsq)
{
    const int c = (int)(blockIdx.x % (unsigned)k);
    const int v = (int)(blockIdx.x / (unsigned)k) * MORPH_THREADS + (int)threadIdx.x;
    if (v >= n) return;
    const double tc = INTERP ? t[c] : 0.0;
    const double* Jc = INTERP ? nullptr : J + (size_t)c * nF * 9;
    double acc[3] = {0.0, 0.0, 0.0};
    const int p1 = m_ptr[v + 1];
    for (int p = m_ptr[v]; p < p1; p++) {
        const int q = m_idx[p];
        const int f = q / 3, j = q - 3 * f;
        double Jf[9];
        if (INTERP) {
            double om[3], S6[6];
#pragma unroll
            for (int e = 0; e < 3; e++) om[e] = omega[3 * (size_t)f + e];
#pragma unroll
            for (int e = 0; e < 6; e++) S6[e] = S[6 * (size_t)f + e];
            morph_interp(om, S6, tc, Jf);
        } else {
#pragma unroll
            for (int e = 0; e < 9; e++) Jf[e] = Jc[9 * (size_t)f + e];
        }
        const double* w = W + 9 * (size_t)f + 3 * j;
        const double wj[3] = {w[0], w[1], w[2]};
        morph_share(Jf, wj, Af[f], acc);
    }
    B[(size_t)(3 * c) * ldb + v] = acc[0];
    B[(size_t)(3 * c + 1) * ldb + v] = acc[1];
    B[(size_t)(3 * c + 2) * ldb + v] = acc[2];
    bsq[(size_t)c * n + v] = acc[0] * acc[0] + acc[1] * acc[1] + acc[2] * acc[2];
}

// U[(3c + d) * ldu + i] = V[3i + d], or with a pose X and times t the blend (1 - t_c) V + t_c X: the start of a solve
__global__ __launch_bounds__(MORPH_THREADS) void k_morph_start(int n, int k, const double* __restrict__ V, const double* __restrict__ X,
                                                               const double* __restrict__ t, double* __restrict__ U, int ldu)
{
    const int c = (int)(blockIdx.x % (unsigned)k);
    const int i = (int)(blockIdx.x / (unsigned)k) * MORPH_THREADS + (int)threadIdx.x;
    if (i >= n) return;
#pragma unroll
    for (int d = 0; d < 3; d++) {
        const double v = V[3 * (size_t)i + d];
        U[(size_t)(3 * c + d) * ldu + i] = X ? morph_blend(v, X[3 * (size_t)i + d], t[c]) : v;
    }
}

// hp[(3c + d) * ldh + r] = the same at vertex pins[r]: the pins' default positions
__global__ __launch_bounds__(MORPH_THREADS) void k_morph_pins(int nh, int k, const int* __restrict__ pins, const double* __restrict__ V,
                                                              const double* __restrict__ X, const double* __restrict__ t, double* __restrict__ hp, int ldh)
{
    const long long g = (long long)blockIdx.x * MORPH_THREADS + threadIdx.x;
    if (g >= (long long)nh * k) return;
    const int c = (int)(g / nh), r = (int)(g - (long long)c * nh);
    const size_t i = (size_t)pins[r];
#pragma unroll
    for (int d = 0; d < 3; d++) {
        const double v = V[3 * i + d];
        hp[(size_t)(3 * c + d) * ldh + r] = X ? morph_blend(v, X[3 * i + d], t[c]) : v;
    }
}

// U[col * ldu + pins[r]] = hp[col * ldh + r] for the ncols columns: the pinned rows of the start are the pins' positions
__global__ __launch_bounds__(MORPH_THREADS) void k_morph_set_pins(int nh, int ncols, const int* __restrict__ pins, const double* __restrict__ hp, int ldh,
                                                                  double* __restrict__ U, int ldu)
{
    const long long g = (long long)blockIdx.x * MORPH_THREADS + threadIdx.x;
    if (g >= (long long)nh * ncols) return;
    const int col = (int)(g / nh), r = (int)(g - (long long)col * nh);
    U[(size_t)col * ldu + pins[r]] = hp[(size_t)col * ldh + r];
}

hipError_t launch_morph_basis(const double* V, const int* F, int nF, double* W, double* nrm, double* Af, hipStream_t st)
{
    if (nF <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_morph_basis, dim3(morph_grid(nF)), dim3(MORPH_THREADS), 0, st, V, F, nF, W, nrm, Af);
    return hipGetLastError();
}

namespace {

// the grid of a (row block, set) kernel; false: it does not fit a grid dimension
bool morph_set_grid(int rows, int k, unsigned* blocks)
{
    const long long b = (long long)morph_grid(rows) * k;
    *blocks = (unsigned)b;
    return b <= 0x7fffffffLL;
}

}  // namespace

hipError_t launch_morph_face_gradient(int nF, int k, const int* Fs, const double* S0, const double* X, size_t set_stride, double* J, hipStream_t st)
{
    if (nF <= 0 || k <= 0) return hipSuccess;
    unsigned blocks = 0;
    if (!morph_set_grid(nF, k, &blocks)) return hipErrorInvalidConfiguration;
    hipLaunchKernelGGL(k_morph_face_gradient, dim3(blocks), dim3(MORPH_THREADS), 0, st, nF, k, Fs, S0, X, set_stride, J);
    return hipGetLastError();
}

hipError_t launch_morph_face_polar(int nF, const int* F, const double* W, const double* nrm, const double* X, double* R, double* omega, double* S,
                                   hipStream_t st)
{
    if (nF <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_morph_face_polar, dim3(morph_grid(nF)), dim3(MORPH_THREADS), 0, st, nF, F, W, nrm, X, R, omega, S);
    return hipGetLastError();
}

hipError_t launch_morph_rhs_gradient(int n, int k, int nF, const int* m_ptr, const int* m_idx, const double* W, const double* Af, const double* J,
                                     double* B, int ldb, double* bsq, hipStream_t st)
{
    if (n <= 0 || k <= 0) return hipSuccess;
    unsigned blocks = 0;
    if (!morph_set_grid(n, k, &blocks)) return hipErrorInvalidConfiguration;
    hipLaunchKernelGGL(k_morph_rhs<false>, dim3(blocks), dim3(MORPH_THREADS), 0, st, n, k, nF, m_ptr, m_idx, W, Af, J, nullptr, nullptr, nullptr, B, ldb,
                       bsq);
    return hipGetLastError();
}

hipError_t launch_morph_rhs_interp(int n, int k, int nF, const int* m_ptr, const int* m_idx, const double* W, const double* Af, const double* omega,
                                   const double* S, const double* t, double* B, int ldb, double* bsq, hipStream_t st)
{
    if (n <= 0 || k <= 0) return hipSuccess;
    unsigned blocks = 0;
    if (!morph_set_grid(n, k, &blocks)) return hipErrorInvalidConfiguration;
    hipLaunchKernelGGL(k_morph_rhs<true>, dim3(blocks), dim3(MORPH_THREADS), 0, st, n, k, nF, m_ptr, m_idx, W, Af, nullptr, omega, S, t, B, ldb, bsq);
    return hipGetLastError();
}

hipError_t launch_morph_start(int n, int k, const double* V, const double* X, const double* t, double* U, int ldu, hipStream_t st)
{
    if (n <= 0 || k <= 0) return hipSuccess;
    unsigned blocks = 0;
    if (!morph_set_grid(n, k, &blocks)) return hipErrorInvalidConfiguration;
    hipLaunchKernelGGL(k_morph_start, dim3(blocks), dim3(MORPH_THREADS), 0, st, n, k, V, X, t, U, ldu);
    return hipGetLastError();
}

hipError_t launch_morph_pins(int nh, int k, const int* pins, const double* V, const double* X, const double* t, double* hp, int ldh, hipStream_t st)
{
    if (nh <= 0 || k <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_morph_pins, dim3(morph_grid((long long)nh * k)), dim3(MORPH_THREADS), 0, st, nh, k, pins, V, X, t, hp, ldh);
    return hipGetLastError();
}

hipError_t launch_morph_set_pins(int nh, int ncols, const int* pins, const double* hp, int ldh, double* U, int ldu, hipStream_t st)
{
    if (nh <= 0 || ncols <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_morph_set_pins, dim3(morph_grid((long long)nh * ncols)), dim3(MORPH_THREADS), 0, st, nh, ncols, pins, hp, ldh, U, ldu);
    return hipGetLastError();
}

}  // namespace smg
