// smg_rd_device.hip -- the kernels of two-species reaction-diffusion on a surface (smg_rd_*, include/smg.h; host side in smg_rd.cpp; the
// arithmetic in smg_rd_inl.hpp).
//
// Layout: u, v, the right-hand sides and the outputs are column-major blocks with a leading dimension, one column per simulation; per-vertex
// terms (squares, m u', m v', changes) are planes of n; the coefficient table is k x 20 row-major.
//
// Grid: one WAVEFRONT per (64 consecutive vertices, column): wave W = 4 blockIdx.x + threadIdx.x / 64 works on column W % k and on the vertices
// 64 (W / k) .. + 63, so the k waves of one vertex range are adjacent and read its masses while they are in cache, and a mesh of fewer than 64
// vertices occupies one wave per column, not one block.  W is formed through readfirstlane: the column and with it the address of its 20
// coefficients are wave-uniform to the compiler, which loads the table with scalar loads into scalar registers; the sub-step loop then runs on
// the lane's u and v and those scalars alone.
//
// Determinism: no atomics; sums and maxima are launch_fixed_sum / launch_fixed_max of per-lane terms.  Expressions are written operation by
// operation (-ffp-contract=off): tests/rd_np.py restates them in numpy in the same order.  Only +, -, *, max and fabs occur.
#include <hip/hip_runtime.h>

#include "smg_device.hpp"
#include "smg_rd_inl.hpp"

namespace smg {

namespace {

constexpr int RD_THREADS = 256, RD_WAVE = 64, RD_WAVES = RD_THREADS / RD_WAVE;

// the blocks of a (64 vertices, column) wave grid; false: it does not fit a grid dimension
bool rd_wave_grid(int rows, int k, unsigned* blocks)
{
    const long long waves = (((long long)rows + RD_WAVE - 1) / RD_WAVE) * k;
    const long long b = (waves + RD_WAVES - 1) / RD_WAVES;
    *blocks = (unsigned)b;
    return b <= 0x7fffffffLL;
}

// the wave's column and the lane's vertex; false: the wave is past the grid's last one or the lane past the last vertex
__device__ __forceinline__ bool rd_lane(int n, int k, int* c, int* v)
{
    const int W = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * RD_WAVES + (threadIdx.x / RD_WAVE)));
    const int waves = ((n + RD_WAVE - 1) / RD_WAVE) * k;   // rd_wave_grid has checked the range
    if (W >= waves) return false;
    *c = W % k;
    *v = (W / k) * RD_WAVE + (int)(threadIdx.x % RD_WAVE);
    return *v < n;
}

}  // namespace

// One lane per (vertex i, column c): (u, v) through `substeps` Euler steps of length h of the column's reaction, then Ru = m_i u*, Rv = m_i v*,
// rsq[c * n + i] = Ru^2, rsq[(k + c) * n + i] = Rv^2, and vout (nullptr ok) = v*
__global__ __launch_bounds__(RD_THREADS) void k_rd_react(int n, int k, const double* __restrict__ m, const double* __restrict__ u,
                                                         const double* __restrict__ v, int ld, const double* __restrict__ coef, double h, int substeps,
                                                         double* __restrict__ Ru, double* __restrict__ Rv, int ldr, double* __restrict__ rsq,
                                                         double* __restrict__ vout, int ldv)
{
    int c, i;
    if (!rd_lane(n, k, &c, &i)) return;
    const double* cc = coef + (size_t)c * RD_COEFFS;
    double cf[RD_COEFFS];
#pragma unroll
    for (int j = 0; j < RD_COEFFS; j++) cf[j] = cc[j];
    double a = u[(size_t)c * ld + i], b = v[(size_t)c * ld + i];
    rd_react(cf, h, substeps, &a, &b);
    const double mi = m[i];
    const double bu = mi * a, bv = mi * b;
    Ru[(size_t)c * ldr + i] = bu;
    Rv[(size_t)c * ldr + i] = bv;
    rsq[(size_t)c * n + i] = bu * bu;
    rsq[((size_t)k + c) * n + i] = bv * bv;
    if (vout) vout[(size_t)c * ldv + i] = b;
}

// One lane per (vertex i, column c): mt[c * n + i] = m_i u', mt[(k + c) * n + i] = m_i v', chg[c * n + i] = max(|u' - u|, |v' - v|)
__global__ __launch_bounds__(RD_THREADS) void k_rd_close(int n, int k, const double* __restrict__ m, const double* __restrict__ u0,
                                                         const double* __restrict__ v0, const double* __restrict__ u1, const double* __restrict__ v1,
                                                         int ld, double* __restrict__ mt, double* __restrict__ chg)
{
    int c, i;
    if (!rd_lane(n, k, &c, &i)) return;
    const size_t e = (size_t)c * ld + i;
    const double mi = m[i], a = u1[e], b = v1[e];
    mt[(size_t)c * n + i] = mi * a;
    mt[((size_t)k + c) * n + i] = mi * b;
    chg[(size_t)c * n + i] = rd_change(u0[e], v0[e], a, b);
}

hipError_t launch_rd_react(int n, int k, const double* m, const double* u, const double* v, int ld, const double* coef, double h, int substeps,
                           double* Ru, double* Rv, int ldr, double* rsq, double* vout, int ldv, hipStream_t st)
{
    if (n <= 0 || k <= 0) return hipSuccess;
    if (!m || !u || !v || !coef || !Ru || !Rv || !rsq || substeps < 1 || ld < n || ldr < n || (vout && ldv < n)) return hipErrorInvalidValue;
    unsigned blocks = 0;
    if (!rd_wave_grid(n, k, &blocks) || (long long)n * k * 2 > 0x7fffffffLL) return hipErrorInvalidConfiguration;
    hipLaunchKernelGGL(k_rd_react, dim3(blocks), dim3(RD_THREADS), 0, st, n, k, m, u, v, ld, coef, h, substeps, Ru, Rv, ldr, rsq, vout, ldv);
    return hipGetLastError();
}

hipError_t launch_rd_close(int n, int k, const double* m, const double* u0, const double* v0, const double* u1, const double* v1, int ld, double* mt,
                           double* chg, hipStream_t st)
{
    if (n <= 0 || k <= 0) return hipSuccess;
    if (!m || !u0 || !v0 || !u1 || !v1 || !mt || !chg || ld < n) return hipErrorInvalidValue;
    unsigned blocks = 0;
    if (!rd_wave_grid(n, k, &blocks) || (long long)n * k * 2 > 0x7fffffffLL) return hipErrorInvalidConfiguration;
    hipLaunchKernelGGL(k_rd_close, dim3(blocks), dim3(RD_THREADS), 0, st, n, k, m, u0, v0, u1, v1, ld, mt, chg);
    return hipGetLastError();
}

}  // namespace smg
