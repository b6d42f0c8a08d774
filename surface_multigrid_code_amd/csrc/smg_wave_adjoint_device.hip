// smg_wave_adjoint_device.hip -- the kernels of the wave object's adjoint pass (smg_wave_gradient, include/smg.h; host side in
// smg_wave_adjoint.cpp; the arithmetic in smg_wave_adjoint_inl.hpp).
//
// Layout: as smg_wave_device.hip.  The adjoint state p, q, the adjoint solve's answer y, the accumulator G and a history block e are column-major
// blocks, one column per shot; a trace row is (receiver slot) x column; the residuals' squares are k planes of (rows x slots).
//
// Grid: the vertex kernels (keep, rhs, advance, scale) run one WAVEFRONT per (64 consecutive vertices, column), the grid of k_wave_advance
// (smg_wave_grid.hpp); the list kernels (residual, inject, signal) one lane per (entry, column).
//
// These are streaming kernels: per (vertex, column) k_wave_adj_keep reads 24 bytes and writes 8, k_wave_adj_rhs reads 16 and writes 16,
// k_wave_adj_advance reads 40 and writes 24; per vertex they read mt and s2 once for the k columns.
//
// Determinism: no atomics.  The receivers are grouped by vertex on the host (wave_group_receivers), so one lane owns a vertex and adds its slots
// in ascending order; a source list holds no vertex twice; sums are launch_fixed_sum of per-lane terms.  Expressions are written operation by
// operation (-ffp-contract=off): tests/wave_adjoint_np.py restates them in numpy in the same order.  Only +, - and * occur.
#include <hip/hip_runtime.h>

#include "smg_device.hpp"
#include "smg_wave_adjoint_inl.hpp"
#include "smg_wave_grid.hpp"

namespace smg {

// One lane per (vertex i, column c): e = dt v - (0.5 s2_i) (u1 - u)
__global__ __launch_bounds__(WAVE_THREADS) void k_wave_adj_keep(int n, int k, const double* __restrict__ s2, double dt, const double* __restrict__ u,
                                                                const double* __restrict__ v, const double* __restrict__ u1, int ld,
                                                                double* __restrict__ e)
{
    int c, i;
    if (!wave_lane(n, k, &c, &i)) return;
    const size_t o = (size_t)c * ld + i;
    e[(size_t)c * n + i] = wave_adj_keep(s2[i], dt, u[o], v[o], u1[o]);
}

// One lane per (entry j of rows x slots, column c): rho = trace - observed, its square into plane c
__global__ __launch_bounds__(WAVE_THREADS) void k_wave_adj_residual(int k, int entries, const double* __restrict__ trace,
                                                                    const double* __restrict__ observed, double* __restrict__ rho,
                                                                    double* __restrict__ sq)
{
    unsigned t;
    int j, c;
    if (!list_lane((unsigned)entries * (unsigned)k, (unsigned)k, &t, &j, &c)) return;
    const double r = observed ? trace[t] - observed[t] : trace[t];
    rho[t] = r;
    sq[(size_t)c * (size_t)entries + (size_t)j] = r * r;
}

// One lane per (group j, column c): p += the group's slots of one trace row, in ascending slot order
__global__ __launch_bounds__(WAVE_THREADS) void k_wave_adj_inject(int k, int n_grp, const int* __restrict__ grp_v, const int* __restrict__ grp_ptr,
                                                                  const int* __restrict__ grp_slot, const double* __restrict__ rho, double* __restrict__ p,
                                                                  int ld)
{
    unsigned t;
    int j, c;
    if (!list_lane((unsigned)n_grp * (unsigned)k, (unsigned)k, &t, &j, &c)) return;
    const int s0 = grp_ptr[j], s1 = grp_ptr[j + 1];
    double x = rho[(size_t)grp_slot[s0] * k + c];
    for (int s = s0 + 1; s < s1; s++) x = x + rho[(size_t)grp_slot[s] * k + c];
    const size_t e = (size_t)c * ld + grp_v[j];
    p[e] = p[e] + x;
}

// One lane per (vertex i, column c): g = p + q2 q and gsq[c * n + i] = g g, both 0.0 where known[i]
__global__ __launch_bounds__(WAVE_THREADS) void k_wave_adj_rhs(int n, int k, const int* __restrict__ known, double q2, const double* __restrict__ p,
                                                               const double* __restrict__ q, int ld, double* __restrict__ g, int ldg,
                                                               double* __restrict__ gsq)
{
    int c, i;
    if (!wave_lane(n, k, &c, &i)) return;
    const size_t e = (size_t)c * ld + i;
    const double x = known && known[i] ? 0.0 : wave_adj_rhs(q2, p[e], q[e]);
    g[(size_t)c * ldg + i] = x;
    gsq[(size_t)c * n + i] = x * x;
}

// One lane per (vertex i, column c): G += y e, t = mt_i y, p' = (s2_i t - p) - (2.0 q2) q, q' = dt t - q; p, q and G in place (the lane reads its
// entries before it writes them)
__global__ __launch_bounds__(WAVE_THREADS) void k_wave_adj_advance(int n, int k, const double* __restrict__ mt, const double* __restrict__ s2, double dt,
                                                                   double q2, const double* __restrict__ y, int ldy, const double* __restrict__ e,
                                                                   double* __restrict__ p, double* __restrict__ q, double* __restrict__ G, int ld)
{
    int c, i;
    if (!wave_lane(n, k, &c, &i)) return;
    const size_t o = (size_t)c * ld + i;
    double pn, qn, Gn;
    wave_adj_advance(mt[i], s2[i], dt, q2, y[(size_t)c * ldy + i], e[(size_t)c * n + i], p[o], q[o], G[o], &pn, &qn, &Gn);
    p[o] = pn;
    q[o] = qn;
    G[o] = Gn;
}

// One lane per (source j, column c): gs0 += a y, gs1 += a y at the source's vertex
__global__ __launch_bounds__(WAVE_THREADS) void k_wave_adj_signal(int k, int n_src, const int* __restrict__ idx, double a, const double* __restrict__ y,
                                                                  int ld, double* __restrict__ gs0, double* __restrict__ gs1)
{
    unsigned t;
    int j, c;
    if (!list_lane((unsigned)n_src * (unsigned)k, (unsigned)k, &t, &j, &c)) return;
    const double x = a * y[(size_t)c * ld + idx[j]];
    gs0[t] = gs0[t] + x;
    gs1[t] = gs1[t] + x;
}

// One lane per (vertex i, column c): out = fac_i G; out may be G itself, so neither is declared __restrict__
__global__ __launch_bounds__(WAVE_THREADS) void k_wave_adj_scale(int n, int k, const double* __restrict__ fac, const double* G, int ld, double* out, int ldo)
{
    int c, i;
    if (!wave_lane(n, k, &c, &i)) return;
    out[(size_t)c * ldo + i] = fac[i] * G[(size_t)c * ld + i];
}

hipError_t launch_wave_adj_keep(int n, int k, const double* s2, double dt, const double* u, const double* v, const double* u1, int ld, double* e, hipStream_t st)
{
    if (n <= 0 || k <= 0) return hipSuccess;
    if (!s2 || !u || !v || !u1 || !e || ld < n) return hipErrorInvalidValue;
    unsigned blocks = 0;
    if (!wave_grid(n, k, &blocks) || (long long)n * k > 0x7fffffffLL) return hipErrorInvalidConfiguration;
    hipLaunchKernelGGL(k_wave_adj_keep, dim3(blocks), dim3(WAVE_THREADS), 0, st, n, k, s2, dt, u, v, u1, ld, e);
    return hipGetLastError();
}

hipError_t launch_wave_adj_residual(int k, long long entries, const double* trace, const double* observed, double* rho, double* sq, hipStream_t st)
{
    if (k <= 0 || entries <= 0) return hipSuccess;
    if (!trace || !rho || !sq) return hipErrorInvalidValue;
    if (entries * k > 0x7fffffffLL) return hipErrorInvalidConfiguration;
    hipLaunchKernelGGL(k_wave_adj_residual, dim3(list_grid((int)entries, k)), dim3(WAVE_THREADS), 0, st, k, (int)entries, trace,
                       observed, rho, sq);
    return hipGetLastError();
}

hipError_t launch_wave_adj_inject(int n, int k, int n_grp, const int* grp_v, const int* grp_ptr, const int* grp_slot, const double* rho, double* p, int ld,
                                  hipStream_t st)
{
    if (n <= 0 || k <= 0 || n_grp <= 0) return hipSuccess;
    if (!grp_v || !grp_ptr || !grp_slot || !rho || !p || ld < n) return hipErrorInvalidValue;
    if ((long long)n_grp * k > 0x7fffffffLL) return hipErrorInvalidConfiguration;
    hipLaunchKernelGGL(k_wave_adj_inject, dim3(list_grid(n_grp, k)), dim3(WAVE_THREADS), 0, st, k, n_grp, grp_v, grp_ptr, grp_slot, rho, p, ld);
    return hipGetLastError();
}

hipError_t launch_wave_adj_rhs(int n, int k, const int* known, double q2, const double* p, const double* q, int ld, double* g, int ldg, double* gsq,
                               hipStream_t st)
{
    if (n <= 0 || k <= 0) return hipSuccess;
    if (!p || !q || !g || !gsq || ld < n || ldg < n) return hipErrorInvalidValue;
    unsigned blocks = 0;
    if (!wave_grid(n, k, &blocks) || (long long)n * k > 0x7fffffffLL) return hipErrorInvalidConfiguration;
    hipLaunchKernelGGL(k_wave_adj_rhs, dim3(blocks), dim3(WAVE_THREADS), 0, st, n, k, known, q2, p, q, ld, g, ldg, gsq);
    return hipGetLastError();
}

hipError_t launch_wave_adj_advance(int n, int k, const double* mt, const double* s2, double dt, double q2, const double* y, int ldy, const double* e, double* p,
                                   double* q, double* G, int ld, hipStream_t st)
{
    if (n <= 0 || k <= 0) return hipSuccess;
    if (!mt || !s2 || !y || !e || !p || !q || !G || ldy < n || ld < n) return hipErrorInvalidValue;
    unsigned blocks = 0;
    if (!wave_grid(n, k, &blocks) || (long long)n * k > 0x7fffffffLL) return hipErrorInvalidConfiguration;
    hipLaunchKernelGGL(k_wave_adj_advance, dim3(blocks), dim3(WAVE_THREADS), 0, st, n, k, mt, s2, dt, q2, y, ldy, e, p, q, G, ld);
    return hipGetLastError();
}

hipError_t launch_wave_adj_signal(int n, int k, int n_src, const int* idx, double a, const double* y, int ld, double* gs0, double* gs1, hipStream_t st)
{
    if (n <= 0 || k <= 0 || n_src <= 0) return hipSuccess;
    if (!idx || !y || !gs0 || !gs1 || ld < n) return hipErrorInvalidValue;
    if ((long long)n_src * k > 0x7fffffffLL) return hipErrorInvalidConfiguration;
    hipLaunchKernelGGL(k_wave_adj_signal, dim3(list_grid(n_src, k)), dim3(WAVE_THREADS), 0, st, k, n_src, idx, a, y, ld, gs0, gs1);
    return hipGetLastError();
}

hipError_t launch_wave_adj_scale(int n, int k, const double* fac, const double* G, int ld, double* out, int ldo, hipStream_t st)
{
    if (n <= 0 || k <= 0) return hipSuccess;
    if (!fac || !G || !out || ld < n || ldo < n) return hipErrorInvalidValue;
    unsigned blocks = 0;
    if (!wave_grid(n, k, &blocks) || (long long)n * k > 0x7fffffffLL) return hipErrorInvalidConfiguration;
    hipLaunchKernelGGL(k_wave_adj_scale, dim3(blocks), dim3(WAVE_THREADS), 0, st, n, k, fac, G, ld, out, ldo);
    return hipGetLastError();
}

}  // namespace smg
