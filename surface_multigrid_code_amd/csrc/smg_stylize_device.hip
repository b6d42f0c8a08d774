// smg_stylize_device.hip -- the local step of cubic and normal-driven stylization (smg_stylize_run, include/smg.h; host side in smg_stylize.cpp;
// DESIGN.md section 25).  The matrix is smg_arap's: the CSR of the rest pose's cotangent matrix L (diagonal included and skipped: N(i) = the
// off-diagonal entries of row i in stored order, w_ij = L_ij); the global step's right-hand side is k_arap_rhs, called unchanged.
//
// Layout: rest positions P0, current positions P, normals and targets are xyz rows (3 doubles per vertex), rotations are 9 contiguous doubles
// per vertex (row-major) as k_arap_rhs gathers them; the ADMM state is 7 planes of n (z, u, rho), read once and written once per lane.
//
// k_stylize_local runs one lane per vertex.  The covariance, the normal, the state and the Jacobi's working set stay in registers for the whole
// ADMM loop; a lane whose stopping test holds leaves the loop and idles until the slowest lane of its wavefront is done.
//
// Determinism: no atomics.  Every per-vertex sum is one lane's sequential loop in the row's (or corner list's) stored order; the energy is the
// fixed-order sum of the vertices' terms (launch_fixed_sum).  The maths is smg_stylize_inl.hpp, the text the host twin compiles too.
#include <hip/hip_runtime.h>

#include "smg_device.hpp"
#include "smg_stylize_inl.hpp"

namespace smg {

namespace {

constexpr int STY_THREADS = 256;

inline int sty_grid(long long n) { return (int)((n + STY_THREADS - 1) / STY_THREADS); }

}  // namespace

// MODE STY_CUBIC: the ADMM loop (p.admm_iters == 1: the hook's single iteration).  STY_TARGETS: one fit against tgt.  STY_ENERGY: the energy
// terms of the rotations in R (tgt != nullptr: the normal-driven term).
template <int MODE>
__global__ __launch_bounds__(STY_THREADS, 4) void k_stylize_local(int n, const int* __restrict__ rowptr, const int* __restrict__ col,
                                                               const double* __restrict__ w, const double* __restrict__ P0,
                                                               const double* __restrict__ P, const double* __restrict__ nrm,
                                                               const double* __restrict__ area, const double* __restrict__ lam, StyFrame Q,
                                                               const double* __restrict__ tgt, StyParams p, int fresh, double* __restrict__ state,
                                                               double* __restrict__ R, double* __restrict__ eterm, int* __restrict__ iters)
{
    const int i = blockIdx.x * STY_THREADS + threadIdx.x;
    if (i >= n) return;
    sty_local_vertex<MODE>(i, n, rowptr, col, w, P0, P, nrm, area, lam, Q, tgt, p, fresh, state, R, eterm, iters);
}

__global__ __launch_bounds__(STY_THREADS) void k_stylize_normals(int n, const int* __restrict__ F, const int* __restrict__ mp, const int* __restrict__ mi,
                                                                 const double* __restrict__ V, double* __restrict__ nrm, double* __restrict__ area)
{
    const int i = blockIdx.x * STY_THREADS + threadIdx.x;
    if (i >= n) return;
    sty_vertex_normal_area(i, F, mp, mi, V, nrm, area);
}

hipError_t launch_stylize_normals(int n, const int* F, const int* mp, const int* mi, const double* V, double* nrm, double* area, hipStream_t st)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_stylize_normals, dim3(sty_grid(n)), dim3(STY_THREADS), 0, st, n, F, mp, mi, V, nrm, area);
    return hipGetLastError();
}

hipError_t launch_stylize_cubic(int n, const int* rowptr, const int* col, const double* w, const double* P0, const double* P, const double* nrm,
                                const double* area, const double* lam, const StyFrame& Q, const StyParams& p, int fresh, double* state, double* R,
                                double* eterm, int* iters, hipStream_t st)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_stylize_local<STY_CUBIC>, dim3(sty_grid(n)), dim3(STY_THREADS), 0, st, n, rowptr, col, w, P0, P, nrm, area, lam, Q, nullptr, p,
                       fresh, state, R, eterm, iters);
    return hipGetLastError();
}

hipError_t launch_stylize_targets(int n, const int* rowptr, const int* col, const double* w, const double* P0, const double* P, const double* nrm,
                                  const double* area, const double* lam, const double* tgt, const StyParams& p, double* R, double* eterm, int* iters,
                                  hipStream_t st)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_stylize_local<STY_TARGETS>, dim3(sty_grid(n)), dim3(STY_THREADS), 0, st, n, rowptr, col, w, P0, P, nrm, area, lam, StyFrame{}, tgt,
                       p, 0, nullptr, R, eterm, iters);
    return hipGetLastError();
}

hipError_t launch_stylize_energy(int n, const int* rowptr, const int* col, const double* w, const double* P0, const double* P, const double* nrm,
                                 const double* area, const double* lam, const StyFrame& Q, const double* tgt, const StyParams& p, const double* R,
                                 double* eterm, hipStream_t st)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_stylize_local<STY_ENERGY>, dim3(sty_grid(n)), dim3(STY_THREADS), 0, st, n, rowptr, col, w, P0, P, nrm, area, lam, Q, tgt, p, 0,
                       nullptr, const_cast<double*>(R), eterm, nullptr);
    return hipGetLastError();
}

}  // namespace smg
