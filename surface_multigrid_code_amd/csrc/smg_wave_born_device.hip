// smg_wave_born_device.hip -- the kernel of the wave object's tangent (Born) run (smg_wave_gauss_newton, include/smg.h; host side in
// smg_wave_born.cpp; the arithmetic in smg_wave_born_inl.hpp).
//
// A tangent step is the forward step itself on the tangent state, with one distributed source added to every right-hand side:
// b += (fac d) e_n, e_n the block the gradient call kept of step n.  k_wave_born is the whole-mesh sibling of k_wave_sources: it adds the source
// and rewrites the squares the step's fixed-order sum reads.
//
// Layout: as smg_wave_device.hip.  b is a column-major block, one column per shot; e and the squares are k planes of n; fd is d_cols planes of n
// (d_cols 1 or k: one direction for every shot, or one per shot).
//
// Grid: one WAVEFRONT per (64 consecutive vertices, column), the grid of k_wave_advance (smg_wave_grid.hpp).
//
// A streaming kernel: per (vertex, column) it reads 24 bytes (b, fd, e; fd from cache where d_cols == 1) and writes 16.
//
// Determinism: no atomics; one lane owns its (vertex, column).  The expression is written operation by operation (-ffp-contract=off):
// tests/wave_gn_np.py restates it in numpy in the same order.  Only + and * occur.
#include <hip/hip_runtime.h>

#include "smg_device.hpp"
#include "smg_wave_born_inl.hpp"
#include "smg_wave_grid.hpp"

namespace smg {

// One lane per (vertex i, column c), off the known rows: x = b + fd[i, c % d_cols] e, b = x, rsq[c * n + i] = x x; a known row keeps both
__global__ __launch_bounds__(WAVE_THREADS) void k_wave_born(int n, int k, int d_cols, const int* __restrict__ known, const double* __restrict__ fd,
                                                            const double* __restrict__ e, double* __restrict__ b, int ldb, double* __restrict__ rsq)
{
    int c, i;
    if (!wave_lane(n, k, &c, &i)) return;
    if (known && known[i]) return;
    const size_t o = (size_t)c * ldb + i, pl = (size_t)c * n + i;
    const double x = wave_born(b[o], fd[(size_t)(c % d_cols) * n + i], e[pl]);
    b[o] = x;
    rsq[pl] = x * x;
}

hipError_t launch_wave_born(int n, int k, int d_cols, const int* known, const double* fd, const double* e, double* b, int ldb, double* rsq, hipStream_t st)
{
    if (n <= 0 || k <= 0) return hipSuccess;
    if (!fd || !e || !b || !rsq || ldb < n || (d_cols != 1 && d_cols != k)) return hipErrorInvalidValue;
    unsigned blocks = 0;
    if (!wave_grid(n, k, &blocks) || (long long)n * k > 0x7fffffffLL) return hipErrorInvalidConfiguration;
    hipLaunchKernelGGL(k_wave_born, dim3(blocks), dim3(WAVE_THREADS), 0, st, n, k, d_cols, known, fd, e, b, ldb, rsq);
    return hipGetLastError();
}

}  // namespace smg
