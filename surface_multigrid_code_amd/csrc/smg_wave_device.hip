// smg_wave_device.hip -- the kernels of the wave equation on a surface (smg_wave_*, include/smg.h; host side in smg_wave.cpp; the arithmetic in
// smg_wave_inl.hpp).
//
// Layout: u, v, the right-hand side b, the warm start z and the solve's answer w are column-major blocks with a leading dimension, one column per
// experiment; mt, s2 and the known mask are planes of n; per-vertex terms (squares, kinetic energies) are k planes of n; signals and traces are
// rows of (source or receiver) x column.
//
// Grid of the two vertex kernels: one WAVEFRONT per (64 consecutive vertices, column), as smg_rd_device.hip: wave W = 4 blockIdx.x +
// threadIdx.x / 64 works on column W % k and on the vertices 64 (W / k) .. + 63, so the k waves of one vertex range are adjacent and read its mt
// and s2 while they are in cache, and a mesh of fewer than 64 vertices occupies one wave per column, not one block.  The source, record and
// clamp kernels run one lane per (list entry, column).
//
// These are streaming kernels: per (vertex, column) k_wave_rhs reads 16 bytes and writes 24, k_wave_advance reads 24 and writes 24, and with the
// next right-hand side 24 more; per vertex both read mt and s2 once for the k columns.
//
// Determinism: no atomics (a source list holds no vertex twice); sums are launch_fixed_sum of per-lane terms.  Expressions are written operation
// by operation (-ffp-contract=off): tests/wave_np.py restates them in numpy in the same order.  Only +, - and * occur.
#include <hip/hip_runtime.h>

#include "smg_device.hpp"
#include "smg_wave_grid.hpp"
#include "smg_wave_inl.hpp"

namespace smg {

// One lane per (vertex i, column c): b = mt_i (s2_i u + dt v), rsq[c * n + i] = b^2 (0.0 where known[i]), z = 2 u + dt v
__global__ __launch_bounds__(WAVE_THREADS) void k_wave_rhs(int n, int k, const double* __restrict__ mt, const double* __restrict__ s2,
                                                           const int* __restrict__ known, double dt, const double* __restrict__ u,
                                                           const double* __restrict__ v, int ld, double* __restrict__ b, double* __restrict__ z, int ldb,
                                                           double* __restrict__ rsq)
{
    int c, i;
    if (!wave_lane(n, k, &c, &i)) return;
    const size_t e = (size_t)c * ld + i, o = (size_t)c * ldb + i;
    double bi, zi;
    wave_rhs(mt[i], s2[i], dt, u[e], v[e], &bi, &zi);
    b[o] = bi;
    z[o] = zi;
    rsq[(size_t)c * n + i] = known && known[i] ? 0.0 : bi * bi;
}

// One lane per (source j, column c): b += a (sig0 + sig1) at the source's vertex, and its square again
__global__ __launch_bounds__(WAVE_THREADS) void k_wave_sources(int n, int k, int n_src, const int* __restrict__ idx, const double* __restrict__ sig0,
                                                               const double* __restrict__ sig1, double a, double* __restrict__ b, int ldb,
                                                               double* __restrict__ rsq)
{
    const long long t = (long long)blockIdx.x * WAVE_THREADS + threadIdx.x;
    if (t >= (long long)n_src * k) return;
    const int j = (int)(t / k), c = (int)(t % k), i = idx[j];
    const size_t o = (size_t)c * ldb + i;
    const double x = wave_source(b[o], a, sig0[t], sig1[t]);
    b[o] = x;
    rsq[(size_t)c * n + i] = x * x;
}

// One lane per (vertex i, column c): u' = w - u, v' = q2 (u' - u) - v, ke[c * n + i] = 0.5 ((mt_i v') v'); NEXT: the right-hand side, its squares
// and the warm start of (u', v'), the expressions of k_wave_rhs.  zn may be w itself (the object's step: the lane reads its w before it writes
// its zn), so neither of the two is declared __restrict__
template <bool NEXT>
__global__ __launch_bounds__(WAVE_THREADS) void k_wave_advance(int n, int k, const double* __restrict__ mt, const double* __restrict__ s2,
                                                               const int* __restrict__ known, double dt, double q2, const double* w, int ldw,
                                                               const double* __restrict__ u, const double* __restrict__ v, int ld,
                                                               double* __restrict__ un, double* __restrict__ vn, int ldn, double* __restrict__ ke,
                                                               double* __restrict__ bn, double* zn, int ldb, double* __restrict__ rsqn)
{
    int c, i;
    if (!wave_lane(n, k, &c, &i)) return;
    const size_t e = (size_t)c * ld + i, o = (size_t)c * ldn + i;
    const double mi = mt[i];
    double u1, v1, kin;
    wave_advance(mi, q2, w[(size_t)c * ldw + i], u[e], v[e], &u1, &v1, &kin);
    un[o] = u1;
    vn[o] = v1;
    ke[(size_t)c * n + i] = kin;
    if (NEXT) {
        double bi, zi;
        wave_rhs(mi, s2[i], dt, u1, v1, &bi, &zi);
        bn[(size_t)c * ldb + i] = bi;
        zn[(size_t)c * ldb + i] = zi;
        rsqn[(size_t)c * n + i] = known && known[i] ? 0.0 : bi * bi;
    }
}

// One lane per (receiver j, column c): out[j * k + c] = u at the receiver's vertex
__global__ __launch_bounds__(WAVE_THREADS) void k_wave_record(int k, int n_rec, const int* __restrict__ idx, const double* __restrict__ u, int ld,
                                                              double* __restrict__ out)
{
    const long long t = (long long)blockIdx.x * WAVE_THREADS + threadIdx.x;
    if (t >= (long long)n_rec * k) return;
    const int j = (int)(t / k), c = (int)(t % k);
    out[t] = u[(size_t)c * ld + idx[j]];
}

// One lane per (listed row j, column c): flag[j * k + c] = 1.0 where u or v is not 0.0 there (a NaN is not 0.0), else 0.0
__global__ __launch_bounds__(WAVE_THREADS) void k_wave_rows_nonzero(int k, int n_rows, const int* __restrict__ rows, const double* __restrict__ u,
                                                                    const double* __restrict__ v, int ld, double* __restrict__ flag)
{
    const long long t = (long long)blockIdx.x * WAVE_THREADS + threadIdx.x;
    if (t >= (long long)n_rows * k) return;
    const int j = (int)(t / k), c = (int)(t % k);
    const size_t e = (size_t)c * ld + rows[j];
    flag[t] = (u[e] != 0.0 || v[e] != 0.0) ? 1.0 : 0.0;
}

hipError_t launch_wave_rhs(int n, int k, const double* mt, const double* s2, const int* known, double dt, const double* u, const double* v, int ld, double* b,
                           double* z, int ldb, double* rsq, hipStream_t st)
{
    if (n <= 0 || k <= 0) return hipSuccess;
    if (!mt || !s2 || !u || !v || !b || !z || !rsq || ld < n || ldb < n) return hipErrorInvalidValue;
    unsigned blocks = 0;
    if (!wave_grid(n, k, &blocks) || (long long)n * k > 0x7fffffffLL) return hipErrorInvalidConfiguration;
    hipLaunchKernelGGL(k_wave_rhs, dim3(blocks), dim3(WAVE_THREADS), 0, st, n, k, mt, s2, known, dt, u, v, ld, b, z, ldb, rsq);
    return hipGetLastError();
}

hipError_t launch_wave_sources(int n, int k, int n_src, const int* idx, const double* sig0, const double* sig1, double a, double* b, int ldb, double* rsq,
                               hipStream_t st)
{
    if (n <= 0 || k <= 0 || n_src <= 0) return hipSuccess;
    if (!idx || !sig0 || !sig1 || !b || !rsq || ldb < n) return hipErrorInvalidValue;
    if ((long long)n_src * k > 0x7fffffffLL) return hipErrorInvalidConfiguration;
    hipLaunchKernelGGL(k_wave_sources, dim3(list_grid(n_src, k)), dim3(WAVE_THREADS), 0, st, n, k, n_src, idx, sig0, sig1, a, b, ldb, rsq);
    return hipGetLastError();
}

hipError_t launch_wave_advance(int n, int k, const double* mt, const double* s2, const int* known, double dt, double q2, const double* w, int ldw,
                               const double* u, const double* v, int ld, double* un, double* vn, int ldn, double* ke, double* bnext, double* znext, int ldb,
                               double* rsqnext, hipStream_t st)
{
    if (n <= 0 || k <= 0) return hipSuccess;
    if (!mt || !w || !u || !v || !un || !vn || !ke || ldw < n || ld < n || ldn < n) return hipErrorInvalidValue;
    if (bnext && (!s2 || !znext || !rsqnext || ldb < n)) return hipErrorInvalidValue;
    unsigned blocks = 0;
    if (!wave_grid(n, k, &blocks) || (long long)n * k > 0x7fffffffLL) return hipErrorInvalidConfiguration;
    if (bnext)
        hipLaunchKernelGGL(k_wave_advance<true>, dim3(blocks), dim3(WAVE_THREADS), 0, st, n, k, mt, s2, known, dt, q2, w, ldw, u, v, ld, un, vn, ldn, ke, bnext,
                           znext, ldb, rsqnext);
    else
        hipLaunchKernelGGL(k_wave_advance<false>, dim3(blocks), dim3(WAVE_THREADS), 0, st, n, k, mt, s2, known, dt, q2, w, ldw, u, v, ld, un, vn, ldn, ke,
                           nullptr, nullptr, ldb, nullptr);
    return hipGetLastError();
}

hipError_t launch_wave_record(int n, int k, int n_rec, const int* idx, const double* u, int ld, double* out, hipStream_t st)
{
    if (n <= 0 || k <= 0 || n_rec <= 0) return hipSuccess;
    if (!idx || !u || !out || ld < n) return hipErrorInvalidValue;
    if ((long long)n_rec * k > 0x7fffffffLL) return hipErrorInvalidConfiguration;
    hipLaunchKernelGGL(k_wave_record, dim3(list_grid(n_rec, k)), dim3(WAVE_THREADS), 0, st, k, n_rec, idx, u, ld, out);
    return hipGetLastError();
}

hipError_t launch_wave_rows_nonzero(int n, int k, int n_rows, const int* rows, const double* u, const double* v, int ld, double* flag, hipStream_t st)
{
    if (n <= 0 || k <= 0 || n_rows <= 0) return hipSuccess;
    if (!rows || !u || !v || !flag || ld < n) return hipErrorInvalidValue;
    if ((long long)n_rows * k > 0x7fffffffLL) return hipErrorInvalidConfiguration;
    hipLaunchKernelGGL(k_wave_rows_nonzero, dim3(list_grid(n_rows, k)), dim3(WAVE_THREADS), 0, st, k, n_rows, rows, u, v, ld, flag);
    return hipGetLastError();
}

}  // namespace smg
