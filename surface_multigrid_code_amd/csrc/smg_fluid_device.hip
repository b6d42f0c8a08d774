// smg_fluid_device.hip -- the kernels of incompressible flow on a surface in vorticity form (smg_fluid_*, include/smg.h; host side in
// smg_fluid.cpp; the arithmetic in smg_fluid_inl.hpp).
//
// Layout: vorticity, stream function, right-hand sides and stage outputs are column-major blocks with a leading dimension, one column per
// simulation; per-vertex terms (rates, m w, squares) are k planes of n; W, nrm, Af are 9, 3, 1 doubles per face (k_hodge_geometry); a velocity is
// 3 doubles per (face, column), column c at c * 3 nF.
//
// Determinism: no atomics.  A vertex's transport is one lane's sequential loop over its corners in corner-list order (faces ascending, the
// segment towards the next vertex before the one towards the previous); sums and maxima are launch_fixed_sum / launch_fixed_max of per-lane
// terms.  Expressions are written operation by operation (-ffp-contract=off): tests/fluid_np.py restates them in numpy in the same order.  Only
// +, -, *, /, max and fabs occur.
//
// Grid order of the (vertex, column) and (face, column) kernels: the k blocks of one vertex (face) block are adjacent (blockIdx.x = block * k + c),
// so a block's corner lists, faces and masses are read for all columns while they are still in cache, as in k_emd_rhs.
#include <hip/hip_runtime.h>

#include "smg_device.hpp"
#include "smg_fluid_inl.hpp"

namespace smg {

namespace {

constexpr int FLUID_THREADS = 256;

inline int fluid_grid(long long n) { return (int)((n + FLUID_THREADS - 1) / FLUID_THREADS); }

// the grid of a (row block, column) kernel; false: it does not fit a grid dimension
bool fluid_column_grid(int rows, int k, unsigned* blocks)
{
    const long long b = (long long)fluid_grid(rows) * k;
    *blocks = (unsigned)b;
    return b <= 0x7fffffffLL;
}

}  // namespace

// One lane per vertex: m[v] = (sum of Af over v's corners, in list order) / 3.0
__global__ __launch_bounds__(FLUID_THREADS) void k_fluid_mass(int n, const int* __restrict__ m_ptr, const int* __restrict__ m_idx,
                                                              const double* __restrict__ Af, double* __restrict__ m)
{
    const int v = blockIdx.x * FLUID_THREADS + threadIdx.x;
    if (v >= n) return;
    double acc = 0.0;
    const int p1 = m_ptr[v + 1];
    for (int p = m_ptr[v]; p < p1; p++) acc += Af[m_idx[p] / 3];
    m[v] = acc / 3.0;
}

// One lane per (vertex v, column c): R[c * ldr + v] = 0.0 - m_v (w - wbar_c), wbar_c = mwsum[c] / *msum (mwsum nullptr: 0.0);
// rsq[c * n + v] = the square, 0.0 on a known row (known nullptr: no row is known)
__global__ __launch_bounds__(FLUID_THREADS) void k_fluid_rhs(int n, int k, const double* __restrict__ m, const int* __restrict__ known,
                                                             const double* __restrict__ w, int ldw, const double* __restrict__ mwsum,
                                                             const double* __restrict__ msum, double* __restrict__ R, int ldr, double* __restrict__ rsq)
{
    const int c = (int)(blockIdx.x % (unsigned)k);
    const int v = (int)(blockIdx.x / (unsigned)k) * FLUID_THREADS + (int)threadIdx.x;
    if (v >= n) return;
    const double wbar = mwsum ? mwsum[c] / msum[0] : 0.0;
    const double r = fluid_rhs(m[v], w[(size_t)c * ldw + v], wbar);
    R[(size_t)c * ldr + v] = r;
    rsq[(size_t)c * n + v] = known && known[v] ? 0.0 : r * r;
}

// One lane per (vertex v, column c), the hot kernel: over v's corners in list order it gathers psi and w at the face's three vertices and
// accumulates the two segments' transport and outflow; rate[c * n + v] = outflow / m_v.  Unless RATES_ONLY: out[c * ldo + v] =
// a wn + b (w + dt_c adv) and mw[c * n + v] = m_v out.  out must not alias w.
template <bool RATES_ONLY>
__global__ __launch_bounds__(FLUID_THREADS) void k_fluid_advect(int n, int k, const int* __restrict__ F, const int* __restrict__ m_ptr,
                                                                const int* __restrict__ m_idx, const double* __restrict__ m,
                                                                const double* __restrict__ psi, int ldp, const double* __restrict__ w, int ldw,
                                                                const double* __restrict__ wn, int ldn, double a, double b,
                                                                const double* __restrict__ dt, double theta, double* __restrict__ out, int ldo,
                                                                double* __restrict__ rate, double* __restrict__ mw)
{
    const int c = (int)(blockIdx.x % (unsigned)k);
    const int v = (int)(blockIdx.x / (unsigned)k) * FLUID_THREADS + (int)threadIdx.x;
    if (v >= n) return;
    const double* pc = psi + (size_t)c * ldp;
    const double* wc = RATES_ONLY ? nullptr : w + (size_t)c * ldw;
    const double pv = pc[v];
    const double wv = RATES_ONLY ? 0.0 : wc[v];
    double acc = 0.0, racc = 0.0;
    const int p1 = m_ptr[v + 1];
    for (int p = m_ptr[v]; p < p1; p++) {
        const int q = m_idx[p];
        const int f = q / 3, i = q - 3 * f;
        const int j = i == 2 ? 0 : i + 1, l = i == 0 ? 2 : i - 1;
        const int vj = F[3 * (size_t)f + j], vk = F[3 * (size_t)f + l];
        if (RATES_ONLY)
            fluid_corner_rate(pv, pc[vj], pc[vk], &racc);
        else
            fluid_corner(pv, pc[vj], pc[vk], wv, wc[vj], wc[vk], theta, &acc, &racc);
    }
    const double mv = m[v];
    rate[(size_t)c * n + v] = racc / mv;
    if (!RATES_ONLY) {
        const double o = fluid_stage(a, b, wn[(size_t)c * ldn + v], wv, dt[c], acc, mv);
        out[(size_t)c * ldo + v] = o;
        mw[(size_t)c * n + v] = mv * o;
    }
}

// One block.  op 0: dt[c] = cfl / rmax[c] (0.0 where rmax is not > 0).  op 1, the end of a step: his_cfl[c] = dt[c] max_s rmax[s * k + c] over
// its stages, time[c] += dt[c], his_time[c] = time[c]
__global__ __launch_bounds__(FLUID_THREADS) void k_fluid_dt(int op, int k, int stages, double cfl, const double* __restrict__ rmax, double* __restrict__ dt,
                                                            double* __restrict__ time, double* __restrict__ his_cfl, double* __restrict__ his_time)
{
    for (int c = (int)threadIdx.x; c < k; c += FLUID_THREADS) {
        if (op == 0) {
            dt[c] = fluid_dt(cfl, rmax[c]);
        } else {
            double r = rmax[c];
            for (int s = 1; s < stages; s++) r = fmax(r, rmax[(size_t)s * k + c]);
            const double t = time[c] + dt[c];
            time[c] = t;
            his_cfl[c] = dt[c] * r;
            his_time[c] = t;
        }
    }
}

// One lane per (face f, column c): U (nullptr ok) = n_f x grad psi_f, 3 doubles per lane, column c at c * 3 nF; terms[c * nF + f] =
// 0.5 (A_f |grad psi_f|^2)
__global__ __launch_bounds__(FLUID_THREADS) void k_fluid_velocity(int nF, int k, const int* __restrict__ F, const double* __restrict__ W,
                                                                  const double* __restrict__ nrm, const double* __restrict__ Af,
                                                                  const double* __restrict__ psi, int ldp, double* __restrict__ U, double* __restrict__ terms)
{
    const int c = (int)(blockIdx.x % (unsigned)k);
    const int f = (int)(blockIdx.x / (unsigned)k) * FLUID_THREADS + (int)threadIdx.x;
    if (f >= nF) return;
    double w9[9], nv[3], u[3], term;
#pragma unroll
    for (int e = 0; e < 9; e++) w9[e] = W[9 * (size_t)f + e];
#pragma unroll
    for (int e = 0; e < 3; e++) nv[e] = nrm[3 * (size_t)f + e];
    const double* pc = psi + (size_t)c * ldp;
    fluid_velocity(w9, nv, Af[f], pc[F[3 * (size_t)f]], pc[F[3 * (size_t)f + 1]], pc[F[3 * (size_t)f + 2]], u, &term);
    if (U) {
        double* o = U + ((size_t)c * nF + f) * 3;
        o[0] = u[0]; o[1] = u[1]; o[2] = u[2];
    }
    terms[(size_t)c * nF + f] = term;
}

// One lane per (vertex v, column c): mw[c * n + v] = m_v w, ew[c * n + v] (nullptr ok) = 0.5 ((m_v w) w)
__global__ __launch_bounds__(FLUID_THREADS) void k_fluid_diag(int n, int k, const double* __restrict__ m, const double* __restrict__ w, int ldw,
                                                              double* __restrict__ mw, double* __restrict__ ew)
{
    const int c = (int)(blockIdx.x % (unsigned)k);
    const int v = (int)(blockIdx.x / (unsigned)k) * FLUID_THREADS + (int)threadIdx.x;
    if (v >= n) return;
    double a, e;
    fluid_diag(m[v], w[(size_t)c * ldw + v], &a, &e);
    mw[(size_t)c * n + v] = a;
    if (ew) ew[(size_t)c * n + v] = e;
}

hipError_t launch_fluid_mass(int n, const int* m_ptr, const int* m_idx, const double* Af, double* m, hipStream_t st)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_fluid_mass, dim3(fluid_grid(n)), dim3(FLUID_THREADS), 0, st, n, m_ptr, m_idx, Af, m);
    return hipGetLastError();
}

hipError_t launch_fluid_rhs(int n, int k, const double* m, const int* known, const double* w, int ldw, const double* mwsum, const double* msum, double* R,
                            int ldr, double* rsq, hipStream_t st)
{
    if (n <= 0 || k <= 0) return hipSuccess;
    unsigned blocks = 0;
    if (!fluid_column_grid(n, k, &blocks)) return hipErrorInvalidConfiguration;
    hipLaunchKernelGGL(k_fluid_rhs, dim3(blocks), dim3(FLUID_THREADS), 0, st, n, k, m, known, w, ldw, mwsum, msum, R, ldr, rsq);
    return hipGetLastError();
}

hipError_t launch_fluid_advect(int n, int k, const int* F, const int* m_ptr, const int* m_idx, const double* m, const double* psi, int ldp,
                               const double* w, int ldw, const double* wn, int ldn, double a, double b, const double* dt, double theta, double* out,
                               int ldo, double* rate, double* mw, bool rates_only, hipStream_t st)
{
    if (n <= 0 || k <= 0) return hipSuccess;
    unsigned blocks = 0;
    if (!fluid_column_grid(n, k, &blocks)) return hipErrorInvalidConfiguration;
    if (!rates_only && (out == w || !out || !mw || !w || !wn || !dt)) return hipErrorInvalidValue;
    if (rates_only)
        hipLaunchKernelGGL(k_fluid_advect<true>, dim3(blocks), dim3(FLUID_THREADS), 0, st, n, k, F, m_ptr, m_idx, m, psi, ldp, w, ldw, wn, ldn, a, b, dt,
                           theta, out, ldo, rate, mw);
    else
        hipLaunchKernelGGL(k_fluid_advect<false>, dim3(blocks), dim3(FLUID_THREADS), 0, st, n, k, F, m_ptr, m_idx, m, psi, ldp, w, ldw, wn, ldn, a, b, dt,
                           theta, out, ldo, rate, mw);
    return hipGetLastError();
}

hipError_t launch_fluid_dt(int op, int k, int stages, double cfl, const double* rmax, double* dt, double* time, double* his_cfl, double* his_time,
                           hipStream_t st)
{
    if (k <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_fluid_dt, dim3(1), dim3(FLUID_THREADS), 0, st, op, k, stages, cfl, rmax, dt, time, his_cfl, his_time);
    return hipGetLastError();
}

hipError_t launch_fluid_velocity(int nF, int k, const int* F, const double* W, const double* nrm, const double* Af, const double* psi, int ldp, double* U,
                                 double* terms, hipStream_t st)
{
    if (nF <= 0 || k <= 0) return hipSuccess;
    unsigned blocks = 0;
    if (!fluid_column_grid(nF, k, &blocks)) return hipErrorInvalidConfiguration;
    hipLaunchKernelGGL(k_fluid_velocity, dim3(blocks), dim3(FLUID_THREADS), 0, st, nF, k, F, W, nrm, Af, psi, ldp, U, terms);
    return hipGetLastError();
}

hipError_t launch_fluid_diag(int n, int k, const double* m, const double* w, int ldw, double* mw, double* ew, hipStream_t st)
{
    if (n <= 0 || k <= 0) return hipSuccess;
    unsigned blocks = 0;
    if (!fluid_column_grid(n, k, &blocks)) return hipErrorInvalidConfiguration;
    hipLaunchKernelGGL(k_fluid_diag, dim3(blocks), dim3(FLUID_THREADS), 0, st, n, k, m, w, ldw, mw, ew);
    return hipGetLastError();
}

}  // namespace smg
