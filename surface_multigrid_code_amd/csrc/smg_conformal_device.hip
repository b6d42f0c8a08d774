// smg_conformal_device.hip -- the kernels of the discrete conformal metric (smg_conformal_*, include/smg.h; host side in smg_conformal.cpp; the
// arithmetic in smg_conformal_inl.hpp).
//
// Layout: u, s, the angle sums and g are vectors of nV; angles, half cotangents, rest and current lengths are nF x 3 in corner order (index
// 3 f + c, the index the corner lists and the assembly recipe carry); the broken flags are a plane of nF doubles (1.0 / 0.0) so that their
// count is a launch_fixed_sum.
//
// Determinism: no atomics.  A vertex's angle sum is one lane's sequential loop over its corner list (faces ascending); an entry of -L~ is one
// lane's loop over the entry's terms in cotmatrix()'s order; the three reductions of an evaluation (sum g^2, max |g|, the broken count) go
// through launch_fixed_sum / launch_fixed_max.  Expressions are written operation by operation (-ffp-contract=off): tests/conformal_np.py
// restates them in numpy in the same order.  exp occurs once per vertex, atan2 three times per face; everything else is +, -, *, / and sqrt.
#include <hip/hip_runtime.h>

#include "smg_conformal_inl.hpp"
#include "smg_device.hpp"

namespace smg {

namespace {

constexpr int CONFORMAL_THREADS = 256;

inline int conformal_grid(int n) { return (n + CONFORMAL_THREADS - 1) / CONFORMAL_THREADS; }

}  // namespace

// One lane per vertex: ut = u + t d (d == nullptr: u) and s = exp(-ut / 2).  A trial of the line search needs no axpy of its own.
__global__ __launch_bounds__(CONFORMAL_THREADS) void k_conformal_scale(int n, const double* __restrict__ u, const double* __restrict__ d, double t,
                                                                       double* __restrict__ ut, double* __restrict__ s)
{
    const int i = blockIdx.x * CONFORMAL_THREADS + threadIdx.x;
    if (i >= n) return;
    const double x = conformal_trial(u, d, t, (size_t)i);
    ut[i] = x;
    s[i] = conformal_scale(x);
}

// One lane per face: reads F, l0, the rest area and three scales; writes 3 angles, 3 half cotangents and the broken flag.
__global__ __launch_bounds__(CONFORMAL_THREADS) void k_conformal_faces(int nF, const int* __restrict__ F, const double* __restrict__ l0,
                                                                       const double* __restrict__ area2, const double* __restrict__ s, double* __restrict__ ang,
                                                                       double* __restrict__ hc, double* __restrict__ broken)
{
    const int f = blockIdx.x * CONFORMAL_THREADS + threadIdx.x;
    if (f >= nF) return;
    double a[3], h[3];
    broken[f] = conformal_face_at(F, l0, area2, s, (size_t)f, a, h);
#pragma unroll
    for (int c = 0; c < 3; c++) {
        ang[3 * (size_t)f + c] = a[c];
        hc[3 * (size_t)f + c] = h[c];
    }
}

// One lane per face: the current lengths l~ = l0 / (s_j s_k) in corner order.
__global__ __launch_bounds__(CONFORMAL_THREADS) void k_conformal_lengths(int nF, const int* __restrict__ F, const double* __restrict__ l0,
                                                                         const double* __restrict__ s, double* __restrict__ lt)
{
    const int f = blockIdx.x * CONFORMAL_THREADS + threadIdx.x;
    if (f >= nF) return;
    double l[3];
    conformal_lengths_at(F, l0, s, (size_t)f, l);
#pragma unroll
    for (int c = 0; c < 3; c++) lt[3 * (size_t)f + c] = l[c];
}

// One lane per vertex: the angle sum, g (0 on a fixed row), the terms g^2 and |g|; WITH_VALUES: the row's values of -L~ as well.
template <bool WITH_VALUES>
__global__ __launch_bounds__(CONFORMAL_THREADS) void k_conformal_rows(int n, const double* __restrict__ ang, const double* __restrict__ hc,
                                                                      const int* __restrict__ m_ptr, const int* __restrict__ m_idx,
                                                                      const double* __restrict__ Theta, const int* __restrict__ fixed,
                                                                      const int* __restrict__ rowptr, const int* __restrict__ l_ptr,
                                                                      const int* __restrict__ l_idx, const signed char* __restrict__ l_sgn,
                                                                      double* __restrict__ sum, double* __restrict__ g, double* __restrict__ gsq,
                                                                      double* __restrict__ gabs, double* __restrict__ val)
{
    const int v = blockIdx.x * CONFORMAL_THREADS + threadIdx.x;
    if (v >= n) return;
    const double a = conformal_angle_sum(ang, m_ptr, m_idx, v);
    const double gv = fixed[v] ? 0.0 : a - Theta[v];
    sum[v] = a;
    g[v] = gv;
    gsq[v] = gv * gv;
    gabs[v] = fabs(gv);
    if (WITH_VALUES) {
        const int e1 = rowptr[v + 1];
        for (int e = rowptr[v]; e < e1; e++) val[e] = conformal_entry(hc, l_ptr, l_idx, l_sgn, e);
    }
}

// u[fixed[i]] = values[i] (values == nullptr: 0)
__global__ __launch_bounds__(CONFORMAL_THREADS) void k_conformal_fix(int nf, const int* __restrict__ list, const double* __restrict__ values,
                                                                     double* __restrict__ u)
{
    const int i = blockIdx.x * CONFORMAL_THREADS + threadIdx.x;
    if (i >= nf) return;
    u[list[i]] = values ? values[i] : 0.0;
}

hipError_t launch_conformal_scale(int n, const double* u, const double* d, double t, double* ut, double* s, hipStream_t st)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_conformal_scale, dim3(conformal_grid(n)), dim3(CONFORMAL_THREADS), 0, st, n, u, d, t, ut, s);
    return hipGetLastError();
}

hipError_t launch_conformal_faces(int nF, const int* F, const double* l0, const double* area2, const double* s, double* ang, double* hc, double* broken,
                                  hipStream_t st)
{
    if (nF <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_conformal_faces, dim3(conformal_grid(nF)), dim3(CONFORMAL_THREADS), 0, st, nF, F, l0, area2, s, ang, hc, broken);
    return hipGetLastError();
}

hipError_t launch_conformal_lengths(int nF, const int* F, const double* l0, const double* s, double* lt, hipStream_t st)
{
    if (nF <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_conformal_lengths, dim3(conformal_grid(nF)), dim3(CONFORMAL_THREADS), 0, st, nF, F, l0, s, lt);
    return hipGetLastError();
}

hipError_t launch_conformal_rows(int n, int nF, const double* ang, const double* hc, const double* broken, const int* m_ptr, const int* m_idx,
                                 const double* Theta, const int* fixed, const int* rowptr, const int* l_ptr, const int* l_idx, const signed char* l_sgn,
                                 double* sum, double* g, double* gsq, double* gabs, double* val, double* part, double* red, hipStream_t st)
{
    if (n <= 0) return hipSuccess;
    if (val)
        hipLaunchKernelGGL(k_conformal_rows<true>, dim3(conformal_grid(n)), dim3(CONFORMAL_THREADS), 0, st, n, ang, hc, m_ptr, m_idx, Theta, fixed, rowptr,
                           l_ptr, l_idx, l_sgn, sum, g, gsq, gabs, val);
    else
        hipLaunchKernelGGL(k_conformal_rows<false>, dim3(conformal_grid(n)), dim3(CONFORMAL_THREADS), 0, st, n, ang, hc, m_ptr, m_idx, Theta, fixed, rowptr,
                           l_ptr, l_idx, l_sgn, sum, g, gsq, gabs, val);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || !red) return e;
    if ((e = launch_fixed_sum(gsq, n, part, red, st)) != hipSuccess) return e;
    if ((e = launch_fixed_max(gabs, n, part, red + 1, st)) != hipSuccess) return e;
    return launch_fixed_sum(broken, nF, part, red + 2, st);
}

hipError_t launch_conformal_fix(int nf, const int* list, const double* values, double* u, hipStream_t st)
{
    if (nf <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_conformal_fix, dim3(conformal_grid(nf)), dim3(CONFORMAL_THREADS), 0, st, nf, list, values, u);
    return hipGetLastError();
}

}  // namespace smg
