// smg_fixed_sum_device.hip -- the sum of n doubles in an order that depends on n alone: the ARAP energy (smg_arap.cpp), the membrane's
// objective and its b . dx (smg_membrane.cpp), the parameterization's energy and distortion statistics (smg_param.cpp); and the maximum of n
// doubles through a tree of the same shape (launch_fixed_max).  No atomics: the terms are summed over fixed row chunks by a fixed tree and the chunks by one
// wave in a fixed order (the scheme of smg_krylov_device.hip), so every run returns the same bits; tests/test_arap_host.py and
// tests/test_membrane_host.py restate the order in numpy.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "smg_device.hpp"

namespace smg {

namespace {
constexpr int SUM_THREADS = 256;
constexpr int SUM_MAX_GROUPS = 1024;

// the two combiners of the tree: MAX == false a + b, MAX == true the larger of the two (a NaN loses against a number)
template <bool MAX>
__device__ __forceinline__ double fixed_identity() { return MAX ? -HUGE_VAL : 0.0; }
template <bool MAX>
__device__ __forceinline__ double fixed_combine(double a, double b) { return MAX ? fmax(a, b) : a + b; }
}  // namespace

// part[g] = the sum of term over row chunk g: rows split over the block's threads with a fixed stride, combined by a fixed halving tree
template <bool MAX>
__global__ __launch_bounds__(SUM_THREADS) void k_fixed_sum_part(const double* __restrict__ term, int n, int groups, double* __restrict__ part)
{
    __shared__ double red[SUM_THREADS];
    const int g = blockIdx.x, rpc = (n + groups - 1) / groups;
    const int r0 = g * rpc, r1 = min(n, r0 + rpc);
    double acc = fixed_identity<MAX>();
    for (int r = r0 + (int)threadIdx.x; r < r1; r += SUM_THREADS) acc = fixed_combine<MAX>(acc, term[r]);
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int half = SUM_THREADS / 2; half > 0; half >>= 1) {
        if ((int)threadIdx.x < half) red[threadIdx.x] = fixed_combine<MAX>(red[threadIdx.x], red[threadIdx.x + half]);
        __syncthreads();
    }
    if (threadIdx.x == 0) part[g] = red[0];
}

// *sum = the sum of the chunks: fixed lane shares, fixed shuffle tree (one wave)
template <bool MAX>
__global__ __launch_bounds__(64) void k_fixed_sum_final(const double* __restrict__ part, int groups, double* __restrict__ sum)
{
    double v = fixed_identity<MAX>();
    for (int g = threadIdx.x; g < groups; g += 64) v = fixed_combine<MAX>(v, part[g]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fixed_combine<MAX>(v, __shfl_down(v, o, 64));
    if (threadIdx.x == 0) *sum = v;
}

int fixed_sum_groups(int n)
{
    const long want = ((long)n + (long)SUM_THREADS * 8 - 1) / ((long)SUM_THREADS * 8);     // at least 8 rows per thread
    return (int)std::max(1L, std::min(want, (long)SUM_MAX_GROUPS));
}

hipError_t launch_fixed_sum(const double* term, int n, double* part, double* sum, hipStream_t st)
{
    if (n <= 0) return hipSuccess;
    const int groups = fixed_sum_groups(n);
    hipLaunchKernelGGL(k_fixed_sum_part<false>, dim3(groups), dim3(SUM_THREADS), 0, st, term, n, groups, part);
    hipLaunchKernelGGL(k_fixed_sum_final<false>, dim3(1), dim3(64), 0, st, part, groups, sum);
    return hipGetLastError();
}

hipError_t launch_fixed_max(const double* term, int n, double* part, double* out, hipStream_t st)
{
    if (n <= 0) return hipSuccess;
    const int groups = fixed_sum_groups(n);
    hipLaunchKernelGGL(k_fixed_sum_part<true>, dim3(groups), dim3(SUM_THREADS), 0, st, term, n, groups, part);
    hipLaunchKernelGGL(k_fixed_sum_final<true>, dim3(1), dim3(64), 0, st, part, groups, out);
    return hipGetLastError();
}

}  // namespace smg
