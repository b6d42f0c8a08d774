// smg_wave_grid.hpp -- the launch shapes the wave object's three kernel files share (smg_wave_device.hip, smg_wave_adjoint_device.hip,
// smg_wave_born_device.hip): one WAVEFRONT
// per (64 consecutive vertices, column) for the vertex kernels, one lane per (list entry, column) for the list kernels.  Device code only.
#pragma once
#include <hip/hip_runtime.h>

namespace smg {

constexpr int WAVE_THREADS = 256, WAVE_LANES = 64, WAVE_WAVES = WAVE_THREADS / WAVE_LANES;

// the blocks of a (64 vertices, column) wave grid; false: it does not fit a grid dimension
inline bool wave_grid(int rows, int k, unsigned* blocks)
{
    const long long waves = (((long long)rows + WAVE_LANES - 1) / WAVE_LANES) * k;
    const long long b = (waves + WAVE_WAVES - 1) / WAVE_WAVES;
    *blocks = (unsigned)b;
    return b <= 0x7fffffffLL;
}

// the wave's column and the lane's vertex; false: the wave is past the grid's last one or the lane past the last vertex
__device__ __forceinline__ bool wave_lane(int n, int k, int* c, int* v)
{
    const int W = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * WAVE_WAVES + (threadIdx.x / WAVE_LANES)));
    const int waves = ((n + WAVE_LANES - 1) / WAVE_LANES) * k;   // wave_grid has checked the range
    if (W >= waves) return false;
    *c = W % k;
    *v = (W / k) * WAVE_LANES + (int)(threadIdx.x % WAVE_LANES);
    return *v < n;
}

// the blocks of one lane per (list entry, column); the launchers have checked that count * k fits an int
inline unsigned list_grid(int count, int k) { return (unsigned)(((long long)count * k + WAVE_THREADS - 1) / WAVE_THREADS); }

// the lane's (list entry, column) of such a grid, in 32-bit arithmetic; false: the lane is past the last one
__device__ __forceinline__ bool list_lane(unsigned total, unsigned k, unsigned* t, int* j, int* c)
{
    *t = blockIdx.x * WAVE_THREADS + threadIdx.x;
    if (*t >= total) return false;
    *j = (int)(*t / k);
    *c = (int)(*t % k);
    return true;
}

}  // namespace smg
