// smg_krylov_device.hip -- the vector work of the V-cycle-preconditioned conjugate gradient solve (smg_solve_pcg, include/smg.h; host side in
// smg_cycle.cpp).  Everything works on the solve's internal blocks: row-major n x k, column c of row i at i * k + c (block hierarchies: n = 3 n_vert
// scalar rows, the DOFs 3v + d in order -- the same flat layout).  Every column runs its own recurrence; its scalars live in KryDev::s.
//
// Reductions are deterministic: a launch over fixed row chunks leaves one partial sum per (chunk, column) -- inside a chunk the rows are split over
// a fixed set of threads and combined by a fixed tree -- and a one-block finalize adds the chunks of a column in a fixed order (a fixed shuffle
// tree over fixed lane shares).  The number of chunks is a function of (n, k) alone: two runs give the same bits.
// Every kernel returns at once when the control block says the loop has ended (Ctrl::done), like the kernels of the V-cycle.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "smg_device.hpp"
#include "smg_device_inl.hpp"

namespace smg {

constexpr int KRY_THREADS = 256;        // reduction launches: one block per (row chunk, group of up to 64 columns)
constexpr int KRY_COLS = 64;
constexpr int KRY_FIN_WAVES = 16;       // finalize: one block, a wave per column (columns w, w + 16, ...)

// the thread layout of a reduction launch: tc = column inside the group, ty = row lane; R rows per pass
struct KryLayout {
    int ct, R, tc, ty, c;
    __device__ KryLayout(int k)
    {
        ct = k < KRY_COLS ? k : KRY_COLS;
        R = KRY_THREADS / ct;
        tc = (int)threadIdx.x % ct;
        ty = (int)threadIdx.x / ct;
        c = (int)blockIdx.y * KRY_COLS + tc;
    }
    __device__ bool active(int k) const { return ty < R && c < k; }
};

// red[ty * ct + tc] over ty = 0 .. R-1 into red[tc]: a fixed halving tree (R need not be a power of two)
__device__ __forceinline__ void kry_tree(double* red, const KryLayout& L)
{
    __syncthreads();
    for (int span = L.R; span > 1;) {
        const int half = (span + 1) >> 1;
        if (L.ty < span - half) red[threadIdx.x] += red[threadIdx.x + half * L.ct];
        __syncthreads();
        span = half;
    }
}

// MODE 0: part[0] = sum_i z_ic r_ic, part[1] = sum_i z_ic q_ic       (a = z, b = r, d = q)
// MODE 1: part[0] = sum_i p_ic q_ic                                    (a = p, d = q)
// MODE 2: x_ic += alpha_c p_ic, r_ic -= alpha_c q_ic, part[0] = sum_i r_ic^2 of the new r   (a = p, b = r, d = q, x)
// part layout: part[(s * groups + g) * k + c]
template <int MODE>
__global__ __launch_bounds__(KRY_THREADS) void k_kry_dots(const double* __restrict__ a, double* b, const double* __restrict__ d, double* x, const double* __restrict__ s,
                                                          double* __restrict__ part, int n, int k, int groups, const int* done)
{
    if (load_flag(done)) return;
    __shared__ double red0[KRY_THREADS];
    __shared__ double red1[MODE == 0 ? KRY_THREADS : 1];
    const KryLayout L(k);
    const int g = blockIdx.x, rpc = (n + groups - 1) / groups;
    const int r0 = g * rpc, r1 = min(n, r0 + rpc);
    double acc0 = 0.0, acc1 = 0.0;
    if (L.active(k)) {
        const double alpha = MODE == 2 ? s[KS_ALPHA * k + L.c] : 0.0;
        for (int r = r0 + L.ty; r < r1; r += L.R) {
            const size_t e = (size_t)r * k + L.c;
            if (MODE == 0) {
                const double z = a[e];
                acc0 += z * b[e];
                acc1 += z * d[e];
            } else if (MODE == 1) {
                acc0 += a[e] * d[e];
            } else {
                const double pe = a[e];
                x[e] = x[e] + alpha * pe;
                const double rn = b[e] - alpha * d[e];
                b[e] = rn;
                acc0 += rn * rn;
            }
        }
    }
    red0[threadIdx.x] = acc0;
    if (MODE == 0) red1[threadIdx.x] = acc1;
    kry_tree(red0, L);
    if (MODE == 0) kry_tree(red1, L);
    if (L.ty == 0 && L.c < k) {
        part[(size_t)g * k + L.c] = red0[threadIdx.x];
        if (MODE == 0) part[((size_t)groups + g) * k + L.c] = red1[threadIdx.x];
    }
}

// the sum over the chunks of column c of partial sum `sidx`, in the calling wave (fixed lane shares, fixed shuffle tree); valid in lane 0
__device__ __forceinline__ double kry_column_sum(const double* part, int sidx, int groups, int k, int c)
{
    const int lane = threadIdx.x & 63;
    double v = 0.0;
    for (int g = lane; g < groups; g += 64) v += part[((size_t)sidx * groups + g) * k + c];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

// MODE 0: rz_c, beta_c = -alpha_prev_c (z.q_prev)_c / rz_prev_c (0 after a restart, or when rz_prev_c == 0); clears the restart flag
// MODE 1: alpha_c = rz_c / (p.q)_c (0 when (p.q)_c == 0), rz_prev_c = rz_c
// MODE 2: rr_c; then |r|_F^2 = sum_c rr_c in column order -> the history and the break test (decide_body)
template <int MODE>
__global__ __launch_bounds__(64 * KRY_FIN_WAVES) void k_kry_finalize(const double* __restrict__ part, int groups, int k, double* s, int* restart, Ctrl* ctrl)
{
    if (ctrl->done) return;
    __shared__ double colsum[MODE == 2 ? 1024 : 1];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int rs = MODE == 0 ? *restart : 0;
    double local = 0.0;   // MODE 2, k > 1024 columns: this wave's share, combined below in wave order
    for (int c = w; c < k; c += KRY_FIN_WAVES) {
        const double s0 = kry_column_sum(part, 0, groups, k, c);
        if (MODE == 0) {
            const double s1 = kry_column_sum(part, 1, groups, k, c);
            if (lane == 0) {
                const double rz_prev = s[KS_RZ_PREV * k + c], alpha_prev = s[KS_ALPHA * k + c];
                s[KS_RZ * k + c] = s0;
                s[KS_BETA * k + c] = (rs || rz_prev == 0.0) ? 0.0 : -alpha_prev * s1 / rz_prev;
            }
        } else if (MODE == 1) {
            if (lane == 0) {
                const double rz = s[KS_RZ * k + c];
                s[KS_ALPHA * k + c] = s0 == 0.0 ? 0.0 : rz / s0;
                s[KS_RZ_PREV * k + c] = rz;
            }
        } else if (lane == 0) {
            if (k <= 1024) colsum[c] = s0;
            else local += s0;
        }
    }
    if (MODE == 0) {
        __syncthreads();
        if (threadIdx.x == 0) *restart = 0;
    }
    if (MODE == 2) {
        __shared__ double wsum[KRY_FIN_WAVES];
        if (lane == 0) wsum[w] = local;
        __syncthreads();
        if (threadIdx.x == 0) {
            double ss = 0.0;
            if (k <= 1024) { for (int c = 0; c < k; c++) ss += colsum[c]; }
            else { for (int q = 0; q < KRY_FIN_WAVES; q++) ss += wsum[q]; }
            ctrl->sumsq = ss;
            decide_body(ctrl, ss);
        }
    }
}

// p = z + beta_c p  (p = z where beta_c == 0: a first or restarted direction never reads the old one)
__global__ void k_kry_direction(const double* __restrict__ z, double* p, const double* __restrict__ s, size_t cnt, int k, const int* done)
{
    if (load_flag(done)) return;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= cnt) return;
    const double beta = s[KS_BETA * k + (int)(i % (size_t)k)];
    p[i] = beta == 0.0 ? z[i] : z[i] + beta * p[i];
}

// the preconditioner's input: b0 = r, u0 = 0 (fp64 V-cycle from a zero guess)
__global__ void k_kry_precond_in(const double* __restrict__ r, double* b0, double* u0, size_t cnt, const int* done)
{
    if (load_flag(done)) return;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < cnt) { b0[i] = r[i]; u0[i] = 0.0; }
}

// z = (double) e32: the result of the fp32 V-cycle
__global__ void k_kry_widen(const float* __restrict__ e, double* z, size_t cnt, const int* done)
{
    if (load_flag(done)) return;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < cnt) z[i] = (double)e[i];
}

__global__ void k_kry_arm(Ctrl* ctrl, int* restart, int reopen)
{
    if (reopen) { ctrl->done = 0; ctrl->n_his -= 1; }
    *restart = 1;
}

int kry_groups(int n, int k)
{
    const int ct = k < KRY_COLS ? k : KRY_COLS, R = KRY_THREADS / ct;
    const long want = ((long)n + (long)R * 8 - 1) / ((long)R * 8);     // at least 8 rows per thread
    return (int)std::max(1L, std::min(want, (long)KRY_MAX_GROUPS));
}

static dim3 kry_grid(const KryDev& K) { return dim3((unsigned)K.groups, (unsigned)((K.k + KRY_COLS - 1) / KRY_COLS)); }
static unsigned flat_blocks(size_t cnt) { return (unsigned)((cnt + 255) / 256); }

hipError_t launch_kry_dots_zr_zq(const KryDev& K, const double* z, const double* r, const double* q, const Ctrl* ctrl, hipStream_t st)
{
    hipLaunchKernelGGL(k_kry_dots<0>, kry_grid(K), dim3(KRY_THREADS), 0, st, z, const_cast<double*>(r), q, nullptr, K.s, K.part, K.n, K.k, K.groups, &ctrl->done);
    hipLaunchKernelGGL(k_kry_finalize<0>, dim3(1), dim3(64 * KRY_FIN_WAVES), 0, st, K.part, K.groups, K.k, K.s, K.restart, const_cast<Ctrl*>(ctrl));
    return hipGetLastError();
}

hipError_t launch_kry_direction(const KryDev& K, const double* z, double* p, const Ctrl* ctrl, hipStream_t st)
{
    const size_t cnt = (size_t)K.n * K.k;
    if (cnt == 0) return hipSuccess;
    hipLaunchKernelGGL(k_kry_direction, dim3(flat_blocks(cnt)), dim3(256), 0, st, z, p, K.s, cnt, K.k, &ctrl->done);
    return hipGetLastError();
}

hipError_t launch_kry_dots_pq(const KryDev& K, const double* p, const double* q, const Ctrl* ctrl, hipStream_t st)
{
    hipLaunchKernelGGL(k_kry_dots<1>, kry_grid(K), dim3(KRY_THREADS), 0, st, p, nullptr, q, nullptr, K.s, K.part, K.n, K.k, K.groups, &ctrl->done);
    hipLaunchKernelGGL(k_kry_finalize<1>, dim3(1), dim3(64 * KRY_FIN_WAVES), 0, st, K.part, K.groups, K.k, K.s, K.restart, const_cast<Ctrl*>(ctrl));
    return hipGetLastError();
}

hipError_t launch_kry_step_decide(const KryDev& K, double* x, double* r, const double* p, const double* q, Ctrl* ctrl, hipStream_t st)
{
    hipLaunchKernelGGL(k_kry_dots<2>, kry_grid(K), dim3(KRY_THREADS), 0, st, p, r, q, x, K.s, K.part, K.n, K.k, K.groups, &ctrl->done);
    hipLaunchKernelGGL(k_kry_finalize<2>, dim3(1), dim3(64 * KRY_FIN_WAVES), 0, st, K.part, K.groups, K.k, K.s, K.restart, ctrl);
    return hipGetLastError();
}

hipError_t launch_kry_precond_in(const double* r, double* b0, double* u0, size_t cnt, const Ctrl* ctrl, hipStream_t st)
{
    if (cnt == 0) return hipSuccess;
    hipLaunchKernelGGL(k_kry_precond_in, dim3(flat_blocks(cnt)), dim3(256), 0, st, r, b0, u0, cnt, &ctrl->done);
    return hipGetLastError();
}

hipError_t launch_kry_widen(const float* e, double* z, size_t cnt, const Ctrl* ctrl, hipStream_t st)
{
    if (cnt == 0) return hipSuccess;
    hipLaunchKernelGGL(k_kry_widen, dim3(flat_blocks(cnt)), dim3(256), 0, st, e, z, cnt, &ctrl->done);
    return hipGetLastError();
}

hipError_t launch_kry_arm(const KryDev& K, Ctrl* ctrl, bool reopen, hipStream_t st)
{
    hipLaunchKernelGGL(k_kry_arm, dim3(1), dim3(1), 0, st, ctrl, K.restart, reopen ? 1 : 0);
    return hipGetLastError();
}

}  // namespace smg
