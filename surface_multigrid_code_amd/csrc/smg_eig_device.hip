// smg_eig_device.hip -- the block work of the LOBPCG eigensolver (smg_eigs, include/smg.h; host side in smg_eig.cpp): Gram products of the
// basis S = [X W P], its recombination S C, and the residual with its norms.  Everything works on the solve's internal blocks: row-major n x m,
// column c of row i at i * m + c (block hierarchies: n = 3 n_vert scalar rows, the same flat layout).
//
// Reductions are deterministic: a launch over fixed row chunks (eig_groups(n), a function of n alone) leaves one partial per chunk, and a
// finalize adds the chunks in chunk order.  Inside a chunk the rows are visited in a fixed order by a fixed thread.  Two runs give the same bits.
// Every kernel returns at once when the control block says the loop has ended (Ctrl::done), like the kernels of the V-cycle.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "smg_device.hpp"
#include "smg_device_inl.hpp"

namespace smg {

constexpr int EIG_THREADS = 256;
constexpr int EIG_RB = 32;              // Gram: rows staged in LDS per pass
constexpr int EIG_TT = EIG_TILE * EIG_TILE;

// column i of the concatenated blocks, row r (column count m per block)
__device__ __forceinline__ const double* eig_col_ptr(const EigBlocks& B, int m, int i) { return B.p[i / m] + i % m; }

// the tile (ti, tj) behind work-group index t: row-major over ta x tb tiles, or over the tiles on and above the diagonal (sym)
__device__ __forceinline__ void eig_tile(int t, int ta, int tb, bool sym, int* ti, int* tj)
{
    if (!sym) { *ti = t / tb; *tj = t % tb; return; }
    int i = 0;
    while (t >= ta - i) { t -= ta - i; i++; }
    *ti = i; *tj = i + t;
}

// part[(t * groups + g) * EIG_TT + li * EIG_TILE + lj] = sum over the rows of chunk g of Sa[r][ti*64+li] w[r] Sb[r][tj*64+lj].
// Thread (pi, pj) = (tid % 16, tid / 16) owns the 4 x 4 entries li = pi + 16 p, lj = pj + 16 q; rows are visited in order.
__global__ __launch_bounds__(EIG_THREADS) void k_eig_gram(EigBlocks Sa, EigBlocks Sb, int n, int m, const double* __restrict__ w, int sym,
                                                          double* __restrict__ part, int groups, const int* done)
{
    if (load_flag(done)) return;
    __shared__ double sa[EIG_RB][EIG_TILE];
    __shared__ double sb[EIG_RB][EIG_TILE];
    const int a = Sa.nb * m, b = Sb.nb * m;
    const int ta = (a + EIG_TILE - 1) / EIG_TILE, tb = (b + EIG_TILE - 1) / EIG_TILE;
    int ti, tj;
    eig_tile((int)blockIdx.y, ta, tb, sym != 0, &ti, &tj);
    const int g = blockIdx.x, rpg = (n + groups - 1) / groups;
    const int r0 = g * rpg, r1 = min(n, r0 + rpg);
    const int tid = threadIdx.x;
    // staging: this thread always loads column cc of the tile, rows tid / 64 + 4 i of a pass
    const int cc = tid % EIG_TILE, rr0 = tid / EIG_TILE;
    const int ca = ti * EIG_TILE + cc, cb = tj * EIG_TILE + cc;
    const double* pa = ca < a ? eig_col_ptr(Sa, m, ca) : nullptr;
    const double* pb = cb < b ? eig_col_ptr(Sb, m, cb) : nullptr;
    const int pi = tid % 16, pj = tid / 16;
    double acc[4][4];
#pragma unroll
    for (int p = 0; p < 4; p++)
#pragma unroll
        for (int q = 0; q < 4; q++) acc[p][q] = 0.0;
    for (int base = r0; base < r1; base += EIG_RB) {
#pragma unroll
        for (int i = 0; i < EIG_RB / 4; i++) {
            const int rr = rr0 + 4 * i, r = base + rr;
            const bool in = r < r1;
            double va = (in && pa) ? pa[(size_t)r * m] : 0.0;
            if (w && in) va *= w[r];
            sa[rr][cc] = va;
            sb[rr][cc] = (in && pb) ? pb[(size_t)r * m] : 0.0;
        }
        __syncthreads();
        const int nr = min(EIG_RB, r1 - base);
        for (int rr = 0; rr < nr; rr++) {
            double av[4], bv[4];
#pragma unroll
            for (int p = 0; p < 4; p++) { av[p] = sa[rr][pi + 16 * p]; bv[p] = sb[rr][pj + 16 * p]; }
#pragma unroll
            for (int p = 0; p < 4; p++)
#pragma unroll
                for (int q = 0; q < 4; q++) acc[p][q] = fma(av[p], bv[q], acc[p][q]);
        }
        __syncthreads();
    }
    double* out = part + ((size_t)blockIdx.y * groups + g) * EIG_TT;
#pragma unroll
    for (int p = 0; p < 4; p++)
#pragma unroll
        for (int q = 0; q < 4; q++) out[(pi + 16 * p) * EIG_TILE + pj + 16 * q] = acc[p][q];
}

// one thread per entry of a tile: the chunks in order; sym: the mirror entry too.  A diagonal tile of the sym form keeps its lower triangle and
// mirrors it (its two triangles differ in rounding: fl(w s_i) s_j against fl(w s_j) s_i), so G comes out exactly symmetric.
__global__ __launch_bounds__(EIG_THREADS) void k_eig_gram_finalize(const double* __restrict__ part, int groups, int a, int b, int ta, int tb, int sym,
                                                                   double* __restrict__ G, const int* done)
{
    if (load_flag(done)) return;
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int t = (int)(e / EIG_TT), l = (int)(e % EIG_TT);
    int ti, tj;
    eig_tile(t, ta, tb, sym != 0, &ti, &tj);
    const int li = l / EIG_TILE, lj = l % EIG_TILE;
    const int i = ti * EIG_TILE + li, j = tj * EIG_TILE + lj;
    if (i >= a || j >= b || (sym && ti == tj && li < lj)) return;
    double s = 0.0;
    for (int g = 0; g < groups; g++) s += part[((size_t)t * groups + g) * EIG_TT + l];
    G[(size_t)i * b + j] = s;
    if (sym && i != j) G[(size_t)j * b + i] = s;
}

// X = S Cx, AX = AS Cx, and P = S' Cp, AP = AS' Cp (blocks 1.. only).  Work-group: rpb rows x jc output columns (jc = min(m, 16)); blockIdx.y
// selects the column chunk, whose coefficients sit in LDS.  Sums run over the columns of S in order.
__global__ __launch_bounds__(EIG_THREADS) void k_eig_combine(EigBlocks S, EigBlocks AS, int n, int m, const double* __restrict__ C, double* __restrict__ X,
                                                             double* __restrict__ AX, double* __restrict__ P, double* __restrict__ AP, const int* done)
{
    if (load_flag(done)) return;
    extern __shared__ double coef[];      // [q][2 jc]: Cx, then Cp
    const int q = S.nb * m, jc = min(m, 16), rpb = EIG_THREADS / jc;
    const int j0 = blockIdx.y * jc;
    for (int e = threadIdx.x; e < q * 2 * jc; e += EIG_THREADS) {
        const int i = e / (2 * jc), l = e % (2 * jc);
        const int j = j0 + (l < jc ? l : l - jc);
        coef[e] = j < m ? C[(size_t)i * 2 * m + (l < jc ? j : m + j)] : 0.0;
    }
    __syncthreads();
    const int jl = threadIdx.x % jc, rl = threadIdx.x / jc;
    const int row = blockIdx.x * rpb + rl, j = j0 + jl;
    if (rl >= rpb || row >= n || j >= m) return;
    double x = 0.0, ax = 0.0, p = 0.0, ap = 0.0;
    for (int bk = 0; bk < S.nb; bk++) {
        const double* sp = S.p[bk] + (size_t)row * m;
        const double* asp = AS.p[bk] + (size_t)row * m;
        for (int c = 0; c < m; c++) {
            const int i = bk * m + c;
            const double s = sp[c], as = asp[c];
            const double cx = coef[i * 2 * jc + jl];
            x = fma(s, cx, x);
            ax = fma(as, cx, ax);
            if (bk > 0) {
                const double cp = coef[i * 2 * jc + jc + jl];
                p = fma(s, cp, p);
                ap = fma(as, cp, ap);
            }
        }
    }
    const size_t o = (size_t)row * m + j;
    X[o] = x;
    AX[o] = ax;
    if (P) { P[o] = p; AP[o] = ap; }
}

// R = AX - mass X lam, the preconditioner's input, and part[g * m + c] = sum over chunk g of r_ic^2 / mass_i.  Thread layout as the Krylov
// reductions: tc = column, ty = row lane (rl = 256 / m rows per pass), then a fixed halving tree over the row lanes.
__global__ __launch_bounds__(EIG_THREADS) void k_eig_residual(const double* __restrict__ X, const double* __restrict__ AX, const double* __restrict__ mass,
                                                              const double* __restrict__ lam, int n, int m, double* __restrict__ b0, double* __restrict__ u0,
                                                              float* __restrict__ b32, float* __restrict__ u32, double* __restrict__ part, int groups,
                                                              const int* done)
{
    if (load_flag(done)) return;
    __shared__ double red[EIG_THREADS];
    const int R = EIG_THREADS / m, tc = threadIdx.x % m, ty = threadIdx.x / m;
    const int g = blockIdx.x, rpg = (n + groups - 1) / groups;
    const int r0 = g * rpg, r1 = min(n, r0 + rpg);
    double acc = 0.0;
    if (ty < R) {
        const double l = lam[tc];
        for (int r = r0 + ty; r < r1; r += R) {
            const size_t e = (size_t)r * m + tc;
            const double mi = mass[r];
            const double res = AX[e] - mi * X[e] * l;
            if (b32) { b32[e] = (float)res; u32[e] = 0.0f; }
            else { b0[e] = res; u0[e] = 0.0; }
            acc += res * res / mi;
        }
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int span = R; span > 1;) {
        const int half = (span + 1) >> 1;
        if (ty < span - half) red[threadIdx.x] += red[threadIdx.x + half * m];
        __syncthreads();
        span = half;
    }
    if (ty == 0) part[(size_t)g * m + tc] = red[threadIdx.x];
}

__global__ void k_eig_residual_finalize(const double* __restrict__ part, int groups, int m, const double* __restrict__ lam, double* __restrict__ res,
                                        const int* done)
{
    if (load_flag(done)) return;
    const int c = threadIdx.x;
    if (c >= m) return;
    double s = 0.0;
    for (int g = 0; g < groups; g++) s += part[(size_t)g * m + c];
    res[c] = sqrt(s) / fabs(lam[c]);
}

int eig_groups(int n)
{
    const long want = ((long)n + 1023) / 1024;      // at least 1024 rows per chunk
    return (int)std::max(1L, std::min(want, (long)EIG_MAX_GROUPS));
}

static int eig_tiles(int a, int b, bool sym)
{
    const int ta = (a + EIG_TILE - 1) / EIG_TILE, tb = (b + EIG_TILE - 1) / EIG_TILE;
    return sym ? ta * (ta + 1) / 2 : ta * tb;
}

size_t eig_gram_part_size(int a, int b, int groups) { return (size_t)eig_tiles(a, b, false) * groups * EIG_TT; }

hipError_t launch_eig_gram(const EigBlocks& Sa, const EigBlocks& Sb, int n, int m, const double* w, bool sym, double* part, int groups,
                           double* G, const Ctrl* ctrl, hipStream_t st)
{
    const int a = Sa.nb * m, b = Sb.nb * m;
    const int tiles = eig_tiles(a, b, sym);
    const int ta = (a + EIG_TILE - 1) / EIG_TILE, tb = (b + EIG_TILE - 1) / EIG_TILE;
    hipLaunchKernelGGL(k_eig_gram, dim3((unsigned)groups, (unsigned)tiles), dim3(EIG_THREADS), 0, st, Sa, Sb, n, m, w, sym ? 1 : 0, part, groups,
                       &ctrl->done);
    const size_t entries = (size_t)tiles * EIG_TT;
    hipLaunchKernelGGL(k_eig_gram_finalize, dim3((unsigned)((entries + EIG_THREADS - 1) / EIG_THREADS)), dim3(EIG_THREADS), 0, st, part, groups, a, b,
                       ta, tb, sym ? 1 : 0, G, &ctrl->done);
    return hipGetLastError();
}

hipError_t launch_eig_combine(const EigBlocks& S, const EigBlocks& AS, int n, int m, const double* C, double* X, double* AX, double* P,
                              double* AP, const Ctrl* ctrl, hipStream_t st)
{
    if (n == 0) return hipSuccess;
    const int jc = std::min(m, 16), rpb = EIG_THREADS / jc;
    const size_t lds = (size_t)S.nb * m * 2 * jc * sizeof(double);
    hipLaunchKernelGGL(k_eig_combine, dim3((unsigned)((n + rpb - 1) / rpb), (unsigned)((m + jc - 1) / jc)), dim3(EIG_THREADS), lds, st, S, AS, n, m, C,
                       X, AX, P, AP, &ctrl->done);
    return hipGetLastError();
}

hipError_t launch_eig_residual(const double* X, const double* AX, const double* mass, const double* lam, int n, int m, double* b0, double* u0,
                               float* b32, float* u32, double* part, int groups, double* res, const Ctrl* ctrl, hipStream_t st)
{
    hipLaunchKernelGGL(k_eig_residual, dim3((unsigned)groups), dim3(EIG_THREADS), 0, st, X, AX, mass, lam, n, m, b0, u0, b32, u32, part, groups,
                       &ctrl->done);
    hipLaunchKernelGGL(k_eig_residual_finalize, dim3(1), dim3(64), 0, st, part, groups, m, lam, res, &ctrl->done);
    return hipGetLastError();
}

}  // namespace smg
