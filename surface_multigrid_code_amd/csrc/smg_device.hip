// smg_device.hip -- hand-written HIP kernels for gfx950 (MI355X, CDNA4, wave64).  See smg_device.hpp.
//
// Everything here is HBM/L2-bandwidth bound irregular fp64 work (arithmetic intensity ~0.13 FLOP/B): no MFMA.
// Design rules followed (cdna_hip_programming.md §2, §6 G2/G11/G13; MI355X_MICROARCH.md):
//   * SELL-64-sigma: one wavefront = one slice, one lane = one row; val/col panels are column-major so a
//     wave's load of panel column j is one contiguous 512 B (val) + 256 B (col) request;
//   * the panel loop is unrolled 8-wide with all index/value loads issued before the dependent x-gathers
//     so each wave keeps >= 8 x 768 B of matrix stream in flight;
//   * blockIdx -> slice mapping is XCD-aware: the 8 XCDs each walk one contiguous eighth of the slices so an
//     XCD's private 4 MiB L2 sees a compact window of x instead of the whole vector;
//   * per-row sums are accumulated sequentially in ascending column order with separate multiply and add
//     (build with -ffp-contract=off): bit-identical to the reference's Eigen CPU kernels.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <type_traits>

#include "smg_device.hpp"
#include "smg_device_inl.hpp"
#include "smg_gj_inl.hpp"

namespace smg {

// ---------------------------------------------------------------------------------------------- SELL kernels

__device__ int g_never_done = 0;
const int* never_done()
{
    static const int* p = nullptr;
    if (!p) { void* q = nullptr; if (hipGetSymbolAddress(&q, HIP_SYMBOL(g_never_done)) == hipSuccess) p = (const int*)q; }
    return p;
}


// what a restriction launch leaves in the coarse level's u (see FirstColour in smg_device.hpp)
// jacobi != 0: the coarse level is smoothed by damped Jacobi -- ALL its rows (n_first = n_rows) get what the first Jacobi sweep from
// u = 0 leaves there, 0 + omega * (rc_i / a_ii - 0).  omega doubles as the damping factor of a SELL_JACOBI launch.
// jacobi == 2: the coarse level is smoothed by Chebyshev-accelerated Jacobi: its first step from u = 0 is d = omega * (rc_i / a_ii - 0),
// u = 0 + d (omega = that step's coefficient), written to u and d.
// SELL_CHEBY launches use d (the step's update vector, own row in / out), c1 (coefficient of the old update; 0 on the first step: d is
// not read then) and omega (coefficient of the scaled residual).
// codes / tab: the matrix of the launch holds weight codes instead of values (SellDev::codes; k_sell takes it as a template argument,
// the other kernels test it at run time).
template <typename T> struct CoarseInit { T* u; const T* gs_val; const int* diag_slot; int n_first; int jacobi; T omega; T* d; T c1; int codes; T tab[4]; };
// the value behind a coded column word: tab[word & 3] as selects (an indexed read of the kernel-argument array would go through scratch)
template <typename T> __device__ __forceinline__ T code_val(const CoarseInit<T>& z, int cw)
{
    const T lo = (cw & 1) ? z.tab[1] : z.tab[0], hi = (cw & 1) ? z.tab[3] : z.tab[2];
    return (cw & 2) ? hi : lo;
}

// One wavefront per slice of 64 rows; lane l owns row row0 + l.
// T = double: the reference arithmetic.  T = float: the fp32 V-cycle of the mixed-precision mode (values, vectors and
// accumulation in fp32; SELL_RESID_SS is never instantiated for it: the outer residual stays fp64).
// Argument order: the first 16 dwords are what the wave needs to issue its first panel loads; built with
// -mllvm -amdgpu-kernarg-preload-count=16 they arrive in SGPRs with the wave instead of through scalar loads (that only works
// for leading scalar / pointer arguments, hence no struct up front).  The rest is fetched in one batch.
// W0C: the number of panel columns requested ahead, fixed at compile time (7: the one-ring of a regular mesh vertex plus the
// diagonal, by far the most common slice width of A) -- straight-line loads, no branch per column; -1: taken from a_w_lo.
// CODED (SELL_AX / SELL_ADD on transfer operators): no value stream, the column words carry a weight code (SellDev::codes); the values are
// decoded from z.tab when the columns arrive, and every sum runs as it does on the value array: the same bits.
template <int MODE, int KB, typename T, int W0C = -1, int WPB = 4, bool CODED = false>
__global__ __launch_bounds__(64 * WPB) void k_sell(const int* a_col, const T* a_val, const int* a_order, const int* a_slice_off, int a_stride,
                                              int a_w_lo, int s_begin, int s_end, int n_blocks, int use_order, const T* x,
                                              const int* a_slice_row, const int* a_slice_w, const T* b, T* y, int ld, const int* done,
                                              double* partials, CoarseInit<T> z)
{
    struct { const int *slice_row, *slice_off, *slice_w, *order, *col; int stride, w_lo; } A = {a_slice_row, a_slice_off, a_slice_w, a_order,
                                                                                               a_col, a_stride, a_w_lo};
    // The convergence flag is requested up front but only consulted right before the stores: the matrix / vector loads
    // of a launch must not wait for that round trip (a launch after convergence does the work and writes nothing).
    constexpr int C = 64;
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    constexpr int wpb = WPB;          // waves (= slices) per block
    // n_blocks < 0 (small colour sweeps only): the launch has 8x the workgroups and only those that land on XCD 0 work, so the
    // values one colour launch writes are still in that XCD's L2 when the next launch gathers them -- a small level's launch chain
    // is pure latency, and this takes the trip to the Infinity Cache out of it (tools/micro/xcd_local.hip: 3.6 -> 2.85 us per launch)
    constexpr bool GS = sell_is_gs(MODE), OOP = sell_is_oop(MODE), JAC = sell_is_jacobi(MODE), CHEB = sell_is_cheby(MODE), HEAD = sell_is_head(MODE);
    constexpr bool RES = sell_has_res(MODE);   // the last colour launch of a pre-smoothing: also stores the residual of its rows (into z.d)
    int bid;
    if (GS && n_blocks < 0) { if (blockIdx.x & 7) return; bid = blockIdx.x >> 3; }
    else bid = xcd_remap(blockIdx.x, n_blocks);
    const int ls = __builtin_amdgcn_readfirstlane(s_begin + bid * wpb + wave);
    double ss = 0.0;
    int stop = 0;
    if (ls < s_end) {
        const int s = (!GS && use_order) ? A.order[ls] : ls;   // colour sweeps never walk the region order
        // Fixed-stride matrices: the panel address comes from s alone, and the first W0 columns (what most slices have; a
        // narrower slice holds padding there) are requested before the slice's table entries have arrived -- the table reads
        // leave the critical path.
        const int W0 = W0C >= 0 ? W0C : (A.w_lo < 8 ? A.w_lo : 8);   // compile-time, or the kernel argument (0 for compact panels)
        const int off0 = (W0C >= 0 || A.stride) ? s * A.stride : A.slice_off[s];   // W0C >= 0: launched on fixed-pitch matrices only
        const int* cp = A.col + (size_t)off0 * C + lane;
        const T* vp = CODED ? nullptr : a_val + (size_t)off0 * C + lane;
        constexpr int U = W0C > 8 ? W0C : 8;   // W0C = 12: the whole pitch of the usual matrices in ONE batch (small launches only)
        int c0[U];
        T v0[U];
#pragma unroll
        for (int t = 0; t < U; t++) {
            // one wave-uniform branch per column, both loads behind it: as two selects this compiled to two branches per column
            // and the longer issue sequence cost 2.5 % of the V-cycle (every launch pays it before its loads are out)
            if (t < W0) { c0[t] = cp[(size_t)t * C]; v0[t] = CODED ? (T)0 : vp[(size_t)t * C]; }
            else { c0[t] = -1; v0[t] = (T)0; }
        }
        // Now -- with the first panel loads in flight -- fetch the remaining kernel arguments in ONE batch of scalar loads
        // (they are otherwise read piecemeal behind branches, each time with its own wait): a value that depends on all of
        // them is made opaque and tested.  (Not `asm volatile`: that counts as a possible store and would turn the table
        // reads below from scalar into vector loads.)
        {
            size_t keep = (size_t)x ^ (size_t)A.slice_row ^ (size_t)A.slice_w ^ (size_t)b ^ (size_t)y ^ (size_t)done ^ (size_t)ld;
            if (MODE == SELL_AX) keep ^= (size_t)z.u ^ (size_t)z.gs_val ^ (size_t)z.diag_slot ^ (size_t)z.n_first ^ (size_t)z.jacobi ^ (size_t)z.d;
            if (CHEB || RES) keep ^= (size_t)z.d;
            asm("" : "+s"(keep));
            if (keep == 0x5a5a5a5a5a5a5a5bull) return;   // never: only there to consume `keep`
        }
        // The convergence flag is requested early but only consulted right before the stores: the matrix / vector loads of a
        // launch must not wait for that round trip (a launch after convergence does the work and writes nothing).
        stop = load_flag(done);
        const int row0 = A.slice_row[s];
        const int nrow = A.slice_row[s + 1] - row0;
        const int w = A.slice_w[s];
        const int rowb = row0 + lane;
        // out-of-place colour launch: rows below `split` (the first row of the launch = of the colour) already have this sweep's value in y
        const int split = OOP ? A.slice_row[s_begin] : 0;
        T acc[KB];
        T accr[KB];  // HEAD modes: sum over ALL stored entries of the row against the old iterate (the residual's own accumulator)
        T diag = (T)1;
        T xi[KB];  // SELL_JACOBI / SELL_CHEBY: the row's own old value (it travels with the gathers: the diagonal entry's column)
        T dold[KB];  // SELL_CHEBY: the row's previous update
        T bv[KB];  // b (or the prolongation's input iterate for SELL_ADD): requested now, consumed after the panel loop
        const bool live = lane < nrow;
        T zd = (T)1;   // restriction with a fused first colour: the coarse diagonal, requested now
        if (MODE == SELL_AX && live && rowb < z.n_first) zd = z.gs_val[z.diag_slot[rowb]];
#pragma unroll
        for (int q = 0; q < KB; q++) {
            acc[q] = (T)0; accr[q] = (T)0; xi[q] = (T)0; dold[q] = (T)0;
            if (MODE == SELL_AX) bv[q] = (T)0;
            else bv[q] = live ? b[(size_t)rowb * ld + q] : (T)0;   // SELL_ADD: b is the iterate the correction is added to (== y in place)
            if (CHEB && live && z.c1 != (T)0) dold[q] = z.d[(size_t)rowb * ld + q];
        }
        // one batch of U panel columns: gather x for all of them, then accumulate in ascending column order
        bool has_diag = false;   // (RES modes)
        auto consume = [&](const int (&cw)[U], const T (&vw)[U]) {
            int c[U];
            T v[U];
#pragma unroll
            for (int t = 0; t < U; t++) {
                if constexpr (CODED) { c[t] = cw[t] >> 2; v[t] = code_val<T>(z, cw[t]); }   // padding: -1 >> 2 == -1
                else { c[t] = cw[t]; v[t] = vw[t]; }
            }
            T xv[U][KB];
            T xo[MODE == SELL_GS_HEAD ? U : 1][KB];   // SELL_GS_HEAD: the OLD iterate at every stored column (xv holds the sweep's operand)
#pragma unroll
            for (int t = 0; t < U; t++) {
                const bool use = (c[t] >= 0) && !(GS && c[t] == rowb);
                if constexpr (MODE == SELL_GS_HEAD) {
                    // old value for every entry (diagonal included) and, for the earlier colours, y's value: two independent requests --
                    // the choice between them is made when they are consumed (written as one select here, the second load waited for
                    // the first: seven dependent round trips per row)
                    gather_kb<KB, T>(x + (size_t)c[t] * ld, c[t] >= 0, xo[t]);
                    gather_kb<KB, T>((const T*)y + (size_t)c[t] * ld, use && c[t] < split, xv[t]);
                } else if constexpr (MODE == SELL_GS_OOP || MODE == SELL_GS_OOP_RES) {
                    gather_kb<KB, T>((c[t] < split ? (const T*)y : x) + (size_t)c[t] * ld, use, xv[t]);
                } else {
                    gather_kb<KB, T>(x + (size_t)c[t] * ld, use, xv[t]);
                }
            }
#pragma unroll
            for (int t = 0; t < U; t++) {
                if (c[t] >= 0) {
                    if (HEAD) {
#pragma unroll
                        for (int q = 0; q < KB; q++) accr[q] += v[t] * (MODE == SELL_GS_HEAD ? xo[t][q] : xv[t][q]);
                    }
                    if (GS && c[t] == rowb) {
                        diag = v[t];
                        if (RES) has_diag = true;
                    } else if ((JAC || CHEB) && c[t] == rowb) {
                        diag = v[t];
#pragma unroll
                        for (int q = 0; q < KB; q++) xi[q] = xv[t][q];
                    } else {
#pragma unroll
                        for (int q = 0; q < KB; q++) acc[q] += v[t] * ((MODE == SELL_GS_HEAD && c[t] >= split) ? xo[t][q] : xv[t][q]);
                    }
                }
            }
        };
        if (W0 > 0) consume(c0, v0);   // columns [0, W0), requested ahead of the table
        for (int j0 = W0; j0 < w; j0 += U) {
            int c[U];
            T v[U];
#pragma unroll
            for (int t = 0; t < U; t++) {
                if ((j0 + t) < w) { c[t] = cp[(size_t)(j0 + t) * C]; v[t] = CODED ? (T)0 : vp[(size_t)(j0 + t) * C]; }   // wave-uniform
                else { c[t] = -1; v[t] = (T)0; }
            }
            consume(c, v);
        }
        // RES modes: the launch covers the LAST colour (launch_sell_mode insists on it), so every row of the level is final once it has stored,
        // and r_i = b_i - sum_j a_ij u_j of its rows needs nothing more than the wave holds.  The colour's rows close the colour-major
        // numbering and are no neighbours of each other: every other stored column of a row is smaller than the row, the diagonal is its LAST
        // stored entry.  SELL_RESID's sum -- one accumulator from +0 over all stored entries in slot order, separate multiply and add -- is
        // therefore the sweep's own sum (same products, same order, the same operands: the final iterate of the other colours) plus one more
        // term, the diagonal times the value just computed.  Slices of any width: nothing is kept, nothing is read twice.
        T unew[KB];
#pragma unroll
        for (int q = 0; q < KB; q++) unew[q] = (T)0;
        if constexpr (RES) {
#pragma unroll
            for (int q = 0; q < KB; q++) {
                unew[q] = (bv[q] - acc[q]) / diag;
                accr[q] = has_diag ? acc[q] + diag * unew[q] : acc[q];
            }
        }
        if (live && !stop) {
            const size_t o = (size_t)rowb * ld;
#pragma unroll
            for (int q = 0; q < KB; q++) {
                if (MODE == SELL_AX) {
                    y[o + q] = acc[q];
                    if (z.u) {
                        const T t = acc[q] / zd;
                        if (z.jacobi == 2) { const T dn = z.omega * (t - (T)0); z.u[o + q] = (T)0 + dn; z.d[o + q] = dn; }
                        else z.u[o + q] = rowb < z.n_first ? (z.jacobi ? (T)0 + z.omega * (t - (T)0) : t) : (T)0;
                    }
                }
                else if (MODE == SELL_RESID) y[o + q] = bv[q] - acc[q];
                else if (MODE == SELL_ADD) y[o + q] = bv[q] + acc[q];
                else if (RES) { y[o + q] = unew[q]; z.d[o + q] = bv[q] - accr[q]; }
                else if (GS) y[o + q] = (bv[q] - acc[q]) / diag;
                else if (JAC) { const T t = (bv[q] - acc[q]) / diag; y[o + q] = xi[q] + z.omega * (t - xi[q]); }
                else if (CHEB) {
                    const T t = (bv[q] - acc[q]) / diag;
                    const T r = t - xi[q];
                    const T dn = z.c1 != (T)0 ? z.c1 * dold[q] + z.omega * r : z.omega * r;
                    y[o + q] = xi[q] + dn;
                    z.d[o + q] = dn;
                }
                else { const double t = (double)(bv[q] - acc[q]); ss += t * t; if (MODE == SELL_RESID_BOTH) y[o + q] = bv[q] - acc[q]; }
                if (HEAD) { const double t = (double)(bv[q] - accr[q]); ss += t * t; }
            }
        }
    }
    if (sell_has_ss(MODE)) {
        __shared__ double red[16];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) ss += __shfl_down(ss, o, 64);
        if (lane == 0) red[wave] = ss;
        __syncthreads();
        if (threadIdx.x == 0 && !stop) {
            double t = 0.0;
            for (int i2 = 0; i2 < wpb; i2++) t += red[i2];
            partials[HEAD ? bid : (int)blockIdx.x] = t;   // (one-XCD colour launches: only every 8th workgroup works)
        }
    }
}

// ---- deep variant for WIDE rows (the operators of the reference's decimated hierarchies: Galerkin matrices of 18 - 30 entries per row, restriction
// rows of 12 on average and 40 at most).  k_sell walks a slice in batches of 8 panel columns, each batch two dependent round trips (columns / values, then
// the gathers): a 40-entry row is ten round trips, and on a level of 16 k rows that chain IS the launch (residual of the 15 804-row Galerkin level: 10.6 us).
// Here the wave requests the WHOLE slice at once -- every panel column it has (guards are per-lane predicates on a per-lane copy of the slice's width:
// a wave-uniform branch between two requests makes the compiler wait for the first), then every gather -- three round trips whatever the width; the sums
// run over the registers in ascending column, separate multiply and add: the bits of k_sell.  fp64, SELL_AX (restriction incl. uc = 0 / fused first colour)
// and SELL_RESID, KB <= 3 columns per lane.
template <int MODE, int KB, int NBMAX>
__global__ __launch_bounds__(256) void k_sell_deep(const int* a_col, const double* a_val, const int* a_order, const int* a_slice_off, int a_stride, int s_begin, int s_end,
                                                   int n_blocks, int use_order, const double* x, const int* a_slice_row, const int* a_slice_w, const double* b, double* y, int ld,
                                                   const int* done, CoarseInit<double> z)
{
    constexpr int C = 64, S = NBMAX * 8;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int bid = xcd_remap(blockIdx.x, n_blocks);
    const int ls = __builtin_amdgcn_readfirstlane(s_begin + bid * 4 + wave);
    if (ls >= s_end) return;
    const int s = use_order ? a_order[ls] : ls;
    const int stop = load_flag(done);
    const int oz = __builtin_amdgcn_mbcnt_lo(~0u, 0u) >> 6;      // 0, opaque: the slice's table entries as per-lane values
    const int row0 = a_slice_row[s + oz], nrow = a_slice_row[s + 1 + oz] - row0, w = a_slice_w[s + oz];
    const int off0 = a_stride ? s * a_stride : a_slice_off[s + oz];
    const int rowb = row0 + lane;
    const bool live = lane < nrow;
    const int* cp = a_col + (size_t)off0 * C + lane;
    const double* vp = a_val + (size_t)off0 * C + lane;
    int c[S];
    double v[S];
#pragma unroll
    for (int bt = 0; bt < NBMAX; bt++) {
        if (bt * 8 < w) {
#pragma unroll
            for (int t = bt * 8; t < bt * 8 + 8; t++) {
                const int tt = t < w ? t : w - 1;        // a column beyond the slice's width: its last one again (same line), dropped below
                c[t] = cp[(size_t)tt * C];
                v[t] = z.codes ? 0.0 : vp[(size_t)tt * C];
            }
        } else {
#pragma unroll
            for (int t = bt * 8; t < bt * 8 + 8; t++) { c[t] = -1; v[t] = 0.0; }
        }
    }
    double zd = 1.0, bv[KB];
    if (MODE == SELL_AX && live && rowb < z.n_first) zd = z.gs_val[z.diag_slot[rowb]];
#pragma unroll
    for (int q = 0; q < KB; q++) bv[q] = (MODE == SELL_RESID && live) ? b[(size_t)rowb * ld + q] : 0.0;
    if (z.codes) {   // weight codes (SellDev::codes)
#pragma unroll
        for (int t = 0; t < S; t++) { v[t] = code_val<double>(z, c[t]); c[t] >>= 2; }
    }
    double xv[S][KB];
#pragma unroll
    for (int t = 0; t < S; t++) {
        const bool use = c[t] >= 0 && t < w;
        if (!use) v[t] = 0.0;                              // padding: +0.0 times 0.0 leaves a sum that started at +0 as it is
        gather_kb<KB, double>(x + (size_t)(use ? c[t] : 0) * ld, use, xv[t]);
    }
    double acc[KB];
#pragma unroll
    for (int q = 0; q < KB; q++) acc[q] = 0.0;
#pragma unroll
    for (int bt = 0; bt < NBMAX; bt++) {
        if (bt * 8 < w) {
#pragma unroll
            for (int t = bt * 8; t < bt * 8 + 8; t++)
#pragma unroll
                for (int q = 0; q < KB; q++) acc[q] += v[t] * xv[t][q];
        }
    }
    if (live && !stop) {
        const size_t o = (size_t)rowb * ld;
#pragma unroll
        for (int q = 0; q < KB; q++) {
            if (MODE == SELL_AX) {
                y[o + q] = acc[q];
                if (z.u) {
                    const double t = acc[q] / zd;
                    if (z.jacobi == 2) { const double dn = z.omega * (t - 0.0); z.u[o + q] = 0.0 + dn; z.d[o + q] = dn; }
                    else z.u[o + q] = rowb < z.n_first ? (z.jacobi ? 0.0 + z.omega * (t - 0.0) : t) : 0.0;
                }
            } else y[o + q] = bv[q] - acc[q];
        }
    }
}
// which launches take the deep variant: SMG_DEEP=0 switches it off (A/B knob; same bits either way)
static bool deep_wanted(int mode, int w_max, int kb)
{
    static const int on = getenv("SMG_DEEP") ? atoi(getenv("SMG_DEEP")) : 1;
    static const int wmin = getenv("SMG_DEEP_MIN_W") ? atoi(getenv("SMG_DEEP_MIN_W")) : 13;
    if (!on || (mode != SELL_AX && mode != SELL_RESID) || w_max < wmin || w_max > 64) return false;
    const int nbm = w_max <= 24 ? 3 : w_max <= 40 ? 5 : 8;
    return nbm == 3 ? kb <= 3 : nbm == 5 ? kb <= 2 : kb == 1;
}

// Row-width classes of the deep variant and their column limits: widest row <= 24 entries NBMAX = 3, KB <= 3; <= 40: 5, KB <= 2; <= 64: 8, KB = 1.
// A group of 4 columns goes 3 + 1, 2 + 2 or 1 + 1 + 1 + 1.  launch_sell_mode launches what this returns; smg_debug_deep_launches reports it.
int deep_split(int mode, int w_max, int kb, int* cols, int* nbmax)
{
    if (kb < 1 || kb > 4) return 0;
    int kd = kb;
    if (kd == 4 && !deep_wanted(mode, w_max, 4) && deep_wanted(mode, w_max, 2)) kd = 2;
    if (!(deep_wanted(mode, w_max, kd) || (kd > 1 && deep_wanted(mode, w_max, 1)))) return 0;
    *nbmax = w_max <= 24 ? 3 : w_max <= 40 ? 5 : 8;
    int n = 0;
    for (int cc = 0; cc < kb;) {
        int kk = kb - cc;
        while (kk > 1 && !deep_wanted(mode, w_max, kk)) kk--;
        cols[n++] = kk;
        cc += kk;
    }
    return n;
}

// ---- wide multi-RHS variant --------------------------------------------------------------------------------------
// For k >= 8 right-hand sides the lanes run ACROSS COLUMNS: lane = (g, c) with c = lane % KW the column inside a block of
// KW in {8,16,32,64} columns and g = lane / KW one of G = 64/KW rows handled concurrently.  A neighbour gather is then
// one contiguous 8*KW-byte segment of the row-major n x k block (the layout was chosen for this), the matrix entry is
// shared by the KW lanes of a group (one request), and all k columns go through ONE launch instead of k/4.
// A wave owns 8*G consecutive rows of a slice (KW/8 waves per slice).  Per (row, column) the sum is still sequential in
// ascending column order: bit-identical to the narrow kernel and to the oracle.
// R rows per lane, U panel columns requested per batch.  (2, 8) streams; (1, 8 / 16 / 32) is for launches of so few waves that the
// chip is mostly idle and a row's chain of dependent batches IS the launch's duration (the Galerkin levels of decimated hierarchies:
// 15 - 30 entries per row): one row per lane, the whole row requested at once.
template <int MODE, int KW, typename T, int R = 2, int U = 8>
__global__ __launch_bounds__(256) void k_sell_wide(const int* a_col, const T* a_val, const int* a_order, const int* a_slice_off, int a_stride,
                                                   int s_begin, int s_end, int n_blocks, int use_order, const T* x,
                                                   const int* a_slice_row, const int* a_slice_w, const T* b, T* y, int ld,
                                                   const int* done, double* partials, CoarseInit<T> z)
{
    struct { const int *slice_row, *slice_off, *slice_w, *order, *col; int stride; } A = {a_slice_row, a_slice_off, a_slice_w, a_order, a_col,
                                                                                        a_stride};
    constexpr bool GS = sell_is_gs(MODE), OOP = sell_is_oop(MODE), JAC = sell_is_jacobi(MODE), CHEB = sell_is_cheby(MODE), HEAD = sell_is_head(MODE);
    const int stop = load_flag(done);
    constexpr int G = 64 / KW;        // rows in flight per wave-instruction
    constexpr int RW = R * G;         // rows per wave
    constexpr int SUB = 64 / RW;      // waves per slice
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int c = lane % KW, g = lane / KW;
    const int bid = xcd_remap(blockIdx.x, n_blocks);
    const int wid = __builtin_amdgcn_readfirstlane(bid * 4 + wave);  // logical wave
    const int ls = s_begin + wid / SUB;
    const int sub = wid % SUB;
    double ss = 0.0;
    if (ls < s_end) {
        const int s = use_order ? A.order[ls] : ls;
        const int row0 = A.slice_row[s];
        const int nrow = A.slice_row[s + 1] - row0;
        const int off0 = A.stride ? s * A.stride : A.slice_off[s];
        const int w = A.slice_w[s];
        const int split = OOP ? A.slice_row[s_begin] : 0;   // see k_sell
        int rl[R];
        T acc[R], accr[R], diag[R], bv[R], zd[R], xi[R], dold[R];
#pragma unroll
        for (int r = 0; r < R; r++) {
            rl[r] = sub * RW + r * G + g;   // row inside the slice
            acc[r] = (T)0; accr[r] = (T)0; diag[r] = (T)1; xi[r] = (T)0; dold[r] = (T)0;
            const bool live = rl[r] < nrow;
            zd[r] = (T)1;
            if (MODE == SELL_AX && live && row0 + rl[r] < z.n_first) zd[r] = z.gs_val[z.diag_slot[row0 + rl[r]]];
            const size_t o = (size_t)(row0 + rl[r]) * ld + c;
            if (MODE == SELL_AX) bv[r] = (T)0;
            else bv[r] = live ? b[o] : (T)0;
            if (CHEB && live && z.c1 != (T)0) dold[r] = z.d[o];
        }
        const int* cp = A.col + (size_t)off0 * 64;
        const T* vp = a_val + (size_t)off0 * 64;
        for (int j0 = 0; j0 < w; j0 += U) {
            int cc[U][R];
            T vv[U][R], xv[U][R];
            T xo[MODE == SELL_GS_HEAD ? U : 1][R];
            constexpr int NL = G == 1 ? 1 : (U * RW + 63) / 64;     // coalesced loads of the batch's entries (G > 1), one entry per lane:
            int cL[NL];                                              // entry e = t * RW + (row inside the wave's RW rows)
            T vL[NL];
            if constexpr (G > 1) {
#pragma unroll
                for (int q = 0; q < NL; q++) {
                    const int e = q * 64 + lane, tt = e / RW, rr = e % RW;
                    const bool in2 = e < U * RW && (j0 + tt) < w;
                    cL[q] = in2 ? cp[(size_t)(j0 + tt) * 64 + sub * RW + rr] : -1;
                    vL[q] = (in2 && !z.codes) ? vp[(size_t)(j0 + tt) * 64 + sub * RW + rr] : (T)0;
                }
            }
#pragma unroll
            for (int t = 0; t < U; t++)
#pragma unroll
                for (int r = 0; r < R; r++) {
                    const bool in = (j0 + t) < w;  // wave-uniform
                    (void)in;
                    if constexpr (G == 1) {        // the row is the same for all lanes: the compiler fetches the entry through the scalar cache
                        cc[t][r] = in ? cp[(size_t)(j0 + t) * 64 + rl[r]] : -1;
                        vv[t][r] = (in && !z.codes) ? vp[(size_t)(j0 + t) * 64 + rl[r]] : (T)0;
                    } else {
                        // G rows per wave-instruction: as a load of its own every slot would have the 64 lanes ask for G distinct words, and
                        // these two loads per slot -- not the gathers -- bound the launch.  The batch's U x RW entries are fetched by
                        // coalesced loads (one entry per lane) above and handed to the lanes of their rows through the LDS crossbar.
                        const int src = t * RW + r * G + g;
                        cc[t][r] = __shfl(cL[(t * RW + r * G) / 64], src & 63, 64);
                        vv[t][r] = __shfl(vL[(t * RW + r * G) / 64], src & 63, 64);
                    }
                    if (z.codes) { vv[t][r] = code_val<T>(z, cc[t][r]); cc[t][r] >>= 2; }   // weight codes (SellDev::codes)
                }
#pragma unroll
            for (int t = 0; t < U; t++)
#pragma unroll
                for (int r = 0; r < R; r++) {
                    const bool use = (cc[t][r] >= 0) && !(GS && cc[t][r] == row0 + rl[r]);
                    if constexpr (MODE == SELL_GS_HEAD) {
                        xo[t][r] = cc[t][r] >= 0 ? x[(size_t)cc[t][r] * ld + c] : (T)0;
                        xv[t][r] = (use && cc[t][r] < split) ? y[(size_t)cc[t][r] * ld + c] : (T)0;   // chosen when consumed, see k_sell
                    } else if constexpr (MODE == SELL_GS_OOP) {
                        const T* src = cc[t][r] < split ? (const T*)y : x;
                        xv[t][r] = use ? src[(size_t)cc[t][r] * ld + c] : (T)0;
                    } else xv[t][r] = use ? x[(size_t)cc[t][r] * ld + c] : (T)0;
                }
#pragma unroll
            for (int t = 0; t < U; t++)
#pragma unroll
                for (int r = 0; r < R; r++) {
                    if (cc[t][r] >= 0) {
                        if (HEAD) accr[r] += vv[t][r] * (MODE == SELL_GS_HEAD ? xo[t][r] : xv[t][r]);
                        if (GS && cc[t][r] == row0 + rl[r]) diag[r] = vv[t][r];
                        else if ((JAC || CHEB) && cc[t][r] == row0 + rl[r]) { diag[r] = vv[t][r]; xi[r] = xv[t][r]; }
                        else acc[r] += vv[t][r] * ((MODE == SELL_GS_HEAD && cc[t][r] >= split) ? xo[t][r] : xv[t][r]);
                    }
                }
        }
#pragma unroll
        for (int r = 0; r < R; r++) {
            if (rl[r] < nrow && !stop) {
                const size_t o = (size_t)(row0 + rl[r]) * ld + c;
                if (MODE == SELL_AX) {
                    y[o] = acc[r];
                    if (z.u) {
                        const T t = acc[r] / zd[r];
                        if (z.jacobi == 2) { const T dn = z.omega * (t - (T)0); z.u[o] = (T)0 + dn; z.d[o] = dn; }
                        else z.u[o] = row0 + rl[r] < z.n_first ? (z.jacobi ? (T)0 + z.omega * (t - (T)0) : t) : (T)0;
                    }
                }
                else if (MODE == SELL_RESID) y[o] = bv[r] - acc[r];
                else if (MODE == SELL_ADD) y[o] = bv[r] + acc[r];
                else if (GS) y[o] = (bv[r] - acc[r]) / diag[r];
                else if (JAC) { const T t = (bv[r] - acc[r]) / diag[r]; y[o] = xi[r] + z.omega * (t - xi[r]); }
                else if (CHEB) {
                    const T t = (bv[r] - acc[r]) / diag[r];
                    const T rr = t - xi[r];
                    const T dn = z.c1 != (T)0 ? z.c1 * dold[r] + z.omega * rr : z.omega * rr;
                    y[o] = xi[r] + dn;
                    z.d[o] = dn;
                }
                else { const double t = (double)(bv[r] - acc[r]); ss += t * t; if (MODE == SELL_RESID_BOTH) y[o] = bv[r] - acc[r]; }
                if (HEAD) { const double t = (double)(bv[r] - accr[r]); ss += t * t; }
            }
        }
    }
    if (sell_has_ss(MODE)) {
        __shared__ double red[4];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) ss += __shfl_down(ss, o, 64);
        if (lane == 0) red[wave] = ss;
        __syncthreads();
        if (threadIdx.x == 0 && !stop) partials[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
    }
}

// ---- companion of SELL_AX for the long rows kept out of the panels (SellDev::long_*): one wave per (row, column).  The lanes form
// the products of up to 64 entries at once (one round trip for the entries, one for the gathers, whatever the row's length); the sum
// is then taken in ascending entry order by broadcasting the products one after the other -- the very sequence of additions the panel
// kernel performs, starting from +0.
template <typename T>
__global__ __launch_bounds__(256) void k_long_ax(const int* rows, const int* ptr, const int* col, const T* val, int nl, const T* x, T* y, int ld, int k,
                                                 const int* done, CoarseInit<T> z)
{
    const int stop = load_flag(done);
    const int lane = threadIdx.x & 63;
    const long wid = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (wid >= (long)nl * k) return;
    const int r = (int)(wid / k), c = (int)(wid % k);
    const int row = rows[r], p0 = ptr[r], p1 = ptr[r + 1];
    T zd = (T)1;
    if (z.u && row < z.n_first) zd = z.gs_val[z.diag_slot[row]];
    T acc = (T)0;
    for (int base = p0; base < p1; base += 64) {
        const int t = base + lane;
        T prod = (T)0;
        if (t < p1) prod = val[t] * x[(size_t)col[t] * ld + c];
        const int n = (p1 - base) < 64 ? (p1 - base) : 64;
        for (int i = 0; i < n; i++) acc += __shfl(prod, i, 64);
    }
    if (lane == 0 && !stop) {
        const size_t o = (size_t)row * ld + c;
        y[o] = acc;
        if (z.u) {
            const T t = acc / zd;
            if (z.jacobi == 2) { const T dn = z.omega * (t - (T)0); z.u[o] = (T)0 + dn; z.d[o] = dn; }
            else z.u[o] = row < z.n_first ? (z.jacobi ? (T)0 + z.omega * (t - (T)0) : t) : (T)0;
        }
    }
}
// the same for many columns (k >= 8): one wave per (row, block of 64 columns), lanes across the COLUMNS, so that every gather is one
// contiguous segment of the row-major block; the entries are fetched 64 at a time and their gathers requested 32 at a time (independent
// loads: the chain is a handful of round trips whatever the row's length), the additions run in entry order.
template <typename T>
__global__ __launch_bounds__(256) void k_long_ax_cols(const int* rows, const int* ptr, const int* col, const T* val, int nl, const T* x, T* y, int ld, int k,
                                                      const int* done, CoarseInit<T> z)
{
    const int stop = load_flag(done);
    const int lane = threadIdx.x & 63;
    const int cblocks = (k + 63) >> 6;
    const long wid = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (wid >= (long)nl * cblocks) return;
    const int r = (int)(wid / cblocks), c = (int)(wid % cblocks) * 64 + lane;
    const bool colok = c < k;
    const int row = rows[r], p0 = ptr[r], p1 = ptr[r + 1];
    T zd = (T)1;
    if (z.u && row < z.n_first) zd = z.gs_val[z.diag_slot[row]];
    T acc = (T)0;
    constexpr int U = 32;
    for (int base = p0; base < p1; base += 64) {
        const int t = base + lane;
        const int ce = t < p1 ? col[t] : 0;
        const T ve = t < p1 ? val[t] : (T)0;
        const int n = (p1 - base) < 64 ? (p1 - base) : 64;
        for (int i0 = 0; i0 < n; i0 += U) {
            T xv[U], vv[U];
#pragma unroll
            for (int i = 0; i < U; i++) {
                const int cc = __shfl(ce, (i0 + i) & 63, 64);
                vv[i] = __shfl(ve, (i0 + i) & 63, 64);
                xv[i] = (i0 + i < n && colok) ? x[(size_t)cc * ld + c] : (T)0;
            }
#pragma unroll
            for (int i = 0; i < U; i++) if (i0 + i < n) acc += vv[i] * xv[i];
        }
    }
    if (colok && !stop) {
        const size_t o = (size_t)row * ld + c;
        y[o] = acc;
        if (z.u) {
            const T t = acc / zd;
            if (z.jacobi == 2) { const T dn = z.omega * (t - (T)0); z.u[o] = (T)0 + dn; z.d[o] = dn; }
            else z.u[o] = row < z.n_first ? (z.jacobi ? (T)0 + z.omega * (t - (T)0) : t) : (T)0;
        }
    }
}
template <typename T> static CoarseInit<T> coarse_init(T* zero_rows, int c0, const FirstColour* first, double omega)
{
    CoarseInit<T> z{zero_rows ? zero_rows + c0 : nullptr, nullptr, nullptr, 0, 0, (T)omega, nullptr, (T)0};
    if (first) {   // Chebyshev step / fused first Chebyshev step: the update vector and the old update's coefficient
        z.d = first->update<T>() ? first->update<T>() + c0 : nullptr;
        z.c1 = (T)first->c1;
    }
    if (zero_rows && first && first->n_first > 0) {
        z.gs_val = first->vals<T>();
        z.diag_slot = first->diag_slot;
        z.n_first = (z.gs_val && z.diag_slot) ? first->n_first : 0;
        z.jacobi = first->jacobi;
        if (first->jacobi) z.omega = (T)first->omega;
    }
    return z;
}
// coarse_init plus the weight-code table of A (SellDev::codes)
template <typename T> static CoarseInit<T> coarse_codes(const SellDev& A, T* zero_rows, int c0, const FirstColour* first, double omega)
{
    CoarseInit<T> z = coarse_init<T>(zero_rows, c0, first, omega);
    z.codes = A.codes;
    for (int i = 0; i < 4; i++) z.tab[i] = A.table<T>()[i];
    return z;
}

// one-row-per-lane variants (see k_sell_wide) up to this many waves
static long wide_latency_max()
{
    static const long v = getenv("SMG_WIDE_LAT_MAX") ? atol(getenv("SMG_WIDE_LAT_MAX")) : 16384;
    return v;
}
bool wide_latency_variant(int n_slices, int kw) { return (long)n_slices * kw <= wide_latency_max(); }

template <int MODE, int KW, typename T>
static void launch_wide_one(const SellDev& A, int s_begin, int s_end, int use_order, const T* x, const T* b, T* y,
                            int k, const int* done, double* partials, CoarseInit<T> zero_rows, hipStream_t st, int* nb_out)
{
    const int ns = s_end - s_begin;
    // (64 columns per wave: a wave spans one or two whole rows anyway, and the longer batches only cost there -- ogre.obj, k = 64:
    // 239 -> 264 us per Chebyshev cycle with one row per lane, 292 with two rows and batches of 32)
    if constexpr (KW < 64) if (wide_latency_variant(ns, KW)) {
        const int nb = (ns * KW + 3) / 4;   // 64 / G = KW waves per slice with one row per lane
#define SMG_WIDE_LAT(UU) hipLaunchKernelGGL((k_sell_wide<MODE, KW, T, 1, UU>), dim3(nb), dim3(256), 0, st, A.col, A.vals<T>(), A.order, A.slice_off, A.stride, \
                                             s_begin, s_end, nb, use_order, x, A.slice_row, A.slice_w, b, y, k, done, partials, zero_rows)
        if (A.w_max <= 8) SMG_WIDE_LAT(8);
        else if (A.w_max <= 16) SMG_WIDE_LAT(16);
        else SMG_WIDE_LAT(32);
#undef SMG_WIDE_LAT
        *nb_out = nb;
        return;
    }
    const int waves = ns * (KW / 2);  // 64 / (R * G) waves per slice, R = 2
    const int nb = (waves + 3) / 4;
    hipLaunchKernelGGL((k_sell_wide<MODE, KW, T>), dim3(nb), dim3(256), 0, st, A.col, A.vals<T>(), A.order, A.slice_off, A.stride, s_begin, s_end, nb, use_order, x,
                       A.slice_row, A.slice_w, b, y, k, done, partials, zero_rows);
    *nb_out = nb;
}

int sell_wide_blocks(int n_slices, int k)
{
    // upper bound of the per-block partial sums the wide path writes for k columns
    int tot = 0, c0 = 0;
    while (k - c0 >= 8) { int kw = 64; while (kw > k - c0) kw >>= 1; tot += (n_slices * kw + 3) / 4; c0 += kw; }   // (one row per lane: the larger of the two variants' counts)
    return tot;
}

// 4 slices (waves) per 256-thread block; 1, 2 and 8 measured the same within noise on C3
static constexpr int sell_wpb() { return 4; }
static int gs_wpb() { static const int v = getenv("SMG_GS_WPB") ? atoi(getenv("SMG_GS_WPB")) : 4; return v; }   // A/B knob: waves per workgroup of the big colour launches
int sell_blocks(int n_slices) { return (n_slices + sell_wpb() - 1) / sell_wpb(); }
// small colour sweeps run on one XCD (see k_sell): grid 8 nb, n_blocks passed negated
static bool one_xcd_launch(bool gs, int nb)
{
    static const int one_xcd_max = getenv("SMG_ONE_XCD_MAX") ? atoi(getenv("SMG_ONE_XCD_MAX")) : 32;
    return gs && nb <= one_xcd_max;
}
// whole-pitch look-ahead: colour sweeps of <= 32 workgroups, and the whole-matrix launches (Jacobi / Chebyshev sweeps,
// residual, transfer) of a level that small, <= 64 workgroups (C3 level 3: 37.3 -> 34.1 us per visit; colour sweeps of 62
// workgroups lose with it)
static bool whole_pitch_ahead(const SellDev& A, bool gs, int nb)
{
    static const int pitch_env = getenv("SMG_PITCH_SPEC_MAX") ? atoi(getenv("SMG_PITCH_SPEC_MAX")) : -1;
    const int pitch_max = pitch_env >= 0 ? pitch_env : (gs ? 32 : 64);
    return nb <= pitch_max && A.stride == 12 && A.w_lo >= 7;
}
// Waves per workgroup of a one-column Gauss-Seidel colour launch (SELL_GS, values not coded) of n_slices slices of A: SMG_GS_WPB = 2 / 8 where the
// launch is not confined to one XCD, does not request the whole pitch ahead, and A has fixed-pitch panels of lower width 7; 4 otherwise.
// launch_narrow branches on this; smg_debug_gs_colour_wpb reports it.
int gs_colour_wpb(const SellDev& A, int n_slices)
{
    const int nb = sell_blocks(n_slices);
    if (A.codes || !(A.stride > 0 && A.w_lo == 7) || one_xcd_launch(true, nb) || whole_pitch_ahead(A, true, nb)) return 4;
    return gs_wpb() == 8 ? 8 : gs_wpb() == 2 ? 2 : 4;
}

// the narrow launches (kb <= 4 columns per lane) of one group of columns; CODED: the matrix holds weight codes (SELL_AX / SELL_ADD only)
template <typename T>
struct NarrowRun {   // what every variant below is launched with
    int s_begin, s_end, use_order;
    const T *xx, *bb;
    T* yy;
    int k;
    const int* done;
    double* pp;
    const CoarseInit<T>& zz;
    hipStream_t st;
};
// W0C: the look-ahead count fixed at compile time (-1: read from the matrix); WPB: waves per workgroup
template <int MODE, int KB, typename T, int W0C, int WPB, bool CODED>
static void narrow_one(const SellDev& A, int grid, int nbarg, const NarrowRun<T>& R)
{
    hipLaunchKernelGGL((k_sell<MODE, KB, T, W0C, WPB, CODED>), dim3(grid), dim3(64 * WPB), 0, R.st, A.col, CODED ? nullptr : A.vals<T>(), A.order, A.slice_off, A.stride, A.w_lo,
                       R.s_begin, R.s_end, nbarg, R.use_order, R.xx, A.slice_row, A.slice_w, R.bb, R.yy, R.k, R.done, R.pp, R.zz);
}
template <int MODE, typename T, bool CODED>
static void launch_narrow(const SellDev& A, int kb, int nb, int ns, int grid, int nbarg, bool one_xcd, const NarrowRun<T>& R)
{
    static_assert(sell_wpb() == 4, "the narrow kernels below are instantiated for 4 waves per workgroup");
    const bool w7 = A.stride > 0 && A.w_lo == 7;
    switch (kb) {
        case 1: {
            // the usual widths get kernels with the look-ahead count fixed at compile time (no branch per panel column)
            const int w0 = A.stride > 0 ? (A.w_lo < 8 ? A.w_lo : 8) : -1;
            const int wpb = (!CODED && MODE == SELL_GS) ? gs_colour_wpb(A, ns) : 4;      // (4 whenever one_xcd or the whole pitch goes ahead)
            if (whole_pitch_ahead(A, sell_is_gs(MODE), nb)) narrow_one<MODE, 1, T, 12, 4, CODED>(A, grid, nbarg, R);
            else if (wpb == 8) narrow_one<SELL_GS, 1, T, 7, 8, false>(A, (ns + 7) / 8, (ns + 7) / 8, R);
            else if (wpb == 2) narrow_one<SELL_GS, 1, T, 7, 2, false>(A, (ns + 1) / 2, (ns + 1) / 2, R);
            else if (w0 == 7) narrow_one<MODE, 1, T, 7, 4, CODED>(A, grid, nbarg, R);
            else if (w0 == 8) narrow_one<MODE, 1, T, 8, 4, CODED>(A, grid, nbarg, R);
            else if (w0 == 2) narrow_one<MODE, 1, T, 2, 4, CODED>(A, grid, nbarg, R);
            else narrow_one<MODE, 1, T, -1, 4, CODED>(A, grid, nbarg, R);
            break;
        }
        case 2:
            if (w7) narrow_one<MODE, 2, T, 7, 4, CODED>(A, grid, nbarg, R);
            else narrow_one<MODE, 2, T, -1, 4, CODED>(A, grid, nbarg, R);
            break;
        case 3:
            if (w7) narrow_one<MODE, 3, T, 7, 4, CODED>(A, grid, nbarg, R);
            else narrow_one<MODE, 3, T, -1, 4, CODED>(A, grid, nbarg, R);
            break;
        default:
            if (w7) narrow_one<MODE, 4, T, 7, 4, CODED>(A, grid, nbarg, R);
            else narrow_one<MODE, 4, T, -1, 4, CODED>(A, grid, nbarg, R);
            break;
    }
}

template <int MODE, typename T>
static hipError_t launch_sell_mode(const SellDev& A, int s_begin, int s_end_in, const T* x, const T* b, T* y,
                                   int k, const Ctrl* ctrl, double* partials, int* n_blocks, hipStream_t st, T* zero_rows, const FirstColour* first,
                                   double omega)
{
    int s_end = s_end_in;
    if (MODE == SELL_ADD && !b) b = y;   // in place: the iterate the correction is added to is the output
    // the residual by-product exists in the narrow kernel only, needs its second output, and is the residual only where the launch's rows
    // are the last of the matrix (see k_sell)
    if constexpr (sell_has_res(MODE)) { if (k >= 8 || !first || !first->d || zero_rows || s_end_in != A.n_slices) return hipErrorInvalidValue; }
    const int ns = s_end - s_begin;
    const int nb = sell_blocks(ns);
    const int* done = ctrl ? &ctrl->done : never_done();
    static const int dbg_empty = getenv("SMG_DEBUG_EMPTY") ? atoi(getenv("SMG_DEBUG_EMPTY")) : 0;  // launch-overhead probe
    if (dbg_empty == 1) s_end = s_begin;
    // the region-major launch order only makes sense for whole-matrix launches
    const int use_order = (A.order && s_begin == 0 && s_end == A.n_slices) ? 1 : 0;
    if (n_blocks) *n_blocks = 0;
    if (ns <= 0) return hipSuccess;
    int c0 = 0;
    size_t poff = 0;  // partial sums written so far
    if constexpr (!sell_has_res(MODE)) {
        while (k - c0 >= 8) {
            int kw = 64;
            while (kw > k - c0) kw >>= 1;
            const T* xx = x ? x + c0 : nullptr;
            const T* bb = b ? b + c0 : nullptr;
            T* yy = y ? y + c0 : nullptr;
            double* pp = partials ? partials + poff : nullptr;
            const CoarseInit<T> zz = coarse_codes<T>(A, zero_rows, c0, first, omega);
            int wnb = 0;
            switch (kw) {
                case 64: launch_wide_one<MODE, 64, T>(A, s_begin, s_end, use_order, xx, bb, yy, k, done, pp, zz, st, &wnb); break;
                case 32: launch_wide_one<MODE, 32, T>(A, s_begin, s_end, use_order, xx, bb, yy, k, done, pp, zz, st, &wnb); break;
                case 16: launch_wide_one<MODE, 16, T>(A, s_begin, s_end, use_order, xx, bb, yy, k, done, pp, zz, st, &wnb); break;
                default: launch_wide_one<MODE, 8, T>(A, s_begin, s_end, use_order, xx, bb, yy, k, done, pp, zz, st, &wnb); break;
            }
            poff += (size_t)wnb;
            c0 += kw;
        }
    }
    const bool one_xcd = one_xcd_launch(sell_is_gs(MODE), nb);
    const int grid = one_xcd ? nb * 8 : nb, nbarg = one_xcd ? -nb : nb;
    for (; c0 < k; c0 += 4) {
        const int kb = (k - c0) < 4 ? (k - c0) : 4;
        const T* xx = x ? x + c0 : nullptr;
        const T* bb = b ? b + c0 : nullptr;
        T* yy = y ? y + c0 : nullptr;
        double* pp = partials ? partials + poff : nullptr;
        const CoarseInit<T> zz = coarse_codes<T>(A, zero_rows, c0, first, omega);
        poff += (size_t)nb;
        if constexpr (std::is_same<T, double>::value && (MODE == SELL_AX || MODE == SELL_RESID)) {
            // (k = 4 on a matrix the deep variant serves with 3 columns per lane: 3 + 1)
            int cols[4], nbm = 0;
            const int n_deep = deep_split(MODE, A.w_max, kb, cols, &nbm);
            if (n_deep > 0) {
                for (int i = 0, cc = 0; i < n_deep; cc += cols[i++]) {
                    const int kk = cols[i];
                    const CoarseInit<T> zc = coarse_codes<T>(A, zero_rows, c0 + cc, first, omega);
#define SMG_DEEP_LAUNCH(KB, NB) hipLaunchKernelGGL((k_sell_deep<MODE, KB, NB>), dim3(nb), dim3(256), 0, st, A.col, A.val, A.order, A.slice_off, A.stride, s_begin, s_end, nb, use_order, \
                                                   xx ? xx + cc : nullptr, A.slice_row, A.slice_w, bb ? bb + cc : nullptr, yy + cc, k, done, zc)
                    if (nbm == 3) { if (kk == 1) SMG_DEEP_LAUNCH(1, 3); else if (kk == 2) SMG_DEEP_LAUNCH(2, 3); else SMG_DEEP_LAUNCH(3, 3); }
                    else if (nbm == 5) { if (kk == 1) SMG_DEEP_LAUNCH(1, 5); else SMG_DEEP_LAUNCH(2, 5); }
                    else SMG_DEEP_LAUNCH(1, 8);
#undef SMG_DEEP_LAUNCH
                }
                continue;
            }
        }
        const NarrowRun<T> run{s_begin, s_end, use_order, xx, bb, yy, k, done, pp, zz, st};
        if constexpr (MODE == SELL_AX || MODE == SELL_ADD) {
            if (A.codes) { launch_narrow<MODE, T, true>(A, kb, nb, ns, grid, nbarg, one_xcd, run); continue; }
        }
        launch_narrow<MODE, T, false>(A, kb, nb, ns, grid, nbarg, one_xcd, run);
    }
    if (MODE == SELL_AX && A.long_n > 0 && s_begin == 0 && s_end_in == A.n_slices && A.long_vals<T>()) {
        // the long rows of the matrix (their panel rows are empty: the launches above left zeros there), all k columns in one launch
        const CoarseInit<T> zz = coarse_codes<T>(A, zero_rows, 0, first, omega);
        if (k >= 8) {
            const long waves = (long)A.long_n * ((k + 63) / 64);
            hipLaunchKernelGGL((k_long_ax_cols<T>), dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, st, A.long_row, A.long_ptr, A.long_col, A.long_vals<T>(), A.long_n, x, y,
                               k, k, done, zz);
        } else {
            const long waves = (long)A.long_n * k;
            hipLaunchKernelGGL((k_long_ax<T>), dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, st, A.long_row, A.long_ptr, A.long_col, A.long_vals<T>(), A.long_n, x, y, k, k,
                               done, zz);
        }
    }
    if (n_blocks) *n_blocks = (int)poff;
    return hipGetLastError();
}

// One dispatch for both precisions.  The fp32 twin serves the mixed-precision V-cycle: it needs A.valf (or weight codes), and the modes of
// sell_fp64_only -- the norms, the level-0 head of an outer iteration, the residual by-product -- are not instantiated for it.
template <typename T>
static hipError_t launch_sell_any(SellMode mode, const SellDev& A, int s_begin, int s_end, const T* x, const T* b,
                                  T* y, int k, const Ctrl* ctrl, double* partials, int* n_blocks, hipStream_t st,
                                  T* zero_rows, const FirstColour* first, double omega)
{
    constexpr bool fp64 = std::is_same<T, double>::value;
    if (!fp64 && ((!A.valf && !A.codes) || partials)) return hipErrorInvalidValue;
    switch (mode) {
#define SMG_SELL_CASE(M) \
        case M: \
            if constexpr (fp64 || !sell_fp64_only(M)) return launch_sell_mode<M, T>(A, s_begin, s_end, x, b, y, k, ctrl, partials, n_blocks, st, zero_rows, first, omega); \
            else return hipErrorInvalidValue;
        SMG_SELL_CASE(SELL_JACOBI) SMG_SELL_CASE(SELL_CHEBY) SMG_SELL_CASE(SELL_AX) SMG_SELL_CASE(SELL_RESID) SMG_SELL_CASE(SELL_RESID_SS)
        SMG_SELL_CASE(SELL_ADD) SMG_SELL_CASE(SELL_GS) SMG_SELL_CASE(SELL_RESID_BOTH) SMG_SELL_CASE(SELL_GS_OOP) SMG_SELL_CASE(SELL_GS_HEAD)
        SMG_SELL_CASE(SELL_JACOBI_HEAD) SMG_SELL_CASE(SELL_CHEBY_HEAD) SMG_SELL_CASE(SELL_GS_RES) SMG_SELL_CASE(SELL_GS_OOP_RES)
#undef SMG_SELL_CASE
    }
    return hipErrorInvalidValue;
}

hipError_t launch_sell(SellMode mode, const SellDev& A, int s_begin, int s_end, const double* x, const double* b,
                       double* y, int k, const Ctrl* ctrl, double* partials, int* n_blocks, hipStream_t st,
                       double* zero_rows, const FirstColour* first, double omega)
{
    return launch_sell_any<double>(mode, A, s_begin, s_end, x, b, y, k, ctrl, partials, n_blocks, st, zero_rows, first, omega);
}
hipError_t launch_sell(SellMode mode, const SellDev& A, int s_begin, int s_end, const float* x, const float* b,
                       float* y, int k, const Ctrl* ctrl, double* partials, int* n_blocks, hipStream_t st,
                       float* zero_rows, const FirstColour* first, double omega)
{
    return launch_sell_any<float>(mode, A, s_begin, s_end, x, b, y, k, ctrl, partials, n_blocks, st, zero_rows, first, omega);
}

// ---- Gershgorin bound of D^-1 A for the Chebyshev-Jacobi smoother: max over rows of (sum_j |a_ij|) / a_ii, the row sums accumulated in
// ascending column order (the order of the SELL panel), the maximum over rows through an integer atomic on the bit pattern (the values
// are positive: order-preserving, and a maximum does not depend on the order it is taken in: deterministic).  *out must be 0 on entry.
__global__ __launch_bounds__(256) void k_gershgorin(const int* a_col, const double* a_val, const int* a_slice_row, const int* a_slice_off, const int* a_slice_w,
                                                    int stride, int n_slices, unsigned long long* out)
{
    const int lane = threadIdx.x & 63, s = blockIdx.x * 4 + (threadIdx.x >> 6);
    double ratio = 0.0;
    if (s < n_slices) {
        const int row0 = a_slice_row[s], nrow = a_slice_row[s + 1] - row0, w = a_slice_w[s];
        const size_t off = (size_t)(stride ? s * stride : a_slice_off[s]) * 64 + lane;
        double sum = 0.0, diag = 0.0;
        for (int j = 0; j < w; j++) {
            const int c = a_col[off + (size_t)j * 64];
            const double v = a_val[off + (size_t)j * 64];
            if (c >= 0) { sum += fabs(v); if (c == row0 + lane) diag = v; }
        }
        if (lane < nrow && diag > 0.0) ratio = sum / diag;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) ratio = fmax(ratio, __shfl_down(ratio, o, 64));
    if (lane == 0 && ratio > 0.0) atomicMax(out, (unsigned long long)__double_as_longlong(ratio));
}
hipError_t launch_gershgorin(const SellDev& A, double* out, hipStream_t st)
{
    hipError_t e = hipMemsetAsync(out, 0, sizeof(double), st);
    if (e != hipSuccess || A.n_slices <= 0) return e;
    hipLaunchKernelGGL(k_gershgorin, dim3((A.n_slices + 3) / 4), dim3(256), 0, st, A.col, A.val, A.slice_row, A.slice_off, A.slice_w, A.stride, A.n_slices,
                       (unsigned long long*)out);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------- solve-loop control

__global__ __launch_bounds__(256) void k_ss_finalize(const double* partials, int n, Ctrl* ctrl, double* out)
{
    if (ctrl->done) return;
    __shared__ double red[256];
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) s += partials[i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) *out = red[0];
}

// single-GPU path: reduction of the partials and the break test in one launch
__global__ __launch_bounds__(256) void k_ss_finalize_decide(const double* partials, int n, Ctrl* ctrl)
{
    // a kernel that is nothing but latency: everything it will need -- the partial sums, the flag, the tolerance, the history
    // length -- is requested up front, in one round trip (same summation order as before)
    __shared__ double red[256];
    const int done = ctrl->done, n_his = ctrl->n_his, his_cap = ctrl->his_cap;
    const double tol = ctrl->tol;
    double* const r_his = ctrl->r_his;
    double s = 0.0;
#pragma unroll 8
    for (int i = threadIdx.x; i < n; i += 256) s += partials[i];
    if (done) return;   // uniform
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double sumsq = red[0], r = sqrt(sumsq);
        ctrl->sumsq = sumsq;
        if (n_his < his_cap) r_his[n_his] = r;
        ctrl->n_his = n_his + 1;
        ctrl->r_prev = ctrl->r_last; ctrl->r_last = r;
        if (!(r == r) || r > 1.7e308) { ctrl->status = -1; ctrl->done = 1; }  // NaN / Inf
        else if (r < tol) ctrl->done = 1;                                       // min_quad_with_fixed_mg.cpp:113-116
    }
}

__global__ void k_decide(Ctrl* ctrl, const double* sumsq)
{
    if (ctrl->done) return;
    decide_body(ctrl, *sumsq);
}

// Many partial sums (64 columns of a million rows leave 250 000 of them: one workgroup spent 40 us reading 2 MB): SS_STAGE_WGS workgroups first, each
// over a fixed contiguous share, into the SS_STAGE_WGS doubles behind the partials (the buffer has that room: ensure_work); the final kernel then sums
// those.  Fixed shares, fixed order inside a share: the same bits on every run and on every rank.
constexpr int SS_STAGE_MIN = 16384, SS_STAGE_WGS = 128;
__global__ __launch_bounds__(256) void k_ss_stage(const double* __restrict__ partials, int n, double* __restrict__ out, const int* done)
{
    if (load_flag(done)) return;
    __shared__ double red[256];
    const int per = (n + SS_STAGE_WGS - 1) / SS_STAGE_WGS;
    const int i0 = blockIdx.x * per, i1 = min(n, i0 + per);
    double s = 0.0;
#pragma unroll 8
    for (int i = i0 + (int)threadIdx.x; i < i1; i += 256) s += partials[i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[blockIdx.x] = red[0];
}
// returns where the (possibly staged) partial sums are and how many
static const double* ss_stage(const double* partials, int& n, const Ctrl* ctrl, hipStream_t st)
{
    if (n < SS_STAGE_MIN) return partials;
    double* out = const_cast<double*>(partials) + n;
    hipLaunchKernelGGL(k_ss_stage, dim3(SS_STAGE_WGS), dim3(256), 0, st, partials, n, out, &ctrl->done);
    n = SS_STAGE_WGS;
    return out;
}
int ss_partials_room() { return SS_STAGE_WGS; }

hipError_t launch_ss_finalize(const double* partials, int n, Ctrl* ctrl, hipStream_t st, double* out)
{
    partials = ss_stage(partials, n, ctrl, st);
    hipLaunchKernelGGL(k_ss_finalize, dim3(1), dim3(256), 0, st, partials, n, ctrl, out ? out : &ctrl->sumsq);
    return hipGetLastError();
}
// Speculative form (multi-GPU: the V-cycle of iteration i runs while the all-reduce of residual i is in flight).
// decide: like k_decide, and remembers in `just_done` that THIS decision ended the loop; restore then puts the saved
// iterate back, so the result is exactly what the non-speculative loop returns.
__global__ void k_decide_spec(Ctrl* ctrl, const double* sumsq)
{
    ctrl->just_done = 0;
    if (ctrl->done) return;
    decide_body(ctrl, *sumsq);
    if (ctrl->done) ctrl->just_done = 1;
}
__global__ void k_copy_unless_done(double* dst, const double* src, size_t n, const int* done)
{
    if (*done) return;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = src[i];
}
__global__ void k_restore_if_just_done(double* dst, const double* src, size_t n, const Ctrl* ctrl)
{
    if (!ctrl->just_done) return;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = src[i];
}
hipError_t launch_decide_spec(Ctrl* ctrl, const double* sumsq, hipStream_t st)
{
    hipLaunchKernelGGL(k_decide_spec, dim3(1), dim3(1), 0, st, ctrl, sumsq);
    return hipGetLastError();
}
hipError_t launch_copy_unless_done(double* dst, const double* src, size_t n, const Ctrl* ctrl, hipStream_t st)
{
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_copy_unless_done, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, dst, src, n, &ctrl->done);
    return hipGetLastError();
}
hipError_t launch_restore_if_just_done(double* dst, const double* src, size_t n, const Ctrl* ctrl, hipStream_t st)
{
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_restore_if_just_done, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, dst, src, n, ctrl);
    return hipGetLastError();
}
hipError_t launch_ss_finalize_decide(const double* partials, int n, Ctrl* ctrl, hipStream_t st)
{
    partials = ss_stage(partials, n, ctrl, st);
    hipLaunchKernelGGL(k_ss_finalize_decide, dim3(1), dim3(256), 0, st, partials, n, ctrl);
    return hipGetLastError();
}
hipError_t launch_decide(Ctrl* ctrl, const double* sumsq, hipStream_t st)
{
    hipLaunchKernelGGL(k_decide, dim3(1), dim3(1), 0, st, ctrl, sumsq);
    return hipGetLastError();
}
// ---------------------------------------------------------------------------------------------- coarsest level

// One wavefront per output row; 16 B per lane per load (1 KiB per wave-instruction); deterministic
// shuffle-tree reduction.  n and lda are multiples of 64, b has lda rows (zero padded).
template <typename T> struct Vec2;
template <> struct Vec2<double> { typedef double type __attribute__((ext_vector_type(2))); };
template <> struct Vec2<float> { typedef float type __attribute__((ext_vector_type(2))); };

template <int KB, typename T>
__global__ __launch_bounds__(256) void k_dense_gemv_add(const T* __restrict__ Ainv, int n, int lda,
                                                        const T* __restrict__ b, T* u, int ld, const int* done)
{
    const int stop = load_flag(done);   // consulted before the store only
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n) return;
    using T2 = typename Vec2<T>::type;
    const T2* a2 = reinterpret_cast<const T2*>(Ainv + (size_t)row * lda);
    T acc[KB];
#pragma unroll
    for (int q = 0; q < KB; q++) acc[q] = (T)0;
    const int n2 = lda >> 1;
#pragma unroll 4
    for (int jj = lane; jj < n2; jj += 64) {
        const T2 a = a2[jj];
#pragma unroll
        for (int q = 0; q < KB; q++) {
            acc[q] += a.x * b[(size_t)(2 * jj) * ld + q];
            acc[q] += a.y * b[(size_t)(2 * jj + 1) * ld + q];
        }
    }
#pragma unroll
    for (int q = 0; q < KB; q++) {
        T s = acc[q];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
        if (lane == 0 && !stop) u[(size_t)row * ld + q] = u[(size_t)row * ld + q] + s;
    }
}

// k >= 16 columns: LDS-tiled GEMM  u[16-row tile, KC cols] += Ainv[tile, :] * b[:, KC cols].  256 threads = 16 rows x 16
// column groups of KC/16 columns; j is walked in tiles of 32 through LDS.  Per (row, column) the sum is sequential in j.
// (fp64 FMA-free multiply-add on the vector ALU; an f64 MFMA would fuse and change rounding.)
template <int KC, typename T>
__global__ __launch_bounds__(256) void k_dense_gemm_tile(const T* __restrict__ Ainv, int n, int lda,
                                                         const T* __restrict__ b, T* u, int ld, const int* done)
{
    constexpr int TR = 16, TJ = 64, CT = KC / 16;
    constexpr int NA = TR * TJ / 256, NB = TJ * KC / 256;  // staged elements per thread
    __shared__ T a_s[TR][TJ + 1];
    __shared__ T b_s[TJ][KC];
    const int stop = load_flag(done);
    const int t = threadIdx.x, tr = t / 16, tc = t % 16;
    const int i0 = blockIdx.x * TR;
    T acc[CT];
#pragma unroll
    for (int q = 0; q < CT; q++) acc[q] = (T)0;
    T ra[NA], rb[NB];  // next tile, prefetched into registers while the current one is consumed from LDS
    auto fetch = [&](int j0) {
#pragma unroll
        for (int e = 0; e < NA; e++) {
            const int idx = t + 256 * e, r = idx / TJ, jj = idx % TJ, row = i0 + r;
            ra[e] = row < n ? Ainv[(size_t)row * lda + j0 + jj] : (T)0;
        }
#pragma unroll
        for (int e = 0; e < NB; e++) {
            const int idx = t + 256 * e, jj = idx / KC, cc = idx % KC;
            rb[e] = b[(size_t)(j0 + jj) * ld + cc];
        }
    };
    fetch(0);
    for (int j0 = 0; j0 < lda; j0 += TJ) {
#pragma unroll
        for (int e = 0; e < NA; e++) { const int idx = t + 256 * e; a_s[idx / TJ][idx % TJ] = ra[e]; }
#pragma unroll
        for (int e = 0; e < NB; e++) { const int idx = t + 256 * e; b_s[idx / KC][idx % KC] = rb[e]; }
        __syncthreads();
        if (j0 + TJ < lda) fetch(j0 + TJ);
#pragma unroll 8
        for (int jj = 0; jj < TJ; jj++) {
            const T a = a_s[tr][jj];
#pragma unroll
            for (int q = 0; q < CT; q++) acc[q] += a * b_s[jj][tc * CT + q];
        }
        __syncthreads();
    }
    const int row = i0 + tr;
    if (row < n && !stop)
#pragma unroll
        for (int q = 0; q < CT; q++) u[(size_t)row * ld + tc * CT + q] = u[(size_t)row * ld + tc * CT + q] + acc[q];
}

// k >= 16 columns, fp64: the same product on the fp64 matrix cores.  One workgroup per 16 x 16 tile of u (grid: row blocks x
// column blocks: 4 x the workgroups of the LDS-tiled kernel above, whose n / 16 workgroups left two thirds of the CUs idle and made the
// coarse solve 40 % of a 64-column cycle on ogre.obj: 113 -> 9 us), the four waves of a workgroup each walk a quarter of the inner index
// in steps of 4 (v_mfma_f64_16x16x4_f64), their partial tiles are summed through LDS in a fixed order (deterministic).  The inverse is
// symmetric (k_mirror_lower), so the A operand A[i][j] is read as Ainv[j][i]: 16 consecutive doubles per j -- both operands are
// 128-byte segments, no staging.  Loads run DEPTH steps ahead of the products (at most one workgroup per CU: occupancy hides nothing).
// The coarse solve is compared with LDL^T to 1e-11, not bit for bit: the fused multiply-adds of the matrix cores are fine here.
typedef double v4f64_t __attribute__((ext_vector_type(4)));
template <int KC>
__global__ __launch_bounds__(256) void k_dense_gemm_mfma(const double* __restrict__ Ainv, int n, int lda, const double* __restrict__ b,
                                                         double* u, int ld, const int* done, int kvalid)
{
    const int stop = load_flag(done);
    constexpr int CB = KC / 16, DEPTH = 12;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int rb = blockIdx.x / CB, cb = blockIdx.x % CB;
    const int row0 = rb * 16, col0 = cb * 16;
    const int lc = lane & 15, lr = lane >> 4;
    const int per = lda / 16;                 // MFMA steps per wave (lda % 64 == 0)
    const int s0 = per * w;
    const double* pa = Ainv + (size_t)(4 * s0 + lr) * lda + row0 + lc;
    const bool colok = col0 + lc < kvalid;    // a block of 8..15 columns runs as a 16-column tile with the excess lanes idle
    const double* pb = b + (size_t)(4 * s0 + lr) * ld + col0 + (colok ? lc : 0);
    const size_t sa = (size_t)4 * lda, sb = (size_t)4 * ld;
    v4f64_t acc = {0.0, 0.0, 0.0, 0.0};
    double av[DEPTH], bv[DEPTH];
#pragma unroll
    for (int t = 0; t < DEPTH; t++) {
        av[t] = t < per ? pa[t * sa] : 0.0;
        bv[t] = (t < per && colok) ? pb[t * sb] : 0.0;
    }
    for (int s = 0; s < per; s += DEPTH) {
        double an[DEPTH], bn[DEPTH];
#pragma unroll
        for (int t = 0; t < DEPTH; t++) {
            const int q = s + DEPTH + t;
            an[t] = q < per ? pa[q * sa] : 0.0;
            bn[t] = (q < per && colok) ? pb[q * sb] : 0.0;
        }
#pragma unroll
        for (int t = 0; t < DEPTH; t++) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av[t], bv[t], acc, 0, 0, 0);   // zero operands past the end
#pragma unroll
        for (int t = 0; t < DEPTH; t++) { av[t] = an[t]; bv[t] = bn[t]; }
    }
    __shared__ double red[4][4][64];
#pragma unroll
    for (int r = 0; r < 4; r++) red[w][r][lane] = acc[r];
    __syncthreads();
    if (w == 0 && !stop) {
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int row = row0 + lr + 4 * r;      // C/D layout: register r of lane -> row (lane >> 4) + 4 r, column lane & 15
            if (row < n && colok) {
                const size_t o = (size_t)row * ld + col0 + lc;
                u[o] = u[o] + ((red[0][r][lane] + red[1][r][lane]) + (red[2][r][lane] + red[3][r][lane]));
            }
        }
    }
}

// The same product with CPW column tiles per workgroup: a wave's operand of the inverse feeds CPW matrix-core products instead of one, so
// the inverse is streamed KC / (16 CPW) times instead of KC / 16 times (at 64 columns and CPW = 1 the launch re-reads 125 MB four times:
// 92 us of a 4.3 ms iteration at C3 x 64; CPW = 2: 75 us).  Same inner ranges per wave, same order of the products, same final sum: the same bits.
template <int KC, int CPW>
__global__ __launch_bounds__(256) void k_dense_gemm_mfma_multi(const double* __restrict__ Ainv, int n, int lda, const double* __restrict__ b,
                                                               double* u, int ld, const int* done, int kvalid)
{
    const int stop = load_flag(done);
    constexpr int CB = KC / 16 / CPW, DEPTH = 6;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int rb = blockIdx.x / CB, cb = blockIdx.x % CB;
    const int row0 = rb * 16, col0 = cb * 16 * CPW;
    const int lc = lane & 15, lr = lane >> 4;
    const int per = lda / 16;                 // MFMA steps per wave (lda % 64 == 0)
    const int s0 = per * w;
    const double* pa = Ainv + (size_t)(4 * s0 + lr) * lda + row0 + lc;
    const double* pb = b + (size_t)(4 * s0 + lr) * ld + col0 + lc;
    const size_t sa = (size_t)4 * lda, sb = (size_t)4 * ld;
    v4f64_t acc[CPW];
#pragma unroll
    for (int c = 0; c < CPW; c++) acc[c] = (v4f64_t){0.0, 0.0, 0.0, 0.0};
    double av[DEPTH], bv[CPW][DEPTH];
#pragma unroll
    for (int t = 0; t < DEPTH; t++) {
        av[t] = t < per ? pa[t * sa] : 0.0;
#pragma unroll
        for (int c = 0; c < CPW; c++) bv[c][t] = (t < per && col0 + 16 * c + lc < kvalid) ? pb[t * sb + 16 * c] : 0.0;
    }
    for (int s = 0; s < per; s += DEPTH) {
        double an[DEPTH], bn[CPW][DEPTH];
#pragma unroll
        for (int t = 0; t < DEPTH; t++) {
            const int q = s + DEPTH + t;
            an[t] = q < per ? pa[q * sa] : 0.0;
#pragma unroll
            for (int c = 0; c < CPW; c++) bn[c][t] = (q < per && col0 + 16 * c + lc < kvalid) ? pb[q * sb + 16 * c] : 0.0;
        }
#pragma unroll
        for (int t = 0; t < DEPTH; t++)
#pragma unroll
            for (int c = 0; c < CPW; c++) acc[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[t], bv[c][t], acc[c], 0, 0, 0);   // zero operands past the end
#pragma unroll
        for (int t = 0; t < DEPTH; t++) {
            av[t] = an[t];
#pragma unroll
            for (int c = 0; c < CPW; c++) bv[c][t] = bn[c][t];
        }
    }
    __shared__ double red[CPW][4][4][64];
#pragma unroll
    for (int c = 0; c < CPW; c++)
#pragma unroll
        for (int r = 0; r < 4; r++) red[c][w][r][lane] = acc[c][r];
    __syncthreads();
    if (!stop) {
        for (int c = w; c < CPW; c += 4) {       // wave c finishes column tile c
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int row = row0 + lr + 4 * r;
                if (row < n && col0 + 16 * c + lc < kvalid) {
                    const size_t o = (size_t)row * ld + col0 + 16 * c + lc;
                    u[o] = u[o] + ((red[c][0][r][lane] + red[c][1][r][lane]) + (red[c][2][r][lane] + red[c][3][r][lane]));
                }
            }
        }
    }
}

// ---- k = 1, symmetric: the inverse of an SPD matrix is symmetric, so one column's product needs only the lower triangle of
// tiles -- half the bytes of the (bandwidth-bound) coarse solve.  Tile (I, J), I >= J, yields A_IJ b_J (a share of y_I) and, off the
// diagonal, A_IJ^T b_I (a share of y_J); the 64-row shares are summed per row in ascending block order by a second small launch:
// deterministic, independent of scheduling.  (The two halves of the stored inverse agree to rounding; using the lower one for
// both is the same operator to 1e-16.)
template <typename T>
__global__ __launch_bounds__(256) void k_sym_gemv_tiles(const T* __restrict__ Ainv, int lda, const T* __restrict__ b, T* __restrict__ part, int nb)
{
    // blockIdx.x enumerates the lower triangle row by row: idx = I (I + 1) / 2 + J
    const int idx = blockIdx.x;
    int I = (int)((sqrtf(8.0f * (float)idx + 1.0f) - 1.0f) * 0.5f);
    I -= (I * (I + 1) / 2 > idx);
    I += ((I + 1) * (I + 2) / 2 <= idx);
    const int J = idx - I * (I + 1) / 2;
    __shared__ T tile[64][65];
    __shared__ T bI[64], bJ[64];
    const int t = threadIdx.x;
#pragma unroll
    for (int e = 0; e < 16; e++) {
        const int idx = e * 256 + t, r = idx >> 6, c = idx & 63;
        tile[r][c] = Ainv[(size_t)(I * 64 + r) * lda + J * 64 + c];
    }
    if (t < 64) bJ[t] = b[J * 64 + t];
    else if (t < 128) bI[t - 64] = b[I * 64 + t - 64];
    __syncthreads();
    // waves 0/1: rows of the tile against b_J (columns 0..31 / 32..63); waves 2/3: columns of the tile against b_I (rows 0..31 / 32..63)
    __shared__ T red[4][64];
    const int g = t >> 6, l = t & 63, h0 = (g & 1) * 32;
    T s = (T)0;
    if (g < 2) {
#pragma unroll 8
        for (int c = h0; c < h0 + 32; c++) s += tile[l][c] * bJ[c];
    } else {
#pragma unroll 8
        for (int r = h0; r < h0 + 32; r++) s += tile[r][l] * bI[r];
    }
    red[g][l] = s;
    __syncthreads();
    if (t < 64) part[((size_t)I * nb + J) * 64 + t] = red[0][t] + red[1][t];
    else if (t < 128 && I != J) part[((size_t)J * nb + I) * 64 + (t - 64)] = red[2][t - 64] + red[3][t - 64];
}
// one workgroup per 64-row block: four waves sum a quarter of the block shares each (ascending), combined in a fixed order
template <typename T>
__global__ __launch_bounds__(256) void k_sym_gemv_sum(const T* __restrict__ part, int nb, int n, T* u, const int* done)
{
    const int stop = load_flag(done);
    __shared__ T red[4][64];
    const int a = blockIdx.x, g = threadIdx.x >> 6, l = threadIdx.x & 63;
    const int q = (nb + 3) / 4, b0 = g * q, b1 = min(nb, b0 + q);
    T s = (T)0;
#pragma unroll 8
    for (int bidx = b0; bidx < b1; bidx++) s += part[((size_t)a * nb + bidx) * 64 + l];
    red[g][l] = s;
    __syncthreads();
    const int i = a * 64 + l;
    if (g == 0 && i < n && !stop) u[i] = u[i] + ((red[0][l] + red[1][l]) + (red[2][l] + red[3][l]));
}

template <typename T>
// k columns of the row-major n x ld blocks b, u (ld >= k: the solve pads its blocks to kernel-friendly row lengths, the product is formed for the caller's columns only)
static hipError_t launch_dense_T(const T* Ainv, int n, int lda, const T* b, T* u, int k, int ld, const Ctrl* ctrl, hipStream_t st, void* sym_work)
{
    const int* done = ctrl ? &ctrl->done : never_done();
    const int nb = (n + 3) / 4;
    if (n <= 0) return hipSuccess;
    if (k == 1 && ld == 1 && sym_work && lda % 64 == 0 && lda >= 512) {
        const int nt = lda / 64;
        hipLaunchKernelGGL((k_sym_gemv_tiles<T>), dim3(nt * (nt + 1) / 2), dim3(256), 0, st, Ainv, lda, b, (T*)sym_work, nt);
        hipLaunchKernelGGL((k_sym_gemv_sum<T>), dim3(nt), dim3(256), 0, st, (const T*)sym_work, nt, n, u, done);
        return hipGetLastError();
    }
    int c0 = 0;
    static const int use_mfma8 = getenv("SMG_COARSE_MFMA") ? atoi(getenv("SMG_COARSE_MFMA")) : 1;
    const int mfma_min = (std::is_same<T, double>::value && use_mfma8 && lda % 64 == 0) ? 8 : 16;   // 8..15 columns: one padded 16-column tile
    while (k - c0 >= mfma_min) {
        int kc = 64;
        while (kc > k - c0 && kc > 16) kc >>= 1;
        const int kv = kc < k - c0 ? kc : k - c0;   // valid columns of this block (< kc only for the padded 16-column tile)
        const int tb = (n + 15) / 16;
        static const int use_mfma = getenv("SMG_COARSE_MFMA") ? atoi(getenv("SMG_COARSE_MFMA")) : 1;   // A/B knob
        if constexpr (std::is_same<T, double>::value) {
            if (use_mfma && lda % 64 == 0) {
                // 64 columns: two column tiles per workgroup (92 -> 75 us at 3 952 unknowns, same bits; four: too few workgroups, 91 us; two tiles at 32
                // columns: 54 -> 63 us).  SMG_COARSE_CPW=1 is the A/B knob.
                static const int cpw = getenv("SMG_COARSE_CPW") ? atoi(getenv("SMG_COARSE_CPW")) : 2;
                if (kc == 64 && cpw == 2) { hipLaunchKernelGGL((k_dense_gemm_mfma_multi<64, 2>), dim3(tb * 2), dim3(256), 0, st, Ainv, n, lda, b + c0, u + c0, ld, done, kv); c0 += kv; continue; }
                switch (kc) {
                    case 64: hipLaunchKernelGGL((k_dense_gemm_mfma<64>), dim3(tb * 4), dim3(256), 0, st, Ainv, n, lda, b + c0, u + c0, ld, done, kv); break;
                    case 32: hipLaunchKernelGGL((k_dense_gemm_mfma<32>), dim3(tb * 2), dim3(256), 0, st, Ainv, n, lda, b + c0, u + c0, ld, done, kv); break;
                    default: hipLaunchKernelGGL((k_dense_gemm_mfma<16>), dim3(tb), dim3(256), 0, st, Ainv, n, lda, b + c0, u + c0, ld, done, kv); break;
                }
                c0 += kv;
                continue;
            }
        }
        switch (kc) {
            case 64: hipLaunchKernelGGL((k_dense_gemm_tile<64, T>), dim3(tb), dim3(256), 0, st, Ainv, n, lda, b + c0, u + c0, ld, done); break;
            case 32: hipLaunchKernelGGL((k_dense_gemm_tile<32, T>), dim3(tb), dim3(256), 0, st, Ainv, n, lda, b + c0, u + c0, ld, done); break;
            default: hipLaunchKernelGGL((k_dense_gemm_tile<16, T>), dim3(tb), dim3(256), 0, st, Ainv, n, lda, b + c0, u + c0, ld, done); break;
        }
        c0 += kc;
    }
    for (; c0 < k; c0 += 4) {
        const int kb = (k - c0) < 4 ? (k - c0) : 4;
        switch (kb) {
            case 1: hipLaunchKernelGGL((k_dense_gemv_add<1, T>), dim3(nb), dim3(256), 0, st, Ainv, n, lda, b + c0, u + c0, ld, done); break;
            case 2: hipLaunchKernelGGL((k_dense_gemv_add<2, T>), dim3(nb), dim3(256), 0, st, Ainv, n, lda, b + c0, u + c0, ld, done); break;
            case 3: hipLaunchKernelGGL((k_dense_gemv_add<3, T>), dim3(nb), dim3(256), 0, st, Ainv, n, lda, b + c0, u + c0, ld, done); break;
            default: hipLaunchKernelGGL((k_dense_gemv_add<4, T>), dim3(nb), dim3(256), 0, st, Ainv, n, lda, b + c0, u + c0, ld, done); break;
        }
    }
    return hipGetLastError();
}
template <typename T>
static hipError_t launch_sym_tiles_T(const T* Ainv, int lda, const T* b, T* part, hipStream_t st)
{
    if (lda <= 0 || lda % 64) return hipErrorInvalidValue;
    const int nt = lda / 64;
    hipLaunchKernelGGL((k_sym_gemv_tiles<T>), dim3(nt * (nt + 1) / 2), dim3(256), 0, st, Ainv, lda, b, part, nt);
    return hipGetLastError();
}
hipError_t launch_sym_gemv_tiles(const double* Ainv, int lda, const double* b, double* part, hipStream_t st) { return launch_sym_tiles_T<double>(Ainv, lda, b, part, st); }
hipError_t launch_sym_gemv_tiles(const float* Ainv, int lda, const float* b, float* part, hipStream_t st) { return launch_sym_tiles_T<float>(Ainv, lda, b, part, st); }
hipError_t launch_dense_gemv_add(const double* Ainv, int n, int lda, const double* b, double* u, int k, int ld,
                                 const Ctrl* ctrl, hipStream_t st, double* sym_work)
{
    return launch_dense_T<double>(Ainv, n, lda, b, u, k, ld, ctrl, st, sym_work);
}
hipError_t launch_dense_gemv_add(const float* Ainv, int n, int lda, const float* b, float* u, int k, int ld,
                                 const Ctrl* ctrl, hipStream_t st, float* sym_work)
{
    return launch_dense_T<float>(Ainv, n, lda, b, u, k, ld, ctrl, st, sym_work);
}

// ---- mixed precision glue: fp64 outer iterate / residual  <->  fp32 V-cycle ----------------------------------------
__global__ void k_cvt_f64_f32(float* dst, const double* src, size_t n)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = (float)src[i];
}
// b32 = (float) r64 ; u32 = 0        (right-hand side and zero initial guess of the correction equation)
__global__ void k_residual_to_f32(float* b32, float* u32, const double* r64, size_t n, const int* done)
{
    if (done && *done) return;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) { b32[i] = (float)r64[i]; u32[i] = 0.0f; }
}
// z64 += (double) e32
__global__ void k_add_correction(double* z, const float* e, size_t n, const int* done)
{
    if (done && *done) return;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) z[i] = z[i] + (double)e[i];
}
hipError_t launch_cvt_f64_f32(float* dst, const double* src, size_t n, hipStream_t st)
{
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_cvt_f64_f32, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, dst, src, n);
    return hipGetLastError();
}
hipError_t launch_residual_to_f32(float* b32, float* u32, const double* r64, size_t n, const Ctrl* ctrl, hipStream_t st)
{
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_residual_to_f32, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, b32, u32, r64, n, ctrl ? &ctrl->done : nullptr);
    return hipGetLastError();
}
hipError_t launch_add_correction(double* z, const float* e, size_t n, const Ctrl* ctrl, hipStream_t st)
{
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_add_correction, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, z, e, n, ctrl ? &ctrl->done : nullptr);
    return hipGetLastError();
}

// Blocked Gauss-Jordan inversion (no pivoting; the matrix is SPD), block size 64, 64x64 update tiles.  Every step streams
// the whole matrix once (read + write), so the block size is the number of passes: 64 halves the traffic of 32; the update
// walks the 64 pivot columns in two halves of 32 to stay inside 64 KB of LDS.
constexpr int GJ_H = 32;   // sub-panel width staged through LDS

// inverse of the first 64 x 64 pivot block (the later ones are inverted by the look-ahead of k_gj_update)
__global__ __launch_bounds__(256) void k_gj_diag(const double* M, int n, int kb, double* dinv)
{
    __shared__ double a[GJ_NB][GJ_NB + 1];
    __shared__ double Rb[16][GJ_NB + 1];
    __shared__ double Cb[GJ_NB][17];
    const int K = kb * GJ_NB;
    for (int e = threadIdx.x; e < GJ_NB * GJ_NB; e += 256) a[e / GJ_NB][e % GJ_NB] = M[(size_t)(K + e / GJ_NB) * n + K + e % GJ_NB];
    __syncthreads();
    gj_invert64(a, Rb, Cb);
    for (int e = threadIdx.x; e < GJ_NB * GJ_NB; e += 256) dinv[e] = a[e / GJ_NB][e % GJ_NB];
}

// Only the lower triangle of tiles is kept up to date (the iterates of Gauss-Jordan on a symmetric matrix are symmetric up to the
// sign of the blocks that couple an already inverted block with one still to come), which halves the traffic and the flops of
// every step; SimplicialLDLT reads the lower triangle only, too.  With pivot block K (tile index kb):
//   column panel  C_I = M[I,K]  = stored tile (I,K) for I > K,   = -(stored tile (K,I))^T for I < K  (I already inverted)
//   row panel     R_J = D^-1 M[K,J],  M[K,J] = stored tile (K,J) for J < K,  = (stored tile (J,K))^T for J > K
// so one source tile per 64 indices feeds both panels.  Block x handles indices [32x, 32x+32).
__global__ __launch_bounds__(256) void k_gj_panels(const double* M, int n, int kb, const double* dinv, double* rowp,
                                                   double* colp)
{
    __shared__ double m_s[GJ_NB][GJ_H + 1];   // m_s[r][c] = M[K + r][j0 + c] (as a full symmetric-iterate matrix would hold it)
    const int K = kb * GJ_NB;
    const int j0 = blockIdx.x * GJ_H;
    const int J = j0 / GJ_NB;
    const int t = threadIdx.x;
    if (J == kb) {   // the pivot columns of the row panel hold D^-1 itself
        for (int e = t; e < GJ_NB * GJ_H; e += 256) {
            const int r = e / GJ_H, c = e % GJ_H;
            rowp[(size_t)r * n + j0 + c] = dinv[r * GJ_NB + j0 + c - K];
        }
        return;
    }
    // all loads of the block are requested up front: the A operands (rows 16 w .. 16 w + 15 of D^-1, straight from L2 into the
    // MFMA operand registers) and the 64 x 32 slab (transposed through LDS when it comes from the column side)
    const int lane = t & 63, w = t >> 6, lr = lane >> 4, lc = lane & 15;
    double av[GJ_NB / 4], mr[8];
#pragma unroll
    for (int q = 0; q < GJ_NB / 4; q++) av[q] = dinv[(16 * w + lc) * GJ_NB + 4 * q + lr];
    if (J < kb) {
#pragma unroll
        for (int e = 0; e < 8; e++) { const int x = t + 256 * e; mr[e] = M[(size_t)(K + x / GJ_H) * n + j0 + x % GJ_H]; }
#pragma unroll
        for (int e = 0; e < 8; e++) { const int x = t + 256 * e; m_s[x / GJ_H][x % GJ_H] = mr[e]; }
    } else {
#pragma unroll
        for (int e = 0; e < 8; e++) { const int x = t + 256 * e; mr[e] = M[(size_t)(j0 + x / GJ_NB) * n + K + x % GJ_NB]; }
#pragma unroll
        for (int e = 0; e < 8; e++) { const int x = t + 256 * e; m_s[x % GJ_NB][x / GJ_NB] = mr[e]; }
    }
    __syncthreads();
    {
        const double sgn = J < kb ? -1.0 : 1.0;
#pragma unroll
        for (int e = 0; e < 8; e++) {
            const int x = t + 256 * e, c = x / GJ_NB, r = x % GJ_NB;
            colp[(size_t)(j0 + c) * GJ_NB + r] = sgn * m_s[r][c];
        }
    }
    // D^-1 (64 x 64) times the 64 x 32 slab on the matrix cores: wave w -> rows 16 w .. 16 w + 15, two 16 x 16 tiles
    v4f64 acc[2] = {(v4f64){0.0, 0.0, 0.0, 0.0}, (v4f64){0.0, 0.0, 0.0, 0.0}};
#pragma unroll
    for (int q = 0; q < GJ_NB / 4; q++) {
#pragma unroll
        for (int ct = 0; ct < 2; ct++) acc[ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[q], m_s[4 * q + lr][16 * ct + lc], acc[ct], 0, 0, 0);
    }
#pragma unroll
    for (int ct = 0; ct < 2; ct++)
#pragma unroll
        for (int r = 0; r < 4; r++) rowp[(size_t)(16 * w + lr + 4 * r) * n + j0 + 16 * ct + lc] = acc[ct][r];
}

// Trailing update  M -= colp (n x 64) * rowp (64 x n)  on the fp64 matrix cores: the one GEMM-shaped piece of the library.
// A workgroup owns a 64 x 64 tile, wave w its rows [16 w, 16 w + 16) as four 16 x 16 MFMA tiles; K = 64 is walked in 16 steps of
// v_mfma_f64_16x16x4_f64 (A: lane -> A[lane & 15][lane >> 4], B: lane -> B[lane >> 4][lane & 15], C/D: register r of lane ->
// row (lane >> 4) + 4 r, column lane & 15).  Operands come straight from the two panels (L1/L2-resident: 2 MB each); the matrix
// itself is read and written once per step, which is what bounds the step.  The result is compared with LDL^T to 1e-11, not
// bit for bit, so the fused multiply-adds are fine here.
// (a 128 x 64 tile per workgroup, one B operand feeding two MFMA tiles, measured slower: 9.1 vs 8.5 ms per inversion)
// Look-ahead: the workgroup that updates the NEXT pivot block (it is dispatched first: block (0,0) trades tiles with it) goes on
// to invert that block and leaves the result in dinv_next, so the pivot-block inversion does not run alone between the
// steps but in the shadow of this kernel.  (1024-thread workgroups of four tiles measured slower: 55 vs 43 us per step.)
__global__ __launch_bounds__(256) void k_gj_update(double* M, int n, int kb, const double* __restrict__ rowp, const double* __restrict__ colp,
                                                    double* dinv_next)
{
    __shared__ double a[GJ_NB][GJ_NB + 1];
    __shared__ double Rb[16][GJ_NB + 1];
    __shared__ double Cb[GJ_NB][17];
    const int K = kb * GJ_NB;
    const int nb = n / 64, nxt = kb + 1;                  // tile index of the next pivot block (none after the last step)
    // one workgroup per tile of the lower triangle, enumerated row by row: idx = by (by + 1) / 2 + bx, bx <= by
    int idx = blockIdx.x;
    if (nxt < nb) {                                       // tile (0,0) trades places with tile (nxt, nxt): that one is dispatched first
        const int inx = nxt * (nxt + 1) / 2 + nxt;
        if (idx == 0) idx = inx;
        else if (idx == inx) idx = 0;
    }
    int by = (int)((sqrtf(8.0f * (float)idx + 1.0f) - 1.0f) * 0.5f);
    by -= (by * (by + 1) / 2 > idx);
    by += ((by + 1) * (by + 2) / 2 <= idx);
    const int bx = idx - by * (by + 1) / 2;
    const bool lookahead = (nxt < nb) && blockIdx.x == 0; // uniform per workgroup: this one goes on to invert the next pivot block
    const int i0 = by * 64, j0 = bx * 64;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lr = lane >> 4, lc = lane & 15;
    if (by == kb) {   // the pivot rows take the scaled row panel (64-row tiles never straddle the pivot block)
#pragma unroll
        for (int c = 0; c < 4; c++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int i = i0 + 16 * wave + lr + 4 * r, j = j0 + 16 * c + lc;
                M[(size_t)i * n + j] = rowp[(size_t)(i - K) * n + j];
            }
    } else {
        const bool jpiv = bx == kb;
        double* mp = M + (size_t)(i0 + 16 * wave + lr) * n + j0 + lc;
        v4f64 old[4];                                     // the tile's old values: requested before the panel operands
#pragma unroll
        for (int c = 0; c < 4; c++)
#pragma unroll
            for (int r = 0; r < 4; r++) old[c][r] = jpiv ? 0.0 : mp[(size_t)(4 * r) * n + 16 * c];
        // operands: this wave's 16 rows of the column panel straight into registers; the 64 x 64 slab of the row panel, which all
        // four waves need, once through LDS (`a` is free until the look-ahead writes its results into it)
        double av[GJ_NB / 4];
        const double* ap = colp + (size_t)(i0 + 16 * wave + lc) * GJ_NB + lr;
#pragma unroll
        for (int s = 0; s < GJ_NB / 4; s++) av[s] = ap[4 * s];
        {
            double br[16];
#pragma unroll
            for (int e = 0; e < 16; e++) { const int x = threadIdx.x + 256 * e; br[e] = rowp[(size_t)(x >> 6) * n + j0 + (x & 63)]; }
#pragma unroll
            for (int e = 0; e < 16; e++) { const int x = threadIdx.x + 256 * e; a[x >> 6][x & 63] = br[e]; }
        }
        __syncthreads();   // workgroup-uniform branch
        v4f64 acc[4];
#pragma unroll
        for (int c = 0; c < 4; c++) acc[c] = (v4f64){0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int s = 0; s < GJ_NB / 4; s++) {
#pragma unroll
            for (int c = 0; c < 4; c++) acc[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[s], a[4 * s + lr][16 * c + lc], acc[c], 0, 0, 0);
        }
        if (lookahead) __syncthreads();   // every wave is done with the slab before the results overwrite it
#pragma unroll
        for (int c = 0; c < 4; c++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const double v = old[c][r] - acc[c][r];
                mp[(size_t)(4 * r) * n + 16 * c] = v;
                if (lookahead) a[16 * wave + lr + 4 * r][16 * c + lc] = v;
            }
    }
    if (!lookahead) return;
    // invert the freshly updated next pivot block with the whole workgroup
    __syncthreads();
    gj_invert64(a, Rb, Cb);
    for (int e = threadIdx.x; e < GJ_NB * GJ_NB; e += 256) dinv_next[e] = a[e / GJ_NB][e % GJ_NB];
}

// upper triangle of tiles <- transpose of the lower one (the multi-column coarse solves read whole rows)
__global__ __launch_bounds__(256) void k_mirror_lower(double* M, int n)
{
    __shared__ double a[64][65];
    const int idx = blockIdx.x;                            // strictly lower tiles: idx = I (I - 1) / 2 + J, J < I
    int I = (int)((sqrtf(8.0f * (float)idx + 1.0f) + 1.0f) * 0.5f);
    I -= (I * (I - 1) / 2 > idx);
    I += ((I + 1) * I / 2 <= idx);
    const int J = idx - I * (I - 1) / 2;
    const int t = threadIdx.x;
#pragma unroll
    for (int e = 0; e < 16; e++) {
        const int q = e * 256 + t, r = q >> 6, c = q & 63;
        a[r][c] = M[(size_t)(I * 64 + r) * n + J * 64 + c];
    }
    __syncthreads();
#pragma unroll
    for (int e = 0; e < 16; e++) {
        const int q = e * 256 + t, r = q >> 6, c = q & 63;
        M[(size_t)(J * 64 + r) * n + I * 64 + c] = a[c][r];
    }
}

// The same update with the operands shared: a workgroup owns a block of GJ_R x 2 tiles (what of it lies in the lower triangle).  A tile costs
// three 32 KB loads as its own workgroup -- its old values, 64 rows of the column panel, a 64-column slab of the row panel -- and at 4.6 - 4.7 TB/s
// of such loads the update is bound by re-reading the panels, not by the matrix cores (a third busy).  Here the 128-column slab is staged in LDS once
// for the block and a tile row's column-panel operand is loaded once for its two tiles: 64 KB per tile instead of 96.
// Workgroup 0 (while a next pivot block exists) is the look-ahead: it updates that block alone and inverts it, as in k_gj_update.
constexpr int GJ_P2 = 2 * GJ_NB + 1;      // pitch of the 128-column slab
// GJ_R tile rows x 2 tile columns per workgroup: 2 for matrices of a few thousand rows (4: too few workgroups there, 3.2 -> 3.6 ms at 3 952), 4 from
// 8 192 rows on (55.4 -> 53.7 ms at 11 856)
static int gj_update2_blocks(int nt, int R)
{
    int w = 0;
    for (int BY = 0; R * BY < nt; BY++) { const int last = R * BY + R - 1 < nt - 1 ? R * BY + R - 1 : nt - 1; w += last / 2 + 1; }
    return w;
}
template <int GJ_R>
__global__ __launch_bounds__(256) void k_gj_update2(double* M, int n, int kb, const double* __restrict__ rowp, const double* __restrict__ colp,
                                                     double* dinv_next)
{
    __shared__ double lds[GJ_NB * GJ_P2];
    const int K = kb * GJ_NB;
    const int nb = n / 64, nxt = kb + 1;
    const bool have_la = nxt < nb;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lr = lane >> 4, lc = lane & 15;
    if (have_la && blockIdx.x == 0) {
        // ---- look-ahead: tile (nxt, nxt), then its inverse (a | Rb | Cb carved out of the slab's space)
        double (*a)[GJ_NB + 1] = reinterpret_cast<double (*)[GJ_NB + 1]>(lds);
        double (*Rb)[GJ_NB + 1] = reinterpret_cast<double (*)[GJ_NB + 1]>(lds + GJ_NB * (GJ_NB + 1));
        double (*Cb)[17] = reinterpret_cast<double (*)[17]>(lds + GJ_NB * (GJ_NB + 1) + 16 * (GJ_NB + 1));
        const int i0 = nxt * 64, j0 = nxt * 64;
        double* mp = M + (size_t)(i0 + 16 * wave + lr) * n + j0 + lc;
        v4f64 old[4];
#pragma unroll
        for (int c = 0; c < 4; c++)
#pragma unroll
            for (int r = 0; r < 4; r++) old[c][r] = mp[(size_t)(4 * r) * n + 16 * c];
        double av[GJ_NB / 4];
        const double* ap = colp + (size_t)(i0 + 16 * wave + lc) * GJ_NB + lr;
#pragma unroll
        for (int s = 0; s < GJ_NB / 4; s++) av[s] = ap[4 * s];
        {
            double br[16];
#pragma unroll
            for (int e = 0; e < 16; e++) { const int x = threadIdx.x + 256 * e; br[e] = rowp[(size_t)(x >> 6) * n + j0 + (x & 63)]; }
#pragma unroll
            for (int e = 0; e < 16; e++) { const int x = threadIdx.x + 256 * e; a[x >> 6][x & 63] = br[e]; }
        }
        __syncthreads();
        v4f64 acc[4];
#pragma unroll
        for (int c = 0; c < 4; c++) acc[c] = (v4f64){0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int s = 0; s < GJ_NB / 4; s++) {
#pragma unroll
            for (int c = 0; c < 4; c++) acc[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[s], a[4 * s + lr][16 * c + lc], acc[c], 0, 0, 0);
        }
        __syncthreads();   // every wave is done with the slab before the results overwrite it
#pragma unroll
        for (int c = 0; c < 4; c++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const double v = old[c][r] - acc[c][r];
                mp[(size_t)(4 * r) * n + 16 * c] = v;
                a[16 * wave + lr + 4 * r][16 * c + lc] = v;
            }
        __syncthreads();
        gj_invert64(a, Rb, Cb);
        for (int e = threadIdx.x; e < GJ_NB * GJ_NB; e += 256) dinv_next[e] = a[e / GJ_NB][e % GJ_NB];
        return;
    }
    // ---- a block of GJ_R x 2 tiles: block row BY holds the block columns BX with 2 BX <= GJ_R BY + GJ_R - 1, enumerated row by row
    const int idx = (int)blockIdx.x - (have_la ? 1 : 0);
    int BY = 0, BX = idx;
    for (;; BY++) { const int cols = (GJ_R * BY + GJ_R - 1) / 2 + 1; if (BX < cols) break; BX -= cols; }      // (<= 64 rounds)
    const int jb = 2 * BX * 64;                                  // first column of the block
    const int ncolt = min(2, nb - 2 * BX);                       // tile columns that exist
    // the row panel's slab for the block's columns: once, through LDS
    {
        double br[32];
#pragma unroll
        for (int e = 0; e < 32; e++) {
            const int x = threadIdx.x + 256 * e, r = x >> 7, c = x & 127;
            br[e] = c < 64 * ncolt ? rowp[(size_t)r * n + jb + c] : 0.0;
        }
#pragma unroll
        for (int e = 0; e < 32; e++) { const int x = threadIdx.x + 256 * e; lds[(x >> 7) * GJ_P2 + (x & 127)] = br[e]; }
    }
    __syncthreads();
    for (int ti = 0; ti < GJ_R; ti++) {
        const int by = GJ_R * BY + ti;
        if (by >= nb) break;
        const int i0 = by * 64;
        if (by == kb) {   // the pivot rows take the scaled row panel
            for (int tj = 0; tj < ncolt; tj++) {
                const int bx = 2 * BX + tj;
                if (bx > by) break;
#pragma unroll
                for (int c = 0; c < 4; c++)
#pragma unroll
                    for (int r = 0; r < 4; r++) {
                        const int i = i0 + 16 * wave + lr + 4 * r, j = bx * 64 + 16 * c + lc;
                        M[(size_t)i * n + j] = rowp[(size_t)(i - K) * n + j];
                    }
            }
            continue;
        }
        // this wave's 16 rows of the column panel: once for the tile row
        double av[GJ_NB / 4];
        const double* ap = colp + (size_t)(i0 + 16 * wave + lc) * GJ_NB + lr;
#pragma unroll
        for (int s = 0; s < GJ_NB / 4; s++) av[s] = ap[4 * s];
        for (int tj = 0; tj < ncolt; tj++) {
            const int bx = 2 * BX + tj;
            if (bx > by) break;
            if (have_la && by == nxt && bx == nxt) continue;      // the look-ahead workgroup's tile
            const bool jpiv = bx == kb;
            double* mp = M + (size_t)(i0 + 16 * wave + lr) * n + bx * 64 + lc;
            v4f64 old[4];
#pragma unroll
            for (int c = 0; c < 4; c++)
#pragma unroll
                for (int r = 0; r < 4; r++) old[c][r] = jpiv ? 0.0 : mp[(size_t)(4 * r) * n + 16 * c];
            v4f64 acc[4];
#pragma unroll
            for (int c = 0; c < 4; c++) acc[c] = (v4f64){0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int s = 0; s < GJ_NB / 4; s++) {
#pragma unroll
                for (int c = 0; c < 4; c++) acc[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[s], lds[(4 * s + lr) * GJ_P2 + 64 * tj + 16 * c + lc], acc[c], 0, 0, 0);
            }
#pragma unroll
            for (int c = 0; c < 4; c++)
#pragma unroll
                for (int r = 0; r < 4; r++) mp[(size_t)(4 * r) * n + 16 * c] = old[c][r] - acc[c][r];
        }
    }
}

hipError_t launch_spd_inverse(double* M, int n, double* work, hipStream_t st)
{
    if (n <= 0) return hipSuccess;
    if (n % 64) return hipErrorInvalidValue;
    const int nt = n / 64;
    double* rowp = work;
    double* colp = work + (size_t)n * GJ_NB;
    double* dinv[2] = {colp + (size_t)n * GJ_NB, colp + (size_t)n * GJ_NB + GJ_NB * GJ_NB};
    hipLaunchKernelGGL(k_gj_diag, dim3(1), dim3(256), 0, st, M, n, 0, dinv[0]);   // only the first pivot block; the others: look-ahead
    for (int kb = 0; kb < nt; kb++) {
        hipLaunchKernelGGL(k_gj_panels, dim3(n / GJ_H), dim3(256), 0, st, M, n, kb, dinv[kb & 1], rowp, colp);
        static const int blocks2 = getenv("SMG_GJ_2X2") ? atoi(getenv("SMG_GJ_2X2")) : 1;     // A/B knob: 2 x 2 tiles per workgroup
        if (blocks2) {
            if (nt >= 128) hipLaunchKernelGGL(k_gj_update2<4>, dim3(gj_update2_blocks(nt, 4) + (kb + 1 < nt ? 1 : 0)), dim3(256), 0, st, M, n, kb, rowp, colp, dinv[(kb + 1) & 1]);
            else hipLaunchKernelGGL(k_gj_update2<2>, dim3(gj_update2_blocks(nt, 2) + (kb + 1 < nt ? 1 : 0)), dim3(256), 0, st, M, n, kb, rowp, colp, dinv[(kb + 1) & 1]);
        } else
            hipLaunchKernelGGL(k_gj_update, dim3(nt * (nt + 1) / 2), dim3(256), 0, st, M, n, kb, rowp, colp, dinv[(kb + 1) & 1]);
    }
    if (nt > 1) hipLaunchKernelGGL(k_mirror_lower, dim3(nt * (nt - 1) / 2), dim3(256), 0, st, M, n);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------- layout helpers

// kin >= k: the internal block's row length (columns k .. kin - 1 are padding: zero on the way in, skipped on the way out)
__global__ void k_gather_in(double* dst, const double* src, const int* map, int n, int k, int kin, int ld_src)
{
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (size_t)n * kin) return;
    const int i = (int)(t / kin), c = (int)(t % kin);
    dst[t] = c < k ? src[(size_t)map[i] + (size_t)c * ld_src] : 0.0;
}
__global__ void k_scatter_out(double* dst, const double* src, const int* map, int n, int k, int kin, int ld_dst)
{
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (size_t)n * k) return;
    const int i = (int)(t / k), c = (int)(t % k);
    dst[(size_t)map[i] + (size_t)c * ld_dst] = src[(size_t)i * kin + c];
}
__global__ void k_scatter_cm(double* dst, const double* src, const int* idx, int n, int k, int ld_src, int ld_dst)
{
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (size_t)n * k) return;
    const int c = (int)(t / n), i = (int)(t % n);
    dst[(size_t)idx[i] + (size_t)c * ld_dst] = src[(size_t)i + (size_t)c * ld_src];
}
__global__ void k_gather_cm(double* dst, const double* src, const int* idx, int n, int k, int ld_src, int ld_dst)
{
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (size_t)n * k) return;
    const int c = (int)(t / n), i = (int)(t % n);
    dst[(size_t)i + (size_t)c * ld_dst] = src[(size_t)idx[i] + (size_t)c * ld_src];
}
__global__ void k_csr_sub(int n_rows, const int* ptr, const int* col, const double* val, const double* x, int ldx,
                          double* y, int ld, int k)
{
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (size_t)n_rows * k) return;
    const int c = (int)(t / n_rows), i = (int)(t % n_rows);
    double s = 0.0;
    for (int p = ptr[i]; p < ptr[i + 1]; p++) s += val[p] * x[(size_t)col[p] + (size_t)c * ldx];
    y[(size_t)i + (size_t)c * ld] = y[(size_t)i + (size_t)c * ld] - s;
}

static inline unsigned grid1d(size_t n, int bs) { return (unsigned)((n + bs - 1) / bs); }

// ---- value-only re-precompute (fixed sparsity): Galerkin recipes and value scatter maps ------------------------------
__global__ void k_recipe(int n_out, const int* ptr, const int* idx, const double* coef, const double* src, double* out)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n_out) return;
    const int b = ptr[e], en = ptr[e + 1];
    double acc = 0.0;
    if (b < en) {
        acc = coef[b] * src[idx[b]];  // first touch assigns (spgemm), then accumulate in ascending k
        for (int t = b + 1; t < en; t++) acc += coef[t] * src[idx[t]];
    }
    out[e] = acc;
}
__global__ void k_gather_vals(double* dst, const double* src, const int* map, size_t n)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int m = map[i];
    if (m >= 0) dst[i] = src[m];      // padding slots keep what the image was built with (+0.0; 1.0 on the diagonal of lanes without a row)
}
__global__ void k_scatter_dense(double* dense, const double* src, const long long* pos, int n)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dense[pos[i]] = src[i];
}
__global__ void k_add_at(double* v, const int* where, int n, double c)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) v[where[i]] += c;
}
__global__ void k_dense_identity(double* dense, int np, int n)
{
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (size_t)np * np) return;
    const int i = (int)(t / np), j = (int)(t % np);
    dense[t] = (i == j && i >= n) ? 1.0 : 0.0;
}

// ---- operator assembly for a fixed connectivity (row f-3).  The expressions mirror smg_mesh.cpp (doublearea,
// edge_lengths, cotmatrix, massmatrix_diag) term by term so the values are bit-identical to the host assembly. ----------
__global__ void k_face_terms(const double* V, const int* F, int nF, int voronoi, double* Qc, double* Qm)
{
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= nF) return;
    const double* a = V + 3 * (size_t)F[3 * f];
    const double* b = V + 3 * (size_t)F[3 * f + 1];
    const double* c = V + 3 * (size_t)F[3 * f + 2];
    const double ux = b[0] - a[0], uy = b[1] - a[1], uz = b[2] - a[2];
    const double vx = c[0] - a[0], vy = c[1] - a[1], vz = c[2] - a[2];
    const double wx = uy * vz - uz * vy, wy = uz * vx - ux * vz, wz = ux * vy - uy * vx;
    const double dA = sqrt(wx * wx + wy * wy + wz * wz);
    double d0x = b[0] - c[0], d0y = b[1] - c[1], d0z = b[2] - c[2];
    double d1x = c[0] - a[0], d1y = c[1] - a[1], d1z = c[2] - a[2];
    double d2x = a[0] - b[0], d2y = a[1] - b[1], d2z = a[2] - b[2];
    const double l0 = sqrt(d0x * d0x + d0y * d0y + d0z * d0z);
    const double l1 = sqrt(d1x * d1x + d1y * d1y + d1z * d1z);
    const double l2 = sqrt(d2x * d2x + d2y * d2y + d2z * d2z);
    const double q0 = l0 * l0, q1 = l1 * l1, q2 = l2 * l2;
    Qc[3 * (size_t)f + 0] = (q1 + q2 - q0) / dA / 4.0;
    Qc[3 * (size_t)f + 1] = (q2 + q0 - q1) / dA / 4.0;
    Qc[3 * (size_t)f + 2] = (q0 + q1 - q2) / dA / 4.0;
    double m0, m1, m2;
    if (!voronoi) {
        m0 = m1 = m2 = dA / 6.0;
    } else {
        const double cs0 = (l2 * l2 + l1 * l1 - l0 * l0) / (l1 * l2 * 2.0);
        const double cs1 = (l0 * l0 + l2 * l2 - l1 * l1) / (l2 * l0 * 2.0);
        const double cs2 = (l1 * l1 + l0 * l0 - l2 * l2) / (l0 * l1 * 2.0);
        const double b0 = cs0 * l0, b1 = cs1 * l1, b2 = cs2 * l2;
        const double bs = b0 + b1 + b2;
        const double p0 = b0 / bs * (dA * 0.5), p1 = b1 / bs * (dA * 0.5), p2 = b2 / bs * (dA * 0.5);
        m0 = (p1 + p2) * 0.5; m1 = (p2 + p0) * 0.5; m2 = (p0 + p1) * 0.5;
        if (cs0 < 0) { m0 = 0.25 * dA; m1 = 0.125 * dA; m2 = 0.125 * dA; }
        if (cs1 < 0) { m0 = 0.125 * dA; m1 = 0.25 * dA; m2 = 0.125 * dA; }
        if (cs2 < 0) { m0 = 0.125 * dA; m1 = 0.125 * dA; m2 = 0.25 * dA; }
    }
    Qm[3 * (size_t)f + 0] = m0; Qm[3 * (size_t)f + 1] = m1; Qm[3 * (size_t)f + 2] = m2;
}
__global__ void k_mass_diag(int nV, const int* m_ptr, const int* m_idx, const double* Qm, double* Md)
{
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= nV) return;
    double s = 0.0;
    for (int t = m_ptr[v]; t < m_ptr[v + 1]; t++) s += Qm[m_idx[t]];
    Md[v] = s;
}
// val[e] = mass_coef * M(e) + lap_coef * L(e);  L(e) = sum of +/- cot terms in cotmatrix() order (first term assigns)
__global__ void k_assemble_vals(int nnz, const int* l_ptr, const int* l_idx, const signed char* l_sgn, const double* Qc,
                                const int* diag_of, const double* Md, double mass_coef, double lap_coef, double* val, double* Lval)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= nnz) return;
    const int b = l_ptr[e], en = l_ptr[e + 1];
    double L = 0.0;
    if (b < en) {
        L = l_sgn[b] > 0 ? Qc[l_idx[b]] : -Qc[l_idx[b]];
        for (int t = b + 1; t < en; t++) L += l_sgn[t] > 0 ? Qc[l_idx[t]] : -Qc[l_idx[t]];
    }
    if (Lval) Lval[e] = L;
    const int d = diag_of[e];
    const double x = lap_coef * L;
    val[e] = d >= 0 ? mass_coef * Md[d] + x : x;
}
hipError_t launch_assemble(int nV, int nF, int nnz, const double* V, const int* F, int voronoi, const int* l_ptr, const int* l_idx,
                           const signed char* l_sgn, const int* m_ptr, const int* m_idx, const int* diag_of, double* Qc, double* Qm,
                           double* Md, double mass_coef, double lap_coef, double* val, double* Lval, hipStream_t st)
{
    hipLaunchKernelGGL(k_face_terms, dim3(grid1d(nF, 256)), dim3(256), 0, st, V, F, nF, voronoi, Qc, Qm);
    hipLaunchKernelGGL(k_mass_diag, dim3(grid1d(nV, 256)), dim3(256), 0, st, nV, m_ptr, m_idx, Qm, Md);
    hipLaunchKernelGGL(k_assemble_vals, dim3(grid1d(nnz, 256)), dim3(256), 0, st, nnz, l_ptr, l_idx, l_sgn, Qc, diag_of, Md, mass_coef, lap_coef, val, Lval);
    return hipGetLastError();
}

hipError_t launch_recipe(int n_out, const int* ptr, const int* idx, const double* coef, const double* src, double* out, hipStream_t st)
{
    if (n_out <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_recipe, dim3(grid1d(n_out, 256)), dim3(256), 0, st, n_out, ptr, idx, coef, src, out);
    return hipGetLastError();
}
// SELL panels of B(i, j) = A(perm[i], perm[j]) filled on the device from A's CSR arrays in the caller's numbering (first precompute of a big
// level: the host neither builds the permuted matrix nor ships 1.7x padded panels).  One wave per slice, one lane per row; an entry's panel
// column is its rank among the row's new column numbers (rows have a handful of entries: the quadratic count is cheaper than a sort and
// needs no scratch).  The panels must hold col = -1, val = 0 on entry.  Entry order inside a row: ascending new column, the order of the
// host's permute() + build_sell(): the very same image.
// transposed: the image of A^T for a structurally symmetric A -- same slots (row o of A^T has the pattern of row o of A), the value of
// slot (o, j) is A(j, o), found by bisection in row j.
// MAP: instead of the image, write for every slot the index of the CSR entry it holds (s_map, preset to -1): what the value-only
// re-precompute gathers the panels' new values through (launch_gather_vals).
template <bool MAP>
__global__ __launch_bounds__(256) void k_sell_fill(const int* __restrict__ ptr, const int* __restrict__ col, const double* __restrict__ val,
                                                   const int* __restrict__ perm, const int* __restrict__ iperm, const int* __restrict__ slice_row,
                                                   const int* __restrict__ slice_off, int stride, int n_slices, int transposed, int* s_col, double* s_val, int* s_map)
{
    const int lane = threadIdx.x & 63, s = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    if (s >= n_slices) return;
    const int row0 = slice_row[s], nrow = slice_row[s + 1] - row0;
    if (lane >= nrow) return;
    const int old = perm[row0 + lane];
    const int p0 = ptr[old], p1 = ptr[old + 1];
    const size_t base = (size_t)(stride ? s * stride : slice_off[s]) * 64 + lane;
    for (int p = p0; p < p1; p++) {
        const int j = col[p];
        const int c = iperm[j];
        int rank = 0;
        for (int q = p0; q < p1; q++) rank += iperm[col[q]] < c ? 1 : 0;
        int from = p;
        if (transposed) {
            int lo = ptr[j], hi = ptr[j + 1];
            while (lo < hi) { const int mid = (lo + hi) >> 1; if (col[mid] < old) lo = mid + 1; else hi = mid; }
            from = lo;      // (the caller has checked that A(j, old) is stored: launch_bit_symmetric)
        }
        if (MAP) s_map[base + (size_t)rank * 64] = from;
        else {
            s_col[base + (size_t)rank * 64] = c;
            s_val[base + (size_t)rank * 64] = val[from];
        }
    }
}
hipError_t launch_sell_fill(const int* ptr, const int* col, const double* val, const int* perm, const int* iperm, const SellDev& S, size_t padded, hipStream_t st,
                            bool transposed)
{
    hipError_t e = hipMemsetAsync(const_cast<int*>(S.col), 0xFF, padded * sizeof(int), st);       // col = -1
    if (e == hipSuccess) e = hipMemsetAsync(const_cast<double*>(S.val), 0, padded * sizeof(double), st);
    if (e != hipSuccess || S.n_slices <= 0) return e;
    hipLaunchKernelGGL(k_sell_fill<false>, dim3((S.n_slices + 3) / 4), dim3(256), 0, st, ptr, col, val, perm, iperm, S.slice_row, S.slice_off, S.stride, S.n_slices,
                       transposed ? 1 : 0, const_cast<int*>(S.col), const_cast<double*>(S.val), (int*)nullptr);
    return hipGetLastError();
}
hipError_t launch_sell_fill_map(const int* ptr, const int* col, const int* perm, const int* iperm, const SellDev& S, size_t padded, bool transposed, int* map, hipStream_t st)
{
    hipError_t e = hipMemsetAsync(map, 0xFF, padded * sizeof(int), st);       // -1: padding
    if (e != hipSuccess || S.n_slices <= 0) return e;
    hipLaunchKernelGGL(k_sell_fill<true>, dim3((S.n_slices + 3) / 4), dim3(256), 0, st, ptr, col, (const double*)nullptr, perm, iperm, S.slice_row, S.slice_off, S.stride,
                       S.n_slices, transposed ? 1 : 0, (int*)nullptr, (double*)nullptr, map);
    return hipGetLastError();
}

// Weight codes of a filled image (SellDev::codes): the code of a slot is the index of its value's bit pattern in tab
__global__ __launch_bounds__(256) void k_sell_encode(const int* __restrict__ s_col, const double* __restrict__ s_val, size_t n, double t0, double t1, double t2,
                                                     double t3, int n_tab, int* __restrict__ out, int* bad)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int c = s_col[i];
    if (c < 0) { out[i] = -1; return; }
    const long long b = __double_as_longlong(s_val[i]);
    const int code = b == __double_as_longlong(t0) ? 0 : (n_tab > 1 && b == __double_as_longlong(t1)) ? 1 : (n_tab > 2 && b == __double_as_longlong(t2)) ? 2
                   : (n_tab > 3 && b == __double_as_longlong(t3)) ? 3 : -1;
    if (code < 0 || c >= (1 << 29)) { atomicOr(bad, 1); out[i] = -1; return; }
    out[i] = (c << 2) | code;
}
hipError_t launch_sell_encode(const SellDev& S, size_t padded, const double* tab, int n_tab, int* out_col, int* bad, hipStream_t st)
{
    if (padded == 0) return hipSuccess;
    hipLaunchKernelGGL(k_sell_encode, dim3(grid1d(padded, 256)), dim3(256), 0, st, S.col, S.val, padded, tab[0], tab[1], tab[2], tab[3], n_tab, out_col, bad);
    return hipGetLastError();
}

// Where the diagonal of every row sits in the value array of a filled square image (SellBuf::diag_slot, what the host computes for the
// images it builds itself): slot[r] = index, or -1; *first_missing = the smallest row without a stored diagonal (n_rows if none).
__global__ __launch_bounds__(256) void k_sell_diag_slots(const int* __restrict__ slice_row, const int* __restrict__ slice_off, const int* __restrict__ slice_w, int stride,
                                                         int n_slices, const int* __restrict__ s_col, int* __restrict__ slot, int* first_missing)
{
    const int lane = threadIdx.x & 63, s = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    if (s >= n_slices) return;
    const int row0 = slice_row[s], nrow = slice_row[s + 1] - row0;
    if (lane >= nrow) return;
    const int r = row0 + lane, w = slice_w[s];
    const size_t base = (size_t)(stride ? s * stride : slice_off[s]) * 64 + lane;
    int at = -1;
    for (int j = 0; j < w; j++) if (s_col[base + (size_t)j * 64] == r) { at = (int)(base + (size_t)j * 64); break; }
    slot[r] = at;
    if (at < 0) atomicMin(first_missing, r);
}
hipError_t launch_sell_diag_slots(const SellDev& S, int* slot, int* first_missing, hipStream_t st)
{
    if (S.n_slices <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_sell_diag_slots, dim3((S.n_slices + 3) / 4), dim3(256), 0, st, S.slice_row, S.slice_off, S.slice_w, S.stride, S.n_slices, S.col, slot, first_missing);
    return hipGetLastError();
}

// An empty launch: the runtime loads a translation unit's code object when one of its kernels is first launched (tens of ms for this
// file); the first precompute asks for that while its host half is still running.
__global__ void k_nothing() {}
hipError_t warm_device_code(hipStream_t st)
{
    hipLaunchKernelGGL(k_nothing, dim3(1), dim3(64), 0, st);
    return hipGetLastError();
}

// A == A^T?  One thread per row: every entry looks its mirror image up by bisection.  *differs: bit 0 set when some value differs from its
// mirror image in any bit, bit 1 when some entry has no mirror image at all (A is not structurally symmetric).
__global__ __launch_bounds__(256) void k_bit_symmetric(int n, const int* __restrict__ ptr, const int* __restrict__ col, const double* __restrict__ val, int* differs)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int d = 0;
    for (int p = ptr[i]; p < ptr[i + 1]; p++) {
        const int j = col[p];
        if (j < 0 || j >= n) { d |= 2; continue; }
        int lo = ptr[j], hi = ptr[j + 1];
        while (lo < hi) { const int mid = (lo + hi) >> 1; if (col[mid] < i) lo = mid + 1; else hi = mid; }
        if (lo >= ptr[j + 1] || col[lo] != i) d |= 2;
        else if (__double_as_longlong(val[lo]) != __double_as_longlong(val[p])) d |= 1;
    }
    if (d) atomicOr(differs, d);
}
hipError_t launch_bit_symmetric(int n, const int* ptr, const int* col, const double* val, int* differs, hipStream_t st)
{
    hipError_t e = hipMemsetAsync(differs, 0, sizeof(int), st);
    if (e != hipSuccess || n <= 0) return e;
    hipLaunchKernelGGL(k_bit_symmetric, dim3(grid1d((size_t)n, 256)), dim3(256), 0, st, n, ptr, col, val, differs);
    return hipGetLastError();
}

hipError_t launch_gather_vals(double* dst, const double* src, const int* map, size_t n, hipStream_t st)
{
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_gather_vals, dim3(grid1d(n, 256)), dim3(256), 0, st, dst, src, map, n);
    return hipGetLastError();
}
hipError_t launch_dense_from_csr(double* dense, int np, int n, const double* src, const long long* pos, int nnz, hipStream_t st)
{
    hipLaunchKernelGGL(k_dense_identity, dim3(grid1d((size_t)np * np, 256)), dim3(256), 0, st, dense, np, n);
    if (nnz > 0) hipLaunchKernelGGL(k_scatter_dense, dim3(grid1d(nnz, 256)), dim3(256), 0, st, dense, src, pos, nnz);
    return hipGetLastError();
}
hipError_t launch_scatter_dense(double* dense, const double* src, const long long* pos, int nnz, hipStream_t st)
{
    if (nnz > 0) hipLaunchKernelGGL(k_scatter_dense, dim3(grid1d(nnz, 256)), dim3(256), 0, st, dense, src, pos, nnz);
    return hipGetLastError();
}
hipError_t launch_dense_identity(double* dense, int np, int n, hipStream_t st)
{
    hipLaunchKernelGGL(k_dense_identity, dim3(grid1d((size_t)np * np, 256)), dim3(256), 0, st, dense, np, n);
    return hipGetLastError();
}
hipError_t launch_add_at(double* v, const int* where, int n, double c, hipStream_t st)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_add_at, dim3(grid1d(n, 256)), dim3(256), 0, st, v, where, n, c);
    return hipGetLastError();
}

hipError_t launch_gather_in(double* dst, const double* src, const int* map, int n, int k, int kin, int ld_src, hipStream_t st)
{
    if ((size_t)n * k == 0) return hipSuccess;
    hipLaunchKernelGGL(k_gather_in, dim3(grid1d((size_t)n * kin, 256)), dim3(256), 0, st, dst, src, map, n, k, kin, ld_src);
    return hipGetLastError();
}
hipError_t launch_scatter_out(double* dst, const double* src, const int* map, int n, int k, int kin, int ld_dst, hipStream_t st)
{
    if ((size_t)n * k == 0) return hipSuccess;
    hipLaunchKernelGGL(k_scatter_out, dim3(grid1d((size_t)n * k, 256)), dim3(256), 0, st, dst, src, map, n, k, kin, ld_dst);
    return hipGetLastError();
}
hipError_t launch_scatter_cm(double* dst, const double* src, const int* idx, int n, int k, int ld_src, int ld_dst,
                             hipStream_t st)
{
    if ((size_t)n * k == 0) return hipSuccess;
    hipLaunchKernelGGL(k_scatter_cm, dim3(grid1d((size_t)n * k, 256)), dim3(256), 0, st, dst, src, idx, n, k, ld_src, ld_dst);
    return hipGetLastError();
}
hipError_t launch_gather_cm(double* dst, const double* src, const int* idx, int n, int k, int ld_src, int ld_dst,
                            hipStream_t st)
{
    if ((size_t)n * k == 0) return hipSuccess;
    hipLaunchKernelGGL(k_gather_cm, dim3(grid1d((size_t)n * k, 256)), dim3(256), 0, st, dst, src, idx, n, k, ld_src, ld_dst);
    return hipGetLastError();
}
hipError_t launch_csr_sub(int n_rows, const int* ptr, const int* col, const double* val, const double* x, int ldx,
                          double* y, int ld, int k, hipStream_t st)
{
    if ((size_t)n_rows * k == 0) return hipSuccess;
    hipLaunchKernelGGL(k_csr_sub, dim3(grid1d((size_t)n_rows * k, 256)), dim3(256), 0, st, n_rows, ptr, col, val, x, ldx, y, ld, k);
    return hipGetLastError();
}

}  // namespace smg
