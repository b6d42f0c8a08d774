// smg_cycle.cpp -- mg_VCycle (reference src/mg_VCycle.cpp:3-201): what a cycle is.  The level vectors, the smoothers, the launch sequence of a
// V-cycle and of the outer residual that goes in front of it, and the entry points that use them on a handle that is NOT in a solve: the V-cycle
// pieces on host blocks, the raw device interface, the cycle benchmarks.  The solve loops that replay these launches live in smg_solve.cpp.
// The V-cycle never leaves the GPU: every kernel is enqueued on the handle's stream.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <memory>
#include <numeric>
#include <string>
#include <thread>
#include <vector>

#include "smg_internal.hpp"

using namespace smg;

// ------------------------------------------------------------------------------------------------ V-cycle

// The level vectors (and the Schur solver's separator pair) of one precision for solves of k columns: allocated and zeroed when k outgrows what is
// there, the second iterate and the update vector when the level's smoother asks for them.  The fp64 set serves more than the cycle -- the outer
// residual and its partial sums, the fused head, the pieces -- and the conditions on `fp64` below are those extras.
template <typename T>
static int ensure_vectors(smg_hierarchy* h, int k)
{
    constexpr bool fp64 = std::is_same<T, double>::value;
    const int L = h->n_levels;
    int& kcap = fp64 ? h->kcap : h->kcap32;
    int rc;
    auto zeroed = [&](DevBuf<T>& v, size_t cnt) -> int {
        HIPCHK(v.alloc(cnt));
        HIPCHK(hipMemsetAsync(v.p, 0, cnt * sizeof(T), h->stream));
        return SMG_OK;
    };
    if (k > kcap) {
        drop_graphs(h);
        size_t maxblocks = 0;
        for (int lv = 0; lv < L; lv++) {
            Level& Lv = h->lv[lv];
            LevelVecs<T>& V = vecs<T>(Lv);
            const size_t rows = (lv == L - 1) ? (size_t)h->nc_pad : (size_t)Lv.n;
            if ((rc = zeroed(V.b, rows * k)) || (rc = zeroed(V.u, rows * k))) return rc;
            V.t.release(); V.d.release();
            const bool has_resid = lv < L - 1 || (fp64 && L == 1);      // (a single level: the outer loop's residual)
            if (has_resid) HIPCHK(V.r.alloc(rows * k));
            if (fp64 && has_resid) {
                if (h->bs == 3) maxblocks = std::max(maxblocks, (size_t)bsr3_blocks(Lv.bA.view.n_slices) * (size_t)k);
                else maxblocks = std::max(maxblocks, (size_t)sell_blocks(Lv.dA.view.n_slices) * ((k + 3) / 4) + (size_t)sell_wide_blocks(Lv.dA.view.n_slices, k));
            }
        }
        if (fp64) {
            // colour by colour (the level-0 head of an outer iteration, enqueue_residual_ss) every launch rounds its block count up on its own
            maxblocks += (h->lv[0].dA.color_slice_ptr.size() + 1) * (size_t)((k + 3) / 4 + 8);
            HIPCHK(h->d_partials.alloc(std::max<size_t>(maxblocks, 1) + (size_t)ss_partials_room()));
        }
        kcap = k;
    }
    // Jacobi-smoothed levels ping-pong between u and a second iterate
    for (int lv = 0; lv < L - 1; lv++) {
        Level& Lv = h->lv[lv];
        LevelVecs<T>& V = vecs<T>(Lv);
        const size_t cnt = (size_t)Lv.n * kcap;
        // (fp64, level 0 always: the first sweep of an outer iteration is written out of place, see enqueue_residual_ss)
        if ((level_is_jacobi(h, lv) || (fp64 && lv == 0)) && V.t.n < cnt) {
            drop_graphs(h);
            if ((rc = zeroed(V.t, cnt))) return rc;
        }
        if (level_kind(h, lv) == LV_CHEBY && V.d.n < cnt) {
            drop_graphs(h);
            if ((rc = zeroed(V.d, cnt))) return rc;
        }
    }
    if (h->coarse_schur) {       // the separator's right-hand side and solution (the solver may have arrived with a value-only re-precompute, after the vectors)
        const size_t need = (size_t)h->sch.view.ns_pad * std::max(kcap, 1);
        DevBuf<T>&g = h->sch.rhs<T>(), &xs = h->sch.sol<T>();
        if (g.n < need || xs.n < need) {
            drop_graphs(h);
            if ((rc = zeroed(g, need)) || (rc = zeroed(xs, need))) return rc;
        }
        SchurDev& S = h->sch.view;
        if constexpr (fp64) { S.g = g.p; S.xs = xs.p; } else { S.g32 = g.p; S.xs32 = xs.p; }
    }
    if (fp64 && h->coarse_sparse) {      // the triangular solves take up to 64 columns per pass: 2 n doubles of scratch per column of a pass
        const size_t need = (size_t)2 * h->chol.n * sparse_coarse_work_cols(std::max(kcap, 1));
        if (h->c_work.n < need) {
            drop_graphs(h);          // the captured launches hold the scratch pointer
            HIPCHK(h->c_work.alloc(need));
            h->c_view.work = h->c_work.p;
        }
    }
    return SMG_OK;
}

int smg::ensure_work(smg_hierarchy* h, int k)
{
    int rc = ensure_vectors<double>(h, k);
    if (rc) return rc;
    if ((rc = prepare_sweep_plans(h, k, h->pre, h->post))) return rc;
    return ensure_spectral_bounds(h);
}

// ---- mixed precision: fp32 images of the operators and an fp32 V-cycle ------------------------------------------------
// The images belong to the matrices (SellBuf / Bsr3Buf::ensure_f32 fill valf and point the matrix's own view at it): both cycles launch on the
// same views.  f32_valid says that the images hold the current values; whoever changes values lowers it (smg_precompute.cpp).
int smg::ensure_fp32(smg_hierarchy* h, int k)
{
    const int L = h->n_levels;
    if (h->union_m > 0) return fail(SMG_ERR_INVALID, "a union handle solves in fp64 (its coarse inverses are per-member blocks: no fp32 image)");
    if (h->coarse_sparse) return fail(SMG_ERR_INVALID, "the mixed-precision cycle is not available with a sparse coarse factorisation (coarsest level of %d unknowns)", h->nc);
    if (!h->f32_valid) {
        drop_graphs(h);
        for (int lv = 0; lv < L; lv++) {
            Level& Lv = h->lv[lv];
            if (lv < L - 1 && h->bs == 3) {     // block hierarchies: the nine value planes of every panel column
                HIPCHK(Lv.bA.ensure_f32(h->stream));
                if (Lv.gs_on_transpose) HIPCHK(Lv.bAT.ensure_f32(h->stream));
            } else if (lv < L - 1) {
                HIPCHK(Lv.dA.ensure_f32(h->stream));
                if (Lv.gs_on_transpose) HIPCHK(Lv.dAT.ensure_f32(h->stream));
            }
            if (lv >= 1) {
                HIPCHK(Lv.dP.ensure_f32(h->stream));
                HIPCHK(Lv.dPT.ensure_f32(h->stream));
            }
        }
        if (h->coarse_schur) {
            HIPCHK(h->sch.arena32.ensure((size_t)h->schur.off_C));          // blocks, panels and the separator's inverse (the products behind them are scratch)
            HIPCHK(launch_cvt_f64_f32(h->sch.arena32.p, h->sch.arena.p, (size_t)h->schur.off_C, h->stream));
            h->sch.view.arena32 = h->sch.arena32.p;
        } else {
            HIPCHK(h->d_Ainv32.ensure((size_t)h->nc_pad * h->nc_pad));
            HIPCHK(launch_cvt_f64_f32(h->d_Ainv32.p, h->d_Ainv.p, (size_t)h->nc_pad * h->nc_pad, h->stream));
        }
        h->f32_valid = true;
    }
    return ensure_vectors<float>(h, k);
}

// ---- the smoother of a level -------------------------------------------------------------------------------------------
// SMG_SMOOTH_GS (default): the reference's relax().  SMG_SMOOTH_JACOBI / _HYBRID: damped Jacobi on all / on the small levels
// (BASELINE.json north_star: "Gauss-Seidel/Jacobi smoothing"; one whole-matrix launch per sweep instead of one per colour).
int smg::level_kind(const smg_hierarchy* h, int lv)
{
    if (lv < 0 || lv >= h->n_levels - 1) return LV_GS;
    switch (h->smoother) {
        case SMG_SMOOTH_JACOBI: return LV_JACOBI;
        case SMG_SMOOTH_HYBRID: return h->lv[lv].n <= h->jacobi_max_rows ? LV_JACOBI : LV_GS;
        case SMG_SMOOTH_CHEBYSHEV: return LV_CHEBY;
        case SMG_SMOOTH_HYBRID_CHEBYSHEV: return h->lv[lv].n <= h->jacobi_max_rows ? LV_CHEBY : LV_GS;
    }
    return LV_GS;
}

// Coefficients of the Chebyshev-Jacobi recurrence (include/smg.h, SMG_SMOOTH_CHEBYSHEV): step s computes d = c1 d + c2 r, u += d.
// The same statements, in the same order, as the CPU restatement used by the tests -- both are compiled without FMA contraction.
struct ChebyCoef { double c1, c2; };
static void cheby_coefs(double lam, double frac, int degree, std::vector<ChebyCoef>& out)
{
    out.resize((size_t)std::max(degree, 0));
    const double lmax = lam, lmin = lam * frac;
    const double theta = (lmax + lmin) / 2.0, delta = (lmax - lmin) / 2.0;
    const double sigma = theta / delta;
    double rho = 1.0 / sigma;
    for (int s = 0; s < degree; s++) {
        if (s == 0) { out[s].c1 = 0.0; out[s].c2 = 1.0 / theta; }
        else {
            const double rho_new = 1.0 / (2.0 * sigma - rho);
            out[s].c1 = rho_new * rho;
            out[s].c2 = 2.0 * rho_new / delta;
            rho = rho_new;
        }
    }
}

// The dense coarse product of a padded solve (internal_cols below) is formed for the caller's columns only: which of its kernels serves a column
// (1 / 2 - 7 / 8 and more columns) then follows the CALLER's column count, as it would without padding -- a column-sharded solve stays bit-identical
// to the fused one (tests/test_gpu_dist.py), and the padding columns' coarse iterate stays the zero the restriction wrote.
static inline int coarse_cols(const smg_hierarchy* h, int k) { return (h->coarse_cols > 0 && h->coarse_cols < k) ? h->coarse_cols : k; }

// Every routine of the cycle is written once for T = double (the reference's arithmetic) and T = float (the mixed-precision V-cycle): the level
// vectors are vecs<T>(level), a matrix view hands out its values of type T (SellDev::vals<T>()), and launch_sell / launch_bsr3 / launch_schur_solve /
// launch_dense_gemv_add are overloaded on the vectors' type.

// what the smoother of a scalar level streams: A^T where A is not bit-symmetric, else A
static const SellBuf& smoothed(const Level& L) { return L.gs_on_transpose ? L.dAT : L.dA; }

// coarseSolve on the coarsest level's b / u; the member blocks of a union and the sparse factorisation exist in fp64 only (ensure_fp32 refuses them)
template <typename T>
static hipError_t coarse_solve(smg_hierarchy* h, Level& L, int k, const Ctrl* ctrl)
{
    LevelVecs<T>& V = vecs<T>(L);
    if constexpr (std::is_same<T, double>::value) {
        if (h->union_m > 0) return launch_blockdiag_gemv_add(h->un.view, h->d_Ainv.p, h->nc, V.b.p, V.u.p, k, ctrl, h->stream);   // the members' own inverses (smg_union.cpp)
        if (h->coarse_sparse) return launch_sparse_coarse_solve(h->c_view, V.b.p, V.u.p, k, ctrl, h->stream);
    }
    if (h->coarse_schur) return launch_schur_solve(h->sch.view, V.b.p, V.u.p, k, ctrl, h->stream);
    return launch_dense_gemv_add(by_type<T>(h->d_Ainv.p, h->d_Ainv32.p), h->nc, h->nc_pad, V.b.p, V.u.p, coarse_cols(h, k), k, ctrl, h->stream, (T*)h->d_sympart.p);
}

// an operation with the level's matrix in whatever format it lives in: SELL panels, or 3 x 3 blocks on block hierarchies.
// smoother_image: the matrix the smoother streams (A^T where A is not bit-symmetric), else A.  s1 < 0: all slices.
template <typename T>
static hipError_t op_A(smg_hierarchy* h, Level& L, bool smoother_image, SellMode m, int s0, int s1, const T* x, const T* bb, T* y, int k, const Ctrl* ctrl,
                       const FirstColour* fc = nullptr, double omega = 1.0)
{
    if (h->bs == 3) {
        const Bsr3Dev& V = (smoother_image && L.gs_on_transpose) ? L.bAT.view : L.bA.view;
        return launch_bsr3(m, V, s0, s1 < 0 ? V.n_slices : s1, x, bb, y, k, ctrl, nullptr, nullptr, h->stream, omega, fc ? fc->c1 : 0.0, fc ? fc->update<T>() : nullptr);
    }
    const SellDev& V = smoother_image ? smoothed(L).view : L.dA.view;
    return launch_sell(m, V, s0, s1 < 0 ? V.n_slices : s1, x, bb, y, k, ctrl, nullptr, nullptr, h->stream, nullptr, fc, omega);
}

// slice ranges of the colours of the matrix the smoother streams
static const std::vector<int>& colour_slices(const smg_hierarchy* h, const Level& Lv)
{
    if (h->bs == 3) return (Lv.gs_on_transpose ? Lv.bAT : Lv.bA).color_slice_ptr;
    return (Lv.gs_on_transpose ? Lv.dAT : Lv.dA).color_slice_ptr;
}

// `iters` forward Gauss-Seidel sweeps in place, with the level's wave / block plan sp (sweep_plan) or one launch per colour (reference relax(),
// src/mg_VCycle.cpp:113-178).  first = FIRST_LAUNCH: the first colour of the first sweep is already in u.  FIRST_SWEEP: the whole first sweep is in `t`:
// the second sweep goes from t back into u (out-of-place colour launches: same values), the rest run in place on u; needs iters >= 2.
// res (one launch per colour, fp64, scalar levels, k < 8; see resid_byproduct below): the last launch of the last sweep also stores the residual of its
// rows there (SELL_GS_RES / SELL_GS_OOP_RES).
template <typename T>
static int enqueue_gs(smg_hierarchy* h, int lv, const SweepPlan& sp, const T* b, T* u, int k, int iters, const Ctrl* ctrl, int first = FIRST_NONE, T* t = nullptr,
                      T* res = nullptr)
{
    Level& Lv = h->lv[lv];
    ProfGuard pg(h, "MG: relaxation");  // PROFC_NODE at src/mg_VCycle.cpp:121
    if (const WgsBuf* W = sp.wave) {      // Galerkin levels of decimated hierarchies: one launch per piece colour (fp64)
        for (int it = 0; it < iters; it++)
            for (size_t c = 0; c + 1 < W->color_ptr.size(); c++)
                HIPCHK(launch_wgs(W->view, W->color_ptr[c], W->color_ptr[c + 1], (const double*)b, (double*)u, k, ctrl, h->stream));
        return SMG_OK;
    }
    if (const BgsBuf* Q = sp.block) {     // many columns: one launch per block colour (fp64)
        for (int it = 0; it < iters; it++)
            for (size_t c = 0; c + 1 < Q->color_ptr.size(); c++)
                HIPCHK(launch_bgs(Q->view, Q->color_ptr[c], Q->color_ptr[c + 1], (const double*)b, (double*)u, k, ctrl, h->stream));
        return SMG_OK;
    }
    const std::vector<int>& cs = colour_slices(h, Lv);
    const SellDev& G = smoothed(Lv).view;
    FirstColour fr;      // (only its update vector is read: the by-product's output)
    fr.set_update(res);
    for (int it = first == FIRST_SWEEP ? 1 : 0; it < iters; it++)
        for (size_t c = (it == 0 && first == FIRST_LAUNCH) ? 1 : 0; c + 1 < cs.size(); c++) {
            const bool last = res && it == iters - 1 && c + 2 == cs.size();
            if (it == 1 && first == FIRST_SWEEP) HIPCHK(launch_sell(last ? SELL_GS_OOP_RES : SELL_GS_OOP, G, cs[c], cs[c + 1], t, b, u, k, ctrl, nullptr, nullptr, h->stream, nullptr, last ? &fr : nullptr));   // (scalar levels only)
            else if (last) HIPCHK(launch_sell(SELL_GS_RES, G, cs[c], cs[c + 1], u, b, u, k, ctrl, nullptr, nullptr, h->stream, nullptr, &fr));
            else HIPCHK(op_A<T>(h, Lv, true, SELL_GS, cs[c], cs[c + 1], u, b, u, k, ctrl));
        }
    return SMG_OK;
}

// relax(iters) as one launch (overlapped tiling, fp64): from buf[*cur] into the other buffer, flips *cur
template <typename T>
static int enqueue_gs_tiled(smg_hierarchy* h, const TiledDev& plan, const T* b, T* const buf[2], int* cur, int k, const Ctrl* ctrl)
{
    ProfGuard pg(h, "MG: relaxation");
    HIPCHK(launch_tiled_gs(plan, (const double*)buf[*cur], (const double*)b, (double*)buf[1 - *cur], k, ctrl, h->stream));
    *cur ^= 1;
    return SMG_OK;
}

// `iters` damped-Jacobi sweeps, ping-pong between buf[0] and buf[1]: sweep s reads buf[*cur], writes the other, flips *cur.
template <typename T>
static int enqueue_jacobi(smg_hierarchy* h, int lv, const T* b, T* const buf[2], int* cur, int k, int iters, const Ctrl* ctrl)
{
    Level& Lv = h->lv[lv];
    ProfGuard pg(h, "MG: relaxation");
    for (int it = 0; it < iters; it++) {
        HIPCHK(op_A<T>(h, Lv, true, SELL_JACOBI, 0, -1, buf[*cur], b, buf[1 - *cur], k, ctrl, nullptr, h->omega));
        *cur ^= 1;
    }
    return SMG_OK;
}

// relax(iters) on a Chebyshev-Jacobi level: ONE polynomial of degree iters + 1, i.e. iters + 1 whole-matrix launches ping-ponging like
// the Jacobi sweeps; first_done: step 0 was produced by the restriction launch.
template <typename T>
static int enqueue_cheby(smg_hierarchy* h, int lv, const T* b, T* const buf[2], int* cur, int k, int iters, const Ctrl* ctrl, bool first_done = false)
{
    if (iters <= 0) return SMG_OK;
    Level& Lv = h->lv[lv];
    ProfGuard pg(h, "MG: relaxation");
    std::vector<ChebyCoef> cf;
    cheby_coefs(Lv.lam, h->cheby_fraction, iters + 1, cf);
    for (int s = first_done ? 1 : 0; s <= iters; s++) {
        FirstColour fc;
        fc.set_update(vecs<T>(Lv).d.p);
        fc.c1 = cf[s].c1;
        HIPCHK(op_A<T>(h, Lv, true, SELL_CHEBY, 0, -1, buf[*cur], b, buf[1 - *cur], k, ctrl, &fc, cf[s].c2));
        *cur ^= 1;
    }
    return SMG_OK;
}

// reference mg_VCycle(), src/mg_VCycle.cpp:3-59.  B and u of level lv are Lv.b / Lv.u (level 0: RHS_u / z_u).
static bool fuse_first_colour() { static const int on = env_int("SMG_FUSE_FIRST", 1); return on != 0; }
// Two quarter passes whose results nobody reads, on the levels smoothed with one launch per colour (A/B knobs; same bits either way):
// the level residual of the last colour's rows comes out of the last pre-smoothing launch, which holds all it takes (SELL_GS_RES in
// smg_device.hpp), and the residual launch walks the other colours only;
static bool resid_byproduct() { static const int on = env_int("SMG_RESID_BYPRODUCT", 1); return on != 0; }
// the prolongation leaves out the slices inside the first colour: the first post-smoothing launch overwrites those rows without reading them.
static bool prolong_skip_first() { static const int on = env_int("SMG_PROLONG_SKIP_FIRST", 1); return on != 0; }

// first: what of this level's first pre-smoothing sweep already exists (FIRST_*).
template <typename T>
static int enqueue_vcycle_t(smg_hierarchy* h, int lv, int k, int pre, int post, const Ctrl* ctrl, int first = FIRST_NONE)
{
    const bool first_done = first != FIRST_NONE;
    const int L = h->n_levels;
    Level& Lv = h->lv[lv];
    if (lv == L - 1) {  // coarseSolve: u = u + solver.solve(B)  (:28-33, :199-200)
        ProfGuard pg(h, "MG: coarse solve");
        HIPCHK(coarse_solve<T>(h, Lv, k, ctrl));
        return SMG_OK;
    }
    Level& Lc = h->lv[lv + 1];
    LevelVecs<T>&V = vecs<T>(Lv), &Vc = vecs<T>(Lc);
    const int kind = level_kind(h, lv);
    const bool jac = kind != LV_GS;
    T* const buf[2] = {V.u.p, V.t.p};   // Jacobi-type levels ping-pong; the level's result always ends in buf[0] = u
    int cur = 0;
    // Gauss-Seidel levels whose relax() runs as one out-of-place launch (overlapped tiling): they ping-pong like the Jacobi-type ones.
    const bool fp64 = std::is_same<T, double>::value;
    const SweepPlan sp_pre = sweep_plan(h, lv, k, pre, fp64, first), sp_post = sweep_plan(h, lv, k, post, fp64, FIRST_NONE);
    int rc;
    // (fp64 only: the fp32 cycle keeps the whole residual launch.  The smoother must stream A itself, and the last launch of the last sweep must exist)
    const bool byprod = fp64 && resid_byproduct() && h->bs == 1 && kind == LV_GS && sp_pre.colours() && pre >= 1 && k < 8 && !Lv.gs_on_transpose &&
                        Lv.dA.n_part > 0 && Lv.dA.color_slice_ptr.size() >= 3 && (first != FIRST_SWEEP || pre >= 2);
    if (kind == LV_JACOBI) {
        if (first_done) cur = 1;
        rc = enqueue_jacobi<T>(h, lv, V.b.p, buf, &cur, k, pre - (first_done ? 1 : 0), ctrl);            // :36
    } else if (kind == LV_CHEBY) {
        if (first_done) cur = 1;
        rc = enqueue_cheby<T>(h, lv, V.b.p, buf, &cur, k, pre, ctrl, first_done);                         // :36
    } else if (sp_pre.tiled) rc = enqueue_gs_tiled<T>(h, *sp_pre.tiled, V.b.p, buf, &cur, k, ctrl);                    // :36, one launch
    else rc = enqueue_gs<T>(h, lv, sp_pre, V.b.p, buf[0], k, pre, ctrl, first, buf[1], byprod ? V.r.p : nullptr);   // :36
    if (rc) return rc;
    {   // r = B - A u  (:40-42); with the by-product: of the rows outside the last colour, in the region order without that colour's slices
        ProfGuard pg(h, "MG: residual");
        if (byprod) HIPCHK(launch_sell(SELL_RESID, Lv.dA.part_view(), 0, Lv.dA.n_part, buf[cur], V.b.p, V.r.p, k, ctrl, nullptr, nullptr, h->stream));
        else HIPCHK(op_A<T>(h, Lv, false, SELL_RESID, 0, -1, buf[cur], V.b.p, V.r.p, k, ctrl));
    }
    // With uc = 0 the first launch of the coarse level's first pre-smoothing sweep computes (rc_i - 0) / a_ii for the rows it covers
    // (the first colour / with Jacobi all rows, damped): the restriction launch writes that itself, bit for bit the same value, and
    // the sweep starts one launch later.
    const SellBuf& Gc = smoothed(Lc);
    const int kind_c = level_kind(h, lv + 1);
    const bool jac_c = kind_c != LV_GS;
    // (block hierarchies: the first launch of a coarse sweep is not a plain division -- row 3v+1 of the first colour already reads 3v; a coarse level with
    // a sweep plan runs all its phases itself)
    const bool fuse = h->bs == 1 && sweep_plan(h, lv + 1, k, pre, fp64, FIRST_NONE).colours() && fuse_first_colour() && lv + 1 < L - 1 && pre > 0 && Gc.view.vals<T>() && (jac_c ? Gc.n_all > 0 : Gc.n_first > 0);
    const int kt = k * h->bs;   // block hierarchies: dP / dPT hold the vertex-level factor of P (x) I_3, applied to 3 k columns
    {   // rc = PT r  (:43-44, :80) and uc = 0 (:46-47) in one launch: both are indexed by the coarse row
        ProfGuard pg(h, "MG: restrict");
        FirstColour fc;
        if (fuse) {
            fc.diag_slot = Gc.diag_slot.p; fc.n_first = jac_c ? Gc.n_all : Gc.n_first;
            fc.val = Gc.view.val; fc.valf = Gc.view.valf;
            fc.jacobi = kind_c == LV_CHEBY ? 2 : (jac_c ? 1 : 0); fc.omega = h->omega;
            if (kind_c == LV_CHEBY) {   // step 0 of the coarse level's polynomial: d = (rc_i / a_ii - 0) / theta, uc = 0 + d
                std::vector<ChebyCoef> cf;
                cheby_coefs(Lc.lam, h->cheby_fraction, 1, cf);
                fc.omega = cf[0].c2;
                fc.set_update(Vc.d.p);
            }
        }
        // Jacobi + fuse: the first sweep's output buffer (t) receives the sweep, u = 0 is never read
        T* init = (fuse && jac_c) ? Vc.t.p : Vc.u.p;
        HIPCHK(launch_sell(SELL_AX, Lc.dPT.view, 0, Lc.dPT.view.n_slices, V.r.p, nullptr, Vc.b.p, kt, ctrl, nullptr, nullptr, h->stream, init, fuse ? &fc : nullptr));
    }
    rc = enqueue_vcycle_t<T>(h, lv + 1, k, pre, post, ctrl, fuse ? FIRST_LAUNCH : FIRST_NONE);  // :48
    if (rc) return rc;
    {   // u = u + P uc  (:51-53, :91).  A Jacobi level with an odd number of post-smoothing sweeps to go adds out of place, so that
        // the last sweep lands in u.
        ProfGuard pg(h, "MG: prolong");
        int dst = cur;
        const int flips = sp_post.tiled ? 1 : kind == LV_CHEBY ? (post > 0 ? post + 1 : 0) : post;   // buffer switches of the post-smoothing
        if ((jac || sp_post.tiled) && ((cur + flips) & 1)) dst = 1 - cur;
        if (!jac && !sp_post.tiled && cur == 1) dst = 0;      // in-place Gauss-Seidel sweeps follow: they work on u
        // in-place colour launches follow: the first of them overwrites the first colour's rows unread, the prolongation leaves their slices out
        const bool skip = prolong_skip_first() && h->bs == 1 && kind == LV_GS && sp_post.colours() && post >= 1 && Lc.dP.n_part > 0;
        const SellDev Pv = skip ? Lc.dP.part_view() : Lc.dP.view;
        HIPCHK(launch_sell(SELL_ADD, Pv, 0, Pv.n_slices, Vc.u.p, buf[cur], buf[dst], kt, ctrl, nullptr, nullptr, h->stream));
        cur = dst;
    }
    if (kind == LV_CHEBY) return enqueue_cheby<T>(h, lv, V.b.p, buf, &cur, k, post, ctrl);   // :57  (ends with cur == 0)
    if (jac) return enqueue_jacobi<T>(h, lv, V.b.p, buf, &cur, k, post, ctrl);   // :57  (ends with cur == 0)
    if (sp_post.tiled) return enqueue_gs_tiled<T>(h, *sp_post.tiled, V.b.p, buf, &cur, k, ctrl);   // :57  (ends with cur == 0)
    return enqueue_gs<T>(h, lv, sp_post, V.b.p, buf[0], k, post, ctrl);          // :57
}

// the cycle of a solve: level 0, the handle's sweeps, in the handle's precision (the fp32 cycle starts from nothing: `first` is the fp64 one's)
int smg::enqueue_vcycle(smg_hierarchy* h, int k, const Ctrl* ctrl, int first)
{
    if (h->precision == 1) return enqueue_vcycle_t<float>(h, 0, k, h->pre, h->post, ctrl);
    return enqueue_vcycle_t<double>(h, 0, k, h->pre, h->post, ctrl, first);
}

int smg::apply_A(smg_hierarchy* h, int lv, SellMode mode, const double* x, const double* b, double* y, int k, const Ctrl* ctrl)
{
    HIPCHK(op_A<double>(h, h->lv[lv], false, mode, 0, -1, x, b, y, k, ctrl));
    return SMG_OK;
}


// relax(iters) of either cycle on device vectors b / u (pieces, raw interface, test hooks): returns the buffer the result is in through *res -- u or,
// after an odd number of out-of-place launches (Jacobi-type sweeps, the one-launch relax()), the level's second iterate.  (The cycle itself arranges its
// prolongation so that the last sweep lands in u, see enqueue_vcycle_t.)
template <typename T>
static int enqueue_relax(smg_hierarchy* h, int lv, const T* b, T* u, int k, int iters, const Ctrl* ctrl, T** res)
{
    const int kind = level_kind(h, lv);
    const SweepPlan sp = sweep_plan(h, lv, k, iters, std::is_same<T, double>::value, FIRST_NONE);
    T* const buf[2] = {u, vecs<T>(h->lv[lv]).t.p};
    int cur = 0, rc;
    if (kind == LV_GS && !sp.tiled) rc = enqueue_gs<T>(h, lv, sp, b, u, k, iters, ctrl);
    else if (kind == LV_GS) rc = enqueue_gs_tiled<T>(h, *sp.tiled, b, buf, &cur, k, ctrl);
    else if (kind == LV_CHEBY) rc = enqueue_cheby<T>(h, lv, b, buf, &cur, k, iters, ctrl);
    else rc = enqueue_jacobi<T>(h, lv, b, buf, &cur, k, iters, ctrl);
    *res = buf[cur];
    return rc;
}
// the fp64 callers want the result in u
static int enqueue_relax_into(smg_hierarchy* h, int lv, const double* b, double* u, int k, int iters, const Ctrl* ctrl)
{
    double* res = nullptr;
    int rc = enqueue_relax<double>(h, lv, b, u, k, iters, ctrl, &res);
    if (rc) return rc;
    if (res != u) HIPCHK(hipMemcpyAsync(u, res, (size_t)h->lv[lv].n * k * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    return SMG_OK;
}

// The outer residual of iterate z (min_quad_with_fixed_mg.cpp:110) and the first pre-smoothing sweep of the V-cycle that follows
// (mg_VCycle.cpp:36) stream the same matrix against the same z: when this returns true the sweep's launches form both -- the sweep's
// result out of place in L0.t (z itself stays intact for the case that the break test stops the loop), the squared residual through a
// second accumulator that repeats SELL_RESID_SS's additions (SELL_*_HEAD in smg_device.hpp) -- and the cycle starts with FIRST_SWEEP.
// fp64 cycles only (the mixed mode's residual IS the right-hand side of its fp32 cycle); Gauss-Seidel needs a second sweep to come back
// into u; a level 0 that smooths on A^T (non-symmetric storage) forms other sums than the residual.
bool smg::head_fusable(smg_hierarchy* h, int k)
{
    static const int on = env_int("SMG_FUSE_HEAD", 1);
    if (!on || h->precision != 0 || h->n_levels < 2 || h->prof_on || h->bs != 1 || h->union_m > 0) return false;      // (a union needs the residual VECTOR: per-member norms)
    Level& L0 = h->lv[0];
    if (L0.gs_on_transpose) return false;
    // block- / piece-sequential sweeps run in place: their head is the residual launch; a level 0 whose relax(pre) is ONE launch (overlapped tiling):
    // residual launch + one launch beat a head of (colours x 2) launches
    if (!sweep_plan(h, 0, k, h->pre, true, FIRST_NONE).colours()) return false;
    const int kind = level_kind(h, 0);
    return kind == LV_GS ? h->pre >= 2 : h->pre >= 1;
}

// sum of squares of RHS_u - A_0 z_u into ctrl->sumsq  (min_quad_with_fixed_mg.cpp:110 / :332)
int smg::enqueue_residual_ss(smg_hierarchy* h, int k, bool fuse_decide, double* sumsq_out)
{
    Level& L0 = h->lv[0];
    int nb = 0;
    if (h->head_fuse) {
        ProfGuard pg(h, "MG: relaxation");
        const int kind = level_kind(h, 0);
        const SellDev& G = L0.dA.view;
        if (kind == LV_GS) {
            const std::vector<int>& cs = L0.dA.color_slice_ptr;
            for (size_t c = 0; c + 1 < cs.size(); c++) {
                int nbc = 0;
                HIPCHK(launch_sell(SELL_GS_HEAD, G, cs[c], cs[c + 1], L0.u.p, L0.b.p, L0.t.p, k, h->d_ctrl.p, h->d_partials.p + nb, &nbc, h->stream));
                nb += nbc;
            }
        } else if (kind == LV_JACOBI) {
            HIPCHK(launch_sell(SELL_JACOBI_HEAD, G, 0, G.n_slices, L0.u.p, L0.b.p, L0.t.p, k, h->d_ctrl.p, h->d_partials.p, &nb, h->stream, nullptr, nullptr, h->omega));
        } else {
            std::vector<ChebyCoef> cf;
            cheby_coefs(L0.lam, h->cheby_fraction, h->pre + 1, cf);
            FirstColour fc;
            fc.d = L0.d.p;
            fc.c1 = cf[0].c1;
            HIPCHK(launch_sell(SELL_CHEBY_HEAD, G, 0, G.n_slices, L0.u.p, L0.b.p, L0.t.p, k, h->d_ctrl.p, h->d_partials.p, &nb, h->stream, nullptr, &fc, cf[0].c2));
        }
        if (fuse_decide) HIPCHK(launch_ss_finalize_decide(h->d_partials.p, nb, h->d_ctrl.p, h->stream));
        else HIPCHK(launch_ss_finalize(h->d_partials.p, nb, h->d_ctrl.p, h->stream, sumsq_out));
        return SMG_OK;
    }
    ProfGuard pg(h, "MG: outer residual");
    if (h->union_m > 0) {
        // independent meshes in one handle: r = RHS - A z as a vector, then every member's own norm, history and break test (smg_union_device.hip)
        if (!fuse_decide) return fail(SMG_ERR_INVALID, "a union handle runs through smg_solve / smg_solve_begin + smg_raw_outer_iteration (no split-phase iteration: its members stop one by one)");
        HIPCHK(launch_sell(SELL_RESID, L0.dA.view, 0, L0.dA.view.n_slices, L0.u.p, L0.b.p, L0.r.p, k, h->d_ctrl.p, nullptr, nullptr, h->stream));
        HIPCHK(launch_union_sumsq_decide(h->un.view, L0.r.p, L0.u.p, k, h->d_ctrl.p, h->stream));
        return SMG_OK;
    }
    if (h->precision == 1 && h->bs == 3)
        HIPCHK(launch_bsr3(SELL_RESID_BOTH, L0.bA.view, 0, L0.bA.view.n_slices, L0.u.p, L0.b.p, L0.r.p, k, h->d_ctrl.p, h->d_partials.p, &nb, h->stream));
    else if (h->precision == 1)   // mixed: the residual itself is the right-hand side of the fp32 correction cycle
        HIPCHK(launch_sell(SELL_RESID_BOTH, L0.dA.view, 0, L0.dA.view.n_slices, L0.u.p, L0.b.p, L0.r.p, k, h->d_ctrl.p, h->d_partials.p, &nb, h->stream));
    else if (h->bs == 3)
        HIPCHK(launch_bsr3(SELL_RESID_SS, L0.bA.view, 0, L0.bA.view.n_slices, L0.u.p, L0.b.p, nullptr, k, h->d_ctrl.p, h->d_partials.p, &nb, h->stream));
    else
        HIPCHK(launch_sell(SELL_RESID_SS, L0.dA.view, 0, L0.dA.view.n_slices, L0.u.p, L0.b.p, nullptr, k, h->d_ctrl.p, h->d_partials.p, &nb, h->stream));
    if (fuse_decide) HIPCHK(launch_ss_finalize_decide(h->d_partials.p, nb, h->d_ctrl.p, h->stream));
    else HIPCHK(launch_ss_finalize(h->d_partials.p, nb, h->d_ctrl.p, h->stream, sumsq_out));
    return SMG_OK;
}

// d_sumsq == nullptr: the break test already ran inside the residual launch (single-GPU path)
int smg::enqueue_cycle_part(smg_hierarchy* h, int k, const double* d_sumsq)
{
    if (d_sumsq) HIPCHK(launch_decide(h->d_ctrl.p, d_sumsq, h->stream));
    {
        ProfGuard pg(h, "MG: total VCycle");  // PROFC_NODE at src/min_quad_with_fixed_mg.cpp:123
        if (h->precision == 1) {
            // z += V32(r): the V-cycle is affine in (B, u), so V(B, z) = z + V(B - A z, 0) in exact arithmetic
            Level& L0 = h->lv[0];
            const size_t cnt = (size_t)L0.n * k;
            HIPCHK(launch_residual_to_f32(L0.f32.b.p, L0.f32.u.p, L0.r.p, cnt, h->d_ctrl.p, h->stream));
            int rc = enqueue_vcycle(h, k, h->d_ctrl.p, FIRST_NONE);
            if (rc) return rc;
            HIPCHK(launch_add_correction(L0.u.p, L0.f32.u.p, cnt, h->d_ctrl.p, h->stream));
        } else {
            int rc = enqueue_vcycle(h, k, h->d_ctrl.p, h->head_fuse ? FIRST_SWEEP : FIRST_NONE);
            if (rc) return rc;
            if (h->union_m > 0) HIPCHK(launch_union_restore(h->un.view, h->lv[0].u.p, k, h->d_ctrl.p, h->stream));   // members whose loop has ended keep their iterate
        }
    }
    return SMG_OK;
}

// The sparse triangular solves raise c_err when a wait gave up (smg_coarse_device.hip): the values they then wrote are NaN.  Every entry point
// that has just synchronised with work that may contain such a solve reads the flag, clears it (it is sticky on the device: later waits give
// up at once while it is set) and fails with SMG_ERR_HIP.  The stream is idle when this runs.
int smg::coarse_stall_check(smg_hierarchy* h)
{
    if (!h->coarse_sparse || !h->c_err.p) return SMG_OK;
    int cerr = 0;
    HIPCHK(hipMemcpy(&cerr, h->c_err.p, sizeof(int), hipMemcpyDeviceToHost));
    if (!cerr) return SMG_OK;
    (void)hipMemset(h->c_err.p, 0, sizeof(int));
    return fail(SMG_ERR_HIP, "the triangular solves of the sparse coarse factorisation stalled (results are NaN)");
}

int smg::check_ready(const smg_hierarchy* h, const char* who)
{
    if (!h) return fail(SMG_ERR_INVALID, "%s: null handle", who);
    if (!h->precomputed) return fail(SMG_ERR_INVALID, "%s: call smg_precompute first", who);
    if (h->device < 0) return fail(SMG_ERR_NO_DEVICE, "%s: no HIP device", who);
    return SMG_OK;
}

// Columns of the solve's internal (row-major n x kin) blocks.  The kernels for 8 and more columns read a row's columns as 64- to 512-byte
// segments; a row length that is no multiple of such a segment puts every row across cache-line boundaries and splits the columns over a
// wide and one or two narrow launches per operation.  C3, ms per outer iteration (tools/k_solve_time.py, same box, SMG_PAD_COLS=0 / 1):
//   k = 5: 1.068 / 1.044   6: 1.180 / 1.045   7: 1.393 / 1.066   (8: 0.97)   12: 1.981 / 1.602   13: 2.857 / 1.602   (16: 1.60)
//   24: 2.91 / 2.87   48: 4.59 / 4.34   (64: 4.33);  33 columns as 64: 4.10 -> 4.37 -- not padded.
// So 5 - 32 columns run as the next power of two and 41 - 63 as 64, with zero columns as padding: a zero right-hand side and iterate stay
// exactly zero through every kernel of the cycle and add exact zeros to the residual's sum of squares.  The sparse kernels compute every
// column independently of how many others there are, and the dense coarse product is formed for the caller's columns only (coarse_cols
// above), so the caller's columns come out bit for bit as without padding (the tool prints a checksum of z; SMG_PAD_COLS=0: A/B knob).
// (Schur / sparse coarse solvers take the padded block as it is.)  Union handles keep their own per-member bookkeeping and are not padded.
int smg::internal_cols(const smg_hierarchy* h, int k)
{
    static const int on = env_int("SMG_PAD_COLS", 1);
    if (!on || k <= 4 || k > 64 || h->union_m > 0) return k;
    if (k > 32) return k > 40 ? 64 : k;
    int p = 8;
    while (p < k) p *= 2;
    return p;
}

static int piece_prolog(smg_hierarchy* h, int lv, int k, const char* who, bool need_coarser);

// replays of graph g (3 warm, then `reps` timed): microseconds per replay; destroys g
static int time_graph(smg_hierarchy* h, hipGraphExec_t g, int reps, double* us)
{
    hipEvent_t e0, e1;
    HIPCHK(hipEventCreate(&e0));
    HIPCHK(hipEventCreate(&e1));
    for (int i = 0; i < 3; i++) HIPCHK(hipGraphLaunch(g, h->stream));
    HIPCHK(hipEventRecord(e0, h->stream));
    for (int i = 0; i < reps; i++) HIPCHK(hipGraphLaunch(g, h->stream));
    HIPCHK(hipEventRecord(e1, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, e0, e1));
    *us = 1e3 * ms / reps;
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1); (void)hipGraphExecDestroy(g);
    return SMG_OK;
}

extern "C" int smg_bench_vcycle(smg_hierarchy* h, int lv, int k, int pre, int post, int reps, double* us_per_cycle)
{
    int rc = piece_prolog(h, lv, k, "smg_bench_vcycle", false);
    if (rc) return rc;
    DeviceScope dsc(h->device);
    if (reps < 1 || !us_per_cycle) return fail(SMG_ERR_INVALID, "smg_bench_vcycle: bad arguments");
    if ((rc = prepare_sweep_plans(h, k, pre, post))) return rc;
    hipGraphExec_t g = nullptr;
    rc = capture_graph(h, &g, [&]() { return enqueue_vcycle_t<double>(h, lv, k, pre, post, nullptr); });
    if (rc) return rc;
    if ((rc = time_graph(h, g, reps, us_per_cycle))) return rc;
    return coarse_stall_check(h);
}

extern "C" int smg_bench_relax(smg_hierarchy* h, int lv, int k, int sweeps, int reps, double* us_per_call)
{
    int rc = piece_prolog(h, lv, k, "smg_bench_relax", true);
    if (rc) return rc;
    DeviceScope dsc(h->device);
    if (reps < 1 || sweeps < 1 || !us_per_call) return fail(SMG_ERR_INVALID, "smg_bench_relax: bad arguments");
    if ((rc = prepare_sweep_plans(h, k, sweeps, sweeps))) return rc;
    Level& Lv = h->lv[lv];
    hipGraphExec_t g = nullptr;
    rc = capture_graph(h, &g, [&]() { return enqueue_relax_into(h, lv, Lv.b.p, Lv.u.p, k, sweeps, nullptr); });
    if (rc) return rc;
    return time_graph(h, g, reps, us_per_call);
}

extern "C" int smg_synchronize(smg_hierarchy* h)
{
    if (!h || h->device < 0) return fail(SMG_ERR_INVALID, "smg_synchronize: no device");
    DeviceScope dsc(h->device);
    HIPCHK(hipStreamSynchronize(h->stream));
    return coarse_stall_check(h);
}

// ------------------------------------------------------------------------------------------------ V-cycle pieces (host blocks)
extern "C" int smg_level_rows(const smg_hierarchy* h, int lv)
{
    if (!h || lv < 0 || lv >= h->n_levels) return SMG_ERR_INVALID;
    return h->lv[lv].n;
}

// host column-major (caller numbering of level lv) -> device internal layout
template <typename T>
static int put_block(smg_hierarchy* h, int lv, const T* src, int k, T* dst)
{
    const Level& Lv = h->lv[lv];
    std::vector<T> tmp((size_t)Lv.n * k);
    for (int i = 0; i < Lv.n; i++)
        for (int c = 0; c < k; c++) tmp[(size_t)i * k + c] = src[(size_t)Lv.ord.perm[i] + (size_t)c * Lv.n];
    HIPCHK(hipMemcpyAsync(dst, tmp.data(), tmp.size() * sizeof(T), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return SMG_OK;
}
template <typename T>
static int get_block(smg_hierarchy* h, int lv, const T* src, int k, T* dst)
{
    const Level& Lv = h->lv[lv];
    std::vector<T> tmp((size_t)Lv.n * k);
    HIPCHK(hipMemcpyAsync(tmp.data(), src, tmp.size() * sizeof(T), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    for (int i = 0; i < Lv.n; i++)
        for (int c = 0; c < k; c++) dst[(size_t)Lv.ord.perm[i] + (size_t)c * Lv.n] = tmp[(size_t)i * k + c];
    return coarse_stall_check(h);      // (the pieces' results leave through here: a stalled coarse solve must not pass for a result)
}

static int piece_prolog(smg_hierarchy* h, int lv, int k, const char* who, bool need_coarser)
{
    int rc = check_ready(h, who);
    if (rc) return rc;
    if (h->in_solve) return fail(SMG_ERR_INVALID, "%s: a split-phase solve is in progress", who);
    if (lv < 0 || lv >= h->n_levels || (need_coarser && lv >= h->n_levels - 1) || k < 1)
        return fail(SMG_ERR_INVALID, "%s: bad level %d or k %d", who, lv, k);
    DeviceScope dsc(h->device);
    return ensure_work(h, k);
}

extern "C" int smg_apply_A(smg_hierarchy* h, int lv, const double* u, int k, double* Au)
{
    int rc = piece_prolog(h, lv, k, "smg_apply_A", true);
    if (rc) return rc;
    DeviceScope dsc(h->device);
    Level& Lv = h->lv[lv];
    if ((rc = put_block(h, lv, u, k, Lv.u.p))) return rc;
    HIPCHK(op_A<double>(h, Lv, false, SELL_AX, 0, -1, Lv.u.p, nullptr, Lv.r.p, k, nullptr));
    return get_block(h, lv, Lv.r.p, k, Au);
}

extern "C" int smg_restrict(smg_hierarchy* h, int lv, const double* x, int k, double* Rx)
{
    int rc = piece_prolog(h, lv, k, "smg_restrict", true);
    if (rc) return rc;
    DeviceScope dsc(h->device);
    Level &Lv = h->lv[lv], &Lc = h->lv[lv + 1];
    if ((rc = put_block(h, lv, x, k, Lv.r.p))) return rc;
    HIPCHK(launch_sell(SELL_AX, Lc.dPT.view, 0, Lc.dPT.view.n_slices, Lv.r.p, nullptr, Lc.b.p, k * h->bs, nullptr, nullptr, nullptr, h->stream));
    return get_block(h, lv + 1, Lc.b.p, k, Rx);
}

extern "C" int smg_prolong(smg_hierarchy* h, int lv, const double* x, int k, double* Px)
{
    int rc = piece_prolog(h, lv, k, "smg_prolong", true);
    if (rc) return rc;
    DeviceScope dsc(h->device);
    Level &Lv = h->lv[lv], &Lc = h->lv[lv + 1];
    if ((rc = put_block(h, lv + 1, x, k, Lc.u.p))) return rc;
    HIPCHK(launch_sell(SELL_AX, Lc.dP.view, 0, Lc.dP.view.n_slices, Lc.u.p, nullptr, Lv.r.p, k * h->bs, nullptr, nullptr, nullptr, h->stream));
    return get_block(h, lv, Lv.r.p, k, Px);
}

extern "C" int smg_relax(smg_hierarchy* h, int lv, const double* B, int k, int iters, double* u)
{
    int rc = piece_prolog(h, lv, k, "smg_relax", true);
    if (rc) return rc;
    DeviceScope dsc(h->device);
    Level& Lv = h->lv[lv];
    if ((rc = prepare_sweep_plans(h, k, iters, iters))) return rc;
    if ((rc = put_block(h, lv, B, k, Lv.b.p))) return rc;
    if ((rc = put_block(h, lv, u, k, Lv.u.p))) return rc;
    if ((rc = enqueue_relax_into(h, lv, Lv.b.p, Lv.u.p, k, iters, nullptr))) return rc;
    return get_block(h, lv, Lv.u.p, k, u);
}

extern "C" int smg_coarse_solve(smg_hierarchy* h, const double* B, int k, double* u)
{
    const int lv = h ? h->n_levels - 1 : 0;
    int rc = piece_prolog(h, lv, k, "smg_coarse_solve", false);
    if (rc) return rc;
    DeviceScope dsc(h->device);
    Level& Lv = h->lv[lv];
    if ((rc = put_block(h, lv, B, k, Lv.b.p))) return rc;
    if ((rc = put_block(h, lv, u, k, Lv.u.p))) return rc;
    HIPCHK(coarse_solve<double>(h, Lv, k, nullptr));
    return get_block(h, lv, Lv.u.p, k, u);
}

extern "C" int smg_vcycle(smg_hierarchy* h, const double* B, int pre, int post, int lv, double* u, int k)
{
    int rc = piece_prolog(h, lv, k, "smg_vcycle", false);
    if (rc) return rc;
    DeviceScope dsc(h->device);
    Level& Lv = h->lv[lv];
    if ((rc = prepare_sweep_plans(h, k, pre, post))) return rc;
    if ((rc = put_block(h, lv, B, k, Lv.b.p))) return rc;
    if ((rc = put_block(h, lv, u, k, Lv.u.p))) return rc;
    if ((rc = enqueue_vcycle_t<double>(h, lv, k, pre, post, nullptr))) return rc;
    return get_block(h, lv, Lv.u.p, k, u);
}

extern "C" int smg_residual_norm(smg_hierarchy* h, int lv, const double* B, const double* u, int k, double* norm)
{
    int rc = piece_prolog(h, lv, k, "smg_residual_norm", true);
    if (rc) return rc;
    DeviceScope dsc(h->device);
    Level& Lv = h->lv[lv];
    if ((rc = put_block(h, lv, B, k, Lv.b.p))) return rc;
    if ((rc = put_block(h, lv, u, k, Lv.u.p))) return rc;
    int nb = 0;
    if ((rc = reset_ctrl(h, (int)h->d_rhis.n))) return rc;
    if (h->bs == 3) HIPCHK(launch_bsr3(SELL_RESID_SS, Lv.bA.view, 0, Lv.bA.view.n_slices, Lv.u.p, Lv.b.p, nullptr, k, nullptr, h->d_partials.p, &nb, h->stream));
    else HIPCHK(launch_sell(SELL_RESID_SS, Lv.dA.view, 0, Lv.dA.view.n_slices, Lv.u.p, Lv.b.p, nullptr, k, nullptr, h->d_partials.p, &nb, h->stream));
    HIPCHK(launch_ss_finalize(h->d_partials.p, nb, h->d_ctrl.p, h->stream));
    double ss = 0.0;
    HIPCHK(hipMemcpyAsync(&ss, &h->d_ctrl.p->sumsq, sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    *norm = std::sqrt(ss);
    return SMG_OK;
}

// ------------------------------------------------------------------------------------------------ the fp32 cycle, piece by piece (test hooks)
// What enqueue_vcycle_t<float> launches for one piece, on the handle's own fp32 buffers, with the handle's control block (whose `done` flag the
// caller picks) -- see include/smg.h, smg_debug_cycle_f32.

// the control block the launches of a hook get: fresh, with the chosen flag
static int hook_ctrl(smg_hierarchy* h, int done)
{
    int rc = reset_ctrl(h, 1);
    if (rc) return rc;
    if (done) {
        static const int one = 1;
        HIPCHK(hipMemcpyAsync(&h->d_ctrl.p->done, &one, sizeof(int), hipMemcpyHostToDevice, h->stream));
    }
    HIPCHK(hipStreamSynchronize(h->stream));
    return SMG_OK;
}

// leaves the handle's control block fresh (not done) however the hook returns
struct HookCtrlReset {
    smg_hierarchy* h;
    ~HookCtrlReset() { if (reset_ctrl(h, 1) == SMG_OK) (void)hipStreamSynchronize(h->stream); }
};

// Every fp32 vector a launch of the cycle may write -- the LevelVecs<float> of every level, the Schur solver's g32 / xs32 -- whole
// allocations, as bytes: with the done flag set none of them may change between the uploads and the end of the launches.
static int snapshot_f32(smg_hierarchy* h, std::vector<float>& out)
{
    out.clear();
    std::vector<const DevBuf<float>*> bufs;
    for (const Level& Lv : h->lv) LevelVecs<float>::each(Lv.f32, [&](const DevBuf<float>& v) { bufs.push_back(&v); });
    bufs.push_back(&h->sch.g32); bufs.push_back(&h->sch.xs32);
    size_t total = 0;
    for (const DevBuf<float>* b : bufs) total += b->n;
    out.resize(total);
    size_t off = 0;
    for (const DevBuf<float>* b : bufs) {
        if (b->n) HIPCHK(hipMemcpyAsync(out.data() + off, b->p, b->n * sizeof(float), hipMemcpyDeviceToHost, h->stream));
        off += b->n;
    }
    HIPCHK(hipStreamSynchronize(h->stream));
    return SMG_OK;
}

// the n x k head of a device buffer against the host block that was uploaded there (same permutation): 1 when a bit differs
template <typename T>
static int block_changed(smg_hierarchy* h, int lv, const T* dev, int k, const T* uploaded, int* changed)
{
    const Level& Lv = h->lv[lv];
    std::vector<T> now((size_t)Lv.n * k);
    int rc = get_block<T>(h, lv, dev, k, now.data());
    if (rc) return rc;
    if (std::memcmp(now.data(), uploaded, now.size() * sizeof(T)) != 0) *changed = 1;
    return SMG_OK;
}

extern "C" int smg_debug_cycle_f32(smg_hierarchy* h, int op, int lv, int k, int pre, int post, int done, const float* in0, const float* in1,
                                   float* out, int* inputs_changed)
{
    return guarded("smg_debug_cycle_f32", [&]() -> int {
        if (!h) return fail(SMG_ERR_INVALID, "smg_debug_cycle_f32: null handle");
        if (op < SMG_F32_A || op > SMG_F32_VCYCLE) return fail(SMG_ERR_INVALID, "smg_debug_cycle_f32: unknown op %d", op);
        if (op == SMG_F32_COARSE) lv = h->n_levels - 1;
        const bool two_in = op == SMG_F32_RESID;
        if (!in0 || !out || (two_in && !in1) || pre < 0 || post < 0) return fail(SMG_ERR_INVALID, "smg_debug_cycle_f32: missing array or negative sweep count");
        int rc = piece_prolog(h, lv, k, "smg_debug_cycle_f32", op != SMG_F32_COARSE && op != SMG_F32_VCYCLE);
        if (rc) return rc;
        DeviceScope dsc(h->device);
        if ((rc = ensure_fp32(h, k))) return rc;
        if ((rc = prepare_sweep_plans(h, k, pre, post))) return rc;
        HookCtrlReset reset_on_exit{h};
        if ((rc = hook_ctrl(h, done))) return rc;
        const Ctrl* ctrl = h->d_ctrl.p;
        const int L = h->n_levels;
        Level& Lv = h->lv[lv];
        LevelVecs<float>& F = Lv.f32;
        int changed = 0;
        std::vector<float> before, after;
        auto uploaded = [&]() -> int { return done ? snapshot_f32(h, before) : SMG_OK; };   // called between an op's uploads and its launches
        switch (op) {
            case SMG_F32_A:          // out = A in0
                if ((rc = put_block<float>(h, lv, in0, k, F.u.p))) return rc;
                if ((rc = put_block<float>(h, lv, out, k, F.r.p)) || (rc = uploaded())) return rc;
                HIPCHK(op_A<float>(h, Lv, false, SELL_AX, 0, -1, F.u.p, nullptr, F.r.p, k, ctrl));
                if ((rc = block_changed<float>(h, lv, F.u.p, k, in0, &changed))) return rc;
                rc = get_block<float>(h, lv, F.r.p, k, out);
                break;
            case SMG_F32_RESID:      // out = in0 - A in1: the residual launch of the cycle
                if ((rc = put_block<float>(h, lv, in0, k, F.b.p))) return rc;
                if ((rc = put_block<float>(h, lv, in1, k, F.u.p))) return rc;
                if ((rc = put_block<float>(h, lv, out, k, F.r.p)) || (rc = uploaded())) return rc;
                HIPCHK(op_A<float>(h, Lv, false, SELL_RESID, 0, -1, F.u.p, F.b.p, F.r.p, k, ctrl));
                if ((rc = block_changed<float>(h, lv, F.b.p, k, in0, &changed))) return rc;
                if ((rc = block_changed<float>(h, lv, F.u.p, k, in1, &changed))) return rc;
                rc = get_block<float>(h, lv, F.r.p, k, out);
                break;
            case SMG_F32_RESTRICT: { // out = [PT in0 | the zeroed coarse iterate]: the restriction launch without a fused first launch
                Level& Lc = h->lv[lv + 1];
                LevelVecs<float>& Fc = Lc.f32;
                const size_t cc = (size_t)Lc.n * k;
                if ((rc = put_block<float>(h, lv, in0, k, F.r.p))) return rc;
                if ((rc = put_block<float>(h, lv + 1, out, k, Fc.b.p))) return rc;
                if ((rc = put_block<float>(h, lv + 1, out + cc, k, Fc.u.p)) || (rc = uploaded())) return rc;
                HIPCHK(launch_sell(SELL_AX, Lc.dPT.view, 0, Lc.dPT.view.n_slices, F.r.p, nullptr, Fc.b.p, k * h->bs, ctrl, nullptr, nullptr, h->stream, Fc.u.p));
                if ((rc = block_changed<float>(h, lv, F.r.p, k, in0, &changed))) return rc;
                if ((rc = get_block<float>(h, lv + 1, Fc.b.p, k, out))) return rc;
                rc = get_block<float>(h, lv + 1, Fc.u.p, k, out + cc);
                break;
            }
            case SMG_F32_PROLONG_ADD: { // out += P in0
                Level& Lc = h->lv[lv + 1];
                LevelVecs<float>& Fc = Lc.f32;
                if ((rc = put_block<float>(h, lv + 1, in0, k, Fc.u.p))) return rc;
                if ((rc = put_block<float>(h, lv, out, k, F.u.p)) || (rc = uploaded())) return rc;
                HIPCHK(launch_sell(SELL_ADD, Lc.dP.view, 0, Lc.dP.view.n_slices, Fc.u.p, F.u.p, F.u.p, k * h->bs, ctrl, nullptr, nullptr, h->stream));
                if ((rc = block_changed<float>(h, lv + 1, Fc.u.p, k, in0, &changed))) return rc;
                rc = get_block<float>(h, lv, F.u.p, k, out);
                break;
            }
            case SMG_F32_RELAX: {    // out = relax(pre) of out with right-hand side in0
                if ((rc = put_block<float>(h, lv, in0, k, F.b.p))) return rc;
                if ((rc = put_block<float>(h, lv, out, k, F.u.p))) return rc;
                if (level_is_jacobi(h, lv) && (rc = put_block<float>(h, lv, out, k, F.t.p))) return rc;   // the second iterate: an output, too
                float* res = nullptr;
                if ((rc = uploaded())) return rc;
                if ((rc = enqueue_relax<float>(h, lv, F.b.p, F.u.p, k, pre, ctrl, &res))) return rc;
                if ((rc = block_changed<float>(h, lv, F.b.p, k, in0, &changed))) return rc;
                rc = get_block<float>(h, lv, res, k, out);
                break;
            }
            case SMG_F32_COARSE:     // out += A^-1 in0 on the coarsest level
                if ((rc = put_block<float>(h, lv, in0, k, F.b.p))) return rc;
                if ((rc = put_block<float>(h, lv, out, k, F.u.p)) || (rc = uploaded())) return rc;
                HIPCHK(coarse_solve<float>(h, Lv, k, ctrl));
                if ((rc = block_changed<float>(h, lv, F.b.p, k, in0, &changed))) return rc;
                rc = get_block<float>(h, lv, F.u.p, k, out);
                break;
            case SMG_F32_VCYCLE:     // out = V(pre, post) from level lv with right-hand side in0
                if ((rc = put_block<float>(h, lv, in0, k, F.b.p))) return rc;
                if ((rc = put_block<float>(h, lv, out, k, F.u.p))) return rc;
                if (lv < L - 1 && level_is_jacobi(h, lv) && (rc = put_block<float>(h, lv, out, k, F.t.p))) return rc;
                if ((rc = uploaded())) return rc;
                if ((rc = enqueue_vcycle_t<float>(h, lv, k, pre, post, ctrl))) return rc;
                if ((rc = block_changed<float>(h, lv, F.b.p, k, in0, &changed))) return rc;
                rc = get_block<float>(h, lv, F.u.p, k, out);
                break;
        }
        if (rc) return rc;
        if (done) {      // nothing the cycle owns in fp32 may have moved: the second iterate, the update vector and the coarser levels included
            if ((rc = snapshot_f32(h, after))) return rc;
            if (before.size() != after.size() || std::memcmp(before.data(), after.data(), after.size() * sizeof(float)) != 0) changed |= 4;
        }
        if (inputs_changed) *inputs_changed = changed;
        return SMG_OK;
    });
}

// the two converters between the fp64 outer loop and the fp32 cycle, on level 0's own buffers.  The room of a buffer behind the n0 x k block
// (a handle that has served more columns before) is filled with sentinel bytes first and must still hold them afterwards.
extern "C" int smg_debug_convert_f32(smg_hierarchy* h, int op, int k, int done, const double* in64, const float* in32, double* out64, float* out_b32,
                                     float* out_u32, int* inputs_changed)
{
    return guarded("smg_debug_convert_f32", [&]() -> int {
        if (!h) return fail(SMG_ERR_INVALID, "smg_debug_convert_f32: null handle");
        if (op != SMG_F32_RESIDUAL_TO_F32 && op != SMG_F32_ADD_CORRECTION) return fail(SMG_ERR_INVALID, "smg_debug_convert_f32: unknown op %d", op);
        if (op == SMG_F32_RESIDUAL_TO_F32 ? (!in64 || !out_b32 || !out_u32) : (!in32 || !out64)) return fail(SMG_ERR_INVALID, "smg_debug_convert_f32: missing array");
        int rc = piece_prolog(h, 0, k, "smg_debug_convert_f32", false);
        if (rc) return rc;
        DeviceScope dsc(h->device);
        if ((rc = ensure_fp32(h, k))) return rc;
        HookCtrlReset reset_on_exit{h};
        if ((rc = hook_ctrl(h, done))) return rc;
        const Ctrl* ctrl = h->d_ctrl.p;
        Level& L0 = h->lv[0];
        LevelVecs<float>& F = L0.f32;
        const size_t cnt = (size_t)L0.n * k;
        int changed = 0;
        // sentinel bytes behind the block, checked after the launch, then cleared again (the buffers start out as zeros)
        auto tail_fill = [&](void* p, size_t have, size_t elem, int byte) -> int {
            if (have > cnt) HIPCHK(hipMemsetAsync((char*)p + cnt * elem, byte, (have - cnt) * elem, h->stream));
            return SMG_OK;
        };
        auto tail_check = [&](const void* p, size_t have, size_t elem) -> int {
            if (have <= cnt) return SMG_OK;
            std::vector<unsigned char> t((have - cnt) * elem);
            HIPCHK(hipMemcpyAsync(t.data(), (const char*)p + cnt * elem, t.size(), hipMemcpyDeviceToHost, h->stream));
            HIPCHK(hipStreamSynchronize(h->stream));
            for (unsigned char c : t) if (c != 0x5B) { changed |= 2; break; }
            return SMG_OK;
        };
        if (op == SMG_F32_RESIDUAL_TO_F32) {      // b32 = (float) r, u32 = 0
            if (h->n_levels < 2) return fail(SMG_ERR_INVALID, "smg_debug_convert_f32: a one-level handle has no residual vector");
            if ((rc = put_block<double>(h, 0, in64, k, L0.r.p))) return rc;
            if ((rc = put_block<float>(h, 0, out_b32, k, F.b.p))) return rc;
            if ((rc = put_block<float>(h, 0, out_u32, k, F.u.p))) return rc;
            if ((rc = tail_fill(F.b.p, F.b.n, sizeof(float), 0x5B)) || (rc = tail_fill(F.u.p, F.u.n, sizeof(float), 0x5B))) return rc;
            HIPCHK(launch_residual_to_f32(F.b.p, F.u.p, L0.r.p, cnt, ctrl, h->stream));
            if ((rc = tail_check(F.b.p, F.b.n, sizeof(float))) || (rc = tail_check(F.u.p, F.u.n, sizeof(float)))) return rc;
            if ((rc = tail_fill(F.b.p, F.b.n, sizeof(float), 0)) || (rc = tail_fill(F.u.p, F.u.n, sizeof(float), 0))) return rc;
            if ((rc = block_changed<double>(h, 0, L0.r.p, k, in64, &changed))) return rc;
            if ((rc = get_block<float>(h, 0, F.b.p, k, out_b32))) return rc;
            if ((rc = get_block<float>(h, 0, F.u.p, k, out_u32))) return rc;
        } else {                                  // z += (double) e
            if ((rc = put_block<double>(h, 0, out64, k, L0.u.p))) return rc;
            if ((rc = put_block<float>(h, 0, in32, k, F.u.p))) return rc;
            if ((rc = tail_fill(L0.u.p, L0.u.n, sizeof(double), 0x5B))) return rc;
            HIPCHK(launch_add_correction(L0.u.p, F.u.p, cnt, ctrl, h->stream));
            if ((rc = tail_check(L0.u.p, L0.u.n, sizeof(double)))) return rc;
            if ((rc = tail_fill(L0.u.p, L0.u.n, sizeof(double), 0))) return rc;
            if ((rc = block_changed<float>(h, 0, F.u.p, k, in32, &changed))) return rc;
            if ((rc = get_block<double>(h, 0, L0.u.p, k, out64))) return rc;
        }
        if (inputs_changed) *inputs_changed = changed;
        return SMG_OK;
    });
}

// ------------------------------------------------------------------------------------------------ raw device interface
extern "C" int smg_raw_spmv(smg_hierarchy* h, int lv, int mode, const double* x, const double* b, double* y, int k)
{
    int rc = check_ready(h, "smg_raw_spmv");
    if (rc) return rc;
    DeviceScope dsc(h->device);
    if (lv < 0 || lv >= h->n_levels - 1 || k < 1 || (mode != SELL_AX && mode != SELL_RESID && mode != SELL_ADD))
        return fail(SMG_ERR_INVALID, "smg_raw_spmv: bad level/mode");
    Level& Lv = h->lv[lv];
    if (h->bs == 3) {
        if (mode == SELL_ADD) return fail(SMG_ERR_INVALID, "smg_raw_spmv: y += A x is not available on block (3-DOF) hierarchies");
        HIPCHK(launch_bsr3((SellMode)mode, Lv.bA.view, 0, Lv.bA.view.n_slices, x, b, y, k, nullptr, nullptr, nullptr, h->stream));
        return SMG_OK;
    }
    HIPCHK(launch_sell((SellMode)mode, Lv.dA.view, 0, Lv.dA.view.n_slices, x, b, y, k, nullptr, nullptr, nullptr, h->stream));
    return SMG_OK;
}

extern "C" int smg_raw_spmv_f32(smg_hierarchy* h, int lv, const float* x, float* y, int k)
{
    int rc = check_ready(h, "smg_raw_spmv_f32");
    if (rc) return rc;
    DeviceScope dsc(h->device);
    if (lv < 0 || lv >= h->n_levels - 1 || k < 1) return fail(SMG_ERR_INVALID, "smg_raw_spmv_f32: bad level");
    if ((rc = ensure_work(h, k))) return rc;
    if ((rc = ensure_fp32(h, k))) return rc;
    Level& Lv = h->lv[lv];
    HIPCHK(launch_sell(SELL_AX, Lv.dA.view, 0, Lv.dA.view.n_slices, x, nullptr, y, k, nullptr, nullptr, nullptr, h->stream));
    return SMG_OK;
}

extern "C" int smg_raw_relax(smg_hierarchy* h, int lv, const double* b, double* u, int k, int iters)
{
    int rc = check_ready(h, "smg_raw_relax");
    if (rc) return rc;
    DeviceScope dsc(h->device);
    if (lv < 0 || lv >= h->n_levels - 1 || k < 1) return fail(SMG_ERR_INVALID, "smg_raw_relax: bad level");
    if ((rc = ensure_work(h, k))) return rc;   // second iterate / update vector / spectral bound of a Jacobi-type level
    if ((rc = prepare_sweep_plans(h, k, iters, iters))) return rc;
    return enqueue_relax_into(h, lv, b, u, k, iters, nullptr);
}

// Algorithmic bytes of one outer iteration OF THE CYCLE THE HANDLE IS SET TO RUN (smoother selection of the
// last solve / smg_hierarchy_set_smoother): per smoothed level
//   relax(iters), Gauss-Seidel:      iters sweeps of  matA + 24 n k  [b, u read, u write]   (the reference also reads A_diag: +8n; the
//                                    HIP kernel takes the diagonal from the row, so it is not counted)
//   relax(iters), damped Jacobi:     iters sweeps of  matA + 24 n k
//   relax(iters), Chebyshev-Jacobi:  ONE polynomial of degree iters + 1 = iters + 1 passes of  matA + 40 n k  [b, u, d read; u, d write],
//                                    the first without the read of d
//   residual:             matA + 24 n k
//   restrict:             12 nnzPT + 4(nc+1) + 8 n k + 8 nc k
//   prolong-add:          12 nnzP + 4(n+1) + 8 nc k + 16 n k
//   + coarsest dense solve 8 nc^2 + 24 nc k, + outer residual matA_0 + 16 n0 k.
// matA = 12 nnz + 4(n+1); on a block hierarchy 76 bytes per 3 x 3 block + 4(n/3+1), and P (x) I_3 streams its vertex-level factor once.
extern "C" long smg_vcycle_bytes(const smg_hierarchy* h, int k, int pre, int post)
{
    if (!h || !h->precomputed) return -1;
    long tot = 0;
    const int L = h->n_levels;
    for (int lv = 0; lv < L - 1; lv++) {
        const Level &Lv = h->lv[lv], &Lc = h->lv[lv + 1];
        const long n = Lv.n, nc = Lc.n, nnz = Lv.A.nnz();
        const long nnzP = h->bs == 3 ? Lc.Pv.nnz() : Lc.P.nnz();
        const long matA = h->bs == 3 ? 76 * Lv.bA.blocks + 4 * (n / 3 + 1) : 12 * nnz + 4 * (n + 1);
        auto relax_bytes = [&](int iters) -> long {
            if (iters <= 0) return 0;
            if (level_kind(h, lv) == LV_CHEBY) return (long)(iters + 1) * (matA + 40 * n * k) - 8 * n * k;
            return (long)iters * (matA + 24 * n * k);
        };
        tot += relax_bytes(pre) + relax_bytes(post);
        tot += matA + 24 * n * k;
        tot += 12 * nnzP + 4 * (nc + 1) + 8 * n * k + 8 * nc * k;
        tot += 12 * nnzP + 4 * (n + 1) + 8 * nc * k + 16 * n * k;
    }
    const long nc = h->lv[L - 1].n;
    if (h->coarse_sparse) tot += (2 * 12 * h->chol.nnzL() + 3 * 8 * nc + 24 * nc) * k;    // both triangles of L, once per column
    else if (h->coarse_schur) tot += 8 * (h->schur.off_P + 2 * (h->schur.off_S - h->schur.off_W) + (long)h->schur.ns_pad * h->schur.ns_pad) + 24 * nc * k;   // blocks, the panels twice, S^-1
    else tot += 8 * nc * nc + 24 * nc * k;
    if (h->bs == 3) tot += 76 * h->lv[0].bA.blocks + 4L * (h->lv[0].n / 3 + 1) + 16L * h->lv[0].n * k;
    else tot += 12 * h->lv[0].A.nnz() + 4L * (h->lv[0].n + 1) + 16L * h->lv[0].n * k;
    return tot;
}
