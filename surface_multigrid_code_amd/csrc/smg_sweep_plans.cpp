// smg_sweep_plans.cpp -- the plan-based Gauss-Seidel sweeps of a level: which one a level uses (sweep_plan), building the plans on demand,
// refreshing their copies of the level values, dropping them, their introspection entry points and their host-side self-checks.  The plans:
// overlapped tiling (smg_tiled.hpp), wave Gauss-Seidel (smg_wgs.hpp), block Gauss-Seidel (smg_bgs.hpp); without one a level sweeps one launch per colour.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <vector>

#include "smg_internal.hpp"

using namespace smg;

// ------------------------------------------------------------------------------------------------ which levels want which plan
// every plan: scalar hierarchies, a smoothed level, Gauss-Seidel
static bool gs_plan_level(const smg_hierarchy* h, int lv)
{
    return h->bs == 1 && lv >= 0 && lv < h->n_levels - 1 && level_kind(h, lv) == LV_GS;
}

// ---- wave Gauss-Seidel on the Galerkin levels of decimated hierarchies: one launch per PIECE colour ------------------
// Which levels: scalar fp64 hierarchies, Gauss-Seidel, any number of columns, SMG_WGS_MIN_ROWS <= rows <= SMG_WGS_MAX_ROWS, no one-launch relax()
// (overlapped tiling) available; automatic mode: only levels the colour launches serve badly -- more than TILED_NCMAX colours or rows of more
// than TILED_WMAX entries, i.e. the Galerkin levels of the reference's own hierarchies (mg_precompute).  smg_hierarchy_set_wave_gs / SMG_WGS=0|1|2.
static int wgs_mode_now(const smg_hierarchy* h)
{
    static const int env = env_int("SMG_WGS", -1);
    return env >= 0 ? (env == 0 ? 0 : env == 1 ? -1 : 1) : h->wgs_mode;      // SMG_WGS: 0 off, 1 automatic, 2 every level in range
}
static bool wgs_in_range(const smg_hierarchy* h, int lv)
{
    static const int max_rows = env_int("SMG_WGS_MAX_ROWS", 600000), min_rows = env_int("SMG_WGS_MIN_ROWS", 512);
    return h->precision == 0 && gs_plan_level(h, lv) && h->lv[lv].n >= min_rows && h->lv[lv].n <= max_rows;
}
// mode 1 (every Gauss-Seidel level in range): what the level needs to sweep piece-wise, whatever k -- such a level takes no one-launch relax (tiled_wanted)
static bool wgs_forced(const smg_hierarchy* h, int lv) { return wgs_mode_now(h) == 1 && wgs_in_range(h, lv); }
static bool wgs_wanted(const smg_hierarchy* h, int lv, int k)
{
    const int mode = wgs_mode_now(h);
    if (mode == 0 || k < 1 || !wgs_in_range(h, lv)) return false;      // (every k: the order of a level's sweep must not depend on how the columns are sharded)
    if (mode == 1) return true;
    const Level& Lv = h->lv[lv];
    const SellBuf& Gs = Lv.gs_on_transpose ? Lv.dAT : Lv.dA;
    return Lv.ord.n_colors() > TILED_NCMAX || Gs.view.w_max > TILED_WMAX;
}
static const WgsBuf* wgs_plan(const smg_hierarchy* h, int lv, int k) { return wgs_wanted(h, lv, k) && h->lv[lv].wgs.view.n_pieces > 0 ? &h->lv[lv].wgs : nullptr; }

// ---- overlapped tiling of the Gauss-Seidel sweeps of the latency-bound levels: relax(sweeps) as ONE launch ----------
// Which levels: scalar fp64 hierarchies, up to 7 columns (groups of 3 per launch; 8 and more take the wide colour kernels), Gauss-Seidel, SMG_TILED_MIN_ROWS <= rows <= SMG_TILED_MAX_ROWS (default 512 ..
// 122880 = one round of 240 parts of 512 rows: above, the redundant halo work of the tiles costs more than the launches it saves -- measured at C3 level 1, 253 k rows, and again on a 160 k-row
// union level; below 2 048 rows it pays as well: a 768-row level 37.5 -> 18.0 us per visit, tools/size_sweep.py), at most 5 colours and 12 entries per row.
// SMG_TILED=0 switches it off (A/B knob; the results are bit-identical either way).
static bool tiled_wanted(const smg_hierarchy* h, int lv, int k, int sweeps)
{
    static const int on = env_int("SMG_TILED", 1), max_rows = env_int("SMG_TILED_MAX_ROWS", 122880), min_rows = env_int("SMG_TILED_MIN_ROWS", 512);
    // smg_hierarchy_set_wave_gs(h, 1): the level sweeps piece-wise for EVERY k (the one-launch relax exists for k <= 7 only, and the order of a level's
    // sweep must not depend on the number of columns: column-sharded == fused)
    if (!on || k < 1 || k > 7 || sweeps < 1 || sweeps > 3 || !gs_plan_level(h, lv) || wgs_forced(h, lv)) return false;
    return h->lv[lv].n >= min_rows && h->lv[lv].n <= max_rows;
}
// the plan of relax(sweeps) on level lv, or nullptr (not wanted / the level does not qualify / not built yet)
static const TiledDev* tiled_plan(const smg_hierarchy* h, int lv, int k, int sweeps)
{
    if (!tiled_wanted(h, lv, k, sweeps)) return nullptr;
    const TiledBuf& B = h->lv[lv].tiled[sweeps];
    // k columns go through the tiles in groups of up to 3, whose iterates share the workgroup's 64 KB of LDS
    return B.view.n_tiles > 0 && (size_t)B.view.max_ext * std::min(k, 3) * sizeof(double) + TILED_LDS_STATIC <= 64 * 1024 ? &B.view : nullptr;
}
// the one-launch relax() has precedence over the wave sweep: a level sweeps piece-wise only where neither relax(sa) nor relax(sb) has a tiled plan
static bool tiled_either(const smg_hierarchy* h, int lv, int k, int sa, int sb) { return tiled_plan(h, lv, k, sa) || tiled_plan(h, lv, k, sb); }

// ---- block Gauss-Seidel for solves with a multiple of 16 columns: one launch per BLOCK colour -----------------
// Which levels: scalar fp64 hierarchies, Gauss-Seidel, k % 16 == 0, at least bgs_min_rows rows (smg_hierarchy_set_block_gs; default: never;
// SMG_BGS_MIN_ROWS; SMG_BGS=0 switches it off).  Measured at C3 (tools/bgs_cycle.py): worth it from ~500 000 rows on.
static bool bgs_wanted(const smg_hierarchy* h, int lv, int k)
{
    static const int on = env_int("SMG_BGS", 1);
    if (!on || h->precision != 0 || k < BGS_COLS || k % BGS_COLS != 0 || h->bgs_min_rows < 0 || !gs_plan_level(h, lv)) return false;
    return h->lv[lv].n >= h->bgs_min_rows;
}
static const BgsBuf* bgs_plan(const smg_hierarchy* h, int lv, int k) { return bgs_wanted(h, lv, k) && h->lv[lv].bgs.view.n_blocks > 0 ? &h->lv[lv].bgs : nullptr; }

// ------------------------------------------------------------------------------------------------ selection
SweepPlan smg::sweep_plan(const smg_hierarchy* h, int lv, int k, int sweeps, bool fp64, int first)
{
    SweepPlan s;
    if (!fp64) return s;                         // the plans' kernels are fp64 only
    if (first != FIRST_SWEEP) {                  // (the one-launch relax computes the first sweep itself)
        const TiledDev* t = tiled_plan(h, lv, k, sweeps);
        if (t && h->lv[lv].t.p) { s.tiled = t; return s; }     // (out of place: needs the second iterate)
    }
    if (first != FIRST_NONE) return s;           // the piece- / block-wise sweeps have no partial first sweep
    if ((s.wave = wgs_plan(h, lv, k))) return s;
    s.block = bgs_plan(h, lv, k);
    return s;
}

// ------------------------------------------------------------------------------------------------ building
// The matrix level lv's smoother streams, in the internal numbering -- A_int, or its transpose where the level sweeps on A^T -- and for each of its
// entries the index into Level::d_Aval: what every plan is built from.
struct SweepMatrix {
    const Level* Lv = nullptr;
    bool on_transpose = false;     // the level sweeps on A^T (Level::gs_on_transpose)
    Csr AT;                        // (then)
    std::vector<int> tsrc;         // ... entry of AT -> entry of A_int
    const Csr* G = nullptr;        // A_int or AT
    std::vector<int> to_level_value(const std::vector<int>& entries) const      // plan slots -> Level::d_Aval (-1: padding)
    {
        std::vector<int> m(entries.size());
        for (size_t i = 0; i < m.size(); i++) m[i] = entries[i] < 0 ? -1 : Lv->A_int_src[(size_t)(on_transpose ? tsrc[(size_t)entries[i]] : entries[i])];
        return m;
    }
};
// by_bits: a handle whose device half never ran (the self-checks on a machine without a GPU) has no images and no Level::gs_on_transpose yet --
// the rule of the first precompute (level_images: A^T wherever the two differ in any bit) is applied here
static int sweep_matrix(smg_hierarchy* h, int lv, SweepMatrix* M, bool by_bits = false)
{
    int rc = ensure_A_int(h, lv);
    if (rc) return rc;
    M->Lv = &h->lv[lv];
    M->on_transpose = M->Lv->gs_on_transpose;
    if (M->on_transpose || by_bits) M->AT = transpose(M->Lv->A_int, &M->tsrc);
    if (by_bits && !M->on_transpose) M->on_transpose = !(M->AT.ptr == M->Lv->A_int.ptr && M->AT.col == M->Lv->A_int.col && M->AT.val == M->Lv->A_int.val);
    M->G = M->on_transpose ? &M->AT : &M->Lv->A_int;
    return SMG_OK;
}

// the plan's values gathered from Level::d_Aval, the maps uploaded on their first use (see refresh_plan_values)
static int gather_plan_values(smg_hierarchy* h, const Level& Lv, PlanValues& V)
{
    auto ensure_map = [](DevBuf<int>& d, const std::vector<int>& host) { return d.n == host.size() && (d.p || host.empty()) ? hipSuccess : d.upload(host); };
    HIPCHK(ensure_map(V.map, V.host_map)); HIPCHK(ensure_map(V.mapd, V.host_mapd));
    HIPCHK(launch_gather_vals(V.val.p, Lv.d_Aval.p, V.map.p, V.val.n, h->stream));
    HIPCHK(launch_gather_vals(V.diag.p, Lv.d_Aval.p, V.mapd.p, V.diag.n, h->stream));
    return SMG_OK;
}
// A plan's copies of the level values on the host: the values as its builder read them from the host copy, and for every slot the index into
// Level::d_Aval (-1: padding the builder wrote -- +0.0 in an entry slot, 1.0 on the diagonal of a lane without a row; refresh_plan_values keeps it).
// What set_plan_values uploads and smg_debug_check_plan_value_maps checks.
struct PlanSlots {
    const std::vector<double> *val = nullptr, *diag = nullptr;
    std::vector<int> map, mapd;
};
static PlanSlots plan_slots(const SweepMatrix& M, const std::vector<double>& val, const std::vector<int>& entry, const std::vector<double>& diag,
                            const std::vector<int>& dentry)
{
    PlanSlots S;
    S.val = &val; S.diag = &diag; S.map = M.to_level_value(entry); S.mapd = M.to_level_value(dentry);
    return S;
}
static PlanSlots plan_slots(const SweepMatrix& M, const TiledGs& P) { return plan_slots(M, P.pval, P.pentry, P.pdiag, P.pdentry); }
static PlanSlots plan_slots(const SweepMatrix& M, const BgsPlan& P) { return plan_slots(M, P.eval, P.eentry, P.udiag, P.dentry); }
static PlanSlots plan_slots(const SweepMatrix& M, const WgsPlan& P) { return plan_slots(M, P.eval, P.eentry, P.diag, P.dentry); }
// a new plan's values and their maps (kept on the host); after a value-only re-precompute the host copy the builder read is stale: the values are
// gathered from the device copy at once
static int set_plan_values(smg_hierarchy* h, const Level& Lv, PlanSlots&& S, PlanValues& V)
{
    HIPCHK(V.val.upload(*S.val)); HIPCHK(V.diag.upload(*S.diag));
    V.host_map = std::move(S.map); V.host_mapd = std::move(S.mapd);
    return h->host_stale && Lv.d_Aval.p ? gather_plan_values(h, Lv, V) : SMG_OK;
}

// ---- the plans of a level as the host builds them (ensure_* below; smg_debug_check_plan_value_maps)
// Tile size (measured at C3, tools/tiled_sweep.sh): parts of 128 .. 256 rows, 512 threads (one row of every colour per thread).
// Smaller tiles put more CUs to work but the halo of P rings then dominates (6x redundant row updates at 64 rows: slower);
// larger ones run too few workgroups.
// Beyond 65 536 rows parts of 256 rows are more workgroups than the part has compute units (a second round of them: tools/size_sweep.py, a
// 69 120-row level 45.8 us per visit against 28 us at 56 320 rows): the parts grow to 512 rows so that the level stays one round up to 122 880
// rows (69 120 rows: 34.2 us, 77 824: 43.4 -> 32.2, 101 376: 47.5 (colour launches) -> 36.7; at 30 720 rows parts of 512 rows lose: 25.1 -> 28.0).
static TiledGs host_tiled_plan(const SweepMatrix& M, int sweeps, int* threads)
{
    static const int rows_env = env_int("SMG_TILED_ROWS", 0), nt_env = env_int("SMG_TILED_NT", 0);
    const Level& Lv = *M.Lv;
    const int tile_rows0 = rows_env > 0 ? rows_env : std::min(512, std::max(256, (Lv.n + 239) / 240));
    constexpr int max_ext = (64 * 1024 - TILED_LDS_STATIC) / 8;    // 64 KB of LDS, the kernel's static header included
    // a tile whose halo makes a colour's panel longer than the workgroup gets smaller tiles
    TiledGs P;
    *threads = 512;
    for (int tile_rows = tile_rows0, tries = 0; tries < 3 && P.empty(); tile_rows = tile_rows * 2 / 3, tries++) {
        *threads = nt_env > 0 ? nt_env : 512;
        P = build_tiled_gs(*M.G, Lv.ord.color_ptr, sweeps, tile_rows, max_ext, *threads);
    }
    return P;
}
static BgsPlan host_bgs_plan(const SweepMatrix& M)
{
    static const int rows_env = env_int("SMG_BGS_ROWS", 64);
    return build_bgs(*M.G, M.Lv->ord.color_ptr, std::min(std::max(rows_env, 8), (int)BGS_ROWS));
}
static WgsPlan host_wgs_plan(const SweepMatrix& M)
{
    static const int rows_env = env_int("SMG_WGS_ROWS", WGS_ROWS), mode_env = env_int("SMG_WGS_PIECES", 1);
    return build_wgs(*M.G, std::min(std::max(rows_env, 8), (int)WGS_ROWS), mode_env);
}

static int ensure_tiled(smg_hierarchy* h, int lv, int sweeps)
{
    Level& Lv = h->lv[lv];
    TiledBuf& B = Lv.tiled[sweeps];
    if (B.tried) return SMG_OK;
    B.tried = true;
    SweepMatrix M;
    { int rc = sweep_matrix(h, lv, &M); if (rc) return rc; }
    int threads = 512;
    const TiledGs P = host_tiled_plan(M, sweeps, &threads);
    if (P.empty()) return SMG_OK;
    HIPCHK(B.hdr.upload(P.hdr)); HIPCHK(B.ext_rows.upload(P.ext_rows)); HIPCHK(B.pcol.upload(P.pcol)); HIPCHK(B.prow.upload(P.prow));
    { int rc = set_plan_values(h, Lv, plan_slots(M, P), B.v); if (rc) return rc; }
    HIPCHK(tiled_gs_prepare(P.max_ext));
    int wmax = 0;
    for (int t = 0; t < P.n_tiles; t++) wmax = std::max(wmax, P.hdr[(size_t)t * TILED_HDR + 2]);
    B.view.threads = threads;
    B.view.n_tiles = P.n_tiles; B.view.nc = P.nc; B.view.P = P.P; B.view.sweeps = sweeps; B.view.max_ext = P.max_ext; B.view.w_max = wmax;
    B.view.hdr = B.hdr.p; B.view.ext_rows = B.ext_rows.p; B.view.pcol = B.pcol.p; B.view.pval = B.v.val.p; B.view.prow = B.prow.p; B.view.pdiag = B.v.diag.p;
    if (env_int("SMG_DEBUG_TILED", 0))
        std::fprintf(stderr, "tiled relax(%d) level %d: %d rows, %d tiles x %d threads, %d phases, extended tile <= %d rows, %.2fx row updates, entries per row <= %d\n", sweeps, lv, Lv.n,
                     P.n_tiles, threads, P.P, P.max_ext, (double)P.updates / ((double)sweeps * Lv.n), wmax);
    return SMG_OK;
}

static int ensure_bgs(smg_hierarchy* h, int lv)
{
    Level& Lv = h->lv[lv];
    BgsBuf& B = Lv.bgs;
    if (B.tried) return SMG_OK;
    B.tried = true;
    SweepMatrix M;
    { int rc = sweep_matrix(h, lv, &M); if (rc) return rc; }
    const auto t_plan0 = std::chrono::steady_clock::now();
    const BgsPlan P = host_bgs_plan(M);
    const double plan_ms = 1e3 * std::chrono::duration<double>(std::chrono::steady_clock::now() - t_plan0).count();
    if (P.empty()) return SMG_OK;
    HIPCHK(B.hdr.upload(P.hdr)); HIPCHK(B.xrow.upload(P.xrow)); HIPCHK(B.ugrow.upload(P.ugrow)); HIPCHK(B.ulrow.upload(P.ulrow)); HIPCHK(B.eidx.upload(P.eidx));
    { int rc = set_plan_values(h, Lv, plan_slots(M, P), B.v); if (rc) return rc; }
    B.view.n_blocks = P.n_blocks; B.view.n_colors = P.n_colors; B.view.xrows = P.xrows;
    B.view.hdr = B.hdr.p; B.view.xrow = B.xrow.p; B.view.ugrow = B.ugrow.p; B.view.ulrow = B.ulrow.p; B.view.udiag = B.v.diag.p; B.view.eidx = B.eidx.p; B.view.eval = B.v.val.p;
    B.color_ptr = P.color_ptr; B.host_rows = P.rows; B.host_blk_ptr = P.blk_ptr; B.rim = P.rim; B.fill = P.fill;
    if (env_int("SMG_DEBUG_BGS", 0))
        std::fprintf(stderr, "block Gauss-Seidel level %d: %d rows, %d blocks in %d colours, %.0f %% of the units' row slots hold a row of their own, rim %.3f rows read per row beyond the iterate, LDS image of %d rows; plan built in %.0f ms\n",
                     lv, Lv.n, P.n_blocks, P.n_colors, 100.0 * P.fill, P.rim, P.xrows, plan_ms);
    return SMG_OK;
}

static int ensure_wgs(smg_hierarchy* h, int lv)
{
    Level& Lv = h->lv[lv];
    WgsBuf& B = Lv.wgs;
    if (B.tried) return SMG_OK;
    B.tried = true;
    SweepMatrix M;
    { int rc = sweep_matrix(h, lv, &M); if (rc) return rc; }
    const auto t_plan0 = std::chrono::steady_clock::now();
    const WgsPlan P = host_wgs_plan(M);
    const double plan_ms = 1e3 * std::chrono::duration<double>(std::chrono::steady_clock::now() - t_plan0).count();
    if (P.empty()) return SMG_OK;
    HIPCHK(B.hdr.upload(P.hdr)); HIPCHK(B.grow.upload(P.grow)); HIPCHK(B.meta.upload(P.meta)); HIPCHK(B.rim.upload(P.rim)); HIPCHK(B.eoff.upload(P.eoff));
    { int rc = set_plan_values(h, Lv, plan_slots(M, P), B.v); if (rc) return rc; }
    B.view.n_pieces = P.n_pieces; B.view.n_colors = P.n_colors; B.view.rim_pitch = P.rim_pitch; B.view.nb_max = P.nb_max;
    B.view.hdr = B.hdr.p; B.view.grow = B.grow.p; B.view.meta = B.meta.p; B.view.diag = B.v.diag.p; B.view.rim = B.rim.p; B.view.eoff = B.eoff.p; B.view.eval = B.v.val.p;
    B.color_ptr = P.color_ptr; B.host_rows = P.rows; B.host_piece_ptr = P.piece_ptr; B.rim_ratio = P.rim_ratio; B.phases_mean = P.phases_mean; B.phases_max = P.phases_max;
    if (env_int("SMG_DEBUG_WGS", 0))
        std::fprintf(stderr, "wave Gauss-Seidel level %d: %d rows, %d pieces in %d colours, phases per piece %.1f (max %d), rim %.2f rows read per row beyond the iterate, rim pitch %d; plan built in %.0f ms\n",
                     lv, Lv.n, P.n_pieces, P.n_colors, P.phases_mean, P.phases_max, P.rim_ratio, P.rim_pitch, plan_ms);
    return SMG_OK;
}

// The plans relax(sa) / relax(sb) of level lv want for k columns, built where not tried yet (host work and uploads: never inside a graph capture).
// drop: a new block / wave plan changes the captured launches, the cached graphs go first.
static int ensure_level_plans(smg_hierarchy* h, int lv, int k, int sa, int sb, bool drop)
{
    Level& Lv = h->lv[lv];
    int rc;
    for (int sw : {sa, sb}) if (tiled_wanted(h, lv, k, sw) && (rc = ensure_tiled(h, lv, sw))) return rc;
    if (bgs_wanted(h, lv, k) && !Lv.bgs.tried) { if (drop) drop_graphs(h); if ((rc = ensure_bgs(h, lv))) return rc; }
    if (wgs_wanted(h, lv, k) && !Lv.wgs.tried && !tiled_either(h, lv, k, sa, sb)) { if (drop) drop_graphs(h); if ((rc = ensure_wgs(h, lv))) return rc; }
    return SMG_OK;
}

// Called by the first precompute for a level whose images exist, while its device half would otherwise wait for the host half (smg_precompute.cpp):
// the plans prepare_sweep_plans() below would build at the first solve with the handle's present selection (smoother, pre / post sweeps), one column.
// Small levels only (a plan of tens of milliseconds at most: the 63 210-row Galerkin level of decimated C3 64 ms, its 252 834-row level 220 ms -- building
// that one here kept level 0's images waiting and cost the precompute more than it saved the first solve).  First smg_solve on a fresh handle:
// bunny.obj 8.4 -> 4.2 ms, ogre.obj 17 -> 11 ms (tools/first_solve.py).
int smg::prepare_level_plans(smg_hierarchy* h, int lv)
{
    static const int on = env_int("SMG_EARLY_PLANS", 1), max_rows = env_int("SMG_EARLY_PLANS_MAX_ROWS", 70000);      // A/B knobs
    if (!on || lv <= 0 || lv >= h->n_levels - 1 || h->precision != 0 || h->lv[lv].n > max_rows) return SMG_OK;
    return ensure_level_plans(h, lv, 1, h->pre, h->post, false);
}

int smg::prepare_sweep_plans(smg_hierarchy* h, int k, int sa, int sb)
{
    for (int lv = 0; lv < h->n_levels - 1; lv++) {
        Level& Lv = h->lv[lv];
        int rc = ensure_level_plans(h, lv, k, sa, sb, true);
        if (rc) return rc;
        if (tiled_either(h, lv, k, sa, sb) && Lv.t.n < (size_t)Lv.n * std::max(h->kcap, 1)) {      // the one-launch relax runs out of place
            drop_graphs(h);
            HIPCHK(Lv.t.alloc((size_t)Lv.n * std::max(h->kcap, 1)));
            HIPCHK(hipMemsetAsync(Lv.t.p, 0, Lv.t.n * sizeof(double), h->stream));
        }
    }
    return SMG_OK;
}

// A value-only re-precompute: every plan's copies of the level values gathered from Level::d_Aval (gather_plan_values, also used by a plan built
// while the host copy is stale).  Precondition of launch_gather_vals, which leaves a slot whose map is -1 untouched: such slots keep the padding the
// builder wrote -- +0.0 in value slots, 1.0 on the diagonals of lanes without a row.
int smg::refresh_plan_values(smg_hierarchy* h)
{
    for (int lv = 0; lv < h->n_levels - 1; lv++) {
        Level& Lv = h->lv[lv];
        int rc;
        for (int s = 1; s <= 3; s++) if (Lv.tiled[s].view.n_tiles > 0 && (rc = gather_plan_values(h, Lv, Lv.tiled[s].v))) return rc;
        if (Lv.wgs.view.n_pieces > 0 && (rc = gather_plan_values(h, Lv, Lv.wgs.v))) return rc;
        if (Lv.bgs.view.n_blocks > 0 && (rc = gather_plan_values(h, Lv, Lv.bgs.v))) return rc;
    }
    return SMG_OK;
}
void smg::drop_sweep_plans(smg_hierarchy* h)
{
    for (auto& Lv : h->lv) { for (auto& B : Lv.tiled) B = TiledBuf(); Lv.bgs = BgsBuf(); Lv.wgs = WgsBuf(); }
}

// ------------------------------------------------------------------------------------------------ C ABI: selection and introspection
extern "C" int smg_hierarchy_set_block_gs(smg_hierarchy* h, int min_rows)
{
    if (!h) return fail(SMG_ERR_INVALID, "smg_hierarchy_set_block_gs: null handle");
    if (h->in_solve) return fail(SMG_ERR_INVALID, "smg_hierarchy_set_block_gs called during a split-phase solve");
    if (min_rows != h->bgs_min_rows) { h->bgs_min_rows = min_rows; if (h->stream) drop_graphs(h); }
    return SMG_OK;
}
extern "C" int smg_level_get_block_gs_order(smg_hierarchy* h, int lv, int k, int* n_blocks, int* n_colors, int* color_ptr, int* blk_ptr, int* rows, double* stats)
{
    int rc = check_ready(h, "smg_level_get_block_gs_order");
    if (rc) return rc;
    if (lv < 0 || lv >= h->n_levels || k < 1) return fail(SMG_ERR_INVALID, "smg_level_get_block_gs_order: bad level / k");
    if (!bgs_wanted(h, lv, k)) return 0;
    if (!h->lv[lv].bgs.tried) { drop_graphs(h); if ((rc = ensure_bgs(h, lv))) return rc; }
    const BgsBuf* Q = bgs_plan(h, lv, k);
    if (!Q) return 0;
    if (n_blocks) *n_blocks = Q->view.n_blocks;
    if (n_colors) *n_colors = Q->view.n_colors;
    if (color_ptr) std::copy(Q->color_ptr.begin(), Q->color_ptr.end(), color_ptr);
    if (blk_ptr) std::copy(Q->host_blk_ptr.begin(), Q->host_blk_ptr.end(), blk_ptr);
    if (rows) std::copy(Q->host_rows.begin(), Q->host_rows.end(), rows);
    if (stats) { stats[0] = Q->rim; stats[1] = Q->fill; }
    return 1;
}

extern "C" int smg_hierarchy_set_wave_gs(smg_hierarchy* h, int mode)
{
    if (!h) return fail(SMG_ERR_INVALID, "smg_hierarchy_set_wave_gs: null handle");
    if (h->in_solve) return fail(SMG_ERR_INVALID, "smg_hierarchy_set_wave_gs called during a split-phase solve");
    if (mode < -1 || mode > 1) return fail(SMG_ERR_INVALID, "smg_hierarchy_set_wave_gs: mode must be -1 (automatic), 0 (never) or 1 (every Gauss-Seidel level in range)");
    if (mode != h->wgs_mode) { h->wgs_mode = mode; if (h->stream) drop_graphs(h); }
    return SMG_OK;
}
extern "C" int smg_level_get_wave_gs_order(smg_hierarchy* h, int lv, int k, int* n_pieces, int* n_colors, int* color_ptr, int* piece_ptr, int* rows, double* stats)
{
    int rc = check_ready(h, "smg_level_get_wave_gs_order");
    if (rc) return rc;
    if (lv < 0 || lv >= h->n_levels || k < 1) return fail(SMG_ERR_INVALID, "smg_level_get_wave_gs_order: bad level / k");
    if (!wgs_wanted(h, lv, k)) return 0;
    DeviceScope dsc(h->device);
    if ((rc = prepare_sweep_plans(h, k, h->pre, h->post))) return rc;
    const WgsBuf* Q = wgs_plan(h, lv, k);
    if (!Q || tiled_either(h, lv, k, h->pre, h->post)) return 0;
    if (n_pieces) *n_pieces = Q->view.n_pieces;
    if (n_colors) *n_colors = Q->view.n_colors;
    if (color_ptr) std::copy(Q->color_ptr.begin(), Q->color_ptr.end(), color_ptr);
    if (piece_ptr) std::copy(Q->host_piece_ptr.begin(), Q->host_piece_ptr.end(), piece_ptr);
    if (rows) std::copy(Q->host_rows.begin(), Q->host_rows.end(), rows);
    if (stats) { stats[0] = Q->rim_ratio; stats[1] = Q->phases_mean; stats[2] = (double)Q->phases_max; }
    return 1;
}

// ------------------------------------------------------------------------------------------------ read-only hooks: which kernel variants run
// the internal matrix of a smoothed level of a scalar handle whose host half of smg_precompute has run, or an error
static int check_level_matrix(smg_hierarchy* h, int lv, const char* who, const Csr** G)
{
    int rc = ensure_A_int(h, lv);
    if (rc) return rc;
    const Level& Lv = h->lv[lv];
    if (Lv.A_int.nr != Lv.n || Lv.n == 0 || h->bs != 1) return fail(SMG_ERR_INVALID, "%s: the host half of smg_precompute has not run (scalar hierarchies only)", who);
    *G = &Lv.A_int;
    return SMG_OK;
}
// The k_wgs launches of one piece colour: launch_wgs's own functions (wgs_kernel_class, wgs_column_split -- same statics, same knobs) walked the way it walks them.
extern "C" int smg_debug_wgs_launches(int n_pieces, int nb_max, int rim_pitch, int k, int* nbmax, int* rimi, int* launches, int cap, int* n_launches)
{
    if (n_pieces < 1 || k < 1 || k > 4 * 65535 || cap < 0 || (cap > 0 && !launches) || !n_launches)
        return fail(SMG_ERR_INVALID, "smg_debug_wgs_launches: bad arguments");
    int nbm = 0, ri = 0;
    if (!wgs_kernel_class(nb_max, rim_pitch, &nbm, &ri))
        return fail(SMG_ERR_INVALID, "smg_debug_wgs_launches: k_wgs has no variant for rows of %d batches and a rim pitch of %d", nb_max, rim_pitch);
    if (nbmax) *nbmax = nbm;
    if (rimi) *rimi = ri;
    int n = 0;
    for (int c0 = 0; c0 < k; n++) {
        int kb = 0, groups = 0;
        wgs_column_split(n_pieces, k, c0, &kb, &groups);
        if (n < cap) { launches[2 * n] = kb; launches[2 * n + 1] = groups; }
        c0 += kb * groups;
    }
    *n_launches = n;
    return SMG_OK;
}
// The plan those launches run on.  from_host 0: the plan relax() of level lv sweeps with for k columns in the handle's present state -- nothing is
// built: a level whose plan no sweep has asked for yet, or that sweeps another way, reports none; 1: the plan as ensure_wgs would build it, on the host.
extern "C" int smg_debug_wgs_level_plan(smg_hierarchy* h, int lv, int k, int from_host, int* n_pieces, int* nb_max, int* rim_pitch)
{
    return guarded("smg_debug_wgs_level_plan", [&]() -> int {
        if (!h || lv < 0 || lv >= h->n_levels - 1 || k < 1 || !n_pieces || !nb_max || !rim_pitch)
            return fail(SMG_ERR_INVALID, "smg_debug_wgs_level_plan: bad arguments");
        *n_pieces = *nb_max = *rim_pitch = 0;
        if (from_host) {
            const Csr* G = nullptr;
            int rc = check_level_matrix(h, lv, "smg_debug_wgs_level_plan", &G);
            if (rc) return rc;
            SweepMatrix M;
            if ((rc = sweep_matrix(h, lv, &M, !h->lv[lv].dA.view.val))) return rc;
            const WgsPlan P = host_wgs_plan(M);
            *n_pieces = P.n_pieces; *nb_max = P.nb_max; *rim_pitch = P.rim_pitch;
            return SMG_OK;
        }
        const WgsBuf* Q = wgs_plan(h, lv, k);
        if (!Q || tiled_either(h, lv, k, h->pre, h->post)) return SMG_OK;
        *n_pieces = Q->view.n_pieces; *nb_max = Q->view.nb_max; *rim_pitch = Q->view.rim_pitch;
        return SMG_OK;
    });
}
// The launches of A x (mode 0) or b - A x (mode 1) with k <= 4 fp64 columns -- one narrow group of launch_sell_mode -- on a level matrix: its own
// deep_split.  Per launch (columns, NBMAX class of k_sell_deep or 0 for k_sell).
extern "C" int smg_debug_deep_launches(const smg_hierarchy* h, int lv, int which, int mode, int k, int* w_max, int* launches, int cap, int* n_launches)
{
    if (!h || lv < 0 || lv >= h->n_levels || which < 0 || which > 2 || mode < 0 || mode > 1 || k < 1 || k > 4 || cap < 0 || (cap > 0 && !launches) || !n_launches)
        return fail(SMG_ERR_INVALID, "smg_debug_deep_launches: bad arguments (one narrow group: 1 <= k <= 4)");
    const SellBuf& S = which == 0 ? h->lv[lv].dA : which == 1 ? h->lv[lv].dP : h->lv[lv].dPT;
    if (h->bs != 1 || S.view.n_slices <= 0) return fail(SMG_ERR_INVALID, "smg_debug_deep_launches: the level has no such scalar device image (smg_precompute first)");
    if (w_max) *w_max = S.view.w_max;
    int cols[4] = {k, 0, 0, 0}, nbm = 0;
    const int nd = deep_split(mode == 0 ? SELL_AX : SELL_RESID, S.view.w_max, k, cols, &nbm), n = std::max(nd, 1);
    for (int i = 0; i < std::min(n, cap); i++) { launches[2 * i] = cols[i]; launches[2 * i + 1] = nd > 0 ? nbm : 0; }
    *n_launches = n;
    return SMG_OK;
}
// Waves per workgroup of a one-column Gauss-Seidel colour launch of n_slices slices on the image level lv sweeps on (A, or A^T where A is not
// bit-symmetric): launch_narrow's own gs_colour_wpb; the image's panel pitch and lower width beside it.
extern "C" int smg_debug_gs_colour_wpb(const smg_hierarchy* h, int lv, int n_slices, int* wpb, int* stride, int* w_lo)
{
    if (!h || lv < 0 || lv >= h->n_levels - 1 || n_slices < 1 || !wpb) return fail(SMG_ERR_INVALID, "smg_debug_gs_colour_wpb: bad arguments");
    const Level& Lv = h->lv[lv];
    const SellBuf& G = Lv.gs_on_transpose ? Lv.dAT : Lv.dA;
    if (h->bs != 1 || G.view.n_slices <= 0 || n_slices > G.view.n_slices)
        return fail(SMG_ERR_INVALID, "smg_debug_gs_colour_wpb: the level has no scalar device image of that many slices (smg_precompute first)");
    *wpb = gs_colour_wpb(G.view, n_slices);
    if (stride) *stride = G.view.stride;
    if (w_lo) *w_lo = G.view.w_lo;
    return SMG_OK;
}

// ------------------------------------------------------------------------------------------------ host-side self-checks
// Each check builds a plan of level lv from A_int on the host and EXECUTES it there the way its kernel does (tiled_sweep_host, bgs_sweep_host,
// wgs_sweep_host), one sweep on fixed test vectors, against a plain sweep: *max_abs_diff must be 0.  Need no GPU once the host half of smg_precompute
// has run.  An empty plan (the level does not qualify) returns SMG_OK with *max_abs_diff = 0.

// the level matrix the checks use (A_int), or an error
static int check_level(smg_hierarchy* h, int lv, bool args_ok, const char* who, const Csr** G)
{
    if (!h || lv < 0 || lv >= h->n_levels - 1 || !args_ok) return fail(SMG_ERR_INVALID, "%s: bad arguments", who);
    return check_level_matrix(h, lv, who, G);
}
// the checks' test vectors: the iterate x, the right-hand side b
static std::vector<double> check_vector(int n, bool rhs)
{
    std::vector<double> v((size_t)n);
    for (int i = 0; i < n; i++) v[(size_t)i] = rhs ? std::cos(0.11 * i) - 0.5 * std::sin(2.1 * i) : std::sin(0.37 * i) + 0.25 * std::cos(1.3 * i);
    return v;
}
static double max_diff(const std::vector<double>& y, const std::vector<double>& ref)
{
    double d = 0.0;
    for (size_t i = 0; i < y.size(); i++) d = std::max(d, std::fabs(y[i] - ref[i]));
    return d;
}
// invariants of a block / wave plan: every row in exactly one part of at most max_rows rows; parts of one colour share no entry
static int check_partition(const Csr& G, const char* plan, const char* part, const char* parts, int n_parts, int n_colors, const std::vector<int>& color_ptr,
                           const std::vector<int>& part_ptr, const std::vector<int>& rows, int max_rows)
{
    const int n = G.nr;
    std::vector<int> part_of((size_t)n, -1), col_of_part((size_t)n_parts, -1);
    for (int c = 0; c < n_colors; c++) for (int q = color_ptr[(size_t)c]; q < color_ptr[(size_t)c + 1]; q++) col_of_part[(size_t)q] = c;
    for (int q = 0; q < n_parts; q++) {
        if (part_ptr[(size_t)q + 1] - part_ptr[(size_t)q] > max_rows) return fail(SMG_ERR_INVALID, "%s: %s %d has more than %d rows", plan, part, q, max_rows);
        for (int t = part_ptr[(size_t)q]; t < part_ptr[(size_t)q + 1]; t++) {
            const int i = rows[(size_t)t];
            if (i < 0 || i >= n || part_of[(size_t)i] >= 0) return fail(SMG_ERR_INVALID, "%s: row %d is not in exactly one %s", plan, i, part);
            part_of[(size_t)i] = q;
        }
    }
    for (int i = 0; i < n; i++) {
        if (part_of[(size_t)i] < 0) return fail(SMG_ERR_INVALID, "%s: row %d is in no %s", plan, i, part);
        for (int p = G.ptr[(size_t)i]; p < G.ptr[(size_t)i + 1]; p++) {
            const int j = G.col[(size_t)p];
            if (part_of[(size_t)j] != part_of[(size_t)i] && col_of_part[(size_t)part_of[(size_t)j]] == col_of_part[(size_t)part_of[(size_t)i]])
                return fail(SMG_ERR_INVALID, "%s: %s %d and %d share an entry and a colour", plan, parts, part_of[(size_t)i], part_of[(size_t)j]);
        }
    }
    return SMG_OK;
}
// the reference's relax() (src/mg_VCycle.cpp:146-160) on the numbering `rows` (position -> row): rows one after the other in that order, products in
// ascending column OF THAT ORDER; one sweep in place on x
static void ordered_sweep(const Csr& G, const std::vector<int>& rows, const std::vector<double>& b, std::vector<double>& x)
{
    const int n = G.nr;
    std::vector<int> pos((size_t)n);
    for (int t = 0; t < n; t++) pos[(size_t)rows[(size_t)t]] = t;
    std::vector<std::pair<int, int>> ent;
    for (int t = 0; t < n; t++) {
        const int i = rows[(size_t)t];
        ent.clear();
        double diag = 1.0;
        for (int p = G.ptr[(size_t)i]; p < G.ptr[(size_t)i + 1]; p++) {
            if (G.col[(size_t)p] == i) diag = G.val[(size_t)p]; else ent.emplace_back(pos[(size_t)G.col[(size_t)p]], p);
        }
        std::sort(ent.begin(), ent.end());
        double acc = 0.0;
        for (const auto& e : ent) acc += G.val[(size_t)e.second] * x[(size_t)G.col[(size_t)e.second]];
        x[(size_t)i] = (b[(size_t)i] - acc) / diag;
    }
}

// The overlapped-tiling plan of relax(sweeps) against the colour-by-colour sweeps in place (what one launch per colour computes).
extern "C" int smg_debug_check_tiling_plan(smg_hierarchy* h, int lv, int sweeps, int tile_rows, int* n_tiles, int* max_ext_rows, double* redundancy,
                                           double* max_abs_diff)
{
    return guarded("smg_debug_check_tiling_plan", [&]() -> int {
        const Csr* G = nullptr;
        int rc = check_level(h, lv, !(sweeps < 1 || tile_rows < 8), "smg_debug_check_tiling_plan", &G);
        if (rc) return rc;
        const int n = G->nr;
        const TiledGs P = build_tiled_gs(*G, h->lv[lv].ord.color_ptr, sweeps, tile_rows, 1 << 20, 1 << 20);
        if (n_tiles) *n_tiles = P.n_tiles;
        if (max_ext_rows) *max_ext_rows = P.max_ext;
        if (redundancy) *redundancy = P.n_tiles ? (double)P.updates / ((double)sweeps * n) : 0.0;
        if (max_abs_diff) *max_abs_diff = 0.0;
        if (P.empty()) return SMG_OK;
        const std::vector<double> x = check_vector(n, false), b = check_vector(n, true);
        std::vector<double> ref = x, y((size_t)n, 0.0);
        const std::vector<int>& cp = h->lv[lv].ord.color_ptr;
        for (int s = 0; s < sweeps; s++)
            for (size_t c = 0; c + 1 < cp.size(); c++)
                for (int i = cp[c]; i < cp[c + 1]; i++) {
                    double acc = 0.0, diag = 1.0;
                    for (int p = G->ptr[(size_t)i]; p < G->ptr[(size_t)i + 1]; p++) {
                        if (G->col[(size_t)p] == i) diag = G->val[(size_t)p];
                        else acc += G->val[(size_t)p] * ref[(size_t)G->col[(size_t)p]];
                    }
                    ref[(size_t)i] = (b[(size_t)i] - acc) / diag;
                }
        const int bad = tiled_sweep_host(P, b.data(), x.data(), y.data());
        if (bad >= 0) return fail(SMG_ERR_INVALID, "tiling plan: tile %d holds a column outside its image", bad);
        if (max_abs_diff) *max_abs_diff = max_diff(y, ref);
        return SMG_OK;
    });
}

// The wave Gauss-Seidel plan of level lv (per piece an image of its rows and its rim, phases in place, packed byte offsets) against the plain
// lexicographic sweep in the wgs order; checks the plan's invariants on the way.  *n_pieces = 0: the level does not qualify.
extern "C" int smg_debug_check_wave_gs_plan(smg_hierarchy* h, int lv, int piece_rows, int pieces_mode, int* n_pieces, int* n_colors, double* stats, double* max_abs_diff)
{
    return guarded("smg_debug_check_wave_gs_plan", [&]() -> int {
        const Csr* G = nullptr;
        int rc = check_level(h, lv, !(piece_rows < 8), "smg_debug_check_wave_gs_plan", &G);
        if (rc) return rc;
        const WgsPlan P = build_wgs(*G, std::min(piece_rows, (int)WGS_ROWS), pieces_mode);
        if (n_pieces) *n_pieces = P.n_pieces;
        if (n_colors) *n_colors = P.n_colors;
        if (stats) { stats[0] = P.rim_ratio; stats[1] = P.phases_mean; stats[2] = (double)P.phases_max; }
        if (max_abs_diff) *max_abs_diff = 0.0;
        if (P.empty()) return SMG_OK;
        if ((rc = check_partition(*G, "wave plan", "piece", "pieces", P.n_pieces, P.n_colors, P.color_ptr, P.piece_ptr, P.rows, WGS_ROWS))) return rc;
        const std::vector<double> x = check_vector(G->nr, false), b = check_vector(G->nr, true);
        std::vector<double> ref = x, y = x;
        ordered_sweep(*G, P.rows, b, ref);
        wgs_sweep_host(P, b.data(), y.data());
        if (max_abs_diff) *max_abs_diff = max_diff(y, ref);
        return SMG_OK;
    });
}

// The block Gauss-Seidel plan of level lv (per block an image of its rows and its rim, units of <= 16 rows updated in place from local indices)
// against the plain lexicographic sweep in the bgs order; checks the plan's invariants on the way.  *n_blocks = 0: the level does not qualify.
extern "C" int smg_debug_check_block_gs_plan(smg_hierarchy* h, int lv, int block_rows, int* n_blocks, int* n_colors, double* rim, double* fill, double* max_abs_diff)
{
    return guarded("smg_debug_check_block_gs_plan", [&]() -> int {
        const Csr* G = nullptr;
        int rc = check_level(h, lv, !(block_rows < 8), "smg_debug_check_block_gs_plan", &G);
        if (rc) return rc;
        const BgsPlan P = build_bgs(*G, h->lv[lv].ord.color_ptr, std::min(block_rows, (int)BGS_ROWS));
        if (n_blocks) *n_blocks = P.n_blocks;
        if (n_colors) *n_colors = P.n_colors;
        if (rim) *rim = P.rim;
        if (fill) *fill = P.fill;
        if (max_abs_diff) *max_abs_diff = 0.0;
        if (P.empty()) return SMG_OK;
        if ((rc = check_partition(*G, "block plan", "block", "blocks", P.n_blocks, P.n_colors, P.color_ptr, P.blk_ptr, P.rows, INT_MAX))) return rc;
        const std::vector<double> x = check_vector(G->nr, false), b = check_vector(G->nr, true);
        std::vector<double> ref = x, y = x;
        ordered_sweep(*G, P.rows, b, ref);
        const long bad = bgs_sweep_host(P, b.data(), y.data());
        if (bad >= 0) return fail(SMG_ERR_INVALID, "block plan: local index %d outside the image of %d rows", P.eidx[(size_t)bad], P.xrows);
        if (max_abs_diff) *max_abs_diff = max_diff(y, ref);
        return SMG_OK;
    });
}

// The value maps of a plan of level lv (which: 0 the overlapped tiling of relax(sweeps), 1 wave, 2 block Gauss-Seidel), built from sweep_matrix()
// as ensure_tiled / ensure_wgs / ensure_bgs build it: every slot with a map holds, bit for bit, the level value the map names (Level::A.val, what
// Level::d_Aval is uploaded from), every entry slot without one +0.0, every diagonal slot without one 1.0 -- what refresh_plan_values relies on.
// against_transpose: the comparison a map of A would pass where the level sweeps on A^T and the reverse (entry (i, j) against a_ji): tests show with
// it that a wrong map is counted.  *on_transpose: the plan was built from A^T -- the level's choice, or on a handle whose device half never ran
// (no GPU) the choice of the first precompute, from the bits.  *n_slots = 0: the level has no such plan.
extern "C" int smg_debug_check_plan_value_maps(smg_hierarchy* h, int lv, int which, int sweeps, int against_transpose, int* n_slots, int* n_padding, int* bad,
                                               int* on_transpose)
{
    return guarded("smg_debug_check_plan_value_maps", [&]() -> int {
        const Csr* A_int = nullptr;
        int rc = check_level(h, lv, which >= 0 && which <= 2 && (which != 0 || (sweeps >= 1 && sweeps <= 3)), "smg_debug_check_plan_value_maps", &A_int);
        if (rc) return rc;
        SweepMatrix M;
        if ((rc = sweep_matrix(h, lv, &M, !h->lv[lv].dA.view.val))) return rc;
        if (on_transpose) *on_transpose = M.on_transpose ? 1 : 0;
        TiledGs T; WgsPlan W; BgsPlan Bp;
        PlanSlots S;
        int threads = 0;
        if (which == 0) { T = host_tiled_plan(M, sweeps, &threads); if (!T.empty()) S = plan_slots(M, T); }
        else if (which == 1) { W = host_wgs_plan(M); if (!W.empty()) S = plan_slots(M, W); }
        else { Bp = host_bgs_plan(M); if (!Bp.empty()) S = plan_slots(M, Bp); }
        if (n_slots) *n_slots = 0;
        if (n_padding) *n_padding = 0;
        if (bad) *bad = 0;
        if (!S.val) return SMG_OK;
        const Csr& A = h->lv[lv].A;
        std::vector<double> mirrored;
        if (against_transpose) {
            std::vector<int> tsrc;
            const Csr AT = transpose(A, &tsrc);
            if (!(AT.ptr == A.ptr && AT.col == A.col)) return fail(SMG_ERR_INVALID, "smg_debug_check_plan_value_maps: level %d is not structurally symmetric", lv);
            mirrored.resize(A.val.size());
            for (size_t e = 0; e < mirrored.size(); e++) mirrored[e] = A.val[(size_t)tsrc[e]];
        }
        const double* level_val = against_transpose ? mirrored.data() : A.val.data();
        const size_t n_level_val = A.val.size();
        auto same_bits = [](double a, double b) { return std::memcmp(&a, &b, sizeof(double)) == 0; };
        int slots = 0, padding = 0, wrong = 0;
        auto check = [&](const std::vector<double>& val, const std::vector<int>& map, double pad) {
            if (val.size() != map.size()) { wrong += (int)std::max(val.size(), map.size()); return; }
            for (size_t i = 0; i < val.size(); i++) {
                slots++;
                if (map[i] < 0) { padding++; wrong += !same_bits(val[i], pad); }
                else wrong += (size_t)map[i] >= n_level_val || !same_bits(val[i], level_val[(size_t)map[i]]);
            }
        };
        check(*S.val, S.map, 0.0);
        check(*S.diag, S.mapd, 1.0);
        if (n_slots) *n_slots = slots;
        if (n_padding) *n_padding = padding;
        if (bad) *bad = wrong;
        return SMG_OK;
    });
}
