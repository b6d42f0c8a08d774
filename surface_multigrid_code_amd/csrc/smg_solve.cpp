// smg_solve.cpp -- min_quad_with_fixed_mg_solve (reference src/min_quad_with_fixed_mg.cpp:80-135, :288-361) behind smg_solve*: everything that
// owns the state of a solve in progress (smg_hierarchy::in_solve).  The replayable steps of the loops and their hipGraph cache, the outer loop
// with its device-side break test (Ctrl, smg_device.hpp) in its stationary, split-phase, speculative, column-sharded and conjugate-gradient
// forms.  What a cycle is -- the launches of a V-cycle, of the outer residual -- lives in smg_cycle.cpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "smg_internal.hpp"

using namespace smg;

// ------------------------------------------------------------------------------------------------ steps and their graphs
static GraphKey current_graph_key(const smg_hierarchy* h)
{
    GraphKey key;
    key.k = h->k; key.k_user = h->k_user; key.pre = h->pre; key.post = h->post; key.precision = h->precision; key.smoother = h->smoother;
    key.jacobi_max_rows = h->jacobi_max_rows; key.omega = h->omega; key.cheby_fraction = h->cheby_fraction; key.head_fuse = h->head_fuse;
    return key;
}

static int graph_iters() { static const int v = std::max(1, std::min(16, env_int("SMG_GRAPH_ITERS", 4))); return v; }
// hipStreamBeginCapture is not allowed on the legacy default stream (smg_hierarchy_set_stream(h, NULL)): eager launches there
static bool graphs_usable(const smg_hierarchy* h) { return h->use_graph && !h->prof_on && h->stream != nullptr; }

static int enqueue_cycle_speculative(smg_hierarchy* h);
static int enqueue_pcg_iteration(smg_hierarchy* h);

// The launches of a step: what capture records and what the eager path (no graphs: profiling, the legacy default stream, use_graph = 0) issues, so
// that replay and eager launches give the same bits.  buf: the reduction buffer of the split pair.
static int enqueue_step(smg_hierarchy* h, Step s, double* buf)
{
    const int k = h->k;
    int rc;
    switch (s) {
    case STEP_ITER:
    case STEP_ITER_N:
        // Between two graph launches the stream idles for the runtime's hand-over (8.7 us in the rocprof timeline of a 316 us iteration); several iterations
        // in one graph pay it once.  Semantics unchanged: every launch of an iteration after the one whose break test fired writes nothing (Ctrl::done), as
        // for iterations enqueued ahead of the host's polling.  SMG_GRAPH_ITERS (default 4; 1 = off): C3 headline 3 168 (1) / 3 174 (2) / 3 194 (4) V-cycles/s, same box, alternating.
        for (int i = 0, n = s == STEP_ITER ? 1 : graph_iters(); i < n; i++) {
            if ((rc = enqueue_residual_ss(h, k, true))) return rc;
            if ((rc = enqueue_cycle_part(h, k, nullptr))) return rc;      // nullptr: the break test already ran inside the residual launch
        }
        return SMG_OK;
    case STEP_HEAD: return enqueue_residual_ss(h, k, true);
    case STEP_TAIL: return enqueue_cycle_part(h, k, nullptr);
    // The two halves of a split-phase iteration work on ONE buffer that the caller all-reduces in between: the residual leaves the local sum of
    // squares there, the cycle's break test reads the reduced value from there (no staging copies: an 8-byte device-to-device copy costs several
    // microseconds of stream time).
    case STEP_SPLIT_RESID: return enqueue_residual_ss(h, k, false, buf);
    case STEP_SPLIT_CYCLE: return enqueue_cycle_part(h, k, buf);
    case STEP_SPEC: return enqueue_cycle_speculative(h);
    case STEP_PCG:
    case STEP_PCG_N:
        for (int i = 0, n = s == STEP_PCG ? 1 : graph_iters(); i < n; i++)
            if ((rc = enqueue_pcg_iteration(h))) return rc;
        return SMG_OK;
    case STEP_COUNT: break;
    }
    return fail(SMG_ERR_INVALID, "enqueue_step: no such step");
}

static int capture_step(smg_hierarchy* h, Step s, double* buf = nullptr)
{
    return capture_graph(h, &h->graphs.exec[s], [&]() { return enqueue_step(h, s, buf); });
}

static int capture_split_pair(smg_hierarchy* h, double* buf)
{
    GraphCache& G = h->graphs;
    G.drop(STEP_SPLIT_RESID, STEP_SPLIT_CYCLE + 1);
    int rc = capture_step(h, STEP_SPLIT_RESID, buf);
    if (rc || (rc = capture_step(h, STEP_SPLIT_CYCLE, buf))) return rc;
    G.sumsq = buf;
    return SMG_OK;
}

// Step s has a graph that describes the handle's current selection.  Steps are captured in groups, at the first use of any member under a key: the
// stationary group (a change of its key drops every graph of the handle), in it the speculative cycle at its own first use and the split pair again
// when the caller hands in another buffer; the PCG pair.
static int ensure_step(smg_hierarchy* h, Step s, double* buf)
{
    GraphCache& G = h->graphs;
    const GraphKey key = current_graph_key(h);
    int rc;
    if (s == STEP_PCG || s == STEP_PCG_N) {
        if (G.exec[STEP_PCG] && G.pcg_key == key) return SMG_OK;
        G.drop(STEP_PCG, STEP_PCG_N + 1);
        if ((rc = capture_step(h, STEP_PCG))) return rc;
        if (graph_iters() > 1 && (rc = capture_step(h, STEP_PCG_N))) return rc;
        G.pcg_key = key;
        return SMG_OK;
    }
    if (!G.exec[STEP_ITER] || G.mg_key != key) {
        G.drop();
        if ((rc = capture_step(h, STEP_ITER))) return rc;
        if (graph_iters() > 1 && (rc = capture_step(h, STEP_ITER_N))) return rc;
        if (!h->union_m) {      // (a union has no split-phase iteration and none the host looks into: its members stop one by one)
            if ((rc = capture_split_pair(h, G.sumsq ? G.sumsq : &h->d_ctrl.p->sumsq))) return rc;
            if ((rc = capture_step(h, STEP_HEAD)) || (rc = capture_step(h, STEP_TAIL))) return rc;
        }
        G.mg_key = key;
    }
    if ((s == STEP_SPLIT_RESID || s == STEP_SPLIT_CYCLE) && G.sumsq != buf) return capture_split_pair(h, buf);
    if (s == STEP_SPEC && !G.exec[STEP_SPEC]) return capture_step(h, STEP_SPEC);
    return SMG_OK;
}

static int run_step(smg_hierarchy* h, Step s, double* buf = nullptr)
{
    if (!graphs_usable(h)) return enqueue_step(h, s, buf);
    int rc = ensure_step(h, s, buf);
    if (rc) return rc;
    HIPCHK(hipGraphLaunch(h->graphs.exec[s], h->stream));
    return SMG_OK;
}

// n iterations, `one` at a time or `many` = graph_iters() of them per launch (worth it for graphs only: eager launches gain nothing from the grouping)
static int enqueue_iterations(smg_hierarchy* h, int n, Step one, Step many)
{
    int rc;
    if (graphs_usable(h) && graph_iters() > 1)
        for (; n >= graph_iters(); n -= graph_iters()) { if ((rc = run_step(h, many))) return rc; h->iters_enqueued += graph_iters(); }
    for (; n > 0; n--) { if ((rc = run_step(h, one))) return rc; h->iters_enqueued++; }
    return SMG_OK;
}

// the control block as the stream has it now (one synchronisation); through page-locked memory
static int read_ctrl(smg_hierarchy* h, Ctrl* out)
{
    HIPCHK(h->pin_ctrl.ensure(1));
    HIPCHK(hipMemcpyAsync(h->pin_ctrl.p, h->d_ctrl.p, sizeof(Ctrl), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    *out = *h->pin_ctrl.p;
    return SMG_OK;
}

// One outer iteration the host looks INTO: residual + break test, a look at the flag, and the V-cycle only if the loop goes on.  An iteration
// enqueued whole runs its cycle even when its own break test has just fired (every launch after the break stores nothing, but does its work):
// the last iteration of every solve -- 0.31 ms at C3, of a 3.6 ms solve; a whole cycle more than the one a tol = 1e-3 solve of a small mesh
// needs.  The host looks at the flag after every chunk of iterations anyway; where the chunk is a single iteration (the end of every solve
// under the adaptive schedule), the look moves in front of the cycle.  Same launches in the same order as the whole iteration.
static int enqueue_checked_iteration(smg_hierarchy* h, Ctrl* seen)
{
    int rc = run_step(h, STEP_HEAD);
    if (rc) return rc;
    h->iters_enqueued++;      // (its residual is recorded whether or not the cycle follows)
    if ((rc = read_ctrl(h, seen))) return rc;      // (the flag and what the adaptive schedule reads)
    return seen->done ? (int)SMG_OK : run_step(h, STEP_TAIL);
}

// ------------------------------------------------------------------------------------------------ solve
// host blocks of up to 1 MiB travel through page-locked staging (pin_vec): packed by the host, one DMA each way
static bool small_host_block(int n, int k) { return (size_t)n * k * 8 <= ((size_t)1 << 20); }

int smg::check_cycle_opts(const smg_solve_opts& o)
{
    if (o.precision != 0 && o.precision != 1) return fail(SMG_ERR_INVALID, "precision must be 0 (fp64) or 1 (mixed)");
    if (o.pre < 0 || o.post < 0) return fail(SMG_ERR_INVALID, "pre / post must be >= 0");
    if (o.smoother < SMG_SMOOTH_GS || o.smoother > SMG_SMOOTH_HYBRID_CHEBYSHEV) return fail(SMG_ERR_INVALID, "smoother must be one of SMG_SMOOTH_*");
    if (o.omega > 2.0 || o.omega != o.omega) return fail(SMG_ERR_INVALID, "omega must be in (0, 2]");
    if (o.cheby_fraction >= 1.0 || o.cheby_fraction != o.cheby_fraction) return fail(SMG_ERR_INVALID, "cheby_fraction must be in (0, 1)");
    return SMG_OK;
}

static void latch_loop_opts(smg_hierarchy* h, const smg_solve_opts& o)      // what a rank without columns takes, too
{
    h->tol = o.tol; h->max_iter = o.max_iter; h->verbosity = o.verbosity;
    h->check_every = std::max(0, o.check_every);
}

int smg::latch_solve_opts(smg_hierarchy* h, const smg_solve_opts& o)
{
    latch_loop_opts(h, o);
    h->pre = o.pre; h->post = o.post; h->use_graph = o.use_graph; h->precision = o.precision;
    int rc = smg_hierarchy_set_smoother(h, o.smoother, o.omega, o.jacobi_max_rows);
    return rc ? rc : smg_hierarchy_set_chebyshev(h, o.cheby_fraction);
}

// A fresh control block, uploaded on the stream: not done, no entries, the handle's tolerance.  The residual history lives in HBM with room for `cap`
// entries (a solve sizes it from max_iter: the reference's r_his grows with the loop, .cpp:112).
int smg::reset_ctrl(smg_hierarchy* h, int cap)
{
    HIPCHK(h->d_rhis.ensure((size_t)std::max(cap, 1)));
    Ctrl& zero = h->host_ctrl;   // lives in the handle: the asynchronous copy may read it after this call returns
    std::memset(&zero, 0, sizeof(zero));
    zero.tol = h->tol;
    zero.r_his = h->d_rhis.p;
    zero.his_cap = (int)std::min<size_t>(h->d_rhis.n, (size_t)std::max(cap, 0));
    HIPCHK(hipMemcpyAsync(h->d_ctrl.p, &zero, sizeof(Ctrl), hipMemcpyHostToDevice, h->stream));
    return SMG_OK;
}

// The end of a loop: control block and the first `cap` history entries through page-locked memory, one synchronisation (whatever else the caller
// has enqueued on the stream is complete, too).  converged as the reference has it (:131-134 / :357-360).
static int fetch_history(smg_hierarchy* h, int cap, Ctrl* hc, double* r_his, int* n_his, int* converged)      // (n_his is not optional here)
{
    HIPCHK(h->pin_his.ensure((size_t)cap));
    HIPCHK(h->pin_ctrl.ensure(1));
    HIPCHK(hipMemcpyAsync(h->pin_ctrl.p, h->d_ctrl.p, sizeof(Ctrl), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(h->pin_his.p, h->d_rhis.p, (size_t)cap * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    *hc = *h->pin_ctrl.p;
    const double* his = h->pin_his.p;
    const int cnt = std::max(0, std::min(std::min(hc->n_his, hc->his_cap), cap));
    if (r_his) for (int i = 0; i < cnt; i++) r_his[i] = his[i];
    *n_his = cnt;
    const double last = cnt > 0 ? his[cnt - 1] : HUGE_VAL;
    if (converged) *converged = (last > h->tol) ? 0 : 1;
    return SMG_OK;
}

static void abandon_solve(smg_hierarchy* h) { h->in_solve = false; h->coarse_cols = 0; }

static int smg_solve_begin_impl(smg_hierarchy* h, const double* RHS, int ld_rhs, const double* known_val, int ld_kv,
                               const double* z0, int ld_z0, int k, int memspace, const smg_solve_opts* opts)
{
    int rc = check_ready(h, "smg_solve_begin");
    if (rc) return rc;
    smg_solve_opts o;
    smg_solve_opts_default(&o);
    if (opts) o = *opts;
    const int n = h->n_full;
    if (!RHS || !z0 || k < 1 || ld_rhs < n || ld_z0 < n) return fail(SMG_ERR_INVALID, "smg_solve: bad RHS/z0/k/ld");
    if (o.max_iter < 0) return fail(SMG_ERR_INVALID, "max_iter must be >= 0");
    if (h->has_known && (!known_val || ld_kv < (int)h->known.size())) return fail(SMG_ERR_INVALID, "known_val missing or ld_kv too small");
    // everything is validated before anything of the handle changes: a refused call leaves the handle as it was
    if ((rc = smg::check_cycle_opts(o))) return rc;
    if (h->in_solve) return fail(SMG_ERR_INVALID, "smg_solve_begin: a split-phase solve is already in progress (smg_solve_end)");
    if (h->union_m > 0 && o.precision != 0) return fail(SMG_ERR_INVALID, "a union handle solves in fp64 (no mixed-precision cycle)");
    if ((rc = latch_solve_opts(h, o))) return rc;
    DeviceScope dsc(h->device);
    const int kin = internal_cols(h, k);
    rc = ensure_work(h, kin);
    if (rc) return rc;
    if (h->precision == 1 && (rc = ensure_fp32(h, kin))) return rc;
    h->k = kin; h->k_user = k;
    h->coarse_cols = kin > k ? k : 0;
    const int nk = (int)h->known.size();
    // stage host inputs
    const double *dR = RHS, *dZ = z0, *dK = known_val;
    int ldR = ld_rhs, ldZ = ld_z0, ldK = ld_kv;
    if (memspace == SMG_HOST) {
        HIPCHK(h->d_stage_rhs.ensure((size_t)n * k));
        HIPCHK(h->d_stage_z.ensure((size_t)n * k));
        if (small_host_block(n, k)) {
            // small blocks: packed into page-locked memory by the host, then ONE copy each
            HIPCHK(h->pin_vec.ensure((size_t)2 * n * k));
            for (int c = 0; c < k; c++) {
                std::memcpy(h->pin_vec.p + (size_t)c * n, RHS + (size_t)c * ld_rhs, (size_t)n * 8);
                std::memcpy(h->pin_vec.p + (size_t)(k + c) * n, z0 + (size_t)c * ld_z0, (size_t)n * 8);
            }
            HIPCHK(hipMemcpyAsync(h->d_stage_rhs.p, h->pin_vec.p, (size_t)n * k * 8, hipMemcpyHostToDevice, h->stream));
            HIPCHK(hipMemcpyAsync(h->d_stage_z.p, h->pin_vec.p + (size_t)n * k, (size_t)n * k * 8, hipMemcpyHostToDevice, h->stream));
        } else {
            HIPCHK(hipMemcpy2DAsync(h->d_stage_rhs.p, (size_t)n * 8, RHS, (size_t)ld_rhs * 8, (size_t)n * 8, k, hipMemcpyHostToDevice, h->stream));
            HIPCHK(hipMemcpy2DAsync(h->d_stage_z.p, (size_t)n * 8, z0, (size_t)ld_z0 * 8, (size_t)n * 8, k, hipMemcpyHostToDevice, h->stream));
        }
        dR = h->d_stage_rhs.p; dZ = h->d_stage_z.p; ldR = n; ldZ = n;
        if (h->has_known) {
            HIPCHK(h->d_stage_kv.ensure((size_t)nk * k));
            HIPCHK(hipMemcpy2DAsync(h->d_stage_kv.p, (size_t)nk * 8, known_val, (size_t)ld_kv * 8, (size_t)nk * 8, k, hipMemcpyHostToDevice, h->stream));
            dK = h->d_stage_kv.p; ldK = nk;
        }
    } else if (h->has_known) {
        // keep a private copy: the caller may reuse its buffer before smg_solve_end scatters z(known)
        HIPCHK(h->d_stage_kv.ensure((size_t)nk * k));
        HIPCHK(hipMemcpy2DAsync(h->d_stage_kv.p, (size_t)nk * 8, known_val, (size_t)ld_kv * 8, (size_t)nk * 8, k, hipMemcpyDeviceToDevice, h->stream));
        dK = h->d_stage_kv.p; ldK = nk;
    }
    h->cur_kv = dK; h->cur_ld_kv = ldK;
    Level& L0 = h->lv[0];
    // z_u = z0(unknown)  (:310-311)  /  z = z0 (:97)
    HIPCHK(launch_gather_in(L0.u.p, dZ, h->d_map0.p, L0.n, k, kin, ldZ, h->stream));
    if (h->has_known) {
        // RHS_u = RHS(unknown) - Auk * known_val  (:316-318)
        const int nu = L0.n;
        HIPCHK(h->d_tmp_cm.ensure((size_t)nu * k));
        HIPCHK(launch_gather_cm(h->d_tmp_cm.p, dR, h->d_unknown.p, nu, k, ldR, nu, h->stream));
        HIPCHK(launch_csr_sub(nu, h->d_auk_ptr.p, h->d_auk_col.p, h->d_auk_val.p, dK, ldK, h->d_tmp_cm.p, nu, k, h->stream));
        HIPCHK(launch_gather_in(L0.b.p, h->d_tmp_cm.p, h->d_perm0.p, nu, k, kin, nu, h->stream));
    } else {
        HIPCHK(launch_gather_in(L0.b.p, dR, h->d_map0.p, L0.n, k, kin, ldR, h->stream));
    }
    if ((rc = reset_ctrl(h, std::max(h->max_iter, 1)))) return rc;
    if (memspace == SMG_HOST) HIPCHK(hipStreamSynchronize(h->stream));  // the caller's host blocks may change after this call
    if (h->union_m > 0) {
        if ((rc = union_begin_solve(h, k))) return rc;
    }
    h->head_fuse = head_fusable(h, kin);   // latched: both halves of every iteration of this solve follow it
    h->iters_enqueued = 0;
    h->in_solve = true;
    return SMG_OK;
}

extern "C" int smg_solve_begin(smg_hierarchy* h, const double* RHS, int ld_rhs, const double* known_val, int ld_kv,
                               const double* z0, int ld_z0, int k, int memspace, const smg_solve_opts* opts)
{
    return guarded("smg_solve_begin", [&]() { return smg_solve_begin_impl(h, RHS, ld_rhs, known_val, ld_kv, z0, ld_z0, k, memspace, opts); });
}

extern "C" int smg_solve_iter_residual(smg_hierarchy* h, double* d_sumsq)
{
    if (!h || !h->in_solve) return fail(SMG_ERR_INVALID, "smg_solve_iter_residual: no solve in progress");
    DeviceScope dsc(h->device);
    return run_step(h, STEP_SPLIT_RESID, d_sumsq ? d_sumsq : &h->d_ctrl.p->sumsq);
}

extern "C" int smg_solve_iter_cycle(smg_hierarchy* h, const double* d_sumsq)
{
    if (!h || !h->in_solve) return fail(SMG_ERR_INVALID, "smg_solve_iter_cycle: no solve in progress");
    DeviceScope dsc(h->device);
    int rc = run_step(h, STEP_SPLIT_CYCLE, d_sumsq ? const_cast<double*>(d_sumsq) : &h->d_ctrl.p->sumsq);
    if (rc) return rc;
    h->iters_enqueued++;
    return SMG_OK;
}

// save z, V-cycle in place -- nothing here reads the reduced residual
static int enqueue_cycle_speculative(smg_hierarchy* h)
{
    Level& L0 = h->lv[0];
    const size_t cnt = (size_t)L0.n * h->k;
    HIPCHK(launch_copy_unless_done(h->d_zsave.p, L0.u.p, cnt, h->d_ctrl.p, h->stream));
    return enqueue_cycle_part(h, h->k, nullptr);   // nullptr: no decide in front of the cycle
}

extern "C" int smg_solve_iter_cycle_speculative(smg_hierarchy* h)
{
    if (!h || !h->in_solve) return fail(SMG_ERR_INVALID, "smg_solve_iter_cycle_speculative: no solve in progress");
    DeviceScope dsc(h->device);
    HIPCHK(h->d_zsave.ensure((size_t)h->lv[0].n * h->k));
    int rc = run_step(h, STEP_SPEC);
    if (rc) return rc;
    h->iters_enqueued++;
    return SMG_OK;
}

extern "C" int smg_solve_iter_commit(smg_hierarchy* h, const double* d_sumsq)
{
    if (!h || !h->in_solve) return fail(SMG_ERR_INVALID, "smg_solve_iter_commit: no solve in progress");
    DeviceScope dsc(h->device);
    Level& L0 = h->lv[0];
    HIPCHK(launch_decide_spec(h->d_ctrl.p, d_sumsq ? d_sumsq : &h->d_ctrl.p->sumsq, h->stream));
    HIPCHK(launch_restore_if_just_done(L0.u.p, h->d_zsave.p, (size_t)L0.n * h->k, h->d_ctrl.p, h->stream));
    return SMG_OK;
}

extern "C" int smg_solve_poll(smg_hierarchy* h, int* done, int* n_his)
{
    if (!h || !h->in_solve) return fail(SMG_ERR_INVALID, "smg_solve_poll: no solve in progress");
    DeviceScope dsc(h->device);
    int hdr[4];
    HIPCHK(hipMemcpyAsync(hdr, h->d_ctrl.p, sizeof(hdr), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (done) *done = hdr[0];
    if (n_his) *n_his = hdr[1];
    return SMG_OK;
}

extern "C" int smg_solve_end(smg_hierarchy* h, double* z, int ld_z, int memspace, double* r_his, int* n_his, int* converged)
{
    if (!h || !h->in_solve) return fail(SMG_ERR_INVALID, "smg_solve_end: no solve in progress");
    DeviceScope dsc(h->device);
    const int n = h->n_full, k = h->k_user;
    if (!z || ld_z < n) return fail(SMG_ERR_INVALID, "smg_solve_end: bad z / ld_z");
    Level& L0 = h->lv[0];
    double* dz = z;
    int ldz = ld_z;
    if (memspace == SMG_HOST) {
        HIPCHK(h->d_stage_z.ensure((size_t)n * k));
        dz = h->d_stage_z.p; ldz = n;
    }
    // z(unknown) = z_u ; z(known) = known_val  (:353-355)
    HIPCHK(launch_scatter_out(dz, L0.u.p, h->d_map0.p, L0.n, k, h->k, ldz, h->stream));
    if (h->has_known)
        HIPCHK(launch_scatter_cm(dz, h->cur_kv, h->d_known.p, (int)h->known.size(), k, h->cur_ld_kv, ldz, h->stream));
    const bool z_pinned = memspace == SMG_HOST && small_host_block(n, k);
    if (z_pinned) {
        HIPCHK(h->pin_vec.ensure((size_t)2 * n * k));
        HIPCHK(hipMemcpyAsync(h->pin_vec.p, dz, (size_t)n * k * 8, hipMemcpyDeviceToHost, h->stream));
    } else if (memspace == SMG_HOST)
        HIPCHK(hipMemcpy2DAsync(z, (size_t)ld_z * 8, dz, (size_t)n * 8, (size_t)n * 8, k, hipMemcpyDeviceToHost, h->stream));
    Ctrl hc;
    int cnt = 0;
    // the history can hold at most one entry per enqueued iteration
    const int cap = (int)std::min<size_t>(h->d_rhis.n, (size_t)std::max(std::min(h->iters_enqueued, std::max(h->max_iter, 1)), 1));
    { int rc = fetch_history(h, cap, &hc, r_his, &cnt, converged); if (rc) return rc; }
    if (n_his) *n_his = cnt;
    const double* his = h->pin_his.p;
    if (z_pinned) for (int c = 0; c < k; c++) std::memcpy(z + (size_t)c * ld_z, h->pin_vec.p + (size_t)c * n, (size_t)n * 8);
    abandon_solve(h);
    prof_collect(h);
    if (h->union_m > 0 && converged) {      // every member's own loop ended below the tolerance (the handle's history holds the norm over all members)
        std::vector<int> md((size_t)h->union_m, 0);
        HIPCHK(hipMemcpy(md.data(), h->un.done.p, md.size() * sizeof(int), hipMemcpyDeviceToHost));
        *converged = (hc.status == 0 && std::all_of(md.begin(), md.end(), [](int d) { return d == 1; })) ? 1 : 0;      // 2 = that member's residual went non-finite
    }
    if (h->verbosity > 0) {
        for (int i = 0; i < cnt; i++) std::printf("MG iteration: %d, residual: %g\n", i, his[i]);  // :111
        if (cnt) std::printf("residual norm: %g\n", his[cnt - 1]);                                    // :127
    }
    { int rc = coarse_stall_check(h); if (rc) return rc; }
    if (hc.status != 0) return fail(SMG_ERR_NONFINITE, "non-finite residual at iteration %d", cnt - 1);
    return SMG_OK;
}

// for (iter < maxIter) { residual; push; if (residual < tol) break; V-cycle }   (:108-125 / :330-347)
// The break happens on the device; the host only decides how many iterations to enqueue before it looks at the flag again.
// check_every >= 1: that many.  check_every == 0 (default): adaptive -- from the two most recent residuals the host extrapolates
// how many more cycles the tolerance needs and enqueues all but the last of them before the next look (the results do not depend
// on this: an iteration enqueued after the break stores nothing).  The schedule is a function of the residual history alone, so the
// ranks of a column-sharded solve -- who all see the same reduced residuals -- enqueue (and reduce) the same number of times.
// budget >= 0: at most that many iterations instead of max_iter (smg_solve_pcg: the entries its first residual and its checks have used are not iterations).
template <typename Iter>
static int run_outer_loop(smg_hierarchy* h, Iter&& iterations, bool look_into_single_iterations = false, int budget = -1)
{
    int it = 0;
    int chunk_next = 1;
    static const int look_env = env_int("SMG_LOOK_INTO", 1);      // A/B knob
    const bool look = look_into_single_iterations && look_env != 0;
    const int max_it = budget >= 0 ? budget : h->max_iter;
    while (it < max_it) {
        const int want = h->check_every > 0 ? h->check_every : chunk_next;
        const int chunk = std::min(want, max_it - it);
        Ctrl hc;
        if (look && chunk == 1) {
            // the look happens between the iteration's break test and its cycle; the cycle is enqueued behind it and the loop goes straight on
            int rc = enqueue_checked_iteration(h, &hc);
            if (rc) return rc;
            if (hc.done) break;
            it += 1;
        } else {
            { int rc = iterations(chunk); if (rc) return rc; }
            it += chunk;
            if (it >= max_it) break;
            { int rc = read_ctrl(h, &hc); if (rc) return rc; }
            if (hc.done) break;
        }
        chunk_next = 1;
        if (h->check_every == 0 && hc.n_his >= 2 && hc.r_last > 0.0 && hc.r_last < hc.r_prev && h->tol > 0.0 && hc.r_last > h->tol) {
            const double need = std::ceil(std::log(h->tol / hc.r_last) / std::log(hc.r_last / hc.r_prev));   // more residuals until < tol
            if (need > 2.0) chunk_next = (int)std::min(need - 1.0, 64.0);
        }
    }
    return SMG_OK;
}

extern "C" int smg_solve(smg_hierarchy* h, const double* RHS, int ld_rhs, const double* known_val, int ld_kv,
                         const double* z0, int ld_z0, int k, int memspace, const smg_solve_opts* opts, double* z, int ld_z,
                         double* r_his, int* n_his, int* converged)
{
    int rc = smg_solve_begin(h, RHS, ld_rhs, known_val, ld_kv, z0, ld_z0, k, memspace, opts);
    if (rc) return rc;
    rc = run_outer_loop(h, [&](int n) { return enqueue_iterations(h, n, STEP_ITER, STEP_ITER_N); }, h->union_m == 0);
    if (rc) { abandon_solve(h); return rc; }
    return smg_solve_end(h, z, ld_z, memspace, r_his, n_his, converged);
}

// ---- conjugate gradients preconditioned by the V-cycle (include/smg.h: smg_solve_pcg) ------------------------------------------------
// Flexible (Polak-Ribiere) PCG, one recurrence per column.  The vectors live in the handle's Krylov buffers; the V-cycle
// keeps its own: its input r goes into L0.b (L0.f32.b), it starts from L0.u = 0 and leaves z in L0.u.  One iteration:
//   z = V(r, 0);  rz = z.r, beta = -alpha_prev z.q / rz_prev;  p = z + beta p;  q = A p;  alpha = rz / p.q;  x += alpha p, r -= alpha q;  |r|_F -> r_his
// and every launch of it starts with `if (done) return`, so iterations enqueued after the break store nothing -- the schedule of the outer loop
// (run_outer_loop) is smg_solve's.
static int ensure_krylov(smg_hierarchy* h)
{
    const int n = h->lv[0].n, k = h->k;
    const size_t cnt = (size_t)n * k;
    const int groups = kry_groups(n, k);
    const size_t npart = (size_t)2 * groups * k, ns = (size_t)KS_SLOTS * k;
    if (h->kry_x.n < cnt || h->kry_part.n < npart || h->kry_s.n < ns || !h->kry_restart.p) {
        drop_graphs(h);      // (the PCG graphs hold these pointers; the MG graphs are recaptured at their next use)
        for (DevBuf<double>* b : {&h->kry_x, &h->kry_r, &h->kry_p, &h->kry_q, &h->kry_b}) {
            HIPCHK(b->ensure(cnt));
            HIPCHK(hipMemsetAsync(b->p, 0, b->n * sizeof(double), h->stream));
        }
        HIPCHK(h->kry_part.ensure(npart));
        HIPCHK(h->kry_s.ensure(ns));
        HIPCHK(hipMemsetAsync(h->kry_s.p, 0, h->kry_s.n * sizeof(double), h->stream));
        HIPCHK(h->kry_restart.ensure(1));
    }
    KryDev& K = h->kry;
    K.n = n; K.k = k; K.groups = groups;
    K.part = h->kry_part.p; K.s = h->kry_s.p; K.restart = h->kry_restart.p;
    return SMG_OK;
}

// (a linear chain of launches: STEP_PCG / STEP_PCG_N)
static int enqueue_pcg_iteration(smg_hierarchy* h)
{
    Level& L0 = h->lv[0];
    const int k = h->k;
    const size_t cnt = (size_t)L0.n * k;
    Ctrl* ctrl = h->d_ctrl.p;
    const KryDev& K = h->kry;
    {
        ProfGuard pg(h, "MG: total VCycle");
        if (h->precision == 1) HIPCHK(launch_residual_to_f32(L0.f32.b.p, L0.f32.u.p, h->kry_r.p, cnt, ctrl, h->stream));     // the fp32 cycle: z = (double) V32((float) r, 0)
        else HIPCHK(launch_kry_precond_in(h->kry_r.p, L0.b.p, L0.u.p, cnt, ctrl, h->stream));
        int rc = enqueue_vcycle(h, k, ctrl, FIRST_NONE);
        if (rc) return rc;
        if (h->precision == 1) HIPCHK(launch_kry_widen(L0.f32.u.p, L0.u.p, cnt, ctrl, h->stream));
    }
    ProfGuard pg(h, "PCG: vectors");
    HIPCHK(launch_kry_dots_zr_zq(K, L0.u.p, h->kry_r.p, h->kry_q.p, ctrl, h->stream));
    HIPCHK(launch_kry_direction(K, L0.u.p, h->kry_p.p, ctrl, h->stream));
    if (int rc = apply_A(h, 0, SELL_AX, h->kry_p.p, nullptr, h->kry_q.p, k, ctrl)) return rc;
    HIPCHK(launch_kry_dots_pq(K, h->kry_p.p, h->kry_q.p, ctrl, h->stream));
    HIPCHK(launch_kry_step_decide(K, h->kry_x.p, h->kry_r.p, h->kry_p.p, h->kry_q.p, ctrl, h->stream));
    return SMG_OK;
}

// r_his[n_his] = |RHS_u - A x| of the iterate in the Krylov buffer x, measured as smg_solve measures it, with the break test.  reopen: it replaces
// the last entry (a recurrence norm that passed the test) and the restart flag is raised.
static int enqueue_pcg_true_residual(smg_hierarchy* h, bool head, bool reopen)
{
    Level& L0 = h->lv[0];
    const size_t bytes = (size_t)L0.n * h->k * sizeof(double);
    HIPCHK(hipMemcpyAsync(L0.u.p, h->kry_x.p, bytes, hipMemcpyDeviceToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(L0.b.p, h->kry_b.p, bytes, hipMemcpyDeviceToDevice, h->stream));
    HIPCHK(launch_kry_arm(h->kry, h->d_ctrl.p, reopen, h->stream));
    h->head_fuse = head;
    int rc = enqueue_residual_ss(h, h->k, true);
    h->head_fuse = false;
    if (rc) return rc;
    // r = RHS_u - A x: the recurrence (re)starts from the true residual
    return apply_A(h, 0, SELL_RESID, h->kry_x.p, h->kry_b.p, h->kry_r.p, h->k, h->d_ctrl.p);
}

static int pcg_loop(smg_hierarchy* h)
{
    if (h->max_iter == 0) return SMG_OK;              // z = z0, no entries (as smg_solve)
    int rc = ensure_krylov(h);
    if (rc) return rc;
    Level& L0 = h->lv[0];
    const size_t bytes = (size_t)L0.n * h->k * sizeof(double);
    const bool head = h->head_fuse;                   // entry 0 and the checks measure as smg_solve does; the iterations never fuse
    h->head_fuse = false;
    HIPCHK(hipMemcpyAsync(h->kry_x.p, L0.u.p, bytes, hipMemcpyDeviceToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->kry_b.p, L0.b.p, bytes, hipMemcpyDeviceToDevice, h->stream));
    if ((rc = enqueue_pcg_true_residual(h, head, false))) return rc;
    h->iters_enqueued = 1;
    int n_true = 1;                                   // entries up to and including the last true residual
    Ctrl hc;
    for (;;) {
        rc = run_outer_loop(h, [&](int n) { return enqueue_iterations(h, n, STEP_PCG, STEP_PCG_N); }, false, h->max_iter - n_true);
        if (rc) return rc;
        if ((rc = read_ctrl(h, &hc))) return rc;
        // a recurrence norm passed the break test: verified on the true residual of x, which replaces it
        if (!hc.done || hc.status != 0 || hc.n_his <= n_true) break;
        if ((rc = enqueue_pcg_true_residual(h, head, true))) return rc;
        if ((rc = read_ctrl(h, &hc))) return rc;
        n_true = hc.n_his;
        if (hc.done || n_true >= h->max_iter) break;  // converged (or non-finite) / no entries left; else restart from x
    }
    HIPCHK(hipMemcpyAsync(L0.u.p, h->kry_x.p, bytes, hipMemcpyDeviceToDevice, h->stream));
    return SMG_OK;
}

extern "C" int smg_solve_pcg(smg_hierarchy* h, const double* RHS, int ld_rhs, const double* known_val, int ld_kv, const double* z0, int ld_z0, int k,
                             int memspace, const smg_solve_opts* opts, double* z, int ld_z, double* r_his, int* n_his, int* converged)
{
    return guarded("smg_solve_pcg", [&]() -> int {
        int rc = check_ready(h, "smg_solve_pcg");
        if (rc) return rc;
        if (h->union_m > 0) return fail(SMG_ERR_INVALID, "smg_solve_pcg: a union handle is not supported (its members stop one by one: use smg_solve)");
        if ((rc = smg_solve_begin_impl(h, RHS, ld_rhs, known_val, ld_kv, z0, ld_z0, k, memspace, opts))) return rc;
        DeviceScope dsc(h->device);
        rc = pcg_loop(h);
        if (rc) { abandon_solve(h); return rc; }
        return smg_solve_end(h, z, ld_z, memspace, r_his, n_his, converged);
    });
}

// ---- column-sharded solve (include/smg.h: smg_solve_sharded) ------------------------------------------------------------------------
// A rank without columns: no vectors, no cycle -- it adds 0 to every reduction and lets the device take the same decision from the
// reduced value as everybody else (same control block, same launch_decide, same polling schedule).
static int solve_sharded_empty(smg_hierarchy* h, const smg_solve_opts* opts, smg_reduce_fn reduce, void* ctx, double* r_his, int* n_his, int* converged)
{
    int rc = check_ready(h, "smg_solve_sharded");
    if (rc) return rc;
    if (h->in_solve) return fail(SMG_ERR_INVALID, "smg_solve_sharded: a split-phase solve is in progress");
    smg_solve_opts o;
    smg_solve_opts_default(&o);
    if (opts) o = *opts;
    if (o.max_iter < 0) return fail(SMG_ERR_INVALID, "max_iter must be >= 0");
    DeviceScope dsc(h->device);
    latch_loop_opts(h, o);
    if ((rc = reset_ctrl(h, std::max(h->max_iter, 1)))) return rc;
    double* buf = &h->d_ctrl.p->sumsq;
    int n_it = 0;
    rc = run_outer_loop(h, [&](int n) -> int {
        for (int i = 0; i < n; i++) {
            HIPCHK(hipMemsetAsync(buf, 0, sizeof(double), h->stream));
            if (reduce(buf, 1, (void*)h->stream, ctx) != 0) return fail(SMG_ERR_REDUCE, "smg_solve_sharded: the caller's reduction failed");
            HIPCHK(launch_decide(h->d_ctrl.p, buf, h->stream));
            n_it++;
        }
        return SMG_OK;
    });
    if (rc) return rc;
    Ctrl hc;
    int cnt = 0;
    if ((rc = fetch_history(h, std::max(std::min(n_it, std::max(h->max_iter, 1)), 1), &hc, r_his, &cnt, converged))) return rc;
    if (n_his) *n_his = cnt;
    if (hc.status != 0) return fail(SMG_ERR_NONFINITE, "non-finite residual at iteration %d", cnt - 1);
    return SMG_OK;
}

extern "C" int smg_solve_sharded(smg_hierarchy* h, const double* RHS, int ld_rhs, const double* known_val, int ld_kv, const double* z0,
                                 int ld_z0, int k_local, int memspace, const smg_solve_opts* opts, smg_reduce_fn reduce, void* ctx,
                                 double* z, int ld_z, double* r_his, int* n_his, int* converged)
{
    return guarded("smg_solve_sharded", [&]() -> int {
        if (!reduce) return fail(SMG_ERR_INVALID, "smg_solve_sharded: no reduction given");
        if (k_local < 0) return fail(SMG_ERR_INVALID, "smg_solve_sharded: k_local must be >= 0");
        if (k_local == 0) return solve_sharded_empty(h, opts, reduce, ctx, r_his, n_his, converged);
        int rc = smg_solve_begin(h, RHS, ld_rhs, known_val, ld_kv, z0, ld_z0, k_local, memspace, opts);
        if (rc) return rc;
        DeviceScope dsc(h->device);
        double* buf = &h->d_ctrl.p->sumsq;   // the word both halves of an iteration work on in place; the reduction too
        rc = run_outer_loop(h, [&](int n) -> int {
            for (int i = 0; i < n; i++) {
                int r = smg_solve_iter_residual(h, buf);
                if (r) return r;
                if (reduce(buf, 1, (void*)h->stream, ctx) != 0) return fail(SMG_ERR_REDUCE, "smg_solve_sharded: the caller's reduction failed");
                if ((r = smg_solve_iter_cycle(h, buf))) return r;
            }
            return SMG_OK;
        });
        if (rc) { abandon_solve(h); return rc; }
        return smg_solve_end(h, z, ld_z, memspace, r_his, n_his, converged);
    });
}

extern "C" int smg_raw_outer_iteration(smg_hierarchy* h, int n_iter)
{
    if (!h || !h->in_solve) return fail(SMG_ERR_INVALID, "smg_raw_outer_iteration: call smg_solve_begin first");
    DeviceScope dsc(h->device);
    return enqueue_iterations(h, n_iter, STEP_ITER, STEP_ITER_N);
}
