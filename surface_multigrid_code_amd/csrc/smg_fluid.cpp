// smg_fluid.cpp -- incompressible flow on a surface in vorticity - stream-function form (include/smg.h: smg_fluid_*):
// (-L) psi = -m (w - wbar), u = n x grad psi, a finite-volume transport of w on the barycentric dual cells whose fluxes are differences of psi, SSP
// Runge-Kutta stages, an optional implicit viscous solve.  The object owns the handles built from the caller's prolongations -- handle[0]: -L with
// vertex 0 (closed) or the boundary vertices (with boundary) known; handle[1] (viscosity > 0): M + viscosity dt (-L), no known rows -- the geometry
// the kernels read (csrc/smg_fluid_device.hip): faces, corner lists, the masses, the gradient basis, normals and areas of k_hodge_geometry, and the
// state: w, psi, dt and the times per column, all on the device.  A stage is one vertex kernel (the right-hand side), ONE k-column solve
// warm-started from the previous psi, the hot vertex kernel (transport and the stage's combination) and the fixed-order reductions of its terms,
// all enqueued on the object's stream, which the handles use too.  Beside the solve's own history the host reads one double per stage, |rhs|_F^2:
// it sets the default tolerance and refuses non-finite input before the solve.  A step writes into blocks beside the state and commits by an index
// swap, so a refused step leaves the state of the last completed one.  Checks, stream, handles, the cotangent system and the inner solve:
// smg_mesh_object.hpp.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <memory>
#include <utility>
#include <vector>

#include "smg_device.hpp"
#include "smg_fluid_inl.hpp"
#include "smg_mesh.hpp"
#include "smg_mesh_object.hpp"

using namespace smg;

struct smg_fluid : MeshObject {            // handle[0]: -L, vertex 0 or the boundary known; handle[1] (viscosity > 0): M + viscosity dt (-L)
    int nV = 0, nF = 0, nb = 0;            // nb: boundary vertices (0: closed)
    int pcg = 1;                           // the inner solver: 1 smg_solve_pcg, 0 smg_solve
    smg_fluid_params p;
    double vdt = 0.0;                      // the viscosity dt that handle[1] holds
    size_t kcap = 0, hcap = 0;             // the columns the state's blocks hold; the steps the histories hold
    int k = 0, cur = 0, pc = 0;            // the state's columns (0: none); which of Wb[3] holds w, which of psi[2] the last psi
    CotanSystem S;                         // the pattern and -L's values, for the viscous system
    std::vector<double> m_host;
    DevBuf<int> F, m_ptr, m_idx, known;    // faces, corner lists per vertex, 1 on the known rows
    DevBuf<double> W, nrm, Af, m, msum;    // gradient basis (9 per face), normals (3), areas; the masses and their sum
    DevBuf<double> val;                    // the viscous system's values
    DevBuf<double> Wb[3], psi[2], R;       // column-major n x k: the state and two stage blocks; psi and the solve's output; the right-hand side
    DevBuf<double> rsq, rate, mw, ew;      // k planes of n: the squares, the rates, m w, (1/2) m w^2
    DevBuf<double> terms, Us;              // k planes of nF: the energy terms; staging of a host call's velocity
    DevBuf<double> part, red;              // the chunk sums; |rhs|^2 (1) and 3 k sums of the diagnostics
    DevBuf<double> dt, time, rmax, mwsum;  // k each; rmax: 3 rows of k
    DevBuf<double> his, zero;              // 2 x steps x k: cfl then time; the known rows' values, zeros
    ~smg_fluid() { quiesce(); }
};

namespace smg {

int fluid_check_operands(const char* who, int op, int nV, int nF, int k, const int* F, const double* V, const double* w, const double* psi, const double* wn,
                         const double* dt, double theta, int rates_only, const double* out)
{
    if (op < SMG_FLUID_RHS || op > SMG_FLUID_DT || nV < 1 || nF < 1 || !F || !V || !out) return fail(SMG_ERR_INVALID, "%s: bad arguments", who);
    const bool full = op == SMG_FLUID_ADVECT && !rates_only;
    const bool needs_w = op == SMG_FLUID_RHS || op == SMG_FLUID_DIAG || op == SMG_FLUID_DT || full;
    const bool needs_psi = op == SMG_FLUID_ADVECT || op == SMG_FLUID_VELOCITY || op == SMG_FLUID_DT;
    if ((needs_w && !w) || (needs_psi && !psi) || (full && (!wn || !dt))) return fail(SMG_ERR_INVALID, "%s: op %d misses an operand", who, op);
    if (k < 1) return fail(SMG_ERR_INVALID, "%s: k = %d, at least one column is needed", who, k);
    if (full && !(theta >= 0.0 && theta <= 1.0)) return fail(SMG_ERR_INVALID, "%s: theta = %g, a value inside [0, 1] is needed", who, theta);
    return check_faces(who, F, nF, nV);
}

}  // namespace smg

namespace {

// the Shu-Osher pairs (a, b) of stage s
void stage_pair(int stages, int s, double* a, double* b)
{
    *a = 0.0; *b = 1.0;
    if (stages == 2 && s == 1) { *a = 0.5; *b = 0.5; }
    if (stages == 3 && s == 1) { *a = 0.75; *b = 0.25; }
    if (stages == 3 && s == 2) { *a = 1.0 / 3.0; *b = 2.0 / 3.0; }
}

int check_params(const char* who, const smg_fluid_params& p)
{
    if (!(p.theta >= 0.0) || !(p.theta <= 1.0)) return fail(SMG_ERR_INVALID, "%s: theta = %g, a value inside [0, 1] is needed", who, p.theta);
    if (p.stages < 1 || p.stages > 3) return fail(SMG_ERR_INVALID, "%s: stages = %d, 1, 2 or 3 is needed", who, p.stages);
    if (!std::isfinite(p.viscosity) || p.viscosity < 0.0) return fail(SMG_ERR_INVALID, "%s: viscosity = %g, a finite value >= 0 is needed", who, p.viscosity);
    if (!std::isfinite(p.dt) || p.dt < 0.0) return fail(SMG_ERR_INVALID, "%s: dt = %g, a finite value >= 0 is needed", who, p.dt);
    if (p.viscosity > 0.0 && p.dt == 0.0) return fail(SMG_ERR_INVALID, "%s: viscosity = %g needs a fixed step, dt > 0", who, p.viscosity);
    if (p.dt == 0.0 && (!std::isfinite(p.cfl) || !(p.cfl > 0.0)))
        return fail(SMG_ERR_INVALID, "%s: cfl = %g, a finite value > 0 is needed when dt == 0", who, p.cfl);
    return SMG_OK;
}

// handle[1]'s values M + vdt (-L) from the kept pattern; first: the pattern-setting precompute, else by values
int viscous_system(smg_fluid* g, double vdt, bool first)
{
    const size_t nnz = g->S.col.size();
    std::vector<double> val(nnz);
    for (int i = 0; i < g->nV; i++)
        for (int q = g->S.ptr[(size_t)i]; q < g->S.ptr[(size_t)i + 1]; q++) {
            const double x = vdt * g->S.L[(size_t)q];
            val[(size_t)q] = g->S.col[(size_t)q] == i ? g->m_host[(size_t)i] + x : x;
        }
    if (first) {
        if (int rc = smg_precompute(g->handle[1], g->nV, g->S.ptr.data(), g->S.col.data(), val.data(), nullptr, 0)) return rc;
    } else {
        HIPCHK(hipStreamSynchronize(g->stream));
        HIPCHK(g->val.ensure(nnz));
        HIPCHK(hipMemcpy(g->val.p, val.data(), nnz * sizeof(double), hipMemcpyHostToDevice));
        if (int rc = smg_precompute_values_device(g->handle[1], g->val.p)) return rc;
    }
    g->vdt = vdt;
    return SMG_OK;
}

int create_impl(const smg_hierarchy* h, const double* V, int nV, const int* F, int nF, const smg_fluid_params* p, smg_fluid** out)
{
    if (out) *out = nullptr;
    const char* who = "smg_fluid_create";
    if (!h || !V || !F || !p || !out || nV <= 0 || nF <= 0) return fail(SMG_ERR_INVALID, "%s: bad arguments", who);
    if (int rc = check_hierarchy(who, h, 1, nV)) return rc;
    if (int rc = check_mesh(who, V, nV, F, nF, true)) return rc;
    std::vector<int> known;
    const int nb = fluid_known_rows(nV, nF, F, known);
    if (nb >= nV) return fail(SMG_ERR_INVALID, "%s: no interior vertex: every vertex is on the boundary", who);
    if (int rc = check_params(who, *p)) return rc;
    if (p->viscosity > 0.0 && h->n_levels < 2) return fail(SMG_ERR_INVALID, "%s: viscosity = %g needs a hierarchy of at least two levels", who, p->viscosity);

    std::unique_ptr<smg_fluid> g(new smg_fluid());
    g->nV = nV; g->nF = nF; g->nb = nb; g->p = *p;
    if (int rc = g->open(who)) return rc;
    if (int rc = g->clone(who, h, 0)) return rc;
    if (p->viscosity > 0.0)
        if (int rc = g->clone(who, h, 1)) return rc;

    // the geometry of a step and the masses, then -L with its known rows: precomputed once
    DevBuf<double> dV;
    HIPCHK(dV.upload(std::vector<double>(V, V + (size_t)nV * 3)));
    if (int rc = upload_faces(F, nF, nV, g->F, g->m_ptr, g->m_idx)) return rc;
    HIPCHK(g->known.upload(known));
    HIPCHK(g->W.alloc((size_t)nF * 9));
    HIPCHK(g->nrm.alloc((size_t)nF * 3));
    HIPCHK(g->Af.alloc((size_t)nF));
    HIPCHK(g->m.alloc((size_t)nV));
    HIPCHK(g->msum.alloc(1));
    HIPCHK(g->part.alloc((size_t)fixed_sum_groups(std::max(nV, nF))));
    HIPCHK(launch_hodge_geometry(dV.p, g->F.p, nF, g->W.p, g->nrm.p, g->Af.p, g->stream));
    HIPCHK(launch_fluid_mass(nV, g->m_ptr.p, g->m_idx.p, g->Af.p, g->m.p, g->stream));
    HIPCHK(launch_fixed_sum(g->m.p, nV, g->part.p, g->msum.p, g->stream));
    g->m_host.resize((size_t)nV);
    HIPCHK(hipMemcpyAsync(g->m_host.data(), g->m.p, (size_t)nV * sizeof(double), hipMemcpyDeviceToHost, g->stream));
    if (int rc = cotan_system(F, nF, nV, dV.p, 0, 0.0, -1.0, g->stream, g->S, false)) return rc;   // synchronises: the masses have arrived
    for (double& x : g->S.L) x = -x;
    std::vector<int> rows;
    for (int v = 0; v < nV; v++)
        if (known[(size_t)v]) rows.push_back(v);
    if (int rc = smg_precompute(g->handle[0], nV, g->S.ptr.data(), g->S.col.data(), g->S.L.data(), rows.data(), (int)rows.size())) return rc;
    if (p->viscosity > 0.0) {
        HIPCHK(g->val.alloc(g->S.col.size()));
        if (int rc = viscous_system(g.get(), p->viscosity * p->dt, true)) return rc;
    }
    *out = g.release();
    return SMG_OK;
}

// the blocks of a k-column state; they grow with the largest k seen and are kept
int ensure_columns(smg_fluid* g, int k)
{
    const size_t n = (size_t)g->nV, nf = (size_t)g->nF, kk = (size_t)k;
    if (g->kcap >= kk) return SMG_OK;
    HIPCHK(hipStreamSynchronize(g->stream));
    for (auto& b : g->Wb) HIPCHK(b.alloc(n * kk));
    for (auto& b : g->psi) HIPCHK(b.alloc(n * kk));
    HIPCHK(g->R.alloc(n * kk));
    HIPCHK(g->rsq.alloc(n * kk));
    HIPCHK(g->rate.alloc(n * kk));
    HIPCHK(g->mw.alloc(n * kk));
    HIPCHK(g->ew.alloc(n * kk));
    HIPCHK(g->terms.alloc(nf * kk));
    HIPCHK(g->part.alloc((size_t)fixed_sum_groups((int)std::max(n * kk, nf))));
    HIPCHK(g->red.alloc(1 + 3 * kk));
    HIPCHK(g->dt.alloc(kk));
    HIPCHK(g->time.alloc(kk));
    HIPCHK(g->rmax.alloc(3 * kk));
    HIPCHK(g->mwsum.alloc(kk));
    const size_t n_known = (size_t)(g->nb > 0 ? g->nb : 1);
    HIPCHK(g->zero.alloc(n_known * kk));
    HIPCHK(hipMemsetAsync(g->zero.p, 0, n_known * kk * sizeof(double), g->stream));
    g->kcap = kk;
    return SMG_OK;
}

// sum m w per column of the block `w` into mwsum (closed meshes: the mean that the right-hand side removes)
int refresh_mean(smg_fluid* g, const double* w)
{
    if (g->nb > 0) return SMG_OK;
    const int n = g->nV;
    HIPCHK(launch_fluid_diag(n, g->k, g->m.p, w, n, g->mw.p, nullptr, g->stream));
    for (int c = 0; c < g->k; c++) HIPCHK(launch_fixed_sum(g->mw.p + (size_t)c * n, n, g->part.p, g->mwsum.p + c, g->stream));
    return SMG_OK;
}

int fill_dt(smg_fluid* g)
{
    if (g->k < 1) return SMG_OK;
    const std::vector<double> d((size_t)g->k, g->p.dt);
    HIPCHK(hipStreamSynchronize(g->stream));
    HIPCHK(hipMemcpy(g->dt.p, d.data(), d.size() * sizeof(double), hipMemcpyHostToDevice));
    return SMG_OK;
}

// one solve of (-L) psi = -m (w - wbar) for the block `w`, whose sums m w are in mwsum: psi[pc] afterwards.  *entries += the loop entries
int stream_solve(smg_fluid* g, const char* who, const double* w, const smg_solve_opts* opts, int step, int* entries)
{
    const int n = g->nV, k = g->k;
    hipStream_t st = g->stream;
    HIPCHK(launch_fluid_rhs(n, k, g->m.p, g->known.p, w, n, g->nb > 0 ? nullptr : g->mwsum.p, g->msum.p, g->R.p, n, g->rsq.p, st));
    HIPCHK(launch_fixed_sum(g->rsq.p, (int)((size_t)n * k), g->part.p, g->red.p, st));
    double ss = 0.0;
    HIPCHK(hipMemcpyAsync(&ss, g->red.p, sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (!std::isfinite(ss)) return fail(SMG_ERR_NONFINITE, "%s: the right-hand side is not finite (step %d)", who, step);
    const smg_solve_opts so = opts_or_default(opts, 1e-10 * std::sqrt(ss), 100);
    int e = 0;
    const int n_known = g->nb > 0 ? g->nb : 1;
    if (int rc = inner_solve(g->handle[0], g->pcg, g->R.p, n, g->zero.p, n_known, g->psi[g->pc].p, n, k, so, g->psi[1 - g->pc].p, n, &e)) return rc;
    g->pc = 1 - g->pc;
    if (entries) *entries += e;
    return SMG_OK;
}

int check_state(const char* who, const smg_fluid* g)
{
    if (!g) return fail(SMG_ERR_INVALID, "%s: null object", who);
    if (g->k < 1) return fail(SMG_ERR_INVALID, "%s: no state: call smg_fluid_set_vorticity first", who);
    return SMG_OK;
}

int set_vorticity_impl(smg_fluid* g, const double* w, int ld, int k, int memspace)
{
    const char* who = "smg_fluid_set_vorticity";
    if (!g || !w) return fail(SMG_ERR_INVALID, "%s: bad arguments", who);
    if (k < 1) return fail(SMG_ERR_INVALID, "%s: k = %d, at least one column is needed", who, k);
    if ((long long)g->nV * k > INT_MAX || 3LL * g->nF * k > INT_MAX)
        return fail(SMG_ERR_INVALID, "%s: k = %d columns of %d vertices and %d faces exceed the index range", who, k, g->nV, g->nF);
    if (bad_memspace(memspace)) return fail(SMG_ERR_INVALID, "%s: memspace must be SMG_HOST or SMG_DEVICE", who);
    if (ld < g->nV) return fail(SMG_ERR_INVALID, "%s: a leading dimension is too small", who);
    DeviceScope dsc(g->device);
    g->k = 0;
    if (int rc = ensure_columns(g, k)) return rc;
    const int n = g->nV;
    const size_t nk = (size_t)n * k, D = sizeof(double);
    hipStream_t st = g->stream;
    g->cur = 0; g->pc = 0; g->k = k;
    HIPCHK(copy_columns(g->Wb[0].p, n, w, ld, n, k, copy_in(memspace), st));
    HIPCHK(hipMemsetAsync(g->psi[0].p, 0, nk * D, st));
    HIPCHK(hipMemsetAsync(g->time.p, 0, (size_t)k * D, st));
    if (int rc = refresh_mean(g, g->Wb[0].p)) return rc;
    return fill_dt(g);
}

int step_impl(smg_fluid* g, int n_steps, const smg_solve_opts* opts, double* cfl_his, double* time, int* cycles, int* n_done)
{
    const char* who = "smg_fluid_step";
    if (n_done) *n_done = 0;
    if (int rc = check_state(who, g)) return rc;
    if (n_steps < 1) return fail(SMG_ERR_INVALID, "%s: n_steps = %d, at least 1 is needed", who, n_steps);
    DeviceScope dsc(g->device);
    const int n = g->nV, k = g->k, stages = g->p.stages;
    const size_t D = sizeof(double), hk = (size_t)n_steps * k;
    const bool adaptive = g->p.dt == 0.0, closed = g->nb == 0;
    hipStream_t st = g->stream;
    if (g->hcap < hk) {
        HIPCHK(hipStreamSynchronize(st));
        HIPCHK(g->his.alloc(2 * hk));
        g->hcap = hk;
    }
    double* h_cfl = g->his.p;
    double* h_time = g->his.p + hk;
    int done = 0, rc = SMG_OK;
    for (int t = 0; t < n_steps && rc == SMG_OK; t++) {
        const int t1 = (g->cur + 1) % 3, t2 = (g->cur + 2) % 3;
        const double* wn = g->Wb[g->cur].p;
        const double* in = wn;
        int res = g->cur, entries = 0;
        for (int s = 0; s < stages && rc == SMG_OK; s++) {
            const int o = s == 1 ? t2 : t1;
            double a, b;
            stage_pair(stages, s, &a, &b);
            if ((rc = stream_solve(g, who, in, opts, t, &entries))) break;
            const double* psi = g->psi[g->pc].p;
            if (s == 0 && adaptive) {
                HIPCHK(launch_fluid_advect(n, k, g->F.p, g->m_ptr.p, g->m_idx.p, g->m.p, psi, n, nullptr, n, nullptr, n, a, b, nullptr, g->p.theta, nullptr,
                                           n, g->rate.p, nullptr, true, st));
                for (int c = 0; c < k; c++) HIPCHK(launch_fixed_max(g->rate.p + (size_t)c * n, n, g->part.p, g->rmax.p + c, st));
                HIPCHK(launch_fluid_dt(0, k, stages, g->p.cfl, g->rmax.p, g->dt.p, nullptr, nullptr, nullptr, st));
            }
            HIPCHK(launch_fluid_advect(n, k, g->F.p, g->m_ptr.p, g->m_idx.p, g->m.p, psi, n, in, n, wn, n, a, b, g->dt.p, g->p.theta, g->Wb[o].p, n,
                                       g->rate.p, g->mw.p, false, st));
            for (int c = 0; c < k; c++) {
                HIPCHK(launch_fixed_max(g->rate.p + (size_t)c * n, n, g->part.p, g->rmax.p + (size_t)s * k + c, st));
                if (closed) HIPCHK(launch_fixed_sum(g->mw.p + (size_t)c * n, n, g->part.p, g->mwsum.p + c, st));
            }
            in = g->Wb[o].p;
            res = o;
        }
        if (rc == SMG_OK && g->p.viscosity > 0.0) {   // (M + viscosity dt (-L)) w_new = m w*: mw holds the right-hand side, w* is the start
            const int o = res == t1 ? t2 : t1;
            // the solve's right-hand side is mw = m w*, which the last stage wrote.  Only its norm is formed here, for the default tolerance and the
            // refusal: k_fluid_rhs without a mean and without known rows writes r = -(m w*) into R, which nothing reads, and rsq = (m w*)^2
            HIPCHK(launch_fluid_rhs(n, k, g->m.p, nullptr, g->Wb[res].p, n, nullptr, g->msum.p, g->R.p, n, g->rsq.p, st));
            HIPCHK(launch_fixed_sum(g->rsq.p, (int)((size_t)n * k), g->part.p, g->red.p, st));
            double ss = 0.0;
            HIPCHK(hipMemcpyAsync(&ss, g->red.p, D, hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
            if (!std::isfinite(ss)) {
                rc = fail(SMG_ERR_NONFINITE, "%s: the right-hand side is not finite (step %d)", who, t);
            } else {
                const smg_solve_opts so = opts_or_default(opts, 1e-10 * std::sqrt(ss), 100);
                int e = 0;
                rc = inner_solve(g->handle[1], g->pcg, g->mw.p, n, nullptr, 0, g->Wb[res].p, n, k, so, g->Wb[o].p, n, &e);
                entries += e;
                res = o;
                if (rc == SMG_OK) rc = refresh_mean(g, g->Wb[res].p);
            }
        }
        if (rc != SMG_OK) break;
        HIPCHK(launch_fluid_dt(1, k, stages, g->p.cfl, g->rmax.p, g->dt.p, g->time.p, h_cfl + (size_t)t * k, h_time + (size_t)t * k, st));
        g->cur = res;
        if (cycles) cycles[t] = entries;
        done = t + 1;
    }
    if (rc != SMG_OK) {   // the state of the last completed step stands; its sums m w are formed again, psi restarts from zero
        const int keep = rc;
        HIPCHK(hipMemsetAsync(g->psi[g->pc].p, 0, (size_t)n * k * D, st));
        if (int r2 = refresh_mean(g, g->Wb[g->cur].p)) return r2;
        rc = keep;
    }
    if (done > 0) {
        if (cfl_his) HIPCHK(hipMemcpyAsync(cfl_his, h_cfl, (size_t)done * k * D, hipMemcpyDeviceToHost, st));
        if (time) HIPCHK(hipMemcpyAsync(time, h_time, (size_t)done * k * D, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(hipStreamSynchronize(st));
    if (n_done) *n_done = done;
    return rc;
}

int vorticity_impl(smg_fluid* g, double* w, int ld, int memspace)
{
    const char* who = "smg_fluid_vorticity";
    if (int rc = check_state(who, g)) return rc;
    if (!w) return fail(SMG_ERR_INVALID, "%s: bad arguments", who);
    if (bad_memspace(memspace)) return fail(SMG_ERR_INVALID, "%s: memspace must be SMG_HOST or SMG_DEVICE", who);
    if (ld < g->nV) return fail(SMG_ERR_INVALID, "%s: a leading dimension is too small", who);
    DeviceScope dsc(g->device);
    HIPCHK(copy_columns(w, ld, g->Wb[g->cur].p, g->nV, g->nV, g->k, copy_out(memspace), g->stream));
    HIPCHK(hipStreamSynchronize(g->stream));
    return SMG_OK;
}

int stream_impl(smg_fluid* g, const smg_solve_opts* opts, double* psi, int ld, int memspace)
{
    const char* who = "smg_fluid_stream";
    if (int rc = check_state(who, g)) return rc;
    if (!psi) return fail(SMG_ERR_INVALID, "%s: bad arguments", who);
    if (bad_memspace(memspace)) return fail(SMG_ERR_INVALID, "%s: memspace must be SMG_HOST or SMG_DEVICE", who);
    if (ld < g->nV) return fail(SMG_ERR_INVALID, "%s: a leading dimension is too small", who);
    DeviceScope dsc(g->device);
    if (int rc = stream_solve(g, who, g->Wb[g->cur].p, opts, 0, nullptr)) return rc;
    HIPCHK(copy_columns(psi, ld, g->psi[g->pc].p, g->nV, g->nV, g->k, copy_out(memspace), g->stream));
    HIPCHK(hipStreamSynchronize(g->stream));
    return SMG_OK;
}

int velocity_impl(smg_fluid* g, const smg_solve_opts* opts, double* U, int memspace)
{
    const char* who = "smg_fluid_velocity";
    if (int rc = check_state(who, g)) return rc;
    if (!U) return fail(SMG_ERR_INVALID, "%s: bad arguments", who);
    if (bad_memspace(memspace)) return fail(SMG_ERR_INVALID, "%s: memspace must be SMG_HOST or SMG_DEVICE", who);
    DeviceScope dsc(g->device);
    const size_t count = 3 * (size_t)g->nF * g->k;
    hipStream_t st = g->stream;
    if (int rc = stream_solve(g, who, g->Wb[g->cur].p, opts, 0, nullptr)) return rc;
    double* dU = U;
    if (memspace == SMG_HOST) {
        HIPCHK(g->Us.ensure(count));
        dU = g->Us.p;
    }
    HIPCHK(launch_fluid_velocity(g->nF, g->k, g->F.p, g->W.p, g->nrm.p, g->Af.p, g->psi[g->pc].p, g->nV, dU, g->terms.p, st));
    if (memspace == SMG_HOST) HIPCHK(hipMemcpyAsync(U, dU, count * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return SMG_OK;
}

int diagnostics_impl(smg_fluid* g, const smg_solve_opts* opts, double* out)
{
    const char* who = "smg_fluid_diagnostics";
    if (int rc = check_state(who, g)) return rc;
    if (!out) return fail(SMG_ERR_INVALID, "%s: bad arguments", who);
    DeviceScope dsc(g->device);
    const int n = g->nV, nF = g->nF, k = g->k;
    hipStream_t st = g->stream;
    if (int rc = stream_solve(g, who, g->Wb[g->cur].p, opts, 0, nullptr)) return rc;
    HIPCHK(launch_fluid_velocity(nF, k, g->F.p, g->W.p, g->nrm.p, g->Af.p, g->psi[g->pc].p, n, nullptr, g->terms.p, st));
    HIPCHK(launch_fluid_diag(n, k, g->m.p, g->Wb[g->cur].p, n, g->mw.p, g->ew.p, st));
    double* d = g->red.p + 1;
    for (int c = 0; c < k; c++) {
        HIPCHK(launch_fixed_sum(g->mw.p + (size_t)c * n, n, g->part.p, d + c, st));
        HIPCHK(launch_fixed_sum(g->ew.p + (size_t)c * n, n, g->part.p, d + k + c, st));
        HIPCHK(launch_fixed_sum(g->terms.p + (size_t)c * nF, nF, g->part.p, d + 2 * (size_t)k + c, st));
    }
    double msum = 0.0;
    HIPCHK(hipMemcpyAsync(out, d, 3 * (size_t)k * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(&msum, g->msum.p, sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    for (int c = 0; c < k; c++) out[3 * (size_t)k + c] = g->nb > 0 ? 0.0 : out[c] / msum;
    return SMG_OK;
}

int set_params_impl(smg_fluid* g, const smg_fluid_params* p)
{
    const char* who = "smg_fluid_set_params";
    if (!g || !p) return fail(SMG_ERR_INVALID, "%s: bad arguments", who);
    if (int rc = check_params(who, *p)) return rc;
    if ((p->viscosity > 0.0) != (g->p.viscosity > 0.0))
        return fail(SMG_ERR_INVALID, "%s: viscosity = %g, but the object was created with viscosity = %g: zero and non-zero cannot change", who, p->viscosity,
                    g->p.viscosity);
    DeviceScope dsc(g->device);
    if (p->viscosity > 0.0 && p->viscosity * p->dt != g->vdt)
        if (int rc = viscous_system(g, p->viscosity * p->dt, false)) return rc;
    g->p = *p;
    return fill_dt(g);
}

}  // namespace

extern "C" smg_fluid_params smg_fluid_params_default(void)
{
    smg_fluid_params p;
    p.theta = 0.0; p.stages = 3; p.viscosity = 0.0; p.dt = 0.0; p.cfl = 0.5;
    return p;
}

extern "C" int smg_fluid_create(const smg_hierarchy* h, const double* V, int nV, const int* F, int nF, const smg_fluid_params* p, smg_fluid** out)
{
    return guarded("smg_fluid_create", [&]() { return create_impl(h, V, nV, F, nF, p, out); });
}

extern "C" void smg_fluid_destroy(smg_fluid* g) { delete g; }

extern "C" int smg_fluid_set_params(smg_fluid* g, const smg_fluid_params* p)
{
    return guarded("smg_fluid_set_params", [&]() { return set_params_impl(g, p); });
}

extern "C" int smg_fluid_set_solver(smg_fluid* g, int pcg)
{
    if (!g) return fail(SMG_ERR_INVALID, "smg_fluid_set_solver: null object");
    latch_solver(g->pcg, pcg);
    return SMG_OK;
}

extern "C" int smg_fluid_is_closed(const smg_fluid* g) { return g && g->nb == 0 ? 1 : 0; }

extern "C" long long smg_fluid_device_bytes(const smg_fluid* g)
{
    if (!g) return 0;   // one list: every DevBuf of the struct
    return device_bytes(*g, g->F, g->m_ptr, g->m_idx, g->known, g->W, g->nrm, g->Af, g->m, g->msum, g->val, g->Wb[0], g->Wb[1], g->Wb[2], g->psi[0],
                        g->psi[1], g->R, g->rsq, g->rate, g->mw, g->ew, g->terms, g->Us, g->part, g->red, g->dt, g->time, g->rmax, g->mwsum, g->his,
                        g->zero);
}

extern "C" int smg_fluid_set_vorticity(smg_fluid* g, const double* w, int ld, int k, int memspace)
{
    return guarded("smg_fluid_set_vorticity", [&]() { return set_vorticity_impl(g, w, ld, k, memspace); });
}

extern "C" int smg_fluid_vorticity(smg_fluid* g, double* w, int ld, int memspace)
{
    return guarded("smg_fluid_vorticity", [&]() { return vorticity_impl(g, w, ld, memspace); });
}

extern "C" int smg_fluid_step(smg_fluid* g, int n_steps, const smg_solve_opts* opts, double* cfl_his, double* time, int* cycles, int* n_done)
{
    return guarded("smg_fluid_step", [&]() { return step_impl(g, n_steps, opts, cfl_his, time, cycles, n_done); });
}

extern "C" int smg_fluid_stream(smg_fluid* g, const smg_solve_opts* opts, double* psi, int ld, int memspace)
{
    return guarded("smg_fluid_stream", [&]() { return stream_impl(g, opts, psi, ld, memspace); });
}

extern "C" int smg_fluid_velocity(smg_fluid* g, const smg_solve_opts* opts, double* U, int memspace)
{
    return guarded("smg_fluid_velocity", [&]() { return velocity_impl(g, opts, U, memspace); });
}

extern "C" int smg_fluid_diagnostics(smg_fluid* g, const smg_solve_opts* opts, double* out)
{
    return guarded("smg_fluid_diagnostics", [&]() { return diagnostics_impl(g, opts, out); });
}

extern "C" int smg_fluid_host(int op, int nV, int nF, int k, const int* F, const double* V, const double* w, const double* psi, const double* wn, double a,
                              double b, const double* dt, double theta, int rates_only, double* out)
{
    return guarded("smg_fluid_host", [&]() -> int {
        const char* who = "smg_fluid_host";
        if (int rc = fluid_check_operands(who, op, nV, nF, k, F, V, w, psi, wn, dt, theta, rates_only, out)) return rc;
        const size_t n = (size_t)nV, f = (size_t)nF, kk = (size_t)k, nk = n * kk, fk = f * kk;
        if (op == SMG_FLUID_DT) {
            fluid_host_dt(k, 3, a, w, psi, out, out + kk, out + 2 * kk);
            return SMG_OK;
        }
        std::vector<int> mp, mi, known;
        vertex_corner_lists(std::vector<int>(F, F + 3 * f), nV, mp, mi);
        const int nb = fluid_known_rows(nV, nF, F, known);
        std::vector<double> A(f), m(n);
        fluid_host_mass(nV, nF, F, V, mp.data(), mi.data(), A.data(), m.data());
        switch (op) {
            case SMG_FLUID_RHS: {
                double *msum = out + n, *mw = out + n + 1, *mwsum = mw + nk, *R = mwsum + kk, *rsq = R + nk;
                std::copy(m.begin(), m.end(), out);
                *msum = flow_host_sum(m.data(), nV);
                std::vector<double> ew(nk);
                fluid_host_diag(nV, k, m.data(), w, mw, ew.data());
                for (int c = 0; c < k; c++) mwsum[c] = flow_host_sum(mw + (size_t)c * n, nV);
                fluid_host_rhs(nV, k, m.data(), known.data(), w, nb > 0 ? nullptr : mwsum, *msum, R, rsq);
                rsq[nk] = flow_host_sum(rsq, (int)nk);
                break;
            }
            case SMG_FLUID_ADVECT:
                if (rates_only) {
                    fluid_host_advect(nV, k, F, mp.data(), mi.data(), m.data(), psi, nullptr, nullptr, a, b, nullptr, theta, nullptr, out, nullptr);
                    for (int c = 0; c < k; c++) out[nk + c] = flow_host_max(out + (size_t)c * n, nV);
                } else {
                    double *rate = out + nk, *mw = out + 2 * nk;
                    fluid_host_advect(nV, k, F, mp.data(), mi.data(), m.data(), psi, w, wn, a, b, dt, theta, out, rate, mw);
                    for (int c = 0; c < k; c++) {
                        out[3 * nk + c] = flow_host_max(rate + (size_t)c * n, nV);
                        out[3 * nk + kk + c] = flow_host_sum(mw + (size_t)c * n, nV);
                    }
                }
                break;
            case SMG_FLUID_VELOCITY:
                fluid_host_velocity(nV, nF, k, F, V, psi, out, out + 3 * fk);
                for (int c = 0; c < k; c++) out[4 * fk + c] = flow_host_sum(out + 3 * fk + (size_t)c * f, nF);
                break;
            default:
                fluid_host_diag(nV, k, m.data(), w, out, out + nk);
                for (int c = 0; c < k; c++) {
                    out[2 * nk + c] = flow_host_sum(out + (size_t)c * n, nV);
                    out[2 * nk + kk + c] = flow_host_sum(out + nk + (size_t)c * n, nV);
                }
                break;
        }
        return SMG_OK;
    });
}
