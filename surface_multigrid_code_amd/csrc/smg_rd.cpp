// smg_rd.cpp -- two-species reaction-diffusion on a surface (include/smg.h: smg_rd_*): per column c
// u_t = Du Laplace u + R_u(u, v; c), v_t = Dv Laplace v + R_v(u, v; c), R_u and R_v bivariate cubics with a coefficient table per column, the
// reaction explicit and the diffusion implicit.  The object owns the handles built from the caller's prolongations -- handle[0]: M + dt Du (-L);
// handle[1] (Du != Dv, Dv > 0 only): M + dt Dv (-L); no known rows -- the masses, the coefficient table and the state: a column-major nV x 2k
// block, u in columns [0, k), v in [k, 2k), so that with Du == Dv a step is ONE 2k-column solve.  A step is the vertex kernel of the reaction
// (the right-hand sides and their squares), the solves warm-started from the state, and the closing kernel with the fixed-order reductions of
// its terms, all enqueued on the object's stream, which the handles use too.  The host reads two doubles before the solves, |m u*|^2 and
// |m v*|^2 -- they set the default tolerances and refuse non-finite input -- and 3k after them: the sums m u', m v' and the changes.  A step
// writes into the block beside the state and commits by an index swap, so a refused step leaves the state of the last completed one.  Checks,
// stream, handles, the cotangent system and the inner solve: smg_mesh_object.hpp.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <memory>
#include <vector>

#include "smg_device.hpp"
#include "smg_mesh.hpp"
#include "smg_mesh_object.hpp"
#include "smg_rd_inl.hpp"

using namespace smg;

namespace {

enum { RD_TWO = 0, RD_ONE = 1, RD_UONLY = 2 };   // two k-column solves | one 2k-column solve | v' = v*, one k-column solve

int rd_case(const smg_rd_params& p) { return p.Dv == 0.0 ? RD_UONLY : p.Du == p.Dv ? RD_ONE : RD_TWO; }

}  // namespace

struct smg_rd : MeshObject {               // handle[0]: M + dt Du (-L); handle[1] (RD_TWO): M + dt Dv (-L)
    int nV = 0, nF = 0;
    int pcg = 1;                           // the inner solver: 1 smg_solve_pcg, 0 smg_solve
    smg_rd_params p;
    double sys[2] = {0.0, 0.0};            // the dt D that each handle holds
    size_t kcap = 0;                       // the columns the state's blocks hold
    int k = 0, cur = 0;                    // the state's columns (0: none); which of S[2] holds the state
    CotanSystem Sys;                       // the pattern and -L's values
    std::vector<double> m_host, red_host;
    DevBuf<double> m, val;                 // the masses; a system's values on their way to a handle
    DevBuf<double> S[2], R;                // column-major n x 2k: the state and the step's output; the right-hand sides
    DevBuf<double> rsq, mt, chg;           // planes of n: 2k squares, 2k mass terms, k changes
    DevBuf<double> coef, part, red;        // k x 20; the chunk sums; |m u*|^2, |m v*|^2, then 2k sums and k maxima
    ~smg_rd() { quiesce(); }
};

namespace smg {

int rd_check_operands(const char* who, int op, int nV, int nF, int k, const int* F, const double* V, const double* u, const double* v, const double* coeff,
                      double dt, int substeps, const double* un, const double* vn, const double* out)
{
    if (op < SMG_RD_REACT || op > SMG_RD_CLOSE || nV < 1 || nF < 1 || !F || !V || !out) return fail(SMG_ERR_INVALID, "%s: bad arguments", who);
    if (!u || !v || (op == SMG_RD_REACT && !coeff) || (op == SMG_RD_CLOSE && (!un || !vn)))
        return fail(SMG_ERR_INVALID, "%s: op %d misses an operand", who, op);
    if (k < 1) return fail(SMG_ERR_INVALID, "%s: k = %d, at least one column is needed", who, k);
    if (op == SMG_RD_REACT) {
        if (substeps < 1) return fail(SMG_ERR_INVALID, "%s: substeps = %d, at least 1 is needed", who, substeps);
        if (!std::isfinite(dt) || !(dt > 0.0)) return fail(SMG_ERR_INVALID, "%s: dt = %g, a finite value > 0 is needed", who, dt);
        for (size_t j = 0; j < (size_t)k * RD_COEFFS; j++)
            if (!std::isfinite(coeff[j]))
                return fail(SMG_ERR_INVALID, "%s: coefficient %d of column %d is not finite", who, (int)(j % RD_COEFFS), (int)(j / RD_COEFFS));
    }
    return check_faces(who, F, nF, nV);
}

}  // namespace smg

namespace {

int check_params(const char* who, const smg_rd_params& p)
{
    if (!std::isfinite(p.Du) || !(p.Du > 0.0)) return fail(SMG_ERR_INVALID, "%s: Du = %g, a finite value > 0 is needed", who, p.Du);
    if (!std::isfinite(p.Dv) || p.Dv < 0.0) return fail(SMG_ERR_INVALID, "%s: Dv = %g, a finite value >= 0 is needed", who, p.Dv);
    if (!std::isfinite(p.dt) || !(p.dt > 0.0)) return fail(SMG_ERR_INVALID, "%s: dt = %g, a finite value > 0 is needed", who, p.dt);
    if (p.react_substeps < 1) return fail(SMG_ERR_INVALID, "%s: react_substeps = %d, at least 1 is needed", who, p.react_substeps);
    if (!(p.stop_change >= 0.0)) return fail(SMG_ERR_INVALID, "%s: stop_change = %g, a value >= 0 is needed", who, p.stop_change);
    return SMG_OK;
}

// handle[slot]'s values M + c (-L) from the kept pattern, c = dt D; first: the pattern-setting precompute, else by values
int rd_system(smg_rd* g, int slot, double c, bool first)
{
    const size_t nnz = g->Sys.col.size();
    std::vector<double> val(nnz);
    for (int i = 0; i < g->nV; i++)
        for (int q = g->Sys.ptr[(size_t)i]; q < g->Sys.ptr[(size_t)i + 1]; q++) {
            const double x = c * g->Sys.L[(size_t)q];
            val[(size_t)q] = g->Sys.col[(size_t)q] == i ? g->m_host[(size_t)i] + x : x;
        }
    if (first) {
        if (int rc = smg_precompute(g->handle[slot], g->nV, g->Sys.ptr.data(), g->Sys.col.data(), val.data(), nullptr, 0)) return rc;
    } else {
        HIPCHK(hipStreamSynchronize(g->stream));
        HIPCHK(hipMemcpy(g->val.p, val.data(), nnz * sizeof(double), hipMemcpyHostToDevice));
        if (int rc = smg_precompute_values_device(g->handle[slot], g->val.p)) return rc;
    }
    g->sys[slot] = c;
    return SMG_OK;
}

int create_impl(const smg_hierarchy* h, const double* V, int nV, const int* F, int nF, const smg_rd_params* p, smg_rd** out)
{
    if (out) *out = nullptr;
    const char* who = "smg_rd_create";
    if (!h || !V || !F || !p || !out || nV <= 0 || nF <= 0) return fail(SMG_ERR_INVALID, "%s: bad arguments", who);
    if (int rc = check_hierarchy(who, h, 1, nV)) return rc;
    if (h->n_levels < 2) return fail(SMG_ERR_INVALID, "%s: a hierarchy of at least two levels is needed", who);
    if (int rc = check_mesh(who, V, nV, F, nF, true)) return rc;
    if (int rc = check_params(who, *p)) return rc;

    std::unique_ptr<smg_rd> g(new smg_rd());
    g->nV = nV; g->nF = nF; g->p = *p;
    if (int rc = g->open(who)) return rc;
    if (int rc = g->clone(who, h, 0)) return rc;
    if (rd_case(*p) == RD_TWO)
        if (int rc = g->clone(who, h, 1)) return rc;

    // the masses and -L, then the constant matrices: precomputed once.  The geometry is read here alone
    DevBuf<double> dV, W, nrm, Af;
    DevBuf<int> dF, m_ptr, m_idx;
    HIPCHK(dV.upload(std::vector<double>(V, V + (size_t)nV * 3)));
    if (int rc = upload_faces(F, nF, nV, dF, m_ptr, m_idx)) return rc;
    HIPCHK(W.alloc((size_t)nF * 9));
    HIPCHK(nrm.alloc((size_t)nF * 3));
    HIPCHK(Af.alloc((size_t)nF));
    HIPCHK(g->m.alloc((size_t)nV));
    HIPCHK(launch_hodge_geometry(dV.p, dF.p, nF, W.p, nrm.p, Af.p, g->stream));
    HIPCHK(launch_fluid_mass(nV, m_ptr.p, m_idx.p, Af.p, g->m.p, g->stream));
    g->m_host.resize((size_t)nV);
    HIPCHK(hipMemcpyAsync(g->m_host.data(), g->m.p, (size_t)nV * sizeof(double), hipMemcpyDeviceToHost, g->stream));
    if (int rc = cotan_system(F, nF, nV, dV.p, 0, 0.0, -1.0, g->stream, g->Sys, false)) return rc;   // synchronises: the masses have arrived
    for (double& x : g->Sys.L) x = -x;
    HIPCHK(g->val.alloc(g->Sys.col.size()));
    if (int rc = rd_system(g.get(), 0, p->dt * p->Du, true)) return rc;
    if (rd_case(*p) == RD_TWO)
        if (int rc = rd_system(g.get(), 1, p->dt * p->Dv, true)) return rc;
    *out = g.release();
    return SMG_OK;
}

// the blocks of a k-column state; they grow with the largest k seen and are kept
int ensure_columns(smg_rd* g, int k)
{
    const size_t n = (size_t)g->nV, kk = (size_t)k;
    if (g->kcap >= kk) return SMG_OK;
    HIPCHK(hipStreamSynchronize(g->stream));
    for (auto& b : g->S) HIPCHK(b.alloc(2 * n * kk));
    HIPCHK(g->R.alloc(2 * n * kk));
    HIPCHK(g->rsq.alloc(2 * n * kk));
    HIPCHK(g->mt.alloc(2 * n * kk));
    HIPCHK(g->chg.alloc(n * kk));
    HIPCHK(g->coef.alloc(kk * RD_COEFFS));
    HIPCHK(g->part.alloc((size_t)fixed_sum_groups((int)(n * kk))));
    HIPCHK(g->red.alloc(2 + 3 * kk));
    g->kcap = kk;
    return SMG_OK;
}

int check_state(const char* who, const smg_rd* g)
{
    if (!g) return fail(SMG_ERR_INVALID, "%s: null object", who);
    if (g->k < 1) return fail(SMG_ERR_INVALID, "%s: no state: call smg_rd_set_state first", who);
    return SMG_OK;
}

int set_state_impl(smg_rd* g, const double* u, const double* v, int ld, int k, const double* coeff, int memspace)
{
    const char* who = "smg_rd_set_state";
    if (!g || !u || !v || !coeff) return fail(SMG_ERR_INVALID, "%s: bad arguments", who);
    if (k < 1) return fail(SMG_ERR_INVALID, "%s: k = %d, at least one column is needed", who, k);
    if (2LL * g->nV * k > INT_MAX) return fail(SMG_ERR_INVALID, "%s: k = %d columns of %d vertices exceed the index range", who, k, g->nV);
    if (bad_memspace(memspace)) return fail(SMG_ERR_INVALID, "%s: memspace must be SMG_HOST or SMG_DEVICE", who);
    if (ld < g->nV) return fail(SMG_ERR_INVALID, "%s: a leading dimension is too small", who);
    for (size_t j = 0; j < (size_t)k * RD_COEFFS; j++)
        if (!std::isfinite(coeff[j]))
            return fail(SMG_ERR_INVALID, "%s: coefficient %d of column %d is not finite", who, (int)(j % RD_COEFFS), (int)(j / RD_COEFFS));
    DeviceScope dsc(g->device);
    g->k = 0;
    if (int rc = ensure_columns(g, k)) return rc;
    const int n = g->nV;
    const size_t nk = (size_t)n * k;
    hipStream_t st = g->stream;
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipMemcpy(g->coef.p, coeff, (size_t)k * RD_COEFFS * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(copy_columns(g->S[0].p, n, u, ld, n, k, copy_in(memspace), st));
    HIPCHK(copy_columns(g->S[0].p + nk, n, v, ld, n, k, copy_in(memspace), st));
    HIPCHK(hipStreamSynchronize(st));
    g->cur = 0; g->k = k;
    return SMG_OK;
}

int state_impl(smg_rd* g, double* u, double* v, int ld, int memspace)
{
    const char* who = "smg_rd_state";
    if (int rc = check_state(who, g)) return rc;
    if (!u || !v) return fail(SMG_ERR_INVALID, "%s: bad arguments", who);
    if (bad_memspace(memspace)) return fail(SMG_ERR_INVALID, "%s: memspace must be SMG_HOST or SMG_DEVICE", who);
    if (ld < g->nV) return fail(SMG_ERR_INVALID, "%s: a leading dimension is too small", who);
    DeviceScope dsc(g->device);
    const int n = g->nV;
    const double* s = g->S[g->cur].p;
    HIPCHK(copy_columns(u, ld, s, n, n, g->k, copy_out(memspace), g->stream));
    HIPCHK(copy_columns(v, ld, s + (size_t)n * g->k, n, n, g->k, copy_out(memspace), g->stream));
    HIPCHK(hipStreamSynchronize(g->stream));
    return SMG_OK;
}

int step_impl(smg_rd* g, int n_steps, const smg_solve_opts* opts, double* mass_his, double* change_his, int* cycles, int* n_done)
{
    const char* who = "smg_rd_step";
    if (n_done) *n_done = 0;
    if (int rc = check_state(who, g)) return rc;
    if (n_steps < 1) return fail(SMG_ERR_INVALID, "%s: n_steps = %d, at least 1 is needed", who, n_steps);
    DeviceScope dsc(g->device);
    const int n = g->nV, k = g->k, mode = rd_case(g->p);
    const size_t nk = (size_t)n * k, D = sizeof(double);
    const double h = g->p.dt / g->p.react_substeps;
    hipStream_t st = g->stream;
    g->red_host.assign(2 + 3 * (size_t)k, 0.0);
    double* rh = g->red_host.data();
    for (int t = 0; t < n_steps; t++) {
        const double* s0 = g->S[g->cur].p;
        double* s1 = g->S[1 - g->cur].p;
        double* R = g->R.p;
        HIPCHK(launch_rd_react(n, k, g->m.p, s0, s0 + nk, n, g->coef.p, h, g->p.react_substeps, R, R + nk, n, g->rsq.p, mode == RD_UONLY ? s1 + nk : nullptr, n,
                               st));
        HIPCHK(launch_fixed_sum(g->rsq.p, (int)nk, g->part.p, g->red.p, st));
        HIPCHK(launch_fixed_sum(g->rsq.p + nk, (int)nk, g->part.p, g->red.p + 1, st));
        HIPCHK(hipMemcpyAsync(rh, g->red.p, 2 * D, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        if (!std::isfinite(rh[0]) || !std::isfinite(rh[1])) return fail(SMG_ERR_NONFINITE, "%s: the right-hand side is not finite (step %d)", who, t);
        int e0 = 0, e1 = 0;
        if (mode == RD_ONE) {
            const smg_solve_opts so = opts_or_default(opts, 1e-10 * std::sqrt(rh[0] + rh[1]), 100);
            if (int rc = inner_solve(g->handle[0], g->pcg, R, n, nullptr, 0, s0, n, 2 * k, so, s1, n, &e0)) return rc;
        } else {
            const smg_solve_opts su = opts_or_default(opts, 1e-10 * std::sqrt(rh[0]), 100);
            if (int rc = inner_solve(g->handle[0], g->pcg, R, n, nullptr, 0, s0, n, k, su, s1, n, &e0)) return rc;
            if (mode == RD_TWO) {
                const smg_solve_opts sv = opts_or_default(opts, 1e-10 * std::sqrt(rh[1]), 100);
                if (int rc = inner_solve(g->handle[1], g->pcg, R + nk, n, nullptr, 0, s0 + nk, n, k, sv, s1 + nk, n, &e1)) return rc;
            }
        }
        HIPCHK(launch_rd_close(n, k, g->m.p, s0, s0 + nk, s1, s1 + nk, n, g->mt.p, g->chg.p, st));
        double* d = g->red.p + 2;
        for (int c = 0; c < 2 * k; c++) HIPCHK(launch_fixed_sum(g->mt.p + (size_t)c * n, n, g->part.p, d + c, st));
        for (int c = 0; c < k; c++) HIPCHK(launch_fixed_max(g->chg.p + (size_t)c * n, n, g->part.p, d + 2 * (size_t)k + c, st));
        HIPCHK(hipMemcpyAsync(rh + 2, d, 3 * (size_t)k * D, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        g->cur = 1 - g->cur;
        if (mass_his) std::copy(rh + 2, rh + 2 + 2 * (size_t)k, mass_his + (size_t)t * 2 * k);
        if (change_his) std::copy(rh + 2 + 2 * (size_t)k, rh + 2 + 3 * (size_t)k, change_his + (size_t)t * k);
        if (cycles) { cycles[2 * (size_t)t] = e0; cycles[2 * (size_t)t + 1] = e1; }
        if (n_done) *n_done = t + 1;
        if (g->p.stop_change > 0.0) {
            bool still = true;
            for (int c = 0; c < k; c++) still = still && rh[2 + 2 * (size_t)k + c] <= g->p.stop_change;
            if (still) break;
        }
    }
    return SMG_OK;
}

int set_params_impl(smg_rd* g, const smg_rd_params* p)
{
    const char* who = "smg_rd_set_params";
    if (!g || !p) return fail(SMG_ERR_INVALID, "%s: bad arguments", who);
    if (int rc = check_params(who, *p)) return rc;
    if (rd_case(*p) != rd_case(g->p))
        return fail(SMG_ERR_INVALID, "%s: Du = %g, Dv = %g, but the object was created with Du = %g, Dv = %g: the handles in use cannot change", who, p->Du,
                    p->Dv, g->p.Du, g->p.Dv);
    DeviceScope dsc(g->device);
    if (p->dt * p->Du != g->sys[0])
        if (int rc = rd_system(g, 0, p->dt * p->Du, false)) return rc;
    if (rd_case(*p) == RD_TWO && p->dt * p->Dv != g->sys[1])
        if (int rc = rd_system(g, 1, p->dt * p->Dv, false)) return rc;
    g->p = *p;
    return SMG_OK;
}

}  // namespace

extern "C" smg_rd_params smg_rd_params_default(void)
{
    smg_rd_params p;
    p.Du = 1.0; p.Dv = 1.0; p.dt = 1.0; p.react_substeps = 1; p.stop_change = 0.0;
    return p;
}

extern "C" int smg_rd_create(const smg_hierarchy* h, const double* V, int nV, const int* F, int nF, const smg_rd_params* p, smg_rd** out)
{
    return guarded("smg_rd_create", [&]() { return create_impl(h, V, nV, F, nF, p, out); });
}

extern "C" void smg_rd_destroy(smg_rd* g) { delete g; }

extern "C" int smg_rd_set_params(smg_rd* g, const smg_rd_params* p)
{
    return guarded("smg_rd_set_params", [&]() { return set_params_impl(g, p); });
}

extern "C" int smg_rd_set_solver(smg_rd* g, int pcg)
{
    if (!g) return fail(SMG_ERR_INVALID, "smg_rd_set_solver: null object");
    latch_solver(g->pcg, pcg);
    return SMG_OK;
}

extern "C" long long smg_rd_device_bytes(const smg_rd* g)
{
    if (!g) return 0;   // one list: every DevBuf of the struct
    return device_bytes(*g, g->m, g->val, g->S[0], g->S[1], g->R, g->rsq, g->mt, g->chg, g->coef, g->part, g->red);
}

extern "C" int smg_rd_set_state(smg_rd* g, const double* u, const double* v, int ld, int k, const double* coeff, int memspace)
{
    return guarded("smg_rd_set_state", [&]() { return set_state_impl(g, u, v, ld, k, coeff, memspace); });
}

extern "C" int smg_rd_state(smg_rd* g, double* u, double* v, int ld, int memspace)
{
    return guarded("smg_rd_state", [&]() { return state_impl(g, u, v, ld, memspace); });
}

extern "C" int smg_rd_step(smg_rd* g, int n_steps, const smg_solve_opts* opts, double* mass_his, double* change_his, int* cycles, int* n_done)
{
    return guarded("smg_rd_step", [&]() { return step_impl(g, n_steps, opts, mass_his, change_his, cycles, n_done); });
}

extern "C" int smg_rd_host(int op, int nV, int nF, int k, const int* F, const double* V, const double* u, const double* v, const double* coeff, double dt,
                           int substeps, const double* un, const double* vn, double* out)
{
    return guarded("smg_rd_host", [&]() -> int {
        const char* who = "smg_rd_host";
        if (int rc = rd_check_operands(who, op, nV, nF, k, F, V, u, v, coeff, dt, substeps, un, vn, out)) return rc;
        const size_t n = (size_t)nV, f = (size_t)nF, kk = (size_t)k, nk = n * kk;
        std::vector<int> mp, mi;
        vertex_corner_lists(std::vector<int>(F, F + 3 * f), nV, mp, mi);
        std::vector<double> A(f), m(n), S0(2 * nk);
        fluid_host_mass(nV, nF, F, V, mp.data(), mi.data(), A.data(), m.data());
        std::copy(u, u + nk, S0.begin());
        std::copy(v, v + nk, S0.begin() + (std::ptrdiff_t)nk);
        if (op == SMG_RD_REACT) {
            double* rsq = out + 2 * nk;
            rd_host_react(nV, k, m.data(), S0.data(), coeff, dt / substeps, substeps, out, rsq, out + 4 * nk);
            out[5 * nk] = flow_host_sum(rsq, (int)nk);
            out[5 * nk + 1] = flow_host_sum(rsq + nk, (int)nk);
        } else {
            std::vector<double> S1(2 * nk);
            std::copy(un, un + nk, S1.begin());
            std::copy(vn, vn + nk, S1.begin() + (std::ptrdiff_t)nk);
            double* chg = out + 2 * nk;
            rd_host_close(nV, k, m.data(), S0.data(), S1.data(), out, chg);
            for (size_t c = 0; c < 2 * kk; c++) out[3 * nk + c] = flow_host_sum(out + c * n, nV);
            for (size_t c = 0; c < kk; c++) out[3 * nk + 2 * kk + c] = flow_host_max(chg + c * n, nV);
        }
        return SMG_OK;
    });
}
