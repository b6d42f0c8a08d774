// smg_wave.cpp -- the wave equation on a surface with shots and receivers (include/smg.h: smg_wave_*): per column
// Mt u_tt + Sigma Mt u_t + C u = f(t), C = -L the cotangent matrix, Mt = diag(m_i / speed_i^2), Sigma = diag(sigma_i), stepped by the trapezoidal
// rule in (u, v = u_t): with w = u + u' one solve of the constant matrix A = diag(0.5 s2 mt) + a C per step, s2 = 2.0 + sigma dt, a = 0.25 dt dt.
// The object owns ONE handle built from the caller's prolongations -- A, precomputed once, with the boundary vertices known when clamped -- the
// planes mt and s2, the geometry the potential energy reads, the source and receiver lists, and the state: a column-major nV x 2k block, u in
// columns [0, k), v in [k, 2k).  A step is the right-hand side (a kernel of its own only where the previous step has not left it), the sources,
// the fixed-order sum of its squares, the solve warm-started from 2u + dt v -- written into the block the solve returns w in: smg_solve and
// smg_solve_pcg gather z0 into the handle before they scatter z, on one stream -- and the advance kernel with the sums of its energies, all enqueued
// on the object's stream, which the handle uses too.  The host reads one double before the solve, |b|_F^2 -- it sets the default tolerance and
// refuses non-finite input -- and 2k after it, the energies.  A step writes into the block beside the state and commits by an index swap, so a
// refused step leaves the state of the last completed one.  The loop takes its state blocks as parameters: smg_wave_gauss_newton
// (smg_wave_born.cpp) runs it on the tangent state with one more launch per step, k_wave_born.  Checks, stream, handle, the cotangent system and the inner solve:
// smg_mesh_object.hpp.  The object's struct and what this file shares with smg_wave_adjoint.cpp (smg_wave_gradient runs the step loop below
// and keeps one block per step): smg_wave_object.hpp.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdlib>
#include <memory>
#include <vector>

#include "smg_device.hpp"
#include "smg_mesh.hpp"
#include "smg_mesh_object.hpp"
#include "smg_wave_inl.hpp"
#include "smg_wave_object.hpp"

using namespace smg;

namespace smg {

int wave_check_operands(const char* who, int op, int nV, int nF, int k, const int* F, const double* V, const double* speed, const double* sigma, int clamped,
                        double dt, const double* u, const double* v, const double* w, const int* idx, int n_idx, const double* sig0, const double* sig1,
                        const double* out)
{
    if (op < SMG_WAVE_RHS || op > SMG_WAVE_RECORD || nV < 1 || nF < 1 || !F || !V || !out) return fail(SMG_ERR_INVALID, "%s: bad arguments", who);
    const bool lists = op == SMG_WAVE_SOURCES || op == SMG_WAVE_RECORD;
    if (!u || (op != SMG_WAVE_RECORD && !v) || (op == SMG_WAVE_ADVANCE && !w) || (lists && !idx) || (op == SMG_WAVE_SOURCES && (!sig0 || !sig1)))
        return fail(SMG_ERR_INVALID, "%s: op %d misses an operand", who, op);
    if (k < 1) return fail(SMG_ERR_INVALID, "%s: k = %d, at least one column is needed", who, k);
    if (!std::isfinite(dt) || !(dt > 0.0)) return fail(SMG_ERR_INVALID, "%s: dt = %g, a finite value > 0 is needed", who, dt);
    if (clamped != 0 && clamped != 1) return fail(SMG_ERR_INVALID, "%s: clamped = %d, 0 or 1 is needed", who, clamped);
    for (int i = 0; speed && i < nV; i++)
        if (!std::isfinite(speed[i]) || !(speed[i] > 0.0)) return fail(SMG_ERR_INVALID, "%s: speed[%d] = %g, a finite value > 0 is needed", who, i, speed[i]);
    for (int i = 0; sigma && i < nV; i++)
        if (!std::isfinite(sigma[i]) || sigma[i] < 0.0) return fail(SMG_ERR_INVALID, "%s: sigma[%d] = %g, a finite value >= 0 is needed", who, i, sigma[i]);
    if (int rc = check_faces(who, F, nF, nV)) return rc;
    if (lists) {
        if (n_idx < 1) return fail(SMG_ERR_INVALID, "%s: n_idx = %d, at least one vertex is needed", who, n_idx);
        std::vector<char> seen((size_t)nV, 0);
        for (int j = 0; j < n_idx; j++) {
            if (idx[j] < 0 || idx[j] >= nV) return fail(SMG_ERR_INVALID, "%s: idx[%d] = %d is outside [0, %d)", who, j, idx[j], nV);
            if (op == SMG_WAVE_SOURCES && seen[(size_t)idx[j]]) return fail(SMG_ERR_INVALID, "%s: vertex %d is listed twice", who, idx[j]);
            seen[(size_t)idx[j]] = 1;
        }
    }
    return SMG_OK;
}

// s2, a, q2 from p and the handle's values diag(0.5 s2 mt) + a (-L) from the kept pattern; first: the pattern-setting precompute with the
// clamped rows known, else by values
int wave_system(smg_wave* g, bool first)
{
    const size_t n = (size_t)g->nV, nnz = g->Sys.col.size();
    const double dt = g->p.dt;
    g->a = 0.25 * dt * dt;
    g->q2 = 2.0 / dt;
    std::vector<double> s2(n), val(nnz);
    for (size_t i = 0; i < n; i++) s2[i] = 2.0 + (g->has_sigma ? g->sigma_host[i] : g->p.damping) * dt;
    for (int i = 0; i < g->nV; i++)
        for (int q = g->Sys.ptr[(size_t)i]; q < g->Sys.ptr[(size_t)i + 1]; q++) {
            const double x = g->a * g->Sys.L[(size_t)q];
            val[(size_t)q] = g->Sys.col[(size_t)q] == i ? 0.5 * s2[(size_t)i] * g->mt_host[(size_t)i] + x : x;
        }
    HIPCHK(hipStreamSynchronize(g->stream));
    HIPCHK(hipMemcpy(g->s2.p, s2.data(), n * sizeof(double), hipMemcpyHostToDevice));
    if (first) {
        if (int rc = smg_precompute(g->handle[0], g->nV, g->Sys.ptr.data(), g->Sys.col.data(), val.data(), g->bnd.empty() ? nullptr : g->bnd.data(),
                                    (int)g->bnd.size()))
            return rc;
    } else {
        HIPCHK(hipMemcpy(g->val.p, val.data(), nnz * sizeof(double), hipMemcpyHostToDevice));
        if (int rc = smg_precompute_values_device(g->handle[0], g->val.p)) return rc;
    }
    g->rhs_valid = false;
    return SMG_OK;
}

int wave_check_steps(const char* who, const smg_wave* g, int n_steps)
{
    if (!g) return fail(SMG_ERR_INVALID, "%s: null object", who);
    if (g->k < 1) return fail(SMG_ERR_INVALID, "%s: no state: call smg_wave_set_state first", who);
    if (n_steps < 1) return fail(SMG_ERR_INVALID, "%s: n_steps = %d, at least 1 is needed", who, n_steps);
    return SMG_OK;
}

int wave_check_signal(const char* who, const smg_wave* g, int n_steps, const double* signal)
{
    if (signal && g->n_src == 0) return fail(SMG_ERR_INVALID, "%s: a signal without sources: call smg_wave_set_sources first", who);
    const int k = g->k;
    const size_t row_s = (size_t)g->n_src * k;
    if (signal)
        for (size_t j = 0; j < ((size_t)n_steps + 1) * row_s; j++)
            if (!std::isfinite(signal[j]))
                return fail(SMG_ERR_INVALID, "%s: the signal is not finite at time %d, source %d, column %d", who, (int)(j / row_s), (int)(j % row_s) / k,
                            (int)(j % row_s) % k);
    return SMG_OK;
}

int wave_forward(smg_wave* g, const char* who, DevBuf<double>* S, int* cur, const WaveBorn* born, int n_steps, const double* signal,
                 const smg_solve_opts* opts, double* energy_his, double* traces, bool record, int* cycles, int* n_done, double* keep)
{
    const int n = g->nV, k = g->k, ns = g->n_src, nr = traces || record ? g->n_rec : 0;
    const size_t nk = (size_t)n * k, D = sizeof(double), row_s = (size_t)ns * k, row_r = (size_t)nr * k;
    DeviceScope dsc(g->device);
    hipStream_t st = g->stream;
    HIPCHK(hipStreamSynchronize(st));
    if (signal) {   // uploaded once per call
        HIPCHK(g->sig.ensure(((size_t)n_steps + 1) * row_s));
        HIPCHK(hipMemcpy(g->sig.p, signal, ((size_t)n_steps + 1) * row_s * D, hipMemcpyHostToDevice));
    }
    if (nr > 0) HIPCHK(g->trace.ensure((size_t)n_steps * row_r));
    g->red_host.assign(1 + 2 * (size_t)k, 0.0);
    double* rh = g->red_host.data();
    const double dt = g->p.dt;
    const int* known = g->nb > 0 ? g->known.p : nullptr;
    int done = 0, rc = SMG_OK;
    for (int t = 0; t < n_steps; t++) {
        const double* s0 = S[*cur].p;
        double* s1 = S[1 - *cur].p;
        if (!g->rhs_valid) HIPCHK(launch_wave_rhs(n, k, g->mt.p, g->s2.p, known, dt, s0, s0 + nk, n, g->B.p, g->Wb.p, n, g->rsq.p, st));
        g->rhs_valid = false;   // the sources change it in place, and the advance kernel overwrites it
        if (signal) HIPCHK(launch_wave_sources(n, k, ns, g->src.p, g->sig.p + (size_t)t * row_s, g->sig.p + ((size_t)t + 1) * row_s, g->a, g->B.p, n, g->rsq.p, st));
        if (born) HIPCHK(launch_wave_born(n, k, born->d_cols, known, born->fd, born->e + (size_t)t * nk, g->B.p, n, g->rsq.p, st));
        HIPCHK(launch_fixed_sum(g->rsq.p, (int)nk, g->part.p, g->red.p, st));
        HIPCHK(hipMemcpyAsync(rh, g->red.p, D, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        if (!std::isfinite(rh[0])) {
            rc = fail(SMG_ERR_NONFINITE, "%s: the right-hand side is not finite (step %d)", who, t);
            break;
        }
        int e = 0;
        if (born && rh[0] == 0.0) {   // as the adjoint loop: w = 0 without a solve
            HIPCHK(hipMemsetAsync(g->Wb.p, 0, nk * D, st));
        } else {
            const smg_solve_opts so = opts_or_default(opts, 1e-10 * std::sqrt(rh[0]), 100);
            if ((rc = inner_solve(g->handle[0], g->pcg, g->B.p, n, g->nb > 0 ? g->zero.p : nullptr, g->nb, g->Wb.p, n, k, so, g->Wb.p, n, &e))) break;
        }
        double* bn = g->fused ? g->B.p : nullptr;
        HIPCHK(launch_wave_advance(n, k, g->mt.p, g->s2.p, known, dt, g->q2, g->Wb.p, n, s0, s0 + nk, n, s1, s1 + nk, n, g->ke.p, bn, g->Wb.p, n, g->rsq.p, st));
        if (energy_his) {
            double* d = g->red.p + 1;
            HIPCHK(launch_fluid_velocity(g->nF, k, g->F.p, g->W.p, g->nrm.p, g->Af.p, s1, n, nullptr, g->terms.p, st));
            for (int c = 0; c < k; c++) {
                HIPCHK(launch_fixed_sum(g->ke.p + (size_t)c * n, n, g->part.p, d + c, st));
                HIPCHK(launch_fixed_sum(g->terms.p + (size_t)c * g->nF, g->nF, g->part.p, d + k + c, st));
            }
            HIPCHK(hipMemcpyAsync(rh + 1, d, 2 * (size_t)k * D, hipMemcpyDeviceToHost, st));
        }
        if (keep) HIPCHK(launch_wave_adj_keep(n, k, g->s2.p, dt, s0, s0 + nk, s1, n, keep + (size_t)t * nk, st));
        if (nr > 0) HIPCHK(launch_wave_record(n, k, nr, g->rec.p, s1, n, g->trace.p + (size_t)t * row_r, st));
        HIPCHK(hipStreamSynchronize(st));
        *cur = 1 - *cur;
        g->rhs_valid = g->fused;
        if (energy_his) std::copy(rh + 1, rh + 1 + 2 * (size_t)k, energy_his + (size_t)t * 2 * k);
        if (cycles) cycles[t] = e;
        done = t + 1;
    }
    if (traces && nr > 0 && done > 0) HIPCHK(hipMemcpy(traces, g->trace.p, (size_t)done * row_r * D, hipMemcpyDeviceToHost));   // once, at the end of the call
    if (n_done) *n_done = done;
    return rc;
}

}  // namespace smg

namespace {

int check_params(const char* who, const smg_wave_params& p)
{
    if (!std::isfinite(p.dt) || !(p.dt > 0.0)) return fail(SMG_ERR_INVALID, "%s: dt = %g, a finite value > 0 is needed", who, p.dt);
    if (!std::isfinite(p.damping) || p.damping < 0.0) return fail(SMG_ERR_INVALID, "%s: damping = %g, a finite value >= 0 is needed", who, p.damping);
    if (p.clamped != 0 && p.clamped != 1) return fail(SMG_ERR_INVALID, "%s: clamped = %d, 0 or 1 is needed", who, p.clamped);
    return SMG_OK;
}

int create_impl(const smg_hierarchy* h, const double* V, int nV, const int* F, int nF, const double* speed, const double* sigma, const smg_wave_params* p,
                smg_wave** out)
{
    if (out) *out = nullptr;
    const char* who = "smg_wave_create";
    if (!h || !V || !F || !p || !out || nV <= 0 || nF <= 0) return fail(SMG_ERR_INVALID, "%s: bad arguments", who);
    if (int rc = check_hierarchy(who, h, 1, nV)) return rc;
    if (h->n_levels < 2) return fail(SMG_ERR_INVALID, "%s: a hierarchy of at least two levels is needed", who);
    if (int rc = check_mesh(who, V, nV, F, nF, true)) return rc;
    if (int rc = check_params(who, *p)) return rc;
    for (int i = 0; speed && i < nV; i++)
        if (!std::isfinite(speed[i]) || !(speed[i] > 0.0)) return fail(SMG_ERR_INVALID, "%s: speed[%d] = %g, a finite value > 0 is needed", who, i, speed[i]);
    for (int i = 0; sigma && i < nV; i++)
        if (!std::isfinite(sigma[i]) || sigma[i] < 0.0) return fail(SMG_ERR_INVALID, "%s: sigma[%d] = %g, a finite value >= 0 is needed", who, i, sigma[i]);
    std::vector<int> bnd;
    if (p->clamped) {
        bnd = boundary_vertices(F, nF, nV);
        if (bnd.empty()) return fail(SMG_ERR_INVALID, "%s: clamped = 1, but the mesh has no boundary", who);
        if ((int)bnd.size() >= nV) return fail(SMG_ERR_INVALID, "%s: no interior vertex: every vertex is on the clamped boundary", who);
    }

    std::unique_ptr<smg_wave> g(new smg_wave());
    g->nV = nV; g->nF = nF; g->p = *p; g->nb = (int)bnd.size();
    g->bnd = bnd;
    if (const char* e = std::getenv("SMG_WAVE_FUSED")) g->fused = std::atoi(e) != 0;   // A/B knob of tools/wave_time.py
    g->has_sigma = sigma != nullptr;
    if (sigma) g->sigma_host.assign(sigma, sigma + nV);
    if (int rc = g->open(who)) return rc;
    if (int rc = g->clone(who, h, 0)) return rc;

    // the geometry of the potential energy, the masses and -L, then the constant matrix: precomputed once.  The positions are read here alone
    DevBuf<double> dV, m;
    DevBuf<int> m_ptr, m_idx;
    HIPCHK(dV.upload(std::vector<double>(V, V + (size_t)nV * 3)));
    if (int rc = upload_faces(F, nF, nV, g->F, m_ptr, m_idx)) return rc;
    HIPCHK(g->W.alloc((size_t)nF * 9));
    HIPCHK(g->nrm.alloc((size_t)nF * 3));
    HIPCHK(g->Af.alloc((size_t)nF));
    HIPCHK(m.alloc((size_t)nV));
    HIPCHK(launch_hodge_geometry(dV.p, g->F.p, nF, g->W.p, g->nrm.p, g->Af.p, g->stream));
    HIPCHK(launch_fluid_mass(nV, m_ptr.p, m_idx.p, g->Af.p, m.p, g->stream));
    g->mt_host.resize((size_t)nV);
    HIPCHK(hipMemcpyAsync(g->mt_host.data(), m.p, (size_t)nV * sizeof(double), hipMemcpyDeviceToHost, g->stream));
    if (int rc = cotan_system(F, nF, nV, dV.p, 0, 0.0, -1.0, g->stream, g->Sys, false)) return rc;   // synchronises: the masses have arrived
    for (double& x : g->Sys.L) x = -x;
    g->m_host = g->mt_host;   // kept for smg_wave_set_speed
    if (speed) g->speed_host.assign(speed, speed + nV);
    for (int i = 0; speed && i < nV; i++) g->mt_host[(size_t)i] = g->mt_host[(size_t)i] / (speed[i] * speed[i]);
    HIPCHK(g->mt.upload(g->mt_host));
    HIPCHK(g->s2.alloc((size_t)nV));
    HIPCHK(g->val.alloc(g->Sys.col.size()));
    if (g->nb > 0) {
        g->on_bnd.assign((size_t)nV, 0);
        for (int v : bnd) g->on_bnd[(size_t)v] = 1;
        HIPCHK(g->known.upload(g->on_bnd));
        HIPCHK(g->rows.upload(bnd));
    }
    if (int rc = wave_system(g.get(), true)) return rc;
    *out = g.release();
    return SMG_OK;
}

// the blocks of a k-column state; they grow with the largest k seen and are kept
int ensure_columns(smg_wave* g, int k)
{
    const size_t n = (size_t)g->nV, nf = (size_t)g->nF, nb = (size_t)g->nb, kk = (size_t)k;
    if (g->kcap >= kk) return SMG_OK;
    HIPCHK(hipStreamSynchronize(g->stream));
    for (auto& b : g->S) HIPCHK(b.alloc(2 * n * kk));
    for (DevBuf<double>* b : {&g->B, &g->Wb, &g->rsq, &g->ke}) HIPCHK(b->alloc(n * kk));
    HIPCHK(g->terms.alloc(nf * kk));
    HIPCHK(g->part.alloc((size_t)fixed_sum_groups((int)std::max(n * kk, nf))));
    HIPCHK(g->red.alloc(1 + 2 * kk));
    if (nb > 0) {
        HIPCHK(g->zero.alloc(nb * kk));
        HIPCHK(g->flag.alloc(nb * kk));
        HIPCHK(hipMemsetAsync(g->zero.p, 0, nb * kk * sizeof(double), g->stream));
    }
    g->kcap = kk;
    return SMG_OK;
}

int check_state(const char* who, const smg_wave* g)
{
    if (!g) return fail(SMG_ERR_INVALID, "%s: null object", who);
    if (g->k < 1) return fail(SMG_ERR_INVALID, "%s: no state: call smg_wave_set_state first", who);
    return SMG_OK;
}

int set_state_impl(smg_wave* g, const double* u, const double* v, int ld, int k, int memspace)
{
    const char* who = "smg_wave_set_state";
    if (!g || !u || !v) return fail(SMG_ERR_INVALID, "%s: bad arguments", who);
    if (k < 1) return fail(SMG_ERR_INVALID, "%s: k = %d, at least one column is needed", who, k);
    if (2LL * g->nV * k > INT_MAX || 3LL * g->nF * k > INT_MAX)
        return fail(SMG_ERR_INVALID, "%s: k = %d columns of %d vertices exceed the index range", who, k, g->nV);
    if (bad_memspace(memspace)) return fail(SMG_ERR_INVALID, "%s: memspace must be SMG_HOST or SMG_DEVICE", who);
    if (ld < g->nV) return fail(SMG_ERR_INVALID, "%s: a leading dimension is too small", who);
    DeviceScope dsc(g->device);
    if (k != g->k) g->lin_valid = false;   // smg_wave_gauss_newton's linearisation point has the columns of the state
    g->k = 0;
    g->rhs_valid = false;
    if (int rc = ensure_columns(g, k)) return rc;
    const int n = g->nV;
    const size_t nk = (size_t)n * k;
    hipStream_t st = g->stream;
    HIPCHK(copy_columns(g->S[0].p, n, u, ld, n, k, copy_in(memspace), st));
    HIPCHK(copy_columns(g->S[0].p + nk, n, v, ld, n, k, copy_in(memspace), st));
    if (g->nb > 0) {   // a clamped row's u and v are 0: one small kernel and one host read
        double any = 0.0;
        HIPCHK(launch_wave_rows_nonzero(n, k, g->nb, g->rows.p, g->S[0].p, g->S[0].p + nk, n, g->flag.p, st));
        HIPCHK(launch_fixed_max(g->flag.p, g->nb * k, g->part.p, g->red.p, st));
        HIPCHK(hipMemcpyAsync(&any, g->red.p, sizeof(double), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        if (any != 0.0) return fail(SMG_ERR_INVALID, "%s: u or v is not 0 on a clamped boundary row", who);
    }
    HIPCHK(hipStreamSynchronize(st));
    g->cur = 0; g->k = k;
    return SMG_OK;
}

int state_impl(smg_wave* g, double* u, double* v, int ld, int memspace)
{
    const char* who = "smg_wave_state";
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

// a source or receiver list: in range, as a source list no vertex twice and none on a clamped row; kept on the device in `buf`
int set_list(smg_wave* g, const char* who, const int* idx, int count, bool sources, DevBuf<int>& buf, int* kept)
{
    if (count < 0 || (count > 0 && !idx)) return fail(SMG_ERR_INVALID, "%s: bad arguments", who);
    std::vector<char> seen(sources ? (size_t)g->nV : 0, 0);
    for (int j = 0; j < count; j++) {
        if (idx[j] < 0 || idx[j] >= g->nV) return fail(SMG_ERR_INVALID, "%s: idx[%d] = %d is outside [0, %d)", who, j, idx[j], g->nV);
        if (!sources) continue;
        if (seen[(size_t)idx[j]]) return fail(SMG_ERR_INVALID, "%s: vertex %d is listed twice", who, idx[j]);
        seen[(size_t)idx[j]] = 1;
        if (g->nb > 0 && g->on_bnd[(size_t)idx[j]]) return fail(SMG_ERR_INVALID, "%s: vertex %d is on the clamped boundary", who, idx[j]);
    }
    DeviceScope dsc(g->device);
    HIPCHK(hipStreamSynchronize(g->stream));
    HIPCHK(buf.ensure((size_t)count));
    if (count > 0) HIPCHK(hipMemcpy(buf.p, idx, (size_t)count * sizeof(int), hipMemcpyHostToDevice));
    *kept = count;
    return SMG_OK;
}

int step_impl(smg_wave* g, int n_steps, const double* signal, const smg_solve_opts* opts, double* energy_his, double* traces, int* cycles, int* n_done)
{
    const char* who = "smg_wave_step";
    if (n_done) *n_done = 0;
    if (int rc = wave_check_steps(who, g, n_steps)) return rc;
    if (int rc = wave_check_signal(who, g, n_steps, signal)) return rc;
    return wave_forward(g, who, g->S, &g->cur, nullptr, n_steps, signal, opts, energy_his, traces, false, cycles, n_done, nullptr);
}

int set_params_impl(smg_wave* g, const smg_wave_params* p)
{
    const char* who = "smg_wave_set_params";
    if (!g || !p) return fail(SMG_ERR_INVALID, "%s: bad arguments", who);
    if (int rc = check_params(who, *p)) return rc;
    if (p->clamped != g->p.clamped)
        return fail(SMG_ERR_INVALID, "%s: clamped = %d, but the object was created with clamped = %d: the known rows cannot change", who, p->clamped,
                    g->p.clamped);
    DeviceScope dsc(g->device);
    g->lin_valid = false;
    const bool changed = p->dt != g->p.dt || (!g->has_sigma && p->damping != g->p.damping);
    const smg_wave_params old = g->p;
    g->p = *p;
    if (changed)
        if (int rc = wave_system(g, false)) {
            g->p = old;
            return rc;
        }
    return SMG_OK;
}

}  // namespace

extern "C" smg_wave_params smg_wave_params_default(void)
{
    smg_wave_params p;
    p.dt = 1.0; p.damping = 0.0; p.clamped = 0;
    return p;
}

extern "C" int smg_wave_create(const smg_hierarchy* h, const double* V, int nV, const int* F, int nF, const double* speed, const double* sigma,
                               const smg_wave_params* p, smg_wave** out)
{
    return guarded("smg_wave_create", [&]() { return create_impl(h, V, nV, F, nF, speed, sigma, p, out); });
}

extern "C" void smg_wave_destroy(smg_wave* g) { delete g; }

extern "C" int smg_wave_set_params(smg_wave* g, const smg_wave_params* p)
{
    return guarded("smg_wave_set_params", [&]() { return set_params_impl(g, p); });
}

extern "C" int smg_wave_set_solver(smg_wave* g, int pcg)
{
    if (!g) return fail(SMG_ERR_INVALID, "smg_wave_set_solver: null object");
    latch_solver(g->pcg, pcg);
    return SMG_OK;
}

extern "C" long long smg_wave_device_bytes(const smg_wave* g)
{
    if (!g) return 0;   // one list: every DevBuf of the struct
    return device_bytes(*g, g->F, g->known, g->rows, g->src, g->rec, g->W, g->nrm, g->Af, g->mt, g->s2, g->val, g->S[0], g->S[1], g->B, g->Wb, g->rsq,
                        g->ke, g->terms, g->part, g->red, g->zero, g->flag, g->sig, g->trace, g->grp_v, g->grp_ptr, g->grp_slot, g->H, g->P, g->Q, g->Y, g->G, g->rho,
                        g->apart, g->ared, g->gs, g->fac, g->T[0], g->T[1], g->fd);
}

extern "C" int smg_wave_set_state(smg_wave* g, const double* u, const double* v, int ld, int k, int memspace)
{
    return guarded("smg_wave_set_state", [&]() { return set_state_impl(g, u, v, ld, k, memspace); });
}

extern "C" int smg_wave_state(smg_wave* g, double* u, double* v, int ld, int memspace)
{
    return guarded("smg_wave_state", [&]() { return state_impl(g, u, v, ld, memspace); });
}

extern "C" int smg_wave_set_sources(smg_wave* g, const int* idx, int n_src)
{
    return guarded("smg_wave_set_sources", [&]() -> int {
        if (!g) return fail(SMG_ERR_INVALID, "smg_wave_set_sources: null object");
        return set_list(g, "smg_wave_set_sources", idx, n_src, true, g->src, &g->n_src);
    });
}

extern "C" int smg_wave_set_receivers(smg_wave* g, const int* idx, int n_rec)
{
    return guarded("smg_wave_set_receivers", [&]() -> int {
        if (!g) return fail(SMG_ERR_INVALID, "smg_wave_set_receivers: null object");
        if (int rc = set_list(g, "smg_wave_set_receivers", idx, n_rec, false, g->rec, &g->n_rec)) return rc;
        g->rec_host.assign(idx, idx + n_rec);   // smg_wave_gradient groups it by vertex at its next call
        g->grouped = false;
        g->lin_valid = false;
        return SMG_OK;
    });
}

extern "C" int smg_wave_step(smg_wave* g, int n_steps, const double* signal, const smg_solve_opts* opts, double* energy_his, double* traces, int* cycles,
                             int* n_done)
{
    return guarded("smg_wave_step", [&]() { return step_impl(g, n_steps, signal, opts, energy_his, traces, cycles, n_done); });
}

extern "C" int smg_wave_host(int op, int nV, int nF, int k, const int* F, const double* V, const double* speed, const double* sigma, int clamped, double dt,
                             const double* u, const double* v, const double* w, const int* idx, int n_idx, const double* sig0, const double* sig1, double* out)
{
    return guarded("smg_wave_host", [&]() -> int {
        const char* who = "smg_wave_host";
        if (int rc = wave_check_operands(who, op, nV, nF, k, F, V, speed, sigma, clamped, dt, u, v, w, idx, n_idx, sig0, sig1, out)) return rc;
        const size_t n = (size_t)nV, f = (size_t)nF, kk = (size_t)k, nk = n * kk;
        if (op == SMG_WAVE_RECORD) {
            wave_host_record(nV, k, n_idx, idx, u, out);
            return SMG_OK;
        }
        std::vector<int> mp, mi, known;
        vertex_corner_lists(std::vector<int>(F, F + 3 * f), nV, mp, mi);
        if (clamped) {
            known.assign(n, 0);
            for (int b : boundary_vertices(F, nF, nV)) known[(size_t)b] = 1;
        }
        const int* kn = clamped ? known.data() : nullptr;
        std::vector<double> A(f), m(n), mt(n), s2(n);
        fluid_host_mass(nV, nF, F, V, mp.data(), mi.data(), A.data(), m.data());
        wave_host_planes(nV, m.data(), speed, sigma, dt, mt.data(), s2.data());
        const double a = 0.25 * dt * dt, q2 = 2.0 / dt;
        if (op == SMG_WAVE_RHS || op == SMG_WAVE_SOURCES) {
            double *b = out, *rsq = out + nk, *z = out + 2 * nk;
            wave_host_rhs(nV, k, mt.data(), s2.data(), kn, dt, u, v, b, rsq, z);
            if (op == SMG_WAVE_SOURCES) wave_host_sources(nV, k, n_idx, idx, sig0, sig1, a, b, rsq);
            out[3 * nk] = flow_host_sum(rsq, (int)nk);
        } else {
            wave_host_advance(nV, k, mt.data(), s2.data(), kn, dt, q2, w, u, v, out, out + nk, out + 2 * nk, nullptr, nullptr, nullptr);
            double* o = out + 3 * nk;
            wave_host_advance(nV, k, mt.data(), s2.data(), kn, dt, q2, w, u, v, o, o + nk, o + 2 * nk, o + 3 * nk, o + 4 * nk, o + 5 * nk);
            std::vector<double> U(3 * f * kk), terms(f * kk);
            fluid_host_velocity(nV, nF, k, F, V, o, U.data(), terms.data());
            double* s = out + 9 * nk;
            for (size_t c = 0; c < kk; c++) {
                s[c] = flow_host_sum(o + 2 * nk + c * n, nV);
                s[kk + c] = flow_host_sum(terms.data() + c * f, nF);
            }
            s[2 * kk] = flow_host_sum(o + 4 * nk, (int)nk);
        }
        return SMG_OK;
    });
}
