// smg_wave_adjoint.cpp -- adjoint-state gradients of a trace misfit through the wave object's own time stepper (include/smg.h: smg_wave_gradient,
// smg_wave_set_speed).  The forward half is smg_wave_step's loop (wave_forward, smg_wave.cpp) with one more launch per step,
// which keeps e_n = dt v_n - (0.5 s2) (u_n+1 - u_n), one n x k block.  The residuals rho = traces - observed and the misfit's fixed-order sums follow.
// A = diag(0.5 s2 mt) + a C is symmetric, so the transposed step is ONE solve of the same handle, warm-started from the previous adjoint solve's
// answer, between pointwise kernels: for n = N - 1 .. 0
//     g = p + q2 q;  A y = g;  G += y e_n;  gs[n], gs[n + 1] += a y[src];  t = mt y;  p = (s2 t - p) - (2.0 q2) q + R' rho_n;  q = dt t - q
// from p = R' rho_N, q = 0.  At the end (p, q) is the gradient with respect to the state the call started from, (-2 mt / speed) G the one with
// respect to the speed and gs the one with respect to the signal.  The adjoint right-hand side and its squares use the forward step's blocks B and
// rsq, so the kept right-hand side is dropped; the next smg_wave_step forms it again, to the same bits.  Everything stays on the device; the host
// reads |g|_F^2 before every solve, as the forward step reads |b|_F^2.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <vector>

#include "smg_device.hpp"
#include "smg_mesh.hpp"
#include "smg_mesh_object.hpp"
#include "smg_wave_adjoint_inl.hpp"
#include "smg_wave_object.hpp"

using namespace smg;

namespace smg {

int wave_adjoint_check_operands(const char* who, int op, int nV, int nF, int k, const int* F, const double* V, const double* speed, const double* sigma,
                                int clamped, double dt, const double* x0, const double* x1, const double* x2, const double* x3, const double* x4, const int* idx,
                                int n_idx, int n_rows, const double* out)
{
    if (op < SMG_WAVE_ADJ_KEEP || op > SMG_WAVE_ADJ_SCALE || nV < 1 || nF < 1 || !F || !V || !out) return fail(SMG_ERR_INVALID, "%s: bad arguments", who);
    const bool list = op == SMG_WAVE_ADJ_INJECT || op == SMG_WAVE_ADJ_SIGNAL;
    const int need = op == SMG_WAVE_ADJ_ADVANCE ? 5 : op == SMG_WAVE_ADJ_KEEP || op == SMG_WAVE_ADJ_SIGNAL ? 3 : op == SMG_WAVE_ADJ_INJECT || op == SMG_WAVE_ADJ_RHS ? 2 : 1;
    const double* x[5] = {x0, x1, x2, x3, x4};
    for (int j = 0; j < need; j++)
        if (!x[j]) return fail(SMG_ERR_INVALID, "%s: op %d misses an operand", who, op);
    if (list && !idx) return fail(SMG_ERR_INVALID, "%s: op %d misses an operand", who, op);
    if (k < 1) return fail(SMG_ERR_INVALID, "%s: k = %d, at least one column is needed", who, k);
    if (!std::isfinite(dt) || !(dt > 0.0)) return fail(SMG_ERR_INVALID, "%s: dt = %g, a finite value > 0 is needed", who, dt);
    if (clamped != 0 && clamped != 1) return fail(SMG_ERR_INVALID, "%s: clamped = %d, 0 or 1 is needed", who, clamped);
    for (int i = 0; speed && i < nV; i++)
        if (!std::isfinite(speed[i]) || !(speed[i] > 0.0)) return fail(SMG_ERR_INVALID, "%s: speed[%d] = %g, a finite value > 0 is needed", who, i, speed[i]);
    for (int i = 0; sigma && i < nV; i++)
        if (!std::isfinite(sigma[i]) || sigma[i] < 0.0) return fail(SMG_ERR_INVALID, "%s: sigma[%d] = %g, a finite value >= 0 is needed", who, i, sigma[i]);
    if (int rc = check_faces(who, F, nF, nV)) return rc;
    if (op == SMG_WAVE_ADJ_RESIDUAL) {
        if (n_rows < 1 || n_idx < 1) return fail(SMG_ERR_INVALID, "%s: n_rows = %d, n_idx = %d, at least one row of one slot is needed", who, n_rows, n_idx);
        if ((long long)n_rows * n_idx * k > INT_MAX) return fail(SMG_ERR_INVALID, "%s: %d rows of %d slots and %d columns exceed the index range", who, n_rows, n_idx, k);
    }
    if (list) {
        if (n_idx < 1) return fail(SMG_ERR_INVALID, "%s: n_idx = %d, at least one vertex is needed", who, n_idx);
        std::vector<char> seen((size_t)nV, 0);
        for (int j = 0; j < n_idx; j++) {
            if (idx[j] < 0 || idx[j] >= nV) return fail(SMG_ERR_INVALID, "%s: idx[%d] = %d is outside [0, %d)", who, j, idx[j], nV);
            if (op == SMG_WAVE_ADJ_SIGNAL && seen[(size_t)idx[j]]) return fail(SMG_ERR_INVALID, "%s: vertex %d is listed twice", who, idx[j]);
            seen[(size_t)idx[j]] = 1;
        }
    }
    return SMG_OK;
}

// the blocks of a gradient call; they grow with the largest shape seen and are kept.  The receivers are grouped by vertex where the list has changed
int wave_ensure_adjoint(smg_wave* g, int n_steps, bool backward, bool observed, bool grad_signal)
{
    const size_t nk = (size_t)g->nV * g->k, ent = (size_t)n_steps * g->n_rec, ek = ent * g->k;
    HIPCHK(hipStreamSynchronize(g->stream));
    HIPCHK(g->rho.ensure((observed ? 3 : 2) * ek));
    HIPCHK(g->apart.ensure((size_t)fixed_sum_groups((int)ent)));
    HIPCHK(g->ared.ensure((size_t)g->k));
    if (!backward) return SMG_OK;
    HIPCHK(g->H.ensure((size_t)n_steps * nk));
    for (DevBuf<double>* b : {&g->P, &g->Q, &g->Y, &g->G}) HIPCHK(b->ensure(nk));
    if (grad_signal) HIPCHK(g->gs.ensure(((size_t)n_steps + 1) * g->n_src * g->k));
    if (!g->grouped) {
        std::vector<int> gv, gp, gl;
        wave_group_receivers(g->nV, g->n_rec, g->rec_host.data(), g->nb > 0 ? g->on_bnd.data() : nullptr, gv, gp, gl);
        g->n_grp = (int)gv.size();
        HIPCHK(g->grp_v.ensure(gv.size()));
        HIPCHK(g->grp_ptr.ensure(gp.size()));
        HIPCHK(g->grp_slot.ensure(gl.size()));
        if (g->n_grp > 0) {
            HIPCHK(hipMemcpy(g->grp_v.p, gv.data(), gv.size() * sizeof(int), hipMemcpyHostToDevice));
            HIPCHK(hipMemcpy(g->grp_slot.p, gl.data(), gl.size() * sizeof(int), hipMemcpyHostToDevice));
        }
        HIPCHK(hipMemcpy(g->grp_ptr.p, gp.data(), gp.size() * sizeof(int), hipMemcpyHostToDevice));
        g->grouped = true;
    }
    if (!g->fac_valid) {
        std::vector<double> fac((size_t)g->nV);
        wave_adj_host_planes(g->nV, g->mt_host.data(), g->speed_host.empty() ? nullptr : g->speed_host.data(), fac.data());
        HIPCHK(g->fac.ensure(fac.size()));
        HIPCHK(hipMemcpy(g->fac.p, fac.data(), fac.size() * sizeof(double), hipMemcpyHostToDevice));
        g->fac_valid = true;
    }
    return SMG_OK;
}

// the backward pass: what smg_wave_gradient and smg_wave_gauss_newton run alike
int wave_backward(smg_wave* g, const char* who, int n_steps, const double* rho, const smg_solve_opts* opts, bool grad_signal, int* cycles)
{
    const int n = g->nV, k = g->k, N = n_steps, ns = g->n_src, nr = g->n_rec;
    const size_t nk = (size_t)n * k, D = sizeof(double), row_s = (size_t)ns * k, row_r = (size_t)nr * k;
    hipStream_t st = g->stream;
    g->rhs_valid = false;   // B and rsq hold the adjoint right-hand side from here on
    for (DevBuf<double>* b : {&g->P, &g->Q, &g->Y, &g->G}) HIPCHK(hipMemsetAsync(b->p, 0, nk * D, st));
    if (grad_signal) HIPCHK(hipMemsetAsync(g->gs.p, 0, ((size_t)N + 1) * row_s * D, st));
    const int* known = g->nb > 0 ? g->known.p : nullptr;
    const double dt = g->p.dt;
    double ss = 0.0;
    HIPCHK(launch_wave_adj_inject(n, k, g->n_grp, g->grp_v.p, g->grp_ptr.p, g->grp_slot.p, rho + (size_t)(N - 1) * row_r, g->P.p, n, st));
    for (int t = N - 1; t >= 0; t--) {
        HIPCHK(launch_wave_adj_rhs(n, k, known, g->q2, g->P.p, g->Q.p, n, g->B.p, n, g->rsq.p, st));
        HIPCHK(launch_fixed_sum(g->rsq.p, (int)nk, g->part.p, g->red.p, st));
        HIPCHK(hipMemcpyAsync(&ss, g->red.p, D, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        if (!std::isfinite(ss)) return fail(SMG_ERR_NONFINITE, "%s: the adjoint right-hand side is not finite (step %d)", who, t);
        int e = 0;
        if (ss == 0.0) {
            HIPCHK(hipMemsetAsync(g->Y.p, 0, nk * D, st));
        } else {
            const smg_solve_opts so = opts_or_default(opts, 1e-10 * std::sqrt(ss), 100);
            if (int rc = inner_solve(g->handle[0], g->pcg, g->B.p, n, g->nb > 0 ? g->zero.p : nullptr, g->nb, g->Y.p, n, k, so, g->Y.p, n, &e)) return rc;
        }
        HIPCHK(launch_wave_adj_advance(n, k, g->mt.p, g->s2.p, dt, g->q2, g->Y.p, n, g->H.p + (size_t)t * nk, g->P.p, g->Q.p, g->G.p, n, st));
        if (grad_signal) HIPCHK(launch_wave_adj_signal(n, k, ns, g->src.p, g->a, g->Y.p, n, g->gs.p + (size_t)t * row_s, g->gs.p + ((size_t)t + 1) * row_s, st));
        if (t >= 1) HIPCHK(launch_wave_adj_inject(n, k, g->n_grp, g->grp_v.p, g->grp_ptr.p, g->grp_slot.p, rho + (size_t)(t - 1) * row_r, g->P.p, n, st));
        if (cycles) cycles[N - 1 - t] = e;
    }
    return SMG_OK;
}

}  // namespace smg

namespace {

int gradient_impl(smg_wave* g, int n_steps, const double* signal, const double* observed, const smg_solve_opts* opts, double* misfit, double* grad_speed, int ld,
                  double* grad_u0, double* grad_v0, int ld0, double* grad_signal, double* traces, int* cycles, int* n_done)
{
    const char* who = "smg_wave_gradient";
    if (n_done) *n_done = 0;
    if (int rc = wave_check_steps(who, g, n_steps)) return rc;
    if (g->n_rec == 0) return fail(SMG_ERR_INVALID, "%s: no receivers: call smg_wave_set_receivers first", who);
    if (int rc = wave_check_signal(who, g, n_steps, signal)) return rc;
    const int n = g->nV, k = g->k, N = n_steps, ns = g->n_src, nr = g->n_rec;
    if ((long long)N * nr * k > INT_MAX) return fail(SMG_ERR_INVALID, "%s: %d steps of %d receivers and %d columns exceed the index range", who, N, nr, k);
    const size_t D = sizeof(double), row_s = (size_t)ns * k, row_r = (size_t)nr * k, ent = (size_t)N * nr, ek = ent * k;
    if (observed)
        for (size_t j = 0; j < ek; j++)
            if (!std::isfinite(observed[j]))
                return fail(SMG_ERR_INVALID, "%s: observed is not finite at step %d, receiver %d, column %d", who, (int)(j / row_r), (int)(j % row_r) / k,
                            (int)(j % row_r) % k);
    if ((grad_speed && ld < n) || ((grad_u0 || grad_v0) && ld0 < n)) return fail(SMG_ERR_INVALID, "%s: a leading dimension is too small", who);
    if (grad_signal && !signal) return fail(SMG_ERR_INVALID, "%s: grad_signal without a signal", who);
    const bool backward = grad_speed || grad_u0 || grad_v0 || grad_signal;
    DeviceScope dsc(g->device);
    hipStream_t st = g->stream;
    // a call with a backward pass regrows and overwrites the history: smg_wave_gauss_newton's linearisation point is this call's once it has
    // completed and none where it has not; a call without one leaves both
    if (backward) g->lin_valid = false;
    if (int rc = wave_ensure_adjoint(g, N, backward, observed != nullptr, grad_signal != nullptr)) return rc;

    // the forward half: smg_wave_step's loop, the traces recorded on the device, e_n kept
    int done = 0;
    const int rcf = wave_forward(g, who, g->S, &g->cur, nullptr, N, signal, opts, nullptr, traces, true, cycles, &done, backward ? g->H.p : nullptr);
    if (n_done) *n_done = done;
    if (rcf != SMG_OK || done < N) return rcf;

    // the residuals and the misfit
    double *rho = g->rho.p, *sq = rho + ek, *obs = observed ? rho + 2 * ek : nullptr;
    if (observed) HIPCHK(hipMemcpyAsync(obs, observed, ek * D, hipMemcpyHostToDevice, st));
    HIPCHK(launch_wave_adj_residual(k, (long long)ent, g->trace.p, obs, rho, sq, st));
    for (int c = 0; c < k; c++) HIPCHK(launch_fixed_sum(sq + (size_t)c * ent, (int)ent, g->apart.p, g->ared.p + c, st));
    std::vector<double> J((size_t)k);
    HIPCHK(hipMemcpyAsync(J.data(), g->ared.p, (size_t)k * D, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    for (int c = 0; misfit && c < k; c++) misfit[c] = 0.5 * J[(size_t)c];
    if (!backward) return SMG_OK;

    // the backward pass
    if (int rc = wave_backward(g, who, N, rho, opts, grad_signal != nullptr, cycles ? cycles + N : nullptr)) return rc;
    if (grad_speed) {
        HIPCHK(launch_wave_adj_scale(n, k, g->fac.p, g->G.p, n, g->G.p, n, st));
        HIPCHK(copy_columns(grad_speed, ld, g->G.p, n, n, k, hipMemcpyDeviceToHost, st));
    }
    if (grad_u0) HIPCHK(copy_columns(grad_u0, ld0, g->P.p, n, n, k, hipMemcpyDeviceToHost, st));
    if (grad_v0) HIPCHK(copy_columns(grad_v0, ld0, g->Q.p, n, n, k, hipMemcpyDeviceToHost, st));
    if (grad_signal) HIPCHK(hipMemcpyAsync(grad_signal, g->gs.p, ((size_t)N + 1) * row_s * D, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    g->lin_valid = true;
    g->lin_steps = N;
    return SMG_OK;
}

int set_speed_impl(smg_wave* g, const double* speed)
{
    const char* who = "smg_wave_set_speed";
    if (!g) return fail(SMG_ERR_INVALID, "%s: null object", who);
    for (int i = 0; speed && i < g->nV; i++)
        if (!std::isfinite(speed[i]) || !(speed[i] > 0.0)) return fail(SMG_ERR_INVALID, "%s: speed[%d] = %g, a finite value > 0 is needed", who, i, speed[i]);
    DeviceScope dsc(g->device);
    const size_t n = (size_t)g->nV;
    const std::vector<double> old_mt = g->mt_host, old_speed = g->speed_host;
    for (size_t i = 0; i < n; i++) g->mt_host[i] = speed ? g->m_host[i] / (speed[i] * speed[i]) : g->m_host[i];
    if (speed) g->speed_host.assign(speed, speed + n); else g->speed_host.clear();
    g->fac_valid = false;
    g->lin_valid = false;
    HIPCHK(hipStreamSynchronize(g->stream));
    HIPCHK(hipMemcpy(g->mt.p, g->mt_host.data(), n * sizeof(double), hipMemcpyHostToDevice));
    if (int rc = wave_system(g, false)) {   // back to the speed it had: the planes, and the handle's values once more, which may have been replaced in part
        g->mt_host = old_mt;
        g->speed_host = old_speed;
        (void)hipMemcpy(g->mt.p, g->mt_host.data(), n * sizeof(double), hipMemcpyHostToDevice);
        (void)wave_system(g, false);        // should this fail too, the next smg_wave_set_speed or smg_wave_set_params re-precomputes every value
        return rc;
    }
    return SMG_OK;
}

}  // namespace

extern "C" int smg_wave_gradient(smg_wave* g, int n_steps, const double* signal, const double* observed, const smg_solve_opts* opts, double* misfit,
                                 double* grad_speed, int ld, double* grad_u0, double* grad_v0, int ld0, double* grad_signal, double* traces, int* cycles,
                                 int* n_done)
{
    return guarded("smg_wave_gradient", [&]() {
        return gradient_impl(g, n_steps, signal, observed, opts, misfit, grad_speed, ld, grad_u0, grad_v0, ld0, grad_signal, traces, cycles, n_done);
    });
}

extern "C" int smg_wave_set_speed(smg_wave* g, const double* speed)
{
    return guarded("smg_wave_set_speed", [&]() { return set_speed_impl(g, speed); });
}

extern "C" int smg_wave_adjoint_host(int op, int nV, int nF, int k, const int* F, const double* V, const double* speed, const double* sigma, int clamped,
                                     double dt, const double* x0, const double* x1, const double* x2, const double* x3, const double* x4, const int* idx, int n_idx,
                                     int n_rows, double* out)
{
    return guarded("smg_wave_adjoint_host", [&]() -> int {
        const char* who = "smg_wave_adjoint_host";
        if (int rc = wave_adjoint_check_operands(who, op, nV, nF, k, F, V, speed, sigma, clamped, dt, x0, x1, x2, x3, x4, idx, n_idx, n_rows, out)) return rc;
        const size_t n = (size_t)nV, f = (size_t)nF, kk = (size_t)k, nk = n * kk;
        if (op == SMG_WAVE_ADJ_RESIDUAL) {
            const size_t ent = (size_t)n_rows * (size_t)n_idx;
            wave_adj_host_residual(k, ent, x0, x1, out, out + ent * kk);
            for (size_t c = 0; c < kk; c++) out[2 * ent * kk + c] = flow_host_sum(out + ent * kk + c * ent, (int)ent);
            return SMG_OK;
        }
        std::vector<int> known;
        if (clamped) {
            known.assign(n, 0);
            for (int b : boundary_vertices(F, nF, nV)) known[(size_t)b] = 1;
        }
        const int* kn = clamped ? known.data() : nullptr;
        const double a = 0.25 * dt * dt, q2 = 2.0 / dt;
        if (op == SMG_WAVE_ADJ_INJECT) {
            std::vector<int> gv, gp, gl;
            wave_group_receivers(nV, n_idx, idx, kn, gv, gp, gl);
            std::copy(x0, x0 + nk, out);
            wave_adj_host_inject(nV, k, (int)gv.size(), gv.data(), gp.data(), gl.data(), x1, out);
            return SMG_OK;
        }
        if (op == SMG_WAVE_ADJ_RHS) {
            wave_adj_host_rhs(nV, k, kn, q2, x0, x1, out, out + nk);
            out[2 * nk] = flow_host_sum(out + nk, (int)nk);
            return SMG_OK;
        }
        if (op == SMG_WAVE_ADJ_SIGNAL) {
            const size_t sk = (size_t)n_idx * kk;
            std::copy(x1, x1 + sk, out);
            std::copy(x2, x2 + sk, out + sk);
            wave_adj_host_signal(nV, k, n_idx, idx, a, x0, out, out + sk);
            return SMG_OK;
        }
        std::vector<int> mp, mi;
        vertex_corner_lists(std::vector<int>(F, F + 3 * f), nV, mp, mi);
        std::vector<double> A(f), m(n), mt(n), s2(n), fac(n);
        fluid_host_mass(nV, nF, F, V, mp.data(), mi.data(), A.data(), m.data());
        wave_host_planes(nV, m.data(), speed, sigma, dt, mt.data(), s2.data());
        if (op == SMG_WAVE_ADJ_KEEP) {
            wave_adj_host_keep(nV, k, s2.data(), dt, x0, x1, x2, out);
        } else if (op == SMG_WAVE_ADJ_ADVANCE) {
            std::copy(x1, x1 + nk, out);
            std::copy(x2, x2 + nk, out + nk);
            std::copy(x4, x4 + nk, out + 2 * nk);
            wave_adj_host_advance(nV, k, mt.data(), s2.data(), dt, q2, x0, x3, out, out + nk, out + 2 * nk);
        } else {
            wave_adj_host_planes(nV, mt.data(), speed, fac.data());
            wave_adj_host_scale(nV, k, fac.data(), x0, out);
        }
        return SMG_OK;
    });
}
