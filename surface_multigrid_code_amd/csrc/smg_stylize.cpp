// smg_stylize.cpp -- cubic and normal-driven stylization on the V-cycle (include/smg.h: smg_stylize_*): as-rigid-as-possible
// deformation with a penalty on each vertex's rotated normal.  The global step is smg_arap's: one handle built from the caller's prolongations
// and precomputed with -L of the rest pose, the pins known; the CSR of L on the device, k_arap_rhs, one warm-started 3-column solve.  The local
// step is k_stylize_local (smg_stylize_device.hip): per vertex an ADMM loop of closest-rotation fits in registers, its state (7 doubles per
// vertex) kept in HBM between the outer iterations of one call, or one fit against the caller's target normals.
// One iteration: rotations + energy terms + iteration counts, the energy (fixed-order reduction), the right-hand side, the solve, the new
// iterate as xyz rows.  All of it is enqueued on the object's stream, which the handle uses too; per iteration the host reads one energy double
// beside the solve's own history.  Checks, stream, handle, the cotangent system and the inner solve: smg_mesh_object.hpp; the loop and its
// stopping rule: smg_local_global.hpp; the energy's sum: launch_fixed_sum.
#include <hip/hip_runtime_api.h>

#include <cmath>
#include <memory>
#include <vector>

#include "smg_device.hpp"
#include "smg_local_global.hpp"
#include "smg_mesh.hpp"
#include "smg_mesh_object.hpp"
#include "smg_stylize_inl.hpp"

using namespace smg;

struct smg_stylize : MeshObject {         // handle[0]: -L of the rest pose, the pins known
    int nV = 0, nh = 0;
    int pcg = 1;                          // the inner solver: 1 smg_solve_pcg, 0 smg_solve
    double scale = 0.0;                   // smg_arap's s: the default inner tolerance is 1e-8 s
    smg_stylize_params p;
    StyFrame Q = {{1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0}};
    bool ran = false;                     // iters holds the counts of a local step
    std::vector<double> pin_rest;         // the rest positions of the pins, nh x 3 column-major: pin_pos == NULL
    DevBuf<int> rowptr, col, pins, iters; // the CSR pattern of L, the pins in the caller's order, the ADMM iterations of the last local step
    DevBuf<double> w, P0, nrm, area;      // the values of L, rest positions and normals (xyz rows), vertex areas
    DevBuf<double> lam, tgt;              // per-vertex lambda / target normals (xyz rows): allocated while set
    DevBuf<double> state;                 // z, u, rho: 7 planes of nV
    DevBuf<double> P, R, eterm, part, E;  // current positions (xyz rows), rotations (9 per vertex), energy terms, their chunk sums, E_t
    DevBuf<double> B, Ua, Ub, hp;         // column-major n x 3: right-hand side, the iterate and the solve's result; pin positions (nh x 3)
    ~smg_stylize() { quiesce(); }
};

namespace smg {

StyParams sty_params(const smg_stylize_params& p) { return StyParams{p.lambda, p.rho0, p.abs_tol, p.rel_tol, p.mu, p.tau, p.admm_iters}; }

const char* stylize_bad_params(const smg_stylize_params& p)
{
    auto positive = [](double x) { return std::isfinite(x) && x > 0.0; };
    if (!std::isfinite(p.lambda) || p.lambda < 0.0) return "lambda must be finite and >= 0";
    if (!positive(p.rho0)) return "rho0 must be finite and > 0";
    if (!positive(p.abs_tol)) return "abs_tol must be finite and > 0";
    if (!positive(p.rel_tol)) return "rel_tol must be finite and > 0";
    if (!std::isfinite(p.mu) || !(p.mu > 1.0)) return "mu must be finite and > 1";
    if (!std::isfinite(p.tau) || !(p.tau > 1.0)) return "tau must be finite and > 1";
    if (p.admm_iters < 1) return "admm_iters must be >= 1";
    return nullptr;
}

int stylize_check_lambda(const char* who, const double* lam, int n)
{
    for (int i = 0; i < n; i++)
        if (!std::isfinite(lam[i]) || lam[i] < 0.0) return fail(SMG_ERR_INVALID, "%s: lambda[%d] must be finite and >= 0", who, i);
    return SMG_OK;
}

int stylize_check_frame(const char* who, const double* Q)
{
    for (int a = 0; a < 3; a++)
        for (int b = 0; b < 3; b++) {
            const double g = Q[a] * Q[b] + Q[3 + a] * Q[3 + b] + Q[6 + a] * Q[6 + b];
            if (!(std::fabs(g - (a == b ? 1.0 : 0.0)) <= 1e-12)) return fail(SMG_ERR_INVALID, "%s: the frame is not orthonormal to 1e-12", who);
        }
    const double det = Q[0] * (Q[4] * Q[8] - Q[5] * Q[7]) - Q[1] * (Q[3] * Q[8] - Q[5] * Q[6]) + Q[2] * (Q[3] * Q[7] - Q[4] * Q[6]);
    if (!(det > 0.0)) return fail(SMG_ERR_INVALID, "%s: the frame is a reflection (det < 0)", who);
    return SMG_OK;
}

int stylize_check_targets(const char* who, const double* T, int n)
{
    for (int i = 0; i < n; i++) {
        const double* t = T + 3 * (size_t)i;
        if (!(std::fabs(std::sqrt(t[0] * t[0] + t[1] * t[1] + t[2] * t[2]) - 1.0) <= 1e-8))
            return fail(SMG_ERR_INVALID, "%s: target %d is not a finite unit vector (to 1e-8)", who, i);
    }
    return SMG_OK;
}

int stylize_check_operands(const char* who, int op, int nV, int nF, const int* F, const int* rowptr, const int* col, const double* w, const double* V0,
                           const double* P, const double* lam, const double* Q, const double* targets, const double* R_in,
                           const smg_stylize_params* p, const double* out, const int* iters)
{
    if (op < SMG_STY_NORMALS || op > SMG_STY_ENERGY || nV < 1 || nF < 1 || !F || !rowptr || !col || !w || !V0 || !p || !out)
        return fail(SMG_ERR_INVALID, "%s: bad arguments", who);
    const bool local = op >= SMG_STY_ADMM_ONE && op <= SMG_STY_LOCAL_TARGETS;
    if ((op != SMG_STY_NORMALS && !P) || (local && !iters) || (op == SMG_STY_LOCAL_TARGETS && !targets) || (op == SMG_STY_ENERGY && !R_in))
        return fail(SMG_ERR_INVALID, "%s: op %d misses an operand", who, op);
    if (const char* why = stylize_bad_params(*p)) return fail(SMG_ERR_INVALID, "%s: %s", who, why);
    if (int rc = check_faces(who, F, nF, nV)) return rc;
    if (rowptr[0] != 0) return fail(SMG_ERR_INVALID, "%s: rowptr[0] != 0", who);
    if (const char* why = check_compressed(nV, nV, rowptr, col)) return fail(SMG_ERR_INVALID, "%s: %s", who, why);
    if (lam) if (int rc = stylize_check_lambda(who, lam, nV)) return rc;
    if (Q) if (int rc = stylize_check_frame(who, Q)) return rc;
    if (targets) if (int rc = stylize_check_targets(who, targets, nV)) return rc;
    return SMG_OK;
}

}  // namespace smg

namespace {

int create_impl(const smg_hierarchy* h, const double* V, int nV, const int* F, int nF, const int* pins, int n_pins, const smg_stylize_params* pp,
                smg_stylize** out)
{
    if (out) *out = nullptr;
    const char* who = "smg_stylize_create";
    if (!h || !V || !F || !pins || !pp || !out || nV <= 0 || nF <= 0) return fail(SMG_ERR_INVALID, "%s: bad arguments", who);
    if (int rc = check_hierarchy(who, h, 1, nV)) return rc;
    if (int rc = check_mesh(who, V, nV, F, nF, true)) return rc;
    if (n_pins < 1) return fail(SMG_ERR_INVALID, "%s: n_pins = %d, at least one pinned vertex is needed", who, n_pins);
    {
        std::vector<char> seen((size_t)nV, 0);
        for (int r = 0; r < n_pins; r++) {
            if (pins[r] < 0 || pins[r] >= nV) return fail(SMG_ERR_INVALID, "%s: pin %d out of range", who, pins[r]);
            if (seen[pins[r]]) return fail(SMG_ERR_INVALID, "%s: pin %d is repeated", who, pins[r]);
            seen[pins[r]] = 1;
        }
    }
    if (n_pins >= nV) return fail(SMG_ERR_INVALID, "%s: every vertex is pinned: nothing to solve", who);
    if (const char* why = stylize_bad_params(*pp)) return fail(SMG_ERR_INVALID, "%s: %s", who, why);

    std::unique_ptr<smg_stylize> s(new smg_stylize());
    s->nV = nV; s->nh = n_pins; s->p = *pp;
    if (int rc = s->open(who)) return rc;
    if (int rc = s->clone(who, h, 0)) return rc;
    hipStream_t st = s->stream;

    // L of the rest pose on the device: its values stay there as the weights, their negatives are the system (smg_arap's create)
    HIPCHK(s->P0.upload(std::vector<double>(V, V + (size_t)nV * 3)));
    CotanSystem S;
    if (int rc = cotan_system(F, nF, nV, s->P0.p, 0, 0.0, -1.0, st, S, false, &s->w)) return rc;
    double ss = 0.0;
    for (int i = 0; i < nV; i++) {
        double row = 0.0;
        for (int q = S.ptr[i]; q < S.ptr[i + 1]; q++) {
            const int j = S.col[q];
            if (j == i) continue;
            const double ex = V[3 * (size_t)i] - V[3 * (size_t)j], ey = V[3 * (size_t)i + 1] - V[3 * (size_t)j + 1], ez = V[3 * (size_t)i + 2] - V[3 * (size_t)j + 2];
            row += std::fabs(S.L[q]) * std::sqrt(ex * ex + ey * ey + ez * ez);
        }
        ss += row * row;
    }
    s->scale = std::sqrt(ss);
    for (double& v : S.L) v = -v;
    if (int rc = smg_precompute(s->handle[0], nV, S.ptr.data(), S.col.data(), S.L.data(), pins, n_pins)) return rc;

    HIPCHK(s->rowptr.upload(S.ptr));
    HIPCHK(s->col.upload(S.col));
    HIPCHK(s->pins.upload(std::vector<int>(pins, pins + n_pins)));
    s->pin_rest.resize(3 * (size_t)n_pins);
    for (int r = 0; r < n_pins; r++)
        for (int c = 0; c < 3; c++) s->pin_rest[(size_t)c * n_pins + r] = V[3 * (size_t)pins[r] + c];
    const size_t n = (size_t)nV;
    HIPCHK(s->nrm.alloc(3 * n));
    HIPCHK(s->area.alloc(n));
    HIPCHK(s->iters.alloc(n));
    HIPCHK(s->state.alloc(STY_STATE * n));
    HIPCHK(s->P.alloc(3 * n));
    HIPCHK(s->R.alloc(9 * n));
    HIPCHK(s->eterm.alloc(n));
    HIPCHK(s->part.alloc((size_t)fixed_sum_groups(nV)));
    HIPCHK(s->B.alloc(3 * n));
    HIPCHK(s->Ua.alloc(3 * n));
    HIPCHK(s->Ub.alloc(3 * n));
    HIPCHK(s->hp.alloc(3 * (size_t)n_pins));
    {   // n_i, a_i once; the faces and the corner lists are needed for nothing else
        DevBuf<int> dF, dmp, dmi;
        if (int rc = upload_faces(F, nF, nV, dF, dmp, dmi)) return rc;
        HIPCHK(launch_stylize_normals(nV, dF.p, dmp.p, dmi.p, s->P0.p, s->nrm.p, s->area.p, st));
        HIPCHK(hipStreamSynchronize(st));
    }
    *out = s.release();
    return SMG_OK;
}

int run_impl(smg_stylize* s, const double* pin_pos, int ld_pp, const double* U0, int ld_u0, int memspace, int max_iter, double rel_tol,
             const smg_solve_opts* opts, double* U, int ld_u, double* energy_his, int* cycles, int* n_iter)
{
    if (!s || !U || bad_memspace(memspace) || max_iter < 0 || !(rel_tol >= 0.0) || !std::isfinite(rel_tol))
        return fail(SMG_ERR_INVALID, "smg_stylize_run: bad arguments");
    const int n = s->nV, nh = s->nh;
    if ((pin_pos && ld_pp < nh) || ld_u < n || (U0 && ld_u0 < n)) return fail(SMG_ERR_INVALID, "smg_stylize_run: a leading dimension is too small");
    DeviceScope dsc(s->device);
    hipStream_t st = s->stream;
    const smg_solve_opts so = opts_or_default(opts, 1e-8 * s->scale, 50);
    HIPCHK(s->E.ensure((size_t)max_iter + 1));
    int t_end = 0;
    if (!n_iter) n_iter = &t_end;
    *n_iter = 0;

    // the start: U0 or the rest pose, the pinned rows from pin_pos; as the solve's column-major block (Ua) and as xyz rows (P)
    if (pin_pos) HIPCHK(copy_columns(s->hp.p, nh, pin_pos, ld_pp, nh, 3, copy_in(memspace), st));
    else HIPCHK(hipMemcpyAsync(s->hp.p, s->pin_rest.data(), 3 * (size_t)nh * sizeof(double), hipMemcpyHostToDevice, st));
    if (U0) HIPCHK(copy_columns(s->Ua.p, n, U0, ld_u0, n, 3, copy_in(memspace), st));
    else HIPCHK(launch_arap_columns(n, s->P0.p, s->Ua.p, n, st));
    HIPCHK(launch_arap_set_handles(nh, s->pins.p, s->hp.p, nh, s->Ua.p, n, st));
    HIPCHK(launch_arap_rows(n, s->Ua.p, n, s->P.p, st));

    const StyParams p = sty_params(s->p);
    const double* lam = s->lam.p;     // null while no per-vertex weights are set
    const double* tgt = s->tgt.p;     // null: the cubic mode
    // local step: R_t from U_t (iteration 0 from the start state), E_t = E(R_t, U_t); the right-hand side is enqueued ahead of the host's look at E_t
    auto local = [&](int t, bool with_rhs, double* E_t) -> int {
        if (tgt) HIPCHK(launch_stylize_targets(n, s->rowptr.p, s->col.p, s->w.p, s->P0.p, s->P.p, s->nrm.p, s->area.p, lam, tgt, p, s->R.p, s->eterm.p, s->iters.p, st));
        else HIPCHK(launch_stylize_cubic(n, s->rowptr.p, s->col.p, s->w.p, s->P0.p, s->P.p, s->nrm.p, s->area.p, lam, s->Q, p, t == 0, s->state.p, s->R.p, s->eterm.p, s->iters.p, st));
        s->ran = true;
        HIPCHK(launch_fixed_sum(s->eterm.p, n, s->part.p, s->E.p + t, st));
        HIPCHK(hipMemcpyAsync(E_t, s->E.p + t, sizeof(double), hipMemcpyDeviceToHost, st));
        if (with_rhs) HIPCHK(launch_arap_rhs(n, s->rowptr.p, s->col.p, s->w.p, s->P0.p, s->R.p, s->B.p, n, st));
        HIPCHK(hipStreamSynchronize(st));
        return SMG_OK;
    };
    // global step: (-L) U_{t+1} = b, pinned rows known, from U_t
    auto global = [&](int, int* entries) -> int {
        if (int rc = inner_solve(s->handle[0], s->pcg, s->B.p, n, s->hp.p, nh, s->Ua.p, n, 3, so, s->Ub.p, n, entries)) return rc;
        std::swap(s->Ua, s->Ub);
        HIPCHK(launch_arap_rows(n, s->Ua.p, n, s->P.p, st));
        return SMG_OK;
    };
    const int rc = local_global(max_iter, rel_tol, local, global, energy_his, cycles, n_iter);
    if (rc == LOCAL_GLOBAL_NONFINITE) return fail(SMG_ERR_NONFINITE, "smg_stylize_run: non-finite energy at iteration %d", *n_iter);
    if (rc) return rc;
    HIPCHK(copy_columns(U, ld_u, s->Ua.p, n, n, 3, copy_out(memspace), st));
    HIPCHK(hipStreamSynchronize(st));
    return SMG_OK;
}

// v (count doubles on the host, checked by the caller) into buf, or buf released when v is null
int set_array(smg_stylize* s, DevBuf<double>& buf, const double* v, size_t count)
{
    DeviceScope dsc(s->device);
    HIPCHK(hipStreamSynchronize(s->stream));
    if (!v) { buf.release(); return SMG_OK; }
    HIPCHK(buf.ensure(count));
    HIPCHK(hipMemcpy(buf.p, v, count * sizeof(double), hipMemcpyHostToDevice));
    return SMG_OK;
}

}  // namespace

extern "C" void smg_stylize_params_default(smg_stylize_params* p)
{
    if (!p) return;
    p->lambda = 0.2; p->rho0 = 1e-4; p->abs_tol = 1e-5; p->rel_tol = 1e-3; p->mu = 10.0; p->tau = 2.0; p->admm_iters = 100;
}

extern "C" int smg_stylize_create(const smg_hierarchy* h, const double* V, int nV, const int* F, int nF, const int* pins, int n_pins,
                                  const smg_stylize_params* p, smg_stylize** out)
{
    return guarded("smg_stylize_create", [&]() { return create_impl(h, V, nV, F, nF, pins, n_pins, p, out); });
}

extern "C" void smg_stylize_destroy(smg_stylize* s) { delete s; }

extern "C" long long smg_stylize_device_bytes(const smg_stylize* s)
{
    if (!s) return 0;   // one list: every DevBuf of the struct
    return device_bytes(*s, s->rowptr, s->col, s->pins, s->iters, s->w, s->P0, s->nrm, s->area, s->lam, s->tgt, s->state, s->P, s->R, s->eterm, s->part,
                        s->E, s->B, s->Ua, s->Ub, s->hp);
}

extern "C" int smg_stylize_set_solver(smg_stylize* s, int pcg)
{
    if (!s) return fail(SMG_ERR_INVALID, "null stylize object");
    latch_solver(s->pcg, pcg);
    return SMG_OK;
}

extern "C" int smg_stylize_set_params(smg_stylize* s, const smg_stylize_params* p)
{
    if (!s || !p) return fail(SMG_ERR_INVALID, "smg_stylize_set_params: bad arguments");
    if (const char* why = stylize_bad_params(*p)) return fail(SMG_ERR_INVALID, "smg_stylize_set_params: %s", why);
    s->p = *p;
    return SMG_OK;
}

extern "C" int smg_stylize_set_lambda(smg_stylize* s, const double* lambda)
{
    return guarded("smg_stylize_set_lambda", [&]() -> int {
        if (!s) return fail(SMG_ERR_INVALID, "smg_stylize_set_lambda: null object");
        if (lambda) if (int rc = stylize_check_lambda("smg_stylize_set_lambda", lambda, s->nV)) return rc;
        return set_array(s, s->lam, lambda, (size_t)s->nV);
    });
}

extern "C" int smg_stylize_set_frame(smg_stylize* s, const double* Q)
{
    if (!s) return fail(SMG_ERR_INVALID, "smg_stylize_set_frame: null object");
    if (Q) if (int rc = stylize_check_frame("smg_stylize_set_frame", Q)) return rc;
    for (int e = 0; e < 9; e++) s->Q.q[e] = Q ? Q[e] : (e % 4 == 0 ? 1.0 : 0.0);
    return SMG_OK;
}

extern "C" int smg_stylize_set_targets(smg_stylize* s, const double* targets)
{
    return guarded("smg_stylize_set_targets", [&]() -> int {
        if (!s) return fail(SMG_ERR_INVALID, "smg_stylize_set_targets: null object");
        if (targets) if (int rc = stylize_check_targets("smg_stylize_set_targets", targets, s->nV)) return rc;
        return set_array(s, s->tgt, targets, 3 * (size_t)s->nV);
    });
}

extern "C" int smg_stylize_normals(smg_stylize* s, double* normals, double* areas)
{
    return guarded("smg_stylize_normals", [&]() -> int {
        if (!s) return fail(SMG_ERR_INVALID, "smg_stylize_normals: null object");
        DeviceScope dsc(s->device);
        HIPCHK(hipStreamSynchronize(s->stream));
        if (normals) HIPCHK(hipMemcpy(normals, s->nrm.p, 3 * (size_t)s->nV * sizeof(double), hipMemcpyDeviceToHost));
        if (areas) HIPCHK(hipMemcpy(areas, s->area.p, (size_t)s->nV * sizeof(double), hipMemcpyDeviceToHost));
        return SMG_OK;
    });
}

extern "C" int smg_stylize_run(smg_stylize* s, const double* pin_pos, int ld_pp, const double* U0, int ld_u0, int memspace, int max_iter,
                               double rel_tol, const smg_solve_opts* opts, double* U, int ld_u, double* energy_his, int* cycles, int* n_iter)
{
    return guarded("smg_stylize_run", [&]() {
        return run_impl(s, pin_pos, ld_pp, U0, ld_u0, memspace, max_iter, rel_tol, opts, U, ld_u, energy_his, cycles, n_iter);
    });
}

extern "C" int smg_stylize_admm_stats(smg_stylize* s, int* min_iters, double* mean_iters, int* max_iters, int* at_cap, int* iters)
{
    return guarded("smg_stylize_admm_stats", [&]() -> int {
        if (!s) return fail(SMG_ERR_INVALID, "smg_stylize_admm_stats: null object");
        if (!s->ran) return fail(SMG_ERR_INVALID, "smg_stylize_admm_stats: no local step has run yet");
        DeviceScope dsc(s->device);
        HIPCHK(hipStreamSynchronize(s->stream));
        std::vector<int> it((size_t)s->nV);
        HIPCHK(hipMemcpy(it.data(), s->iters.p, it.size() * sizeof(int), hipMemcpyDeviceToHost));
        int lo = it[0], hi = it[0], cap = 0;
        long long sum = 0;
        for (int v : it) { lo = v < lo ? v : lo; hi = v > hi ? v : hi; sum += v; cap += v >= s->p.admm_iters ? 1 : 0; }
        if (min_iters) *min_iters = lo;
        if (max_iters) *max_iters = hi;
        if (mean_iters) *mean_iters = (double)sum / (double)s->nV;
        if (at_cap) *at_cap = cap;
        if (iters) for (size_t i = 0; i < it.size(); i++) iters[i] = it[i];
        return SMG_OK;
    });
}

extern "C" int smg_stylize_local_host(int op, int nV, int nF, const int* F, const int* rowptr, const int* col, const double* w, const double* V0,
                                      const double* P, const double* lambda, const double* Q, const double* targets, const double* state_in,
                                      const double* R_in, const smg_stylize_params* p, double* out, int* iters)
{
    return guarded("smg_stylize_local_host", [&]() -> int {
        const char* who = "smg_stylize_local_host";
        if (int rc = stylize_check_operands(who, op, nV, nF, F, rowptr, col, w, V0, P, lambda, Q, targets, R_in, p, out, iters)) return rc;
        std::vector<int> mp, mi;
        vertex_corner_lists(std::vector<int>(F, F + 3 * (size_t)nF), nV, mp, mi);
        StyFrame fr = {{1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0}};
        if (Q) for (int e = 0; e < 9; e++) fr.q[e] = Q[e];
        sty_local_host(op, nV, F, mp.data(), mi.data(), rowptr, col, w, V0, P, lambda, fr, targets, state_in, R_in, sty_params(*p), out, iters);
        return SMG_OK;
    });
}
