// smg_pd.cpp -- projective-dynamics steps of a membrane with triangle-strain constraints on the scalar V-cycle (include/smg.h: smg_pd_*;
// DESIGN.md section 23; Bouaziz, Martin, Liu, Kavan, Pauly 2014).
// The object owns one handle built from the caller's prolongations and precomputed ONCE with (rho / h^2) M0 - k L of the rest pose (Voronoi
// mass, the pinned vertices known): the same matrix for x, y and z and for the life of the object.  On the device it keeps the faces, the
// corner lists of the vertices, the rest constants of every face (k_pd_rest), the rest mass, the state (x, v) and the buffers of a step.
// One step: the pressure force at the start pose (launch_membrane_pressure), the prediction s (k_pd_predict), the pin rows, q_0 = s; then the
// local / global alternation of smg_local_global.hpp.  One iteration: projections, face energy terms and corner shares (k_pd_faces), the
// right-hand side and the inertia terms (k_pd_vertices), the energy (one fixed-order reduction over nF + nV terms), one 3-column solve
// warm-started at the iterate.  All of it is enqueued on the object's stream, which the handle uses too; per iteration the host reads one
// energy double beside the solve's own history (at iteration 0, without options, also |b_0|_F^2).  Then v = (q - x) / h, x = q (k_pd_finish).
// Checks, stream, handle, the cotangent system and the inner solve: smg_mesh_object.hpp; the sums: launch_fixed_sum / launch_fixed_max.
#include <hip/hip_runtime_api.h>

#include <cmath>
#include <memory>
#include <vector>

#include "smg_device.hpp"
#include "smg_local_global.hpp"
#include "smg_mesh_object.hpp"
#include "smg_pd_inl.hpp"

using namespace smg;

struct smg_pd : MeshObject {              // handle[0]: (rho / h^2) M0 - k L of the rest pose, the pins known
    int nV = 0, nF = 0, np = 0;
    int pcg = 1;                          // the inner solver: 1 smg_solve_pcg, 0 smg_solve
    smg_pd_params p;
    double c_mass = 0.0;                  // rho / h^2, the coefficient of M0 in the matrix, in b and in E
    DevBuf<int> F, m_ptr, m_idx, pins;    // faces; the corner lists t = 3 f + i of every vertex, faces ascending; the pinned vertices
    DevBuf<double> V0, rest, m0;          // rest positions (xyz rows), rest constants (4 planes), Voronoi mass of the rest pose
    DevBuf<double> x, vel, fext, Qn;      // the state (xyz rows), the pressure force at the start pose, its scratch (6 planes)
    DevBuf<double> hp, hpN, hrow;         // pin positions (np x 3 column-major): current, of the call; the caller's rows
    DevBuf<double> S, B, Ua, Ub;          // column-major nV x 3: prediction, right-hand side, the iterate and the solve's result
    DevBuf<double> share, terms, part, E; // corner shares (9 planes), the terms nF faces + nV vertices + nV |b_v|^2, chunk sums, E_t and |b_0|^2
    DevBuf<double> Fg, sigma, T, sterms, stats;   // the strain query: planes (6, 2, 6), the statistics' terms (5 planes), their reductions (5)
    ~smg_pd() { quiesce(); }
};

namespace {

const char* bad_params(const smg_pd_params& p)
{
    auto positive = [](double x) { return std::isfinite(x) && x > 0.0; };
    if (!positive(p.dt)) return "dt must be finite and > 0";
    if (!positive(p.density)) return "density must be finite and > 0";
    if (!positive(p.stiffness)) return "stiffness must be finite and > 0";
    return nullptr;
}

const char* bad_band(double smin, double smax)
{
    if (!std::isfinite(smin) || !std::isfinite(smax) || !(0.0 <= smin && smin <= smax)) return "the strain limits must be finite with 0 <= sigma_min <= sigma_max";
    return nullptr;
}

const char* bad_forces(double pressure, const double* g)
{
    if (!std::isfinite(pressure)) return "pressure must be finite";
    if (g && !(std::isfinite(g[0]) && std::isfinite(g[1]) && std::isfinite(g[2]))) return "gravity must be finite";
    return nullptr;
}

int create_impl(const smg_hierarchy* h, const double* V, int nV, const int* F, int nF, const int* pins, int n_pins, const smg_pd_params* pp, smg_pd** out)
{
    if (out) *out = nullptr;
    const char* who = "smg_pd_create";
    if (!h || !V || !F || !pp || !out || nV <= 0 || nF <= 0 || n_pins < 0 || (n_pins > 0 && !pins)) return fail(SMG_ERR_INVALID, "%s: bad arguments", who);
    if (int rc = check_hierarchy(who, h, 1, nV)) return rc;
    if (int rc = check_mesh(who, V, nV, F, nF, true)) return rc;
    if (const char* why = bad_params(*pp)) return fail(SMG_ERR_INVALID, "%s: %s", who, why);
    if (const char* why = bad_band(pp->sigma_min, pp->sigma_max)) return fail(SMG_ERR_INVALID, "%s: %s", who, why);
    if (const char* why = bad_forces(pp->pressure, pp->gravity)) return fail(SMG_ERR_INVALID, "%s: %s", who, why);
    {
        std::vector<char> seen((size_t)nV, 0);
        for (int r = 0; r < n_pins; r++) {
            if (pins[r] < 0 || pins[r] >= nV) return fail(SMG_ERR_INVALID, "%s: pin %d out of range", who, pins[r]);
            if (seen[pins[r]]) return fail(SMG_ERR_INVALID, "%s: pin %d is repeated", who, pins[r]);
            seen[pins[r]] = 1;
        }
    }
    if (n_pins >= nV) return fail(SMG_ERR_INVALID, "%s: every vertex is pinned: nothing to solve", who);

    std::unique_ptr<smg_pd> d(new smg_pd());
    d->nV = nV; d->nF = nF; d->np = n_pins; d->p = *pp;
    d->c_mass = pp->density / (pp->dt * pp->dt);
    if (int rc = d->open(who)) return rc;
    if (int rc = d->clone(who, h, 0)) return rc;
    hipStream_t st = d->stream;

    // the one matrix of the object: c_mass M0 - k L, assembled on the device, precomputed with the pins known
    HIPCHK(d->V0.upload(std::vector<double>(V, V + 3 * (size_t)nV)));
    CotanSystem S;
    if (int rc = cotan_system(F, nF, nV, d->V0.p, 1, d->c_mass, -pp->stiffness, st, S, true)) return rc;
    if (int rc = smg_precompute(d->handle[0], nV, S.ptr.data(), S.col.data(), S.val.data(), n_pins ? pins : nullptr, n_pins)) return rc;

    if (int rc = upload_faces(F, nF, nV, d->F, d->m_ptr, d->m_idx)) return rc;
    const size_t n = (size_t)nV, nf = (size_t)nF, npn = (size_t)std::max(n_pins, 1);
    HIPCHK(d->pins.upload(n_pins ? std::vector<int>(pins, pins + n_pins) : std::vector<int>(1, 0)));
    HIPCHK(d->rest.alloc(4 * nf));
    HIPCHK(d->m0.alloc(n));
    HIPCHK(d->Qn.alloc(6 * nf));
    for (DevBuf<double>* b : {&d->x, &d->vel, &d->fext, &d->S, &d->B, &d->Ua, &d->Ub}) HIPCHK(b->alloc(3 * n));
    for (DevBuf<double>* b : {&d->hp, &d->hpN, &d->hrow}) HIPCHK(b->alloc(3 * npn));
    HIPCHK(d->share.alloc(9 * nf));
    HIPCHK(d->terms.alloc(nf + 2 * n));
    HIPCHK(d->part.alloc((size_t)fixed_sum_groups(nF + nV)));
    HIPCHK(d->Fg.alloc(6 * nf));
    HIPCHK(d->sigma.alloc(2 * nf));
    HIPCHK(d->T.alloc(6 * nf));
    HIPCHK(d->sterms.alloc(5 * nf));
    HIPCHK(d->stats.alloc(5));

    // the rest constants; the rest mass by the expressions the assembler's diagonal is summed from (k_face_terms, k_mass_diag), in its order
    HIPCHK(launch_pd_rest(nF, d->F.p, d->V0.p, d->rest.p, st));
    HIPCHK(launch_membrane_pressure(nV, nF, d->F.p, d->V0.p, d->m_ptr.p, d->m_idx.p, 0.0, d->Qn.p, d->m0.p, nullptr, st));
    // the state starts as (V, 0), the pins at their rest positions
    HIPCHK(hipMemcpyAsync(d->x.p, d->V0.p, 3 * n * sizeof(double), hipMemcpyDeviceToDevice, st));
    HIPCHK(hipMemsetAsync(d->vel.p, 0, 3 * n * sizeof(double), st));
    std::vector<double> rows(3 * (size_t)n_pins);       // alive until the stream is synchronised below
    if (n_pins) {
        for (int r = 0; r < n_pins; r++)
            for (int l = 0; l < 3; l++) rows[3 * (size_t)r + l] = V[3 * (size_t)pins[r] + l];
        HIPCHK(hipMemcpyAsync(d->hrow.p, rows.data(), rows.size() * sizeof(double), hipMemcpyHostToDevice, st));
        HIPCHK(launch_arap_columns(n_pins, d->hrow.p, d->hp.p, n_pins, st));
    }
    HIPCHK(hipStreamSynchronize(st));
    *out = d.release();
    return SMG_OK;
}

int step_impl(smg_pd* d, const double* pin_pos, int memspace, int max_iter, double rel_tol, const smg_solve_opts* opts, double* energy_his, int* cycles,
              int* n_iter)
{
    if (n_iter) *n_iter = 0;
    if (!d || bad_memspace(memspace) || max_iter < 0 || !(rel_tol >= 0.0) || !std::isfinite(rel_tol)) return fail(SMG_ERR_INVALID, "smg_pd_step: bad arguments");
    DeviceScope dsc(d->device);
    hipStream_t st = d->stream;
    const smg_pd_params& p = d->p;
    const int n = d->nV, nF = d->nF, np = d->np;
    HIPCHK(d->E.ensure((size_t)max_iter + 2));
    double* bsum = d->E.p + max_iter + 1;
    int t_end = 0;
    if (!n_iter) n_iter = &t_end;

    // the pins of this call; they become the object's only when the step succeeds
    const double* hp = d->hp.p;
    if (pin_pos && np) {
        HIPCHK(hipMemcpyAsync(d->hrow.p, pin_pos, 3 * (size_t)np * sizeof(double), copy_in(memspace), st));
        HIPCHK(launch_arap_columns(np, d->hrow.p, d->hpN.p, np, st));
        hp = d->hpN.p;
    }
    // forces at the start pose, the prediction, the pin rows, q_0 = s
    HIPCHK(launch_membrane_pressure(n, nF, d->F.p, d->x.p, d->m_ptr.p, d->m_idx.p, p.pressure, d->Qn.p, nullptr, d->fext.p, st));
    HIPCHK(launch_pd_predict(n, d->x.p, d->vel.p, d->fext.p, d->m0.p, p.dt, p.density, p.gravity, d->S.p, n, st));
    HIPCHK(launch_arap_set_handles(np, d->pins.p, hp, np, d->S.p, n, st));
    HIPCHK(hipMemcpyAsync(d->Ua.p, d->S.p, 3 * (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, st));

    smg_solve_opts so = opts_or_default(opts, 0.0, 50);
    double* terms = d->terms.p;
    // local step: T_t from q_t, E_t; the right-hand side is a by-product of the same two launches
    auto local = [&](int t, bool, double* E_t) -> int {
        HIPCHK(launch_pd_faces(nF, d->F.p, d->rest.p, d->Ua.p, 1, (size_t)n, p.stiffness, p.sigma_min, p.sigma_max, terms, d->share.p, nullptr, nullptr,
                               nullptr, st));
        HIPCHK(launch_pd_vertices(n, nF, d->m_ptr.p, d->m_idx.p, d->share.p, d->m0.p, d->c_mass, d->S.p, d->Ua.p, n, d->B.p, n, terms + nF, terms + nF + n, st));
        HIPCHK(launch_fixed_sum(terms, nF + n, d->part.p, d->E.p + t, st));
        HIPCHK(hipMemcpyAsync(E_t, d->E.p + t, sizeof(double), hipMemcpyDeviceToHost, st));
        double b2 = 0.0;
        if (t == 0 && !opts) {      // the default tolerance of this step's solves: 1e-8 |b_0|_F
            HIPCHK(launch_fixed_sum(terms + nF + n, n, d->part.p, bsum, st));
            HIPCHK(hipMemcpyAsync(&b2, bsum, sizeof(double), hipMemcpyDeviceToHost, st));
        }
        HIPCHK(hipStreamSynchronize(st));
        if (t == 0 && !opts) so.tol = 1e-8 * std::sqrt(b2);
        return SMG_OK;
    };
    // global step: ((rho / h^2) M0 - k L) q_{t+1} = b, pin rows known, from q_t
    auto global = [&](int, int* entries) -> int {
        if (int rc = inner_solve(d->handle[0], d->pcg, d->B.p, n, np ? hp : nullptr, np, d->Ua.p, n, 3, so, d->Ub.p, n, entries)) return rc;
        std::swap(d->Ua, d->Ub);
        return SMG_OK;
    };
    const int rc = local_global(max_iter, rel_tol, local, global, energy_his, cycles, n_iter);
    if (rc == LOCAL_GLOBAL_NONFINITE) {
        HIPCHK(hipStreamSynchronize(st));
        return fail(SMG_ERR_NONFINITE, "smg_pd_step: non-finite energy at iteration %d", *n_iter);
    }
    if (rc) return rc;
    HIPCHK(launch_pd_finish(n, d->Ua.p, n, p.dt, d->x.p, d->vel.p, st));
    HIPCHK(hipStreamSynchronize(st));
    if (hp == d->hpN.p) std::swap(d->hp, d->hpN);
    return SMG_OK;
}

int state_impl(smg_pd* d, double* pos, double* vel, const double* pos_in, const double* vel_in, int memspace, bool set)
{
    if (!d || bad_memspace(memspace)) return fail(SMG_ERR_INVALID, "smg_pd_%s_state: bad arguments", set ? "set" : "get");
    DeviceScope dsc(d->device);
    hipStream_t st = d->stream;
    const size_t vec = 3 * (size_t)d->nV * sizeof(double);
    if (set) {
        if (pos_in) HIPCHK(hipMemcpyAsync(d->x.p, pos_in, vec, copy_in(memspace), st));
        if (vel_in) HIPCHK(hipMemcpyAsync(d->vel.p, vel_in, vec, copy_in(memspace), st));
    } else {
        if (pos) HIPCHK(hipMemcpyAsync(pos, d->x.p, vec, copy_out(memspace), st));
        if (vel) HIPCHK(hipMemcpyAsync(vel, d->vel.p, vec, copy_out(memspace), st));
    }
    HIPCHK(hipStreamSynchronize(st));
    return SMG_OK;
}

int strain_impl(smg_pd* d, int memspace, double* sigma, double* stats)
{
    if (!d || !stats || bad_memspace(memspace)) return fail(SMG_ERR_INVALID, "smg_pd_strain: bad arguments");
    DeviceScope dsc(d->device);
    hipStream_t st = d->stream;
    const smg_pd_params& p = d->p;
    const int nF = d->nF;
    const size_t nf = (size_t)nF;
    // the state through the step's own face buffers: no iteration is in flight between two calls
    HIPCHK(launch_pd_faces(nF, d->F.p, d->rest.p, d->x.p, 3, 1, p.stiffness, p.sigma_min, p.sigma_max, d->terms.p, d->share.p, d->Fg.p, d->sigma.p, d->T.p, st));
    HIPCHK(launch_pd_strain_terms(nF, d->rest.p, d->Fg.p, d->sigma.p, d->T.p, p.sigma_min, p.sigma_max, d->sterms.p, st));
    HIPCHK(launch_fixed_max(d->sterms.p, nF, d->part.p, d->stats.p, st));
    HIPCHK(launch_fixed_max(d->sterms.p + nf, nF, d->part.p, d->stats.p + 1, st));
    for (int e = 2; e < 5; e++) HIPCHK(launch_fixed_sum(d->sterms.p + e * nf, nF, d->part.p, d->stats.p + e, st));
    double s[5];
    HIPCHK(hipMemcpyAsync(s, d->stats.p, sizeof s, hipMemcpyDeviceToHost, st));
    if (sigma) HIPCHK(hipMemcpyAsync(sigma, d->sigma.p, 2 * nf * sizeof(double), copy_out(memspace), st));
    HIPCHK(hipStreamSynchronize(st));
    stats[0] = s[0];                // max sigma1
    stats[1] = 0.0 - s[1];          // min sigma2
    stats[2] = s[2];                // faces outside the band
    stats[3] = s[3] / s[4];         // the rest-area-weighted mean of |F - T|_F^2
    return SMG_OK;
}

}  // namespace

extern "C" void smg_pd_params_default(smg_pd_params* p)
{
    if (!p) return;
    p->dt = 1e-2; p->density = 1.0; p->stiffness = 1.0; p->sigma_min = 1.0; p->sigma_max = 1.0; p->pressure = 0.0;
    p->gravity[0] = p->gravity[1] = p->gravity[2] = 0.0;
}

extern "C" int smg_pd_create(const smg_hierarchy* h, const double* V, int nV, const int* F, int nF, const int* pins, int n_pins, const smg_pd_params* p,
                             smg_pd** out)
{
    return guarded("smg_pd_create", [&]() { return create_impl(h, V, nV, F, nF, pins, n_pins, p, out); });
}

extern "C" void smg_pd_destroy(smg_pd* d) { delete d; }

extern "C" long long smg_pd_device_bytes(const smg_pd* d)
{
    if (!d) return 0;   // one list: every DevBuf of the struct
    return device_bytes(*d, d->F, d->m_ptr, d->m_idx, d->pins, d->V0, d->rest, d->m0, d->x, d->vel, d->fext, d->Qn, d->hp, d->hpN, d->hrow, d->S, d->B, d->Ua,
                        d->Ub, d->share, d->terms, d->part, d->E, d->Fg, d->sigma, d->T, d->sterms, d->stats);
}

extern "C" int smg_pd_set_solver(smg_pd* d, int pcg)
{
    if (!d) return fail(SMG_ERR_INVALID, "null pd object");
    latch_solver(d->pcg, pcg);
    return SMG_OK;
}

extern "C" int smg_pd_set_state(smg_pd* d, const double* pos, const double* vel, int memspace)
{
    return guarded("smg_pd_set_state", [&]() { return state_impl(d, nullptr, nullptr, pos, vel, memspace, true); });
}

extern "C" int smg_pd_get_state(smg_pd* d, double* pos, double* vel, int memspace)
{
    return guarded("smg_pd_get_state", [&]() { return state_impl(d, pos, vel, nullptr, nullptr, memspace, false); });
}

extern "C" int smg_pd_set_forces(smg_pd* d, double pressure, const double* gravity)
{
    if (!d) return fail(SMG_ERR_INVALID, "smg_pd_set_forces: null object");
    if (const char* why = bad_forces(pressure, gravity)) return fail(SMG_ERR_INVALID, "smg_pd_set_forces: %s", why);
    d->p.pressure = pressure;
    if (gravity)
        for (int l = 0; l < 3; l++) d->p.gravity[l] = gravity[l];
    return SMG_OK;
}

extern "C" int smg_pd_set_strain_limits(smg_pd* d, double sigma_min, double sigma_max)
{
    if (!d) return fail(SMG_ERR_INVALID, "smg_pd_set_strain_limits: null object");
    if (const char* why = bad_band(sigma_min, sigma_max)) return fail(SMG_ERR_INVALID, "smg_pd_set_strain_limits: %s", why);
    d->p.sigma_min = sigma_min;
    d->p.sigma_max = sigma_max;
    return SMG_OK;
}

extern "C" int smg_pd_step(smg_pd* d, const double* pin_pos, int memspace, int max_iter, double rel_tol, const smg_solve_opts* opts, double* energy_his,
                           int* cycles, int* n_iter)
{
    return guarded("smg_pd_step", [&]() { return step_impl(d, pin_pos, memspace, max_iter, rel_tol, opts, energy_his, cycles, n_iter); });
}

extern "C" int smg_pd_strain(smg_pd* d, int memspace, double* sigma, double* stats)
{
    return guarded("smg_pd_strain", [&]() { return strain_impl(d, memspace, sigma, stats); });
}

extern "C" int smg_pd_project_host(const double* V0, const double* P, int nV, const int* F, int nF, double sigma_min, double sigma_max, double* Fg,
                                   double* sigma, double* T, int* guard_hits)
{
    return guarded("smg_pd_project_host", [&]() -> int {
        const char* who = "smg_pd_project_host";
        if (!V0 || !P || !F || nV <= 0 || nF <= 0) return fail(SMG_ERR_INVALID, "%s: bad arguments", who);
        if (const char* why = bad_band(sigma_min, sigma_max)) return fail(SMG_ERR_INVALID, "%s: %s", who, why);
        if (int rc = check_mesh(who, V0, nV, F, nF, false)) return rc;
        const size_t nf = (size_t)nF;
        int hits = 0;
        for (size_t f = 0; f < nf; f++) {
            const size_t v0 = 3 * (size_t)F[3 * f], v1 = 3 * (size_t)F[3 * f + 1], v2 = 3 * (size_t)F[3 * f + 2];
            double r[4], g[6], s[2], t[6];
            pd_rest(V0 + v0, V0 + v1, V0 + v2, r);
            pd_gradient(r, P + v0, P + v1, P + v2, g);
            hits += pd_project(g, sigma_min, sigma_max, s, t);
            for (int e = 0; e < 6; e++) {
                if (Fg) Fg[e * nf + f] = g[e];
                if (T) T[e * nf + f] = t[e];
            }
            if (sigma) { sigma[f] = s[0]; sigma[nf + f] = s[1]; }
        }
        if (guard_hits) *guard_hits = hits;
        return SMG_OK;
    });
}
