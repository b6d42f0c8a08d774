// smg_denoise.cpp -- feature-preserving denoising of a triangle mesh on the scalar V-cycle (include/smg.h: smg_denoise_*; DESIGN.md section
// 24): the bilateral normal filter of Zheng, Fu, Au, Tai 2011 (local scheme), then vertex positions that follow the filtered normals.
// The object owns one handle built from the caller's prolongations and precomputed ONCE with fidelity M - L of the input mesh (Voronoi mass):
// the same matrix for x, y and z and for the life of the object.  On the device it keeps the faces, the corner lists of the vertices, N(f)
// (the faces that share a vertex with f, built on the host from the corner lists), the rest constants of every face (k_denoise_rest), the mass,
// three normal fields (the latched m and the filter's ping-pong pair) and the buffers of an update.
// The filter: normal_iters launches of k_denoise_filter, the host swapping the pair between them; no host read sits in that loop.
// The update: the local / global alternation of smg_local_global.hpp.  One iteration: the projections, the face energy terms and the corner
// shares (k_denoise_project), the right-hand side and the fidelity terms (launch_pd_vertices with S = V and c_mass = fidelity), the energy (one
// fixed-order reduction over nF + nV terms), one 3-column solve warm-started at the iterate.  All of it is enqueued on the object's stream, which
// the handle uses too; per iteration the host reads one energy double beside the solve's own history (at iteration 0, without options, also
// |b_0|_F^2).  Checks, stream, handle, the cotangent system and the inner solve: smg_mesh_object.hpp; the sums: launch_fixed_sum.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cmath>
#include <memory>
#include <vector>

#include "smg_denoise_inl.hpp"
#include "smg_device.hpp"
#include "smg_local_global.hpp"
#include "smg_mesh.hpp"
#include "smg_mesh_object.hpp"

using namespace smg;

struct smg_denoise : MeshObject {             // handle[0]: fidelity M - L of the input mesh
    int nV = 0, nF = 0;
    int pcg = 1;                              // the inner solver: 1 smg_solve_pcg, 0 smg_solve
    smg_denoise_params p;                     // sigma_s: the value in use
    DevBuf<int> F, m_ptr, m_idx;              // faces; the corner lists t = 3 f + i of every vertex, faces ascending
    DevBuf<int> nb_ptr, nb_idx;               // N(f)
    DevBuf<double> V0, Vc, rest, m0;          // the input positions (xyz rows; column-major), rest constants (10 planes), Voronoi mass
    DevBuf<double> m, ma, mb;                 // normal fields (3 planes each): the latched one, the filter's pair
    DevBuf<double> rows;                      // a call's xyz rows on their way in or out: 3 max(nV, nF)
    DevBuf<double> B, Ua, Ub;                 // column-major nV x 3: right-hand side, the iterate and the solve's result
    DevBuf<double> share, terms, part, E;     // corner shares (9 planes), the terms nF faces + nV vertices + nV |b_v|^2, chunk sums, E_t and |b_0|^2
    ~smg_denoise() { quiesce(); }
};

namespace {

const char* bad_params(const smg_denoise_params& p)
{
    auto positive = [](double x) { return std::isfinite(x) && x > 0.0; };
    if (!positive(p.sigma_r)) return "sigma_r must be finite and > 0";
    if (!positive(p.fidelity)) return "fidelity must be finite and > 0";
    if (!std::isfinite(p.sigma_s)) return "sigma_s must be finite (<= 0: the mean centroid distance of the neighbourhoods)";
    if (p.normal_iters < 0) return "normal_iters must be >= 0";
    return nullptr;
}

int create_impl(const smg_hierarchy* h, const double* V, int nV, const int* F, int nF, const smg_denoise_params* pp, smg_denoise** out)
{
    if (out) *out = nullptr;
    const char* who = "smg_denoise_create";
    if (!h || !V || !F || !pp || !out || nV <= 0 || nF <= 0) return fail(SMG_ERR_INVALID, "%s: bad arguments", who);
    if (int rc = check_hierarchy(who, h, 1, nV)) return rc;
    if (int rc = check_mesh(who, V, nV, F, nF, true)) return rc;
    if (const char* why = bad_params(*pp)) return fail(SMG_ERR_INVALID, "%s: %s", who, why);

    std::unique_ptr<smg_denoise> d(new smg_denoise());
    d->nV = nV; d->nF = nF; d->p = *pp;
    if (int rc = d->open(who)) return rc;
    if (int rc = d->clone(who, h, 0)) return rc;
    hipStream_t st = d->stream;

    // the one matrix of the object: fidelity M - L, assembled on the device
    HIPCHK(d->V0.upload(std::vector<double>(V, V + 3 * (size_t)nV)));
    CotanSystem S;
    if (int rc = cotan_system(F, nF, nV, d->V0.p, 1, pp->fidelity, -1.0, st, S, true)) return rc;
    if (int rc = smg_precompute(d->handle[0], nV, S.ptr.data(), S.col.data(), S.val.data(), nullptr, 0)) return rc;

    std::vector<int> mp, mi, np, ni;
    if (int rc = upload_faces(F, nF, nV, d->F, d->m_ptr, d->m_idx, &mp, &mi)) return rc;
    if (!face_neighbours(std::vector<int>(F, F + 3 * (size_t)nF), mp, mi, np, ni)) return fail(SMG_ERR_INVALID, "%s: the neighbourhoods have more than 2^31 - 1 entries", who);
    const size_t pairs = ni.size();
    if (ni.empty()) ni.push_back(0);                     // one face alone: no row is walked
    HIPCHK(d->nb_ptr.upload(np));
    HIPCHK(d->nb_idx.upload(ni));
    const size_t n = (size_t)nV, nf = (size_t)nF;
    HIPCHK(d->rest.alloc(DN_REST * nf));
    HIPCHK(d->m0.alloc(n));
    for (DevBuf<double>* b : {&d->m, &d->ma, &d->mb}) HIPCHK(b->alloc(3 * nf));
    for (DevBuf<double>* b : {&d->Vc, &d->B, &d->Ua, &d->Ub}) HIPCHK(b->alloc(3 * n));
    HIPCHK(d->rows.alloc(3 * std::max(n, nf)));
    HIPCHK(d->share.alloc(9 * nf));
    HIPCHK(d->terms.alloc(nf + 2 * n));
    HIPCHK(d->part.alloc((size_t)fixed_sum_groups(nF + nV)));
    HIPCHK(d->E.alloc(2));

    // the rest constants, m = n; the mass by the expressions the assembler's diagonal is summed from, in its order (share: 6 planes of scratch)
    HIPCHK(launch_denoise_rest(nF, d->F.p, d->V0.p, d->rest.p, st));
    HIPCHK(hipMemcpyAsync(d->m.p, d->rest.p, 3 * nf * sizeof(double), hipMemcpyDeviceToDevice, st));
    HIPCHK(launch_membrane_pressure(nV, nF, d->F.p, d->V0.p, d->m_ptr.p, d->m_idx.p, 0.0, d->share.p, d->m0.p, nullptr, st));
    HIPCHK(launch_arap_columns(nV, d->V0.p, d->Vc.p, nV, st));
    if (!(pp->sigma_s > 0.0)) {     // the rule: the mean of |c_f - c_g| over the ordered pairs of N, a fixed-order sum
        double sum = 0.0;
        HIPCHK(launch_denoise_spacing(nF, d->nb_ptr.p, d->nb_idx.p, d->rest.p, d->terms.p, st));
        HIPCHK(launch_fixed_sum(d->terms.p, nF, d->part.p, d->E.p, st));
        HIPCHK(hipMemcpyAsync(&sum, d->E.p, sizeof(double), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        d->p.sigma_s = pairs ? sum / (double)pairs : 1.0;
    }
    HIPCHK(hipStreamSynchronize(st));
    *out = d.release();
    return SMG_OK;
}

// xyz rows of the caller (count x 3, in memspace) as planes / a column-major block with leading dimension count, through d->rows
int rows_in(smg_denoise* d, const double* src, int memspace, int count, double* planes)
{
    HIPCHK(hipMemcpyAsync(d->rows.p, src, 3 * (size_t)count * sizeof(double), copy_in(memspace), d->stream));
    HIPCHK(launch_arap_columns(count, d->rows.p, planes, count, d->stream));
    return SMG_OK;
}

int rows_out(smg_denoise* d, const double* planes, int count, int memspace, double* dst)
{
    HIPCHK(launch_arap_rows(count, planes, count, d->rows.p, d->stream));
    HIPCHK(hipMemcpyAsync(dst, d->rows.p, 3 * (size_t)count * sizeof(double), copy_out(memspace), d->stream));
    return SMG_OK;
}

int filter_impl(smg_denoise* d, const double* normals_in, int memspace, double* normals_out)
{
    if (!d || bad_memspace(memspace)) return fail(SMG_ERR_INVALID, "smg_denoise_filter: bad arguments");
    DeviceScope dsc(d->device);
    hipStream_t st = d->stream;
    const int nF = d->nF;
    if (normals_in) {
        if (int rc = rows_in(d, normals_in, memspace, nF, d->ma.p)) return rc;
    } else {
        HIPCHK(hipMemcpyAsync(d->ma.p, d->rest.p, 3 * (size_t)nF * sizeof(double), hipMemcpyDeviceToDevice, st));
    }
    for (int it = 0; it < d->p.normal_iters; it++) {
        HIPCHK(launch_denoise_filter(nF, d->nb_ptr.p, d->nb_idx.p, d->rest.p, d->ma.p, d->p.sigma_s, d->p.sigma_r, d->mb.p, st));
        std::swap(d->ma, d->mb);
    }
    if (normals_out)
        if (int rc = rows_out(d, d->ma.p, nF, memspace, normals_out)) return rc;
    HIPCHK(hipStreamSynchronize(st));
    std::swap(d->m, d->ma);           // latched only now: a failed call leaves m as it was
    return SMG_OK;
}

int update_impl(smg_denoise* d, const double* X0, int memspace, int max_iter, double rel_tol, const smg_solve_opts* opts, double* X, double* energy_his,
                int* cycles, int* n_iter)
{
    if (n_iter) *n_iter = 0;
    if (!d || !X || bad_memspace(memspace) || max_iter < 0 || !(rel_tol >= 0.0) || !std::isfinite(rel_tol)) return fail(SMG_ERR_INVALID, "smg_denoise_update: bad arguments");
    DeviceScope dsc(d->device);
    hipStream_t st = d->stream;
    const int n = d->nV, nF = d->nF;
    HIPCHK(d->E.ensure((size_t)max_iter + 2));
    double* bsum = d->E.p + max_iter + 1;
    int t_end = 0;
    if (!n_iter) n_iter = &t_end;

    if (X0) {
        if (int rc = rows_in(d, X0, memspace, n, d->Ua.p)) return rc;
    } else {
        HIPCHK(hipMemcpyAsync(d->Ua.p, d->Vc.p, 3 * (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, st));
    }
    smg_solve_opts so = opts_or_default(opts, 0.0, 50);
    double* terms = d->terms.p;
    // local step: t_{f,k} from x_t, E_t; the right-hand side is a by-product of the same two launches
    auto local = [&](int t, bool, double* E_t) -> int {
        HIPCHK(launch_denoise_project(nF, d->F.p, d->rest.p, d->m.p, d->Ua.p, 1, (size_t)n, terms, d->share.p, st));
        HIPCHK(launch_pd_vertices(n, nF, d->m_ptr.p, d->m_idx.p, d->share.p, d->m0.p, d->p.fidelity, d->Vc.p, d->Ua.p, n, d->B.p, n, terms + nF, terms + nF + n, st));
        HIPCHK(launch_fixed_sum(terms, nF + n, d->part.p, d->E.p + t, st));
        HIPCHK(hipMemcpyAsync(E_t, d->E.p + t, sizeof(double), hipMemcpyDeviceToHost, st));
        double b2 = 0.0;
        if (t == 0 && !opts) {      // the default tolerance of this call's solves: 1e-8 |b_0|_F
            HIPCHK(launch_fixed_sum(terms + nF + n, n, d->part.p, bsum, st));
            HIPCHK(hipMemcpyAsync(&b2, bsum, sizeof(double), hipMemcpyDeviceToHost, st));
        }
        HIPCHK(hipStreamSynchronize(st));
        if (t == 0 && !opts) so.tol = 1e-8 * std::sqrt(b2);
        return SMG_OK;
    };
    // global step: (fidelity M - L) x_{t+1} = fidelity M V + b, from x_t
    auto global = [&](int, int* entries) -> int {
        if (int rc = inner_solve(d->handle[0], d->pcg, d->B.p, n, nullptr, 0, d->Ua.p, n, 3, so, d->Ub.p, n, entries)) return rc;
        std::swap(d->Ua, d->Ub);
        return SMG_OK;
    };
    const int rc = local_global(max_iter, rel_tol, local, global, energy_his, cycles, n_iter);
    if (rc == LOCAL_GLOBAL_NONFINITE) {
        HIPCHK(hipStreamSynchronize(st));
        return fail(SMG_ERR_NONFINITE, "smg_denoise_update: non-finite energy at iteration %d", *n_iter);
    }
    if (rc) return rc;
    if (int rc2 = rows_out(d, d->Ua.p, n, memspace, X)) return rc2;
    HIPCHK(hipStreamSynchronize(st));
    return SMG_OK;
}

}  // namespace

extern "C" void smg_denoise_params_default(smg_denoise_params* p)
{
    if (!p) return;
    p->sigma_s = 0.0; p->sigma_r = 0.35; p->fidelity = 1.0; p->normal_iters = 20;
}

extern "C" int smg_denoise_create(const smg_hierarchy* h, const double* V, int nV, const int* F, int nF, const smg_denoise_params* p, smg_denoise** out)
{
    return guarded("smg_denoise_create", [&]() { return create_impl(h, V, nV, F, nF, p, out); });
}

extern "C" void smg_denoise_destroy(smg_denoise* d) { delete d; }

extern "C" long long smg_denoise_device_bytes(const smg_denoise* d)
{
    if (!d) return 0;   // one list: every DevBuf of the struct
    return device_bytes(*d, d->F, d->m_ptr, d->m_idx, d->nb_ptr, d->nb_idx, d->V0, d->Vc, d->rest, d->m0, d->m, d->ma, d->mb, d->rows, d->B, d->Ua, d->Ub,
                        d->share, d->terms, d->part, d->E);
}

extern "C" int smg_denoise_set_solver(smg_denoise* d, int pcg)
{
    if (!d) return fail(SMG_ERR_INVALID, "null denoise object");
    latch_solver(d->pcg, pcg);
    return SMG_OK;
}

extern "C" double smg_denoise_sigma_s(const smg_denoise* d) { return d ? d->p.sigma_s : 0.0; }

extern "C" int smg_denoise_set_filter(smg_denoise* d, double sigma_s, double sigma_r, int normal_iters)
{
    if (!d) return fail(SMG_ERR_INVALID, "smg_denoise_set_filter: null object");
    if (!std::isfinite(sigma_s) || !std::isfinite(sigma_r)) return fail(SMG_ERR_INVALID, "smg_denoise_set_filter: sigma_s and sigma_r must be finite");
    if (sigma_s > 0.0) d->p.sigma_s = sigma_s;
    if (sigma_r > 0.0) d->p.sigma_r = sigma_r;
    if (normal_iters >= 0) d->p.normal_iters = normal_iters;
    return SMG_OK;
}

extern "C" int smg_denoise_filter(smg_denoise* d, const double* normals_in, int memspace, double* normals_out)
{
    return guarded("smg_denoise_filter", [&]() { return filter_impl(d, normals_in, memspace, normals_out); });
}

extern "C" int smg_denoise_update(smg_denoise* d, const double* X0, int memspace, int max_iter, double rel_tol, const smg_solve_opts* opts, double* X,
                                  double* energy_his, int* cycles, int* n_iter)
{
    return guarded("smg_denoise_update", [&]() { return update_impl(d, X0, memspace, max_iter, rel_tol, opts, X, energy_his, cycles, n_iter); });
}

extern "C" int smg_denoise_run(smg_denoise* d, int memspace, int max_iter, double rel_tol, const smg_solve_opts* opts, double* X, double* energy_his,
                               int* cycles, int* n_iter)
{
    return guarded("smg_denoise_run", [&]() -> int {
        if (n_iter) *n_iter = 0;
        if (!d || !X || bad_memspace(memspace) || max_iter < 0 || !(rel_tol >= 0.0) || !std::isfinite(rel_tol)) return fail(SMG_ERR_INVALID, "smg_denoise_run: bad arguments");
        if (int rc = filter_impl(d, nullptr, memspace, nullptr)) return rc;
        return update_impl(d, nullptr, memspace, max_iter, rel_tol, opts, X, energy_his, cycles, n_iter);
    });
}

extern "C" int smg_denoise_faces_host(int op, int nV, int nF, const int* F, const double* V0, const double* P, const double* in,
                                      const smg_denoise_params* p, double* out)
{
    return guarded("smg_denoise_faces_host", [&]() -> int {
        const char* who = "smg_denoise_faces_host";
        if (op < SMG_DN_REST || op > SMG_DN_PROJECT || nV < 1 || nF < 1 || !F || !V0 || !p || !out) return fail(SMG_ERR_INVALID, "%s: bad arguments", who);
        if ((op == SMG_DN_PROJECT && !P) || (op >= SMG_DN_FILTER && !in)) return fail(SMG_ERR_INVALID, "%s: op %d misses an operand", who, op);
        if (op == SMG_DN_FILTER && (!(p->sigma_s > 0.0) || !(p->sigma_r > 0.0) || p->normal_iters < 0))
            return fail(SMG_ERR_INVALID, "%s: the filter takes sigma_s > 0, sigma_r > 0 and normal_iters >= 0", who);
        if (int rc = check_faces(who, F, nF, nV)) return rc;
        std::vector<int> mp, mi, np, ni;
        if (op == SMG_DN_SPACING || op == SMG_DN_FILTER) {
            const std::vector<int> Fv(F, F + 3 * (size_t)nF);
            vertex_corner_lists(Fv, nV, mp, mi);
            if (!face_neighbours(Fv, mp, mi, np, ni)) return fail(SMG_ERR_INVALID, "%s: the neighbourhoods have more than 2^31 - 1 entries", who);
        }
        dn_faces_host(op, nF, F, V0, P, in, p->sigma_s, p->sigma_r, p->normal_iters, np.data(), ni.data(), out);
        return SMG_OK;
    });
}
