// smg_flow.cpp -- the conformalized mean-curvature flow of Kazhdan, Solomon and Ben-Chen 2012 on the scalar V-cycle, and the conformal map to the
// sphere it converges to on a closed genus-0 mesh (include/smg.h: smg_flow_*; the reference's
// 05_example_mean_curvature_flow).  L_0 is assembled once from the rest mesh and kept on the device with its CSR pattern; a step rebuilds the
// barycentric mass of the current positions, solves (M_t - delta L_0) U' = M_t U from U and normalises to unit area.  The object owns one handle
// built from the caller's prolongations: one pattern-setting smg_precompute at create, smg_precompute_values_device on every step.  A step is
// enqueued on the object's stream, which the handle uses too; beside what the inner solve reads itself the host reads one double per step, the
// sphericity.  Kernels: csrc/smg_flow_device.hip.  Checks, stream, handle, the cotangent system and the inner solve: smg_mesh_object.hpp; the
// sums: launch_fixed_sum / launch_fixed_max.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <memory>
#include <vector>

#include "smg_device.hpp"
#include "smg_flow_inl.hpp"
#include "smg_mesh.hpp"
#include "smg_mesh_object.hpp"

using namespace smg;

struct smg_flow : MeshObject {             // handle[0]: M_t - delta L_0, re-precomputed by values on every step
    int nV = 0, nF = 0, nnz = 0;
    int pcg = 1;                           // the inner solver: 1 smg_solve_pcg, 0 smg_solve
    int closed = 0, chi = 0;               // what smg_flow_sphere refuses: 0 a closed manifold of characteristic 2, 1 a boundary edge, 2 a non-manifold edge, 3 chi != 2
    smg_flow_params p;
    DevBuf<int> F, m_ptr, m_idx, rowptr, diag;   // faces, corner lists per vertex; L_0's row pointers and the position of every row's diagonal
    DevBuf<double> L0, val;                // L_0's values in the CSR's order; this step's M_t - delta L_0
    DevBuf<double> V0, Ua, Ub, Z;          // column-major nV x 3: the (normalised) rest mesh, the state, the next state, the solve's result
    DevBuf<double> mass, B;                // this step's masses and right-hand side (nV x 3 column-major)
    DevBuf<double> a, r, term, part, s;    // the sphericity's masses and radii, the planes of terms, the chunk sums, the block of sums
    DevBuf<double> S, sigma;               // the sphere map: nV x 3 column-major, 2 planes of nF
    ~smg_flow() { quiesce(); }
};

namespace smg {

int flow_check_params(const char* who, const smg_flow_params& p)
{
    if (!std::isfinite(p.delta) || !(p.delta > 0.0)) return fail(SMG_ERR_INVALID, "%s: delta = %g, a finite time step > 0 is needed", who, p.delta);
    if (p.normalize != 0 && p.normalize != 1) return fail(SMG_ERR_INVALID, "%s: normalize = %d, 0 or 1 is needed", who, p.normalize);
    if (!std::isfinite(p.stop_sphericity) || p.stop_sphericity < 0.0)
        return fail(SMG_ERR_INVALID, "%s: stop_sphericity = %g, a finite value >= 0 is needed", who, p.stop_sphericity);
    return SMG_OK;
}

int flow_check_operands(const char* who, int op, int nV, int nF, const int* F, const double* U, const double* V0, const int* rowptr, const int* col,
                        const double* L0, double delta, const double* out)
{
    if (op < SMG_FLOW_SYSTEM || op > SMG_FLOW_SPHERE || nV < 1 || nF < 1 || !F || !U || !out) return fail(SMG_ERR_INVALID, "%s: bad arguments", who);
    if ((op == SMG_FLOW_SYSTEM && (!rowptr || !col || !L0)) || (op == SMG_FLOW_SPHERE && !V0))
        return fail(SMG_ERR_INVALID, "%s: op %d misses an operand", who, op);
    if (int rc = check_faces(who, F, nF, nV)) return rc;
    if (op != SMG_FLOW_SYSTEM) return SMG_OK;
    if (!std::isfinite(delta) || !(delta > 0.0)) return fail(SMG_ERR_INVALID, "%s: delta = %g, a finite time step > 0 is needed", who, delta);
    if (rowptr[0] != 0) return fail(SMG_ERR_INVALID, "%s: rowptr does not start at 0", who);
    for (int v = 0; v < nV; v++) {
        if (rowptr[v + 1] < rowptr[v]) return fail(SMG_ERR_INVALID, "%s: rowptr is not monotone", who);
        int nd = 0;
        for (int j = rowptr[v]; j < rowptr[v + 1]; j++) {
            if (col[j] < 0 || col[j] >= nV) return fail(SMG_ERR_INVALID, "%s: column index out of range", who);
            nd += col[j] == v ? 1 : 0;
        }
        if (nd != 1) return fail(SMG_ERR_INVALID, "%s: row %d stores %d diagonal entries, one is needed", who, v, nd);
    }
    return SMG_OK;
}

void flow_diagonal(int nV, const int* rowptr, const int* col, std::vector<int>& diag)
{
    diag.assign((size_t)nV, 0);
    for (int v = 0; v < nV; v++)
        for (int j = rowptr[v]; j < rowptr[v + 1]; j++)
            if (col[j] == v) diag[(size_t)v] = j;
}

}  // namespace smg

namespace {

// 0: every edge has two faces and nV - nE + nF == 2; 1: an edge with one face; 2: an edge with more than two; 3: another characteristic (*chi)
int closed_sphere(const int* F, int nF, int nV, int* chi)
{
    std::vector<uint64_t> e;
    e.reserve(3 * (size_t)nF);
    for (size_t f = 0; f < (size_t)nF; f++)
        for (int c = 0; c < 3; c++) {
            const uint64_t a = (uint64_t)F[3 * f + c], b = (uint64_t)F[3 * f + (c + 1) % 3];
            e.push_back(std::min(a, b) << 32 | std::max(a, b));
        }
    std::sort(e.begin(), e.end());
    long long nE = 0;
    int worst = 0;
    for (size_t i = 0; i < e.size();) {
        size_t j = i;
        while (j < e.size() && e[j] == e[i]) j++;
        if (j - i == 1) worst = std::max(worst, 1);
        if (j - i > 2) worst = 2;
        nE++;
        i = j;
    }
    *chi = (int)((long long)nV - nE + nF);
    if (worst) return worst;
    return *chi == 2 ? 0 : 3;
}

int create_impl(const smg_hierarchy* h, const double* V, int nV, const int* F, int nF, const smg_flow_params* p, smg_flow** out)
{
    if (out) *out = nullptr;
    const char* who = "smg_flow_create";
    if (!h || !V || !F || !p || !out || nV <= 0 || nF <= 0) return fail(SMG_ERR_INVALID, "%s: bad arguments", who);
    if (int rc = check_hierarchy(who, h, 1, nV)) return rc;
    if (h->n_levels < 2) return fail(SMG_ERR_INVALID, "%s: a hierarchy of at least two levels is needed: every step re-precomputes by values", who);
    if (int rc = check_mesh(who, V, nV, F, nF, true)) return rc;
    if (int rc = flow_check_params(who, *p)) return rc;

    std::unique_ptr<smg_flow> m(new smg_flow());
    m->nV = nV; m->nF = nF; m->p = *p;
    m->closed = closed_sphere(F, nF, nV, &m->chi);
    if (int rc = m->open(who)) return rc;
    if (int rc = m->clone(who, h, 0)) return rc;
    hipStream_t st = m->stream;
    const size_t n = (size_t)nV, nf = (size_t)nF;

    if (int rc = upload_faces(F, nF, nV, m->F, m->m_ptr, m->m_idx)) return rc;
    for (DevBuf<double>* b : {&m->V0, &m->Ua, &m->Ub, &m->Z, &m->B, &m->S}) HIPCHK(b->alloc(3 * n));
    HIPCHK(m->mass.alloc(n));
    HIPCHK(m->a.alloc(n));
    HIPCHK(m->r.alloc(n));
    HIPCHK(m->term.alloc(std::max(4 * nf, 3 * n)));
    HIPCHK(m->part.alloc((size_t)fixed_sum_groups(std::max(nF, nV))));
    HIPCHK(m->s.alloc(FLOW_SUMS));
    HIPCHK(m->sigma.alloc(2 * nf));
    HIPCHK(hipMemsetAsync(m->s.p, 0, FLOW_SUMS * sizeof(double), st));

    // the rest mesh: the caller's rows as columns, normalised by the step's own kernels; back as rows for the assembler
    DevBuf<double> rows;
    HIPCHK(rows.upload(std::vector<double>(V, V + 3 * n)));
    if (p->normalize) {
        HIPCHK(launch_arap_columns(nV, rows.p, m->Z.p, nV, st));
        HIPCHK(launch_flow_normalize(nV, nF, m->F.p, m->Z.p, nV, m->term.p, m->part.p, m->s.p, m->V0.p, nV, st));
        HIPCHK(launch_arap_rows(nV, m->V0.p, nV, rows.p, st));
    } else {
        HIPCHK(launch_arap_columns(nV, rows.p, m->V0.p, nV, st));
    }
    HIPCHK(hipMemcpyAsync(m->Ua.p, m->V0.p, 3 * n * sizeof(double), hipMemcpyDeviceToDevice, st));

    // L_0 once, kept with its pattern; M_0 - delta L_0 sets the handle's pattern
    CotanSystem S;
    if (int rc = cotan_system(F, nF, nV, rows.p, 0, 1.0, -p->delta, st, S, true, &m->L0)) return rc;
    m->nnz = (int)S.col.size();
    std::vector<int> diag;
    flow_diagonal(nV, S.ptr.data(), S.col.data(), diag);
    HIPCHK(m->rowptr.upload(S.ptr));
    HIPCHK(m->diag.upload(diag));
    HIPCHK(m->val.alloc((size_t)m->nnz));
    if (int rc = smg_precompute(m->handle[0], nV, S.ptr.data(), S.col.data(), S.val.data(), nullptr, 0)) return rc;
    HIPCHK(hipStreamSynchronize(st));
    *out = m.release();
    return SMG_OK;
}

// the sphericity of the state into s[0] and, one double, onto the host
int measure(smg_flow* m, double* q)
{
    hipStream_t st = m->stream;
    HIPCHK(launch_flow_sphericity(m->nV, m->Ua.p, m->nV, m->F.p, m->m_ptr.p, m->m_idx.p, m->a.p, m->r.p, m->term.p, m->part.p, m->s.p, st));
    HIPCHK(hipMemcpyAsync(q, m->s.p, sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return SMG_OK;
}

int step_impl(smg_flow* m, int n_steps, const smg_solve_opts* opts, double* his, int* cycles, int* n_done)
{
    const char* who = "smg_flow_step";
    if (n_done) *n_done = 0;
    if (!m) return fail(SMG_ERR_INVALID, "%s: null object", who);
    if (n_steps < 0) return fail(SMG_ERR_INVALID, "%s: n_steps = %d, at least 0 is needed", who, n_steps);
    DeviceScope dsc(m->device);
    hipStream_t st = m->stream;
    const int n = m->nV, nF = m->nF;
    const smg_solve_opts so = opts_or_default(opts, 5e-7);
    int t_end = 0;
    if (!n_done) n_done = &t_end;
    for (int t = 0; t < n_steps; t++) {
        *n_done = t;
        double q = 0.0;
        if (int rc = measure(m, &q)) return rc;
        if (his) his[t] = q;
        if (!std::isfinite(q)) return fail(SMG_ERR_NONFINITE, "%s: non-finite sphericity at step %d", who, t);
        if (m->p.stop_sphericity > 0.0 && q <= m->p.stop_sphericity) return SMG_OK;
        // the sphericity of this very state has just left its masses in `a`
        HIPCHK(launch_flow_system(n, m->Ua.p, n, m->F.p, m->m_ptr.p, m->m_idx.p, m->rowptr.p, m->diag.p, m->L0.p, m->p.delta, m->a.p, m->mass.p, m->B.p, n,
                                  m->val.p, st));
        if (int rc = smg_precompute_values_device(m->handle[0], m->val.p)) return rc;
        double* z = m->p.normalize ? m->Z.p : m->Ub.p;
        int entries = 0;
        if (int rc = inner_solve(m->handle[0], m->pcg, m->B.p, n, nullptr, 0, m->Ua.p, n, 3, so, z, n, &entries)) return rc;
        if (cycles) cycles[t] = entries;
        if (m->p.normalize) HIPCHK(launch_flow_normalize(n, nF, m->F.p, z, n, m->term.p, m->part.p, m->s.p, m->Ub.p, n, st));
        std::swap(m->Ua, m->Ub);
    }
    *n_done = n_steps;
    double q = 0.0;
    if (int rc = measure(m, &q)) return rc;
    if (his) his[n_steps] = q;
    if (!std::isfinite(q)) return fail(SMG_ERR_NONFINITE, "%s: non-finite sphericity at step %d", who, n_steps);
    return SMG_OK;
}

int positions_impl(smg_flow* m, int memspace, double* U, const double* U_in, int ld_u, bool set)
{
    const char* who = set ? "smg_flow_set_positions" : "smg_flow_positions";
    if (!m || !(set ? (const void*)U_in : (const void*)U)) return fail(SMG_ERR_INVALID, "%s: bad arguments", who);
    if (bad_memspace(memspace)) return fail(SMG_ERR_INVALID, "%s: memspace must be SMG_HOST or SMG_DEVICE", who);
    if (ld_u < m->nV) return fail(SMG_ERR_INVALID, "%s: a leading dimension is too small", who);
    DeviceScope dsc(m->device);
    hipStream_t st = m->stream;
    if (set) HIPCHK(copy_columns(m->Ua.p, m->nV, U_in, ld_u, m->nV, 3, copy_in(memspace), st));
    else HIPCHK(copy_columns(U, ld_u, m->Ua.p, m->nV, m->nV, 3, copy_out(memspace), st));
    HIPCHK(hipStreamSynchronize(st));
    return SMG_OK;
}

int sphere_impl(smg_flow* m, int memspace, double* S, int ld_s, double* sigma, double* stats)
{
    const char* who = "smg_flow_sphere";
    if (!m || !stats) return fail(SMG_ERR_INVALID, "%s: bad arguments", who);
    if (bad_memspace(memspace)) return fail(SMG_ERR_INVALID, "%s: memspace must be SMG_HOST or SMG_DEVICE", who);
    if (S && ld_s < m->nV) return fail(SMG_ERR_INVALID, "%s: a leading dimension is too small", who);
    if (m->closed == 1) return fail(SMG_ERR_INVALID, "%s: the mesh has a boundary edge: the sphere map needs a closed mesh", who);
    if (m->closed == 2) return fail(SMG_ERR_INVALID, "%s: the mesh has a non-manifold edge", who);
    if (m->closed == 3) return fail(SMG_ERR_INVALID, "%s: nV - nE + nF = %d, a sphere has 2", who, m->chi);
    DeviceScope dsc(m->device);
    hipStream_t st = m->stream;
    const int n = m->nV, nF = m->nF;
    HIPCHK(launch_flow_sphericity(n, m->Ua.p, n, m->F.p, m->m_ptr.p, m->m_idx.p, m->a.p, m->r.p, m->term.p, m->part.p, m->s.p, st));
    HIPCHK(launch_flow_sphere(n, nF, m->F.p, m->Ua.p, n, m->V0.p, n, m->s.p, m->S.p, n, m->sigma.p, m->term.p, m->part.p, m->s.p + 12, st));
    double s[FLOW_SUMS];
    HIPCHK(hipMemcpyAsync(s, m->s.p, sizeof s, hipMemcpyDeviceToHost, st));
    if (S) HIPCHK(copy_columns(S, ld_s, m->S.p, n, n, 3, copy_out(memspace), st));
    if (sigma) HIPCHK(hipMemcpyAsync(sigma, m->sigma.p, 2 * (size_t)nF * sizeof(double), copy_out(memspace), st));
    HIPCHK(hipStreamSynchronize(st));
    stats[0] = s[12] / s[13];       // the rest-area-weighted mean of sigma1 / sigma2
    stats[1] = s[14];               // its maximum
    stats[2] = s[15];               // the flipped faces
    stats[3] = s[0];                // the sphericity of the state
    return SMG_OK;
}

}  // namespace

extern "C" smg_flow_params smg_flow_params_default(void)
{
    smg_flow_params p;
    p.delta = 0.01; p.normalize = 1; p.stop_sphericity = 0.0;
    return p;
}

extern "C" int smg_flow_create(const smg_hierarchy* h, const double* V, int nV, const int* F, int nF, const smg_flow_params* p, smg_flow** out)
{
    return guarded("smg_flow_create", [&]() { return create_impl(h, V, nV, F, nF, p, out); });
}

extern "C" void smg_flow_destroy(smg_flow* f) { delete f; }

extern "C" int smg_flow_set_params(smg_flow* f, const smg_flow_params* p)
{
    const char* who = "smg_flow_set_params";
    if (!f || !p) return fail(SMG_ERR_INVALID, "%s: bad arguments", who);
    if (int rc = flow_check_params(who, *p)) return rc;
    if (p->normalize != f->p.normalize) return fail(SMG_ERR_INVALID, "%s: normalize is fixed at create (the rest mesh was %s)", who, f->p.normalize ? "normalised" : "taken as given");
    f->p = *p;
    return SMG_OK;
}

extern "C" int smg_flow_set_solver(smg_flow* f, int pcg)
{
    if (!f) return fail(SMG_ERR_INVALID, "smg_flow_set_solver: null object");
    latch_solver(f->pcg, pcg);
    return SMG_OK;
}

extern "C" long long smg_flow_device_bytes(const smg_flow* f)
{
    if (!f) return 0;   // one list: every DevBuf of the struct
    return device_bytes(*f, f->F, f->m_ptr, f->m_idx, f->rowptr, f->diag, f->L0, f->val, f->V0, f->Ua, f->Ub, f->Z, f->mass, f->B, f->a, f->r, f->term,
                        f->part, f->s, f->S, f->sigma);
}

extern "C" int smg_flow_step(smg_flow* f, int n_steps, const smg_solve_opts* opts, double* sphericity_his, int* cycles, int* n_done)
{
    return guarded("smg_flow_step", [&]() { return step_impl(f, n_steps, opts, sphericity_his, cycles, n_done); });
}

extern "C" int smg_flow_positions(smg_flow* f, int memspace, double* U, int ld_u)
{
    return guarded("smg_flow_positions", [&]() { return positions_impl(f, memspace, U, nullptr, ld_u, false); });
}

extern "C" int smg_flow_set_positions(smg_flow* f, const double* U, int ld_u, int memspace)
{
    return guarded("smg_flow_set_positions", [&]() { return positions_impl(f, memspace, nullptr, U, ld_u, true); });
}

extern "C" int smg_flow_reset(smg_flow* f)
{
    return guarded("smg_flow_reset", [&]() -> int {
        if (!f) return fail(SMG_ERR_INVALID, "smg_flow_reset: null object");
        DeviceScope dsc(f->device);
        HIPCHK(hipMemcpyAsync(f->Ua.p, f->V0.p, 3 * (size_t)f->nV * sizeof(double), hipMemcpyDeviceToDevice, f->stream));
        HIPCHK(hipStreamSynchronize(f->stream));
        return SMG_OK;
    });
}

extern "C" int smg_flow_sphere(smg_flow* f, int memspace, double* S, int ld_s, double* sigma, double* stats)
{
    return guarded("smg_flow_sphere", [&]() { return sphere_impl(f, memspace, S, ld_s, sigma, stats); });
}

extern "C" int smg_flow_host(int op, int nV, int nF, const int* F, const double* U, const double* V0, const int* rowptr, const int* col,
                             const double* L0, double delta, double* out)
{
    return guarded("smg_flow_host", [&]() -> int {
        const char* who = "smg_flow_host";
        if (int rc = flow_check_operands(who, op, nV, nF, F, U, V0, rowptr, col, L0, delta, out)) return rc;
        const size_t n = (size_t)nV, nf = (size_t)nF;
        std::vector<int> mp, mi;
        if (op != SMG_FLOW_NORMALIZE) vertex_corner_lists(std::vector<int>(F, F + 3 * nf), nV, mp, mi);
        switch (op) {
            case SMG_FLOW_SYSTEM: flow_host_system(nV, F, mp.data(), mi.data(), U, rowptr, col, L0, delta, out, out + n, out + 4 * n); break;
            case SMG_FLOW_NORMALIZE: flow_host_normalize(nV, nF, F, U, out); break;
            case SMG_FLOW_SPHERICITY: flow_host_sphericity(nV, F, mp.data(), mi.data(), U, out); break;
            default: flow_host_sphere(nV, nF, F, mp.data(), mi.data(), U, V0, out, out + 3 * n, out + 3 * n + 2 * nf, out + 3 * n + 6 * nf); break;
        }
        return SMG_OK;
    });
}
