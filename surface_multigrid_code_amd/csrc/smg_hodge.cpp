// smg_hodge.cpp -- the Helmholtz-Hodge decomposition of per-face tangent vector fields with vertex potentials (include/smg.h: smg_hodge_*;
// DESIGN.md section 28; Tong, Lombeyda, Hirani, Desbrun 2003): Xt = grad u + n x grad v + H with (-L) u = b and (-L) v = c.
// The object owns the handles built from the caller's prolongations and precomputed with -L -- one on a closed mesh (vertex 0 known), two on a
// mesh with boundary (vertex 0 known for u, the boundary vertices known for v) -- and the geometry the kernels read (csrc/smg_hodge_device.hip):
// faces, corner lists, positions, the gradient basis W, the normals and the areas.  A query is one vertex kernel that writes the 2k right-hand
// sides, the fixed-order sums of their squares, ONE 2k-column solve on a closed mesh (two k-column solves with boundary) from a zero start with
// zero known values, and one face kernel for the parts and the energy terms.  All of it is enqueued on the object's stream, which the handles use
// too; beside the solve's own history the host reads the sums once per call: they set the default tolerance and refuse non-finite input before
// the solve.  Checks, stream, handles, the cotangent system and the inner solve: smg_mesh_object.hpp.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <memory>
#include <utility>
#include <vector>

#include "smg_device.hpp"
#include "smg_hodge_inl.hpp"
#include "smg_mesh.hpp"
#include "smg_mesh_object.hpp"

using namespace smg;

struct smg_hodge : MeshObject {            // handle[0]: -L, vertex 0 known; handle[1] (a mesh with boundary): -L, the boundary vertices known
    int nV = 0, nF = 0, nb = 0;            // nb: boundary vertices (0: closed)
    int pcg = 1;                           // the inner solver: 1 smg_solve_pcg, 0 smg_solve
    size_t kcap = 0;                       // the sets the query blocks hold
    DevBuf<int> F, m_ptr, m_idx;           // faces, corner lists per vertex
    DevBuf<double> V, W, nrm, Af;          // positions (xyz rows), gradient basis (9 per face), normals (3 per face), face areas
    DevBuf<double> Xs, Ps;                 // staging of a host call's field and parts
    DevBuf<double> B, Z, zero;             // column-major n x 2k: right-hand sides (b then c), potentials (u then v); zeros: the start and the known values
    DevBuf<double> bsq, part, terms, sums; // b^2 and c^2 per (vertex, set), the chunk sums, the energy terms (4k planes of nF), 2 + 4k sums
    ~smg_hodge() { quiesce(); }
};

namespace smg {

int hodge_check_operands(const char* who, int op, int nV, int nF, int k, const int* F, const double* V, const double* X, const double* u, const double* v,
                         const double* out)
{
    if (op < SMG_HODGE_RHS || op > SMG_HODGE_FIELD || nV < 1 || nF < 1 || !F || !V || !out) return fail(SMG_ERR_INVALID, "%s: bad arguments", who);
    const bool needs_x = op != SMG_HODGE_FIELD, needs_uv = op != SMG_HODGE_RHS;
    if ((needs_x && !X) || (needs_uv && (!u || !v))) return fail(SMG_ERR_INVALID, "%s: op %d misses an operand", who, op);
    if (k < 1) return fail(SMG_ERR_INVALID, "%s: k = %d, at least one field is needed", who, k);
    return check_faces(who, F, nF, nV);
}

}  // namespace smg

namespace {

int create_impl(const smg_hierarchy* h, const double* V, int nV, const int* F, int nF, smg_hodge** out)
{
    if (out) *out = nullptr;
    const char* who = "smg_hodge_create";
    if (!h || !V || !F || !out || nV <= 0 || nF <= 0) return fail(SMG_ERR_INVALID, "%s: bad arguments", who);
    if (int rc = check_hierarchy(who, h, 1, nV)) return rc;
    if (int rc = check_mesh(who, V, nV, F, nF, true)) return rc;
    const std::vector<int> bnd = boundary_vertices(F, nF, nV);
    if ((int)bnd.size() >= nV) return fail(SMG_ERR_INVALID, "%s: no interior vertex: every vertex is on the boundary", who);

    std::unique_ptr<smg_hodge> g(new smg_hodge());
    g->nV = nV; g->nF = nF; g->nb = (int)bnd.size();
    if (int rc = g->open(who)) return rc;
    if (int rc = g->clone(who, h, 0)) return rc;
    if (g->nb > 0)
        if (int rc = g->clone(who, h, 1)) return rc;

    // the geometry of a query, then -L with the known rows of each handle: precomputed once
    HIPCHK(g->V.upload(std::vector<double>(V, V + (size_t)nV * 3)));
    if (int rc = upload_faces(F, nF, nV, g->F, g->m_ptr, g->m_idx)) return rc;
    HIPCHK(g->W.alloc((size_t)nF * 9));
    HIPCHK(g->nrm.alloc((size_t)nF * 3));
    HIPCHK(g->Af.alloc((size_t)nF));
    HIPCHK(launch_hodge_geometry(g->V.p, g->F.p, nF, g->W.p, g->nrm.p, g->Af.p, g->stream));
    CotanSystem S;
    if (int rc = cotan_system(F, nF, nV, g->V.p, 0, 0.0, -1.0, g->stream, S, false)) return rc;
    for (double& x : S.L) x = -x;
    const int pin = 0;
    if (int rc = smg_precompute(g->handle[0], nV, S.ptr.data(), S.col.data(), S.L.data(), &pin, 1)) return rc;
    if (g->nb > 0)
        if (int rc = smg_precompute(g->handle[1], nV, S.ptr.data(), S.col.data(), S.L.data(), bnd.data(), g->nb)) return rc;
    *out = g.release();
    return SMG_OK;
}

// what the two queries check alike, in this order: the object and the required blocks, k, the memspace, the leading dimensions
int check_call(const char* who, const smg_hodge* g, const double* X, const double* u, int ld_u, const double* v, int ld_v, int k, int memspace)
{
    if (!g || !X || !u || !v) return fail(SMG_ERR_INVALID, "%s: bad arguments", who);
    if (k < 1) return fail(SMG_ERR_INVALID, "%s: k = %d, at least one field is needed", who, k);
    if (2LL * g->nV * k > INT_MAX || 4LL * g->nF * k > INT_MAX)
        return fail(SMG_ERR_INVALID, "%s: k = %d fields of %d vertices and %d faces exceed the index range", who, k, g->nV, g->nF);
    if (bad_memspace(memspace)) return fail(SMG_ERR_INVALID, "%s: memspace must be SMG_HOST or SMG_DEVICE", who);
    if (ld_u < g->nV || ld_v < g->nV) return fail(SMG_ERR_INVALID, "%s: a leading dimension is too small", who);
    return SMG_OK;
}

// the blocks of a k-field query; they grow with the largest k seen and are kept
int ensure_sets(smg_hodge* g, int k)
{
    const size_t n = (size_t)g->nV, nf = (size_t)g->nF, cols = 2 * (size_t)k;
    if (g->kcap >= (size_t)k) return SMG_OK;
    HIPCHK(hipStreamSynchronize(g->stream));
    HIPCHK(g->B.alloc(n * cols));
    HIPCHK(g->Z.alloc(n * cols));
    HIPCHK(g->zero.alloc(n * cols));
    HIPCHK(g->bsq.alloc(n * cols));
    HIPCHK(g->terms.alloc(4 * nf * k));
    HIPCHK(g->part.alloc((size_t)fixed_sum_groups((int)std::max(n * cols, nf))));
    HIPCHK(g->sums.alloc(2 + 4 * (size_t)k));
    HIPCHK(hipMemsetAsync(g->zero.p, 0, n * cols * sizeof(double), g->stream));
    g->kcap = (size_t)k;
    return SMG_OK;
}

int decompose_impl(smg_hodge* g, const double* X, int k, int memspace, const smg_solve_opts* opts, double* u, int ld_u, double* v, int ld_v,
                   double* parts, double* energy, int* cycles)
{
    const char* who = "smg_hodge_decompose";
    if (int rc = check_call(who, g, X, u, ld_u, v, ld_v, k, memspace)) return rc;
    DeviceScope dsc(g->device);
    const int n = g->nV, nF = g->nF;
    const size_t nk = (size_t)n * k;
    hipStream_t st = g->stream;
    if (int rc = ensure_sets(g, k)) return rc;
    const double* dX = X;
    if (memspace == SMG_HOST) {
        HIPCHK(g->Xs.ensure((size_t)k * nF * 3));
        HIPCHK(hipMemcpyAsync(g->Xs.p, X, (size_t)k * nF * 3 * sizeof(double), hipMemcpyHostToDevice, st));
        dX = g->Xs.p;
    }
    double* b = g->B.p;
    double* c = g->B.p + nk;
    HIPCHK(launch_hodge_rhs(n, k, nF, g->m_ptr.p, g->m_idx.p, g->F.p, g->V.p, g->nrm.p, dX, b, c, n, g->bsq.p, st));

    // |rhs|_F^2 over each solve's columns: closed, the 2k columns of the one solve; with boundary, b's and c's
    double ss[2] = {0.0, 0.0};
    const bool closed = g->nb == 0;
    if (closed) {
        HIPCHK(launch_fixed_sum(g->bsq.p, (int)(2 * nk), g->part.p, g->sums.p, st));
    } else {
        HIPCHK(launch_fixed_sum(g->bsq.p, (int)nk, g->part.p, g->sums.p, st));
        HIPCHK(launch_fixed_sum(g->bsq.p + nk, (int)nk, g->part.p, g->sums.p + 1, st));
    }
    HIPCHK(hipMemcpyAsync(ss, g->sums.p, (closed ? 1 : 2) * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (!std::isfinite(ss[0]) || !std::isfinite(ss[1])) return fail(SMG_ERR_NONFINITE, "%s: the right-hand side is not finite", who);

    double* zu = g->Z.p;
    double* zv = g->Z.p + nk;
    int entries[2] = {0, 0};
    if (closed) {
        const smg_solve_opts so = opts_or_default(opts, 1e-10 * std::sqrt(ss[0]), 100);
        if (int rc = inner_solve(g->handle[0], g->pcg, b, n, g->zero.p, 1, g->zero.p, n, 2 * k, so, zu, n, &entries[0])) return rc;
        entries[1] = entries[0];
    } else {
        const smg_solve_opts su = opts_or_default(opts, 1e-10 * std::sqrt(ss[0]), 100);
        if (int rc = inner_solve(g->handle[0], g->pcg, b, n, g->zero.p, 1, g->zero.p, n, k, su, zu, n, &entries[0])) return rc;
        const smg_solve_opts sv = opts_or_default(opts, 1e-10 * std::sqrt(ss[1]), 100);
        if (int rc = inner_solve(g->handle[1], g->pcg, c, n, g->zero.p, g->nb, g->zero.p, n, k, sv, zv, n, &entries[1])) return rc;
    }
    HIPCHK(copy_columns(u, ld_u, zu, n, n, k, copy_out(memspace), st));
    HIPCHK(copy_columns(v, ld_v, zv, n, n, k, copy_out(memspace), st));

    if (parts || energy) {
        double* dP = parts;
        if (parts && memspace == SMG_HOST) {
            HIPCHK(g->Ps.ensure((size_t)k * nF * 9));
            dP = g->Ps.p;
        }
        HIPCHK(launch_hodge_parts(nF, k, g->F.p, g->W.p, g->nrm.p, g->Af.p, dX, zu, n, zv, n, dP, g->terms.p, st));
        if (parts && memspace == SMG_HOST) HIPCHK(hipMemcpyAsync(parts, dP, (size_t)k * nF * 9 * sizeof(double), hipMemcpyDeviceToHost, st));
        if (energy) {
            for (int e = 0; e < 4 * k; e++) HIPCHK(launch_fixed_sum(g->terms.p + (size_t)e * nF, nF, g->part.p, g->sums.p + 2 + e, st));
            HIPCHK(hipMemcpyAsync(energy, g->sums.p + 2, 4 * (size_t)k * sizeof(double), hipMemcpyDeviceToHost, st));
        }
    }
    HIPCHK(hipStreamSynchronize(st));
    if (cycles) { cycles[0] = entries[0]; cycles[1] = entries[1]; }
    return SMG_OK;
}

int field_impl(smg_hodge* g, const double* u, int ld_u, const double* v, int ld_v, int k, int memspace, double* X)
{
    const char* who = "smg_hodge_field";
    if (int rc = check_call(who, g, X, u, ld_u, v, ld_v, k, memspace)) return rc;
    DeviceScope dsc(g->device);
    const int n = g->nV, nF = g->nF;
    const size_t nk = (size_t)n * k, count = (size_t)k * nF * 3;
    hipStream_t st = g->stream;
    if (int rc = ensure_sets(g, k)) return rc;
    if (memspace == SMG_HOST) {
        HIPCHK(g->Xs.ensure(count));
        HIPCHK(copy_columns(g->Z.p, n, u, ld_u, n, k, hipMemcpyHostToDevice, st));
        HIPCHK(copy_columns(g->Z.p + nk, n, v, ld_v, n, k, hipMemcpyHostToDevice, st));
        HIPCHK(launch_hodge_field(nF, k, g->F.p, g->W.p, g->nrm.p, g->Z.p, n, g->Z.p + nk, n, g->Xs.p, st));
        HIPCHK(hipMemcpyAsync(X, g->Xs.p, count * sizeof(double), hipMemcpyDeviceToHost, st));
    } else {
        HIPCHK(launch_hodge_field(nF, k, g->F.p, g->W.p, g->nrm.p, u, ld_u, v, ld_v, X, st));
    }
    HIPCHK(hipStreamSynchronize(st));
    return SMG_OK;
}

}  // namespace

extern "C" int smg_hodge_create(const smg_hierarchy* h, const double* V, int nV, const int* F, int nF, smg_hodge** out)
{
    return guarded("smg_hodge_create", [&]() { return create_impl(h, V, nV, F, nF, out); });
}

extern "C" void smg_hodge_destroy(smg_hodge* g) { delete g; }

extern "C" int smg_hodge_set_solver(smg_hodge* g, int pcg)
{
    if (!g) return fail(SMG_ERR_INVALID, "smg_hodge_set_solver: null object");
    latch_solver(g->pcg, pcg);
    return SMG_OK;
}

extern "C" int smg_hodge_is_closed(const smg_hodge* g) { return g && g->nb == 0 ? 1 : 0; }

extern "C" long long smg_hodge_device_bytes(const smg_hodge* g)
{
    if (!g) return 0;   // one list: every DevBuf of the struct
    return device_bytes(*g, g->F, g->m_ptr, g->m_idx, g->V, g->W, g->nrm, g->Af, g->Xs, g->Ps, g->B, g->Z, g->zero, g->bsq, g->part, g->terms, g->sums);
}

extern "C" int smg_hodge_decompose(smg_hodge* g, const double* X, int k, int memspace, const smg_solve_opts* opts, double* u, int ld_u, double* v,
                                   int ld_v, double* parts, double* energy, int* cycles)
{
    return guarded("smg_hodge_decompose", [&]() { return decompose_impl(g, X, k, memspace, opts, u, ld_u, v, ld_v, parts, energy, cycles); });
}

extern "C" int smg_hodge_field(smg_hodge* g, const double* u, int ld_u, const double* v, int ld_v, int k, int memspace, double* X)
{
    return guarded("smg_hodge_field", [&]() { return field_impl(g, u, ld_u, v, ld_v, k, memspace, X); });
}

extern "C" int smg_hodge_host(int op, int nV, int nF, int k, const int* F, const double* V, const double* X, const double* u, const double* v, double* out)
{
    return guarded("smg_hodge_host", [&]() -> int {
        const char* who = "smg_hodge_host";
        if (int rc = hodge_check_operands(who, op, nV, nF, k, F, V, X, u, v, out)) return rc;
        const size_t f = (size_t)nF, nk = (size_t)nV * k;
        if (op == SMG_HODGE_RHS) {
            std::vector<int> mp, mi;
            vertex_corner_lists(std::vector<int>(F, F + 3 * f), nV, mp, mi);
            hodge_host_rhs(nV, nF, k, F, V, mp.data(), mi.data(), X, out, out + nk, out + 2 * nk);
        } else if (op == SMG_HODGE_PARTS) {
            hodge_host_parts(nV, nF, k, F, V, X, u, v, out, out + 9 * f * k, out + 13 * f * k);
        } else {
            hodge_host_field(nV, nF, k, F, V, u, v, out);
        }
        return SMG_OK;
    });
}
