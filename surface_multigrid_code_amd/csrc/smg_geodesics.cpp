// smg_geodesics.cpp -- geodesic distance by the heat method on the V-cycle (include/smg.h: smg_geodesics_*).
// The object owns two handles built from the caller's prolongations -- the heat handle (M - tL) and the Poisson handle (-L, vertex 0 pinned)
// -- and the geometry the three kernels of a query read (csrc/smg_geodesics_device.hip).  A query: scatter the indicator block, heat solve,
// the fused gradient / normalise / divergence kernel, Poisson solve, shift by the sources' mean.  All of it is enqueued on one stream that
// both handles use; the only host synchronisations are the solves' own.  Checks, stream, handles and the cotangent system: smg_mesh_object.hpp.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cmath>
#include <memory>
#include <vector>

#include "smg_device.hpp"
#include "smg_mesh_object.hpp"

using namespace smg;

struct smg_geodesics : MeshObject {
    enum { HEAT = 0, POIS = 1 };          // handle[]: M - tL, and -L with vertex 0 pinned
    int nV = 0, nF = 0, voronoi = 0;
    double t = 0.0, area = 0.0;
    int heat_pcg = 1, pois_pcg = 1;
    DevBuf<int> F, m_ptr, m_idx;          // faces, corner lists per vertex
    DevBuf<double> W, Af;                 // gradient basis (9 per face), face areas
    DevBuf<int> d_src_ptr, d_src;         // the query's source lists
    DevBuf<double> B, U, Z, mean;         // n x kcap blocks: heat RHS / Poisson RHS / staging of D, heat solution / phi, zeros; k means
    int kcap = 0;
    std::vector<int> h_src_ptr, h_src;    // host side of the source lists (alive until the next query: the uploads are asynchronous)
    ~smg_geodesics() { quiesce(); }
};

namespace {

int create_impl(const smg_hierarchy* h, const double* V, int nV, const int* F, int nF, double t, int voronoi, smg_geodesics** out)
{
    if (!h || !V || !F || !out || nV <= 0 || nF <= 0) return fail(SMG_ERR_INVALID, "smg_geodesics_create: bad arguments");
    *out = nullptr;
    const char* who = "smg_geodesics_create";
    double area2 = 0.0;
    if (int rc = check_hierarchy(who, h, 1, nV)) return rc;
    if (int rc = check_mesh(who, V, nV, F, nF, true, &area2)) return rc;
    if (!std::isfinite(t) || t < 0.0) return fail(SMG_ERR_INVALID, "%s: t must be finite and >= 0 (0: the default)", who);
    if (t == 0.0) {   // default: (bounding-box diagonal / 12)^2
        double lo[3], hi[3];
        for (int d = 0; d < 3; d++) lo[d] = hi[d] = V[d];
        for (size_t i = 0; i < (size_t)nV; i++)
            for (int d = 0; d < 3; d++) { lo[d] = std::min(lo[d], V[3 * i + d]); hi[d] = std::max(hi[d], V[3 * i + d]); }
        const double diag = std::sqrt((hi[0] - lo[0]) * (hi[0] - lo[0]) + (hi[1] - lo[1]) * (hi[1] - lo[1]) + (hi[2] - lo[2]) * (hi[2] - lo[2]));
        t = (diag / 12.0) * (diag / 12.0);
    }

    std::unique_ptr<smg_geodesics> g(new smg_geodesics());
    g->nV = nV; g->nF = nF; g->voronoi = voronoi ? 1 : 0; g->t = t; g->area = 0.5 * area2;
    if (int rc = g->open(who)) return rc;
    if (int rc = g->clone(who, h, g->HEAT)) return rc;
    if (int rc = g->clone(who, h, g->POIS)) return rc;

    // the geometry of a query, then M - tL and L on the device and the two precomputes
    DevBuf<double> dV;
    HIPCHK(dV.upload(std::vector<double>(V, V + (size_t)nV * 3)));
    if (int rc = upload_faces(F, nF, nV, g->F, g->m_ptr, g->m_idx)) return rc;
    HIPCHK(g->W.alloc((size_t)nF * 9));
    HIPCHK(g->Af.alloc((size_t)nF));
    HIPCHK(launch_geo_basis(dV.p, g->F.p, nF, g->W.p, g->Af.p, g->stream));
    CotanSystem S;
    if (int rc = cotan_system(F, nF, nV, dV.p, g->voronoi, 1.0, -t, g->stream, S, true)) return rc;
    for (double& v : S.L) v = -v;
    if (int rc = smg_precompute(g->handle[g->HEAT], nV, S.ptr.data(), S.col.data(), S.val.data(), nullptr, 0)) return rc;
    const int pin = 0;
    if (int rc = smg_precompute(g->handle[g->POIS], nV, S.ptr.data(), S.col.data(), S.L.data(), &pin, 1)) return rc;
    *out = g.release();
    return SMG_OK;
}

int solve_impl(smg_geodesics* g, int k, const int* src_ptr, const int* src, int memspace, const smg_solve_opts* heat_opts,
               const smg_solve_opts* poisson_opts, double* D, int ld_d, int* cycles)
{
    if (!g || k < 1 || !src_ptr || !src || !D || ld_d < g->nV || bad_memspace(memspace))
        return fail(SMG_ERR_INVALID, "smg_geodesics_solve: bad arguments");
    const int n = g->nV;
    for (int c = 0; c < k; c++)
        if (src_ptr[c + 1] <= src_ptr[c]) return fail(SMG_ERR_INVALID, "smg_geodesics_solve: source set %d is empty", c);
    const int p0 = src_ptr[0], total = src_ptr[k] - p0;
    for (int p = p0; p < src_ptr[k]; p++)
        if (src[p] < 0 || src[p] >= n) return fail(SMG_ERR_INVALID, "smg_geodesics_solve: source index %d out of range", src[p]);
    DeviceScope dsc(g->device);
    if (k > g->kcap) {
        HIPCHK(hipStreamSynchronize(g->stream));
        HIPCHK(g->B.alloc((size_t)n * k));
        HIPCHK(g->U.alloc((size_t)n * k));
        HIPCHK(g->Z.alloc((size_t)n * k));
        HIPCHK(g->mean.alloc((size_t)k));
        HIPCHK(hipMemsetAsync(g->Z.p, 0, (size_t)n * k * sizeof(double), g->stream));
        g->kcap = k;
    }
    HIPCHK(hipStreamSynchronize(g->stream));   // the previous query's uploads read h_src_ptr / h_src
    g->h_src_ptr.resize((size_t)k + 1);
    for (int c = 0; c <= k; c++) g->h_src_ptr[c] = src_ptr[c] - p0;
    g->h_src.assign(src + p0, src + p0 + total);
    HIPCHK(g->d_src_ptr.ensure((size_t)k + 1));
    HIPCHK(g->d_src.ensure((size_t)total));
    HIPCHK(hipMemcpyAsync(g->d_src_ptr.p, g->h_src_ptr.data(), ((size_t)k + 1) * sizeof(int), hipMemcpyHostToDevice, g->stream));
    HIPCHK(hipMemcpyAsync(g->d_src.p, g->h_src.data(), (size_t)total * sizeof(int), hipMemcpyHostToDevice, g->stream));

    const smg_solve_opts ho = opts_or_default(heat_opts, 1e-11 * std::sqrt((double)total), 100);
    const smg_solve_opts po = opts_or_default(poisson_opts, 1e-11 * std::sqrt((double)k * g->area), 100);
    smg_hierarchy *heat = g->handle[g->HEAT], *pois = g->handle[g->POIS];

    // 1. heat: (M - tL) U = indicator block B
    HIPCHK(launch_geo_scatter(n, k, g->d_src_ptr.p, g->d_src.p, g->B.p, n, g->stream));
    if (int rc = inner_solve(heat, g->heat_pcg, g->B.p, n, nullptr, 0, g->Z.p, n, k, ho, g->U.p, n, cycles)) return rc;
    // 2. B = -div X, X = -grad U / |grad U|
    HIPCHK(launch_geo_divergence(n, k, g->F.p, g->W.p, g->Af.p, g->m_ptr.p, g->m_idx.p, g->U.p, n, g->B.p, n, g->stream));
    // 3. Poisson: -L phi = B, phi_0 = 0 (known values: the zero block read with leading dimension 1)
    if (int rc = inner_solve(pois, g->pois_pcg, g->B.p, n, g->Z.p, 1, g->Z.p, n, k, po, g->U.p, n, cycles ? cycles + 1 : nullptr)) return rc;
    // 4. D = phi - mean over the sources
    if (memspace == SMG_DEVICE) {
        HIPCHK(launch_geo_shift(n, k, g->d_src_ptr.p, g->d_src.p, g->U.p, n, g->mean.p, D, ld_d, g->stream));
        HIPCHK(hipStreamSynchronize(g->stream));
    } else {
        HIPCHK(launch_geo_shift(n, k, g->d_src_ptr.p, g->d_src.p, g->U.p, n, g->mean.p, g->B.p, n, g->stream));
        HIPCHK(copy_columns(D, ld_d, g->B.p, n, n, k, hipMemcpyDeviceToHost, g->stream));
        HIPCHK(hipStreamSynchronize(g->stream));
    }
    return SMG_OK;
}

}  // namespace

extern "C" int smg_geodesics_create(const smg_hierarchy* h, const double* V, int nV, const int* F, int nF, double t, int voronoi, smg_geodesics** out)
{
    return guarded("smg_geodesics_create", [&]() { return create_impl(h, V, nV, F, nF, t, voronoi, out); });
}

extern "C" void smg_geodesics_destroy(smg_geodesics* g) { delete g; }

extern "C" double smg_geodesics_time(const smg_geodesics* g) { return g ? g->t : 0.0; }

extern "C" int smg_geodesics_set_solver(smg_geodesics* g, int heat_pcg, int poisson_pcg)
{
    if (!g) return fail(SMG_ERR_INVALID, "null geodesics object");
    latch_solver(g->heat_pcg, heat_pcg);
    latch_solver(g->pois_pcg, poisson_pcg);
    return SMG_OK;
}

extern "C" long long smg_geodesics_device_bytes(const smg_geodesics* g)
{
    return g ? device_bytes(*g, g->F, g->m_ptr, g->m_idx, g->W, g->Af, g->d_src_ptr, g->d_src, g->B, g->U, g->Z, g->mean) : 0;
}

extern "C" int smg_geodesics_solve(smg_geodesics* g, int k, const int* src_ptr, const int* src, int memspace, const smg_solve_opts* heat_opts,
                                   const smg_solve_opts* poisson_opts, double* D, int ld_d, int* cycles)
{
    return guarded("smg_geodesics_solve", [&]() { return solve_impl(g, k, src_ptr, src, memspace, heat_opts, poisson_opts, D, ld_d, cycles); });
}
