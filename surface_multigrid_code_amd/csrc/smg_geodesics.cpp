// smg_geodesics.cpp -- geodesic distance by the heat method on the V-cycle (include/smg.h: smg_geodesics_*).
// The object owns two handles built from the caller's prolongations -- the heat handle (M - tL) and the Poisson handle (-L, vertex 0 pinned)
// -- and the geometry the three kernels of a query read (csrc/smg_geodesics_device.hip).  A query: scatter the indicator block, heat solve,
// the fused gradient / normalise / divergence kernel, Poisson solve, shift by the sources' mean.  All of it is enqueued on one stream that
// both handles use; the only host synchronisations are the solves' own.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <numeric>
#include <string>
#include <vector>

#include "smg_bsr3.hpp"
#include "smg_device.hpp"
#include "smg_internal.hpp"

using namespace smg;

struct smg_geodesics {
    smg_hierarchy* heat = nullptr;
    smg_hierarchy* pois = nullptr;
    hipStream_t stream = nullptr;
    int device = -1;
    int nV = 0, nF = 0, voronoi = 0;
    double t = 0.0, area = 0.0;
    int heat_pcg = 1, pois_pcg = 1;
    DevBuf<int> F, m_ptr, m_idx;          // faces, corner lists per vertex
    DevBuf<double> W, Af;                 // gradient basis (9 per face), face areas
    DevBuf<int> d_src_ptr, d_src;         // the query's source lists
    DevBuf<double> B, U, Z, mean;         // n x kcap blocks: heat RHS / Poisson RHS / staging of D, heat solution / phi, zeros; k means
    int kcap = 0;
    std::vector<int> h_src_ptr, h_src;    // host side of the source lists (alive until the next query: the uploads are asynchronous)
    ~smg_geodesics()
    {
        if (stream) (void)hipStreamSynchronize(stream);
        if (pois) smg_hierarchy_destroy(pois);
        if (heat) smg_hierarchy_destroy(heat);
        F.release(); m_ptr.release(); m_idx.release(); W.release(); Af.release(); d_src_ptr.release(); d_src.release();
        B.release(); U.release(); Z.release(); mean.release();
        if (stream) (void)hipStreamDestroy(stream);
    }
};

// ---- what every object built on a mesh and a caller's hierarchy checks and copies (smg_internal.hpp; smg_arap.cpp uses them too) ----
namespace smg {

// twice the area of face f, the expression of k_face_terms / k_geo_basis
double double_area(const double* V, const int* F, int f)
{
    const double* a = V + 3 * (size_t)F[3 * (size_t)f];
    const double* b = V + 3 * (size_t)F[3 * (size_t)f + 1];
    const double* c = V + 3 * (size_t)F[3 * (size_t)f + 2];
    const double ux = b[0] - a[0], uy = b[1] - a[1], uz = b[2] - a[2];
    const double vx = c[0] - a[0], vy = c[1] - a[1], vz = c[2] - a[2];
    const double wx = uy * vz - uz * vy, wy = uz * vx - ux * vz, wz = ux * vy - uy * vx;
    return std::sqrt(wx * wx + wy * wy + wz * wz);
}

// number of connected components of the vertex graph of F (a vertex in no face is a component of its own)
int components(const int* F, int nF, int nV)
{
    std::vector<int> parent(nV);
    std::iota(parent.begin(), parent.end(), 0);
    auto find = [&](int x) { while (parent[x] != x) { parent[x] = parent[parent[x]]; x = parent[x]; } return x; };
    for (size_t f = 0; f < (size_t)nF; f++)
        for (int c = 1; c < 3; c++) {
            const int a = find(F[3 * f]), b = find(F[3 * f + c]);
            if (a != b) parent[std::max(a, b)] = std::min(a, b);
        }
    int n = 0;
    for (int v = 0; v < nV; v++) n += find(v) == v ? 1 : 0;
    return n;
}

// rows of level 0 of a hierarchy whose prolongations are set (-1: none set)
int level0_rows(const smg_hierarchy* h)
{
    if (h->n_levels >= 2) return h->lv[1].P_full.nr > 0 ? h->lv[1].P_full.nr : -1;
    return h->lv[0].V.empty() ? -1 : (int)(h->lv[0].V.size() / 3);
}

long long handle_bytes(const smg_hierarchy* h)
{
    std::vector<char> buf(1 << 16);
    if (smg_debug_device_bytes(h, buf.data(), (int)buf.size()) != SMG_OK) return 0;
    const char* tot = std::strstr(buf.data(), "total ");
    return tot ? std::atoll(tot + 6) : 0;
}

int copy_prolongations(const smg_hierarchy* src, smg_hierarchy* dst)
{
    for (int lv = 1; lv < src->n_levels; lv++) {
        Csr P = src->lv[lv].P_full;
        if (int rc = set_prolong(dst, lv, std::move(P))) return rc;
    }
    return SMG_OK;
}

}  // namespace smg

namespace {

int create_impl(const smg_hierarchy* h, const double* V, int nV, const int* F, int nF, double t, int voronoi, smg_geodesics** out)
{
    if (!h || !V || !F || !out || nV <= 0 || nF <= 0) return fail(SMG_ERR_INVALID, "smg_geodesics_create: bad arguments");
    *out = nullptr;
    if (!std::isfinite(t) || t < 0.0) return fail(SMG_ERR_INVALID, "smg_geodesics_create: t must be finite and >= 0 (0: the default)");
    if (h->union_m > 0) return fail(SMG_ERR_INVALID, "smg_geodesics_create: union handles are not supported");
    Csr Pv;
    if (h->bs == 3 || h->block_mode == 3 || (h->n_levels >= 2 && h->lv[1].P_full.nr > 0 && kron3_factor(h->lv[1].P_full, Pv)))
        return fail(SMG_ERR_INVALID, "smg_geodesics_create: block (3-DOF) hierarchies are not supported");
    const int rows = level0_rows(h);
    if (rows != nV) return fail(SMG_ERR_INVALID, "smg_geodesics_create: nV = %d, but level 0 of the hierarchy has %d rows", nV, rows);
    for (size_t i = 0; i < (size_t)nF * 3; i++)
        if (F[i] < 0 || F[i] >= nV) return fail(SMG_ERR_INVALID, "smg_geodesics_create: face index out of range");
    double area2 = 0.0;
    for (int f = 0; f < nF; f++) {
        const double dA = double_area(V, F, f);
        if (!(dA > 0.0)) return fail(SMG_ERR_INVALID, "smg_geodesics_create: face %d has zero double area", f);
        area2 += dA;
    }
    for (size_t i = 0; i < (size_t)nV * 3; i++)
        if (!std::isfinite(V[i])) return fail(SMG_ERR_INVALID, "smg_geodesics_create: non-finite vertex coordinate");
    if (const int nc = components(F, nF, nV); nc != 1)
        return fail(SMG_ERR_INVALID, "smg_geodesics_create: the mesh has %d connected components (vertices in no face count)", nc);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(SMG_ERR_NO_DEVICE, "smg_geodesics_create: no HIP device: libsmg has no CPU fallback");

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
    HIPCHK(hipGetDevice(&g->device));
    HIPCHK(hipStreamCreateWithFlags(&g->stream, hipStreamNonBlocking));
    g->heat = smg_hierarchy_create(h->n_levels);
    g->pois = smg_hierarchy_create(h->n_levels);
    if (!g->heat || !g->pois) return fail(SMG_ERR_ALLOC, "smg_geodesics_create: out of memory");
    if (int rc = copy_prolongations(h, g->heat)) return rc;
    if (int rc = copy_prolongations(h, g->pois)) return rc;
    if (int rc = smg_hierarchy_set_stream(g->heat, g->stream)) return rc;
    if (int rc = smg_hierarchy_set_stream(g->pois, g->stream)) return rc;

    // M - tL and L on the device (smg_assemble), then the two precomputes
    smg_assembler* a = nullptr;
    if (int rc = smg_assembler_create(F, nF, nV, &a)) return rc;
    struct AsmOwner { smg_assembler* a; ~AsmOwner() { smg_assembler_destroy(a); } } own_a{a};
    int nnz = 0;
    smg_assembler_pattern(a, &nnz, nullptr, nullptr);
    std::vector<int> ptr((size_t)nV + 1), col((size_t)nnz);
    smg_assembler_pattern(a, nullptr, ptr.data(), col.data());
    std::vector<double> hval((size_t)nnz), lval((size_t)nnz);
    {
        DevBuf<double> dV, dval, dL;
        std::vector<double> Vh(V, V + (size_t)nV * 3);
        HIPCHK(dV.upload(Vh));
        HIPCHK(dval.alloc((size_t)nnz));
        HIPCHK(dL.alloc((size_t)nnz));
        if (int rc = smg_assemble(a, dV.p, g->voronoi, 1.0, -t, dval.p, nullptr, dL.p, g->stream)) return rc;
        std::vector<int> Fh(F, F + (size_t)nF * 3), mp, mi;
        vertex_corner_lists(Fh, nV, mp, mi);
        HIPCHK(g->F.upload(Fh));
        HIPCHK(g->m_ptr.upload(mp));
        HIPCHK(g->m_idx.upload(mi));
        HIPCHK(g->W.alloc((size_t)nF * 9));
        HIPCHK(g->Af.alloc((size_t)nF));
        HIPCHK(launch_geo_basis(dV.p, g->F.p, nF, g->W.p, g->Af.p, g->stream));
        HIPCHK(hipStreamSynchronize(g->stream));
        HIPCHK(hipMemcpy(hval.data(), dval.p, (size_t)nnz * sizeof(double), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(lval.data(), dL.p, (size_t)nnz * sizeof(double), hipMemcpyDeviceToHost));
    }
    for (double& v : lval) v = -v;
    if (int rc = smg_precompute(g->heat, nV, ptr.data(), col.data(), hval.data(), nullptr, 0)) return rc;
    const int pin = 0;
    if (int rc = smg_precompute(g->pois, nV, ptr.data(), col.data(), lval.data(), &pin, 1)) return rc;
    *out = g.release();
    return SMG_OK;
}

int solve_impl(smg_geodesics* g, int k, const int* src_ptr, const int* src, int memspace, const smg_solve_opts* heat_opts,
               const smg_solve_opts* poisson_opts, double* D, int ld_d, int* cycles)
{
    if (!g || k < 1 || !src_ptr || !src || !D || ld_d < g->nV || (memspace != SMG_HOST && memspace != SMG_DEVICE))
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

    smg_solve_opts ho, po;
    if (heat_opts) ho = *heat_opts;
    else { smg_solve_opts_default(&ho); ho.max_iter = 100; ho.tol = 1e-11 * std::sqrt((double)total); }
    if (poisson_opts) po = *poisson_opts;
    else { smg_solve_opts_default(&po); po.max_iter = 100; po.tol = 1e-11 * std::sqrt((double)k * g->area); }
    std::vector<double> his((size_t)std::max(1, std::max(ho.max_iter, po.max_iter)));
    int nh = 0, conv = 0, rc = SMG_OK;

    // 1. heat: (M - tL) U = indicator block B
    HIPCHK(launch_geo_scatter(n, k, g->d_src_ptr.p, g->d_src.p, g->B.p, n, g->stream));
    rc = (g->heat_pcg ? smg_solve_pcg : smg_solve)(g->heat, g->B.p, n, nullptr, 0, g->Z.p, n, k, SMG_DEVICE, &ho, g->U.p, n, his.data(), &nh, &conv);
    if (rc) return rc;
    if (cycles) cycles[0] = nh;
    // 2. B = -div X, X = -grad U / |grad U|
    HIPCHK(launch_geo_divergence(n, k, g->F.p, g->W.p, g->Af.p, g->m_ptr.p, g->m_idx.p, g->U.p, n, g->B.p, n, g->stream));
    // 3. Poisson: -L phi = B, phi_0 = 0 (known values: the zero block read with leading dimension 1)
    rc = (g->pois_pcg ? smg_solve_pcg : smg_solve)(g->pois, g->B.p, n, g->Z.p, 1, g->Z.p, n, k, SMG_DEVICE, &po, g->U.p, n, his.data(), &nh, &conv);
    if (rc) return rc;
    if (cycles) cycles[1] = nh;
    // 4. D = phi - mean over the sources
    if (memspace == SMG_DEVICE) {
        HIPCHK(launch_geo_shift(n, k, g->d_src_ptr.p, g->d_src.p, g->U.p, n, g->mean.p, D, ld_d, g->stream));
        HIPCHK(hipStreamSynchronize(g->stream));
    } else {
        HIPCHK(launch_geo_shift(n, k, g->d_src_ptr.p, g->d_src.p, g->U.p, n, g->mean.p, g->B.p, n, g->stream));
        HIPCHK(hipMemcpy2DAsync(D, (size_t)ld_d * sizeof(double), g->B.p, (size_t)n * sizeof(double), (size_t)n * sizeof(double), (size_t)k,
                                hipMemcpyDeviceToHost, g->stream));
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
    if (heat_pcg >= 0) g->heat_pcg = heat_pcg ? 1 : 0;
    if (poisson_pcg >= 0) g->pois_pcg = poisson_pcg ? 1 : 0;
    return SMG_OK;
}

extern "C" long long smg_geodesics_device_bytes(const smg_geodesics* g)
{
    if (!g) return 0;
    auto B = [](const auto& d) { return (long long)(d.n * sizeof(*d.p)); };
    return handle_bytes(g->heat) + handle_bytes(g->pois) + B(g->F) + B(g->m_ptr) + B(g->m_idx) + B(g->W) + B(g->Af) + B(g->d_src_ptr) +
           B(g->d_src) + B(g->B) + B(g->U) + B(g->Z) + B(g->mean);
}

extern "C" int smg_geodesics_solve(smg_geodesics* g, int k, const int* src_ptr, const int* src, int memspace, const smg_solve_opts* heat_opts,
                                   const smg_solve_opts* poisson_opts, double* D, int ld_d, int* cycles)
{
    return guarded("smg_geodesics_solve", [&]() { return solve_impl(g, k, src_ptr, src, memspace, heat_opts, poisson_opts, D, ld_d, cycles); });
}
