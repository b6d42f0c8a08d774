// smg_param.cpp -- harmonic and as-rigid-as-possible flattening of a disk mesh on the V-cycle (include/smg.h: smg_param_*).
// The object owns two handles built from the caller's prolongations, both precomputed with -L of the mesh: handle[0] with the boundary loop
// known (the harmonic map to the circle), handle[1] with the loop's first vertex known (the global step of ARAP).  On the device it keeps the
// faces, the rest constants of every face (k_param_rest), the corner lists of the vertices and the buffers of an iteration.
// One ARAP iteration: rotations + energy terms (k_param_local), the energy (fixed-order reduction), the right-hand side (k_param_rhs), one
// 2-column solve warm-started at the iterate.  All of it is enqueued on the object's stream, which the handles use too; per iteration the host
// reads one energy double beside the solve's own history.  Checks, stream, handles, the cotangent system and the inner solve:
// smg_mesh_object.hpp; the loop and its stopping rule: smg_local_global.hpp; the sums: launch_fixed_sum / launch_fixed_max.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <memory>
#include <vector>

#include "smg_device.hpp"
#include "smg_local_global.hpp"
#include "smg_mesh.hpp"
#include "smg_mesh_object.hpp"
#include "smg_param_inl.hpp"

using namespace smg;

struct smg_param : MeshObject {           // handle[0]: -L, the boundary loop known; handle[1]: -L, loop[0] known
    int nV = 0, nF = 0, nl = 0;
    int pcg = 1;                          // the inner solver: 1 smg_solve_pcg, 0 smg_solve
    double scale_arap = 0.0;              // s = sqrt(sum_v (sum over v's corners of param_corner_bound)^2) >= |rhs|_F for every set of rotations
    double scale_harmonic = 0.0;          // |-(-L)_ub u_b|_F, the reduced right-hand side of the harmonic solve
    std::vector<int> loop;                // the boundary loop, as smg_mesh_boundary_loop returns it
    DevBuf<int> F, m_ptr, m_idx;          // faces; the corner lists t = 3 f + i of every vertex, faces ascending
    DevBuf<double> rest, circle;          // rest constants (6 planes); the circle positions of the loop (nl x 2 column-major)
    DevBuf<double> R, eterm, part, E;     // rotations (2 planes), energy terms, their chunk sums, E_t
    DevBuf<double> B, Ua, Ub, pin;        // column-major nV x 2: right-hand side, the iterate and the solve's result; the pinned row (1 x 2)
    DevBuf<double> sigma, terms, stats;   // distortion: sigma (2 planes), the statistics' terms (7 planes), their reductions (7)
    ~smg_param() { quiesce(); }
};

namespace {

// The topology of a disk: every edge in at most two faces (and then once in each direction), one boundary loop, Euler characteristic 1.
int check_disk(const char* who, const int* F, int nF, int nV)
{
    std::vector<uint64_t> keys((size_t)nF * 3);           // (lo, hi, direction) of every half-edge
    for (size_t f = 0; f < (size_t)nF; f++)
        for (int i = 0; i < 3; i++) {
            const int a = F[3 * f + i], b = F[3 * f + (i + 1) % 3];
            if (a == b) return fail(SMG_ERR_INVALID, "%s: face %d repeats vertex %d", who, (int)f, a);
            const uint64_t lo = (uint64_t)std::min(a, b), hi = (uint64_t)std::max(a, b);
            keys[3 * f + i] = (lo << 33) | (hi << 1) | (a < b ? 0u : 1u);
        }
    std::sort(keys.begin(), keys.end());
    long long nE = 0, nB = 0;
    std::vector<int> next((size_t)nV, -1);                // the boundary half-edge that leaves a vertex
    for (size_t q = 0; q < keys.size();) {
        size_t e = q;
        while (e < keys.size() && (keys[e] >> 1) == (keys[q] >> 1)) e++;
        const int lo = (int)(keys[q] >> 33), hi = (int)((keys[q] >> 1) & 0xffffffffu);
        if (e - q > 2) return fail(SMG_ERR_INVALID, "%s: edge (%d, %d) is shared by %d faces: the mesh is not manifold", who, lo, hi, (int)(e - q));
        if (e - q == 2 && keys[q] == keys[q + 1])
            return fail(SMG_ERR_INVALID, "%s: the two faces at edge (%d, %d) are not consistently oriented", who, lo, hi);
        if (e - q == 1) {
            const int from = (keys[q] & 1) ? hi : lo, to = (keys[q] & 1) ? lo : hi;
            if (next[from] >= 0) return fail(SMG_ERR_INVALID, "%s: boundary vertex %d is not manifold", who, from);
            next[from] = to;
            nB++;
        }
        nE++;
        q = e;
    }
    if (nB == 0) return fail(SMG_ERR_INVALID, "%s: the mesh is closed: a disk has one boundary loop", who);
    int loops = 0;
    std::vector<char> seen((size_t)nV, 0);
    for (int s = 0; s < nV; s++) {
        if (next[s] < 0 || seen[s]) continue;
        loops++;
        for (int v = s; v >= 0 && !seen[v]; v = next[v]) seen[v] = 1;
    }
    if (loops != 1) return fail(SMG_ERR_INVALID, "%s: the mesh has %d boundary loops, a disk has one", who, loops);
    const long long chi = (long long)nV - nE + nF;
    if (chi != 1) return fail(SMG_ERR_INVALID, "%s: Euler characteristic %lld, a disk has 1", who, chi);
    return SMG_OK;
}

// the loop on the circle of area `area`, by cumulative 3D edge length from angle 0 (libigl's map_vertices_to_circle, scaled); nl x 2 column-major
std::vector<double> circle_positions(const double* V, const std::vector<int>& loop, double area)
{
    const size_t nl = loop.size();
    auto dist = [&](int a, int b) {
        const double dx = V[3 * (size_t)a] - V[3 * (size_t)b], dy = V[3 * (size_t)a + 1] - V[3 * (size_t)b + 1], dz = V[3 * (size_t)a + 2] - V[3 * (size_t)b + 2];
        return std::sqrt(dx * dx + dy * dy + dz * dz);
    };
    std::vector<double> len(nl, 0.0), uv(2 * nl);
    for (size_t i = 1; i < nl; i++) len[i] = len[i - 1] + dist(loop[i - 1], loop[i]);
    const double total = len[nl - 1] + dist(loop[nl - 1], loop[0]);
    const double pi = 3.141592653589793, radius = std::sqrt(area / pi);
    for (size_t i = 0; i < nl; i++) {
        const double theta = len[i] * (2.0 * pi) / total;
        uv[i] = radius * std::cos(theta);
        uv[nl + i] = radius * std::sin(theta);
    }
    return uv;
}

int create_impl(const smg_hierarchy* h, const double* V, int nV, const int* F, int nF, smg_param** out)
{
    if (out) *out = nullptr;
    const char* who = "smg_param_create";
    if (!h || !V || !F || !out || nV <= 0 || nF <= 0) return fail(SMG_ERR_INVALID, "%s: bad arguments", who);
    if (int rc = check_hierarchy(who, h, 1, nV)) return rc;
    double area2 = 0.0;
    if (int rc = check_mesh(who, V, nV, F, nF, true, &area2)) return rc;
    if (int rc = check_disk(who, F, nF, nV)) return rc;

    std::unique_ptr<smg_param> p(new smg_param());
    p->nV = nV; p->nF = nF;
    Mesh m;
    m.F.assign(F, F + 3 * (size_t)nF);
    p->loop = boundary_loop(m);
    p->nl = (int)p->loop.size();
    if (p->nl >= nV) return fail(SMG_ERR_INVALID, "%s: every vertex is on the boundary: nothing to solve", who);

    const std::vector<double> circle = circle_positions(V, p->loop, 0.5 * area2);

    if (int rc = p->open(who)) return rc;
    if (int rc = p->clone(who, h, 0)) return rc;
    if (int rc = p->clone(who, h, 1)) return rc;

    // the rest constants on the host (the text the device compiles): the scale of the ARAP right-hand side
    std::vector<int> mp, mi;
    if (int rc = upload_faces(F, nF, nV, p->F, p->m_ptr, p->m_idx, &mp, &mi)) return rc;
    {
        std::vector<double> bound(3 * (size_t)nF);
        for (size_t f = 0; f < (size_t)nF; f++) {
            double r[6];
            param_rest(V + 3 * (size_t)F[3 * f], V + 3 * (size_t)F[3 * f + 1], V + 3 * (size_t)F[3 * f + 2], r);
            for (int i = 0; i < 3; i++) bound[3 * f + i] = param_corner_bound(r, i);
        }
        double ss = 0.0;
        for (int v = 0; v < nV; v++) {
            double row = 0.0;
            for (int q = mp[v]; q < mp[v + 1]; q++) row += bound[mi[q]];
            ss += row * row;
        }
        p->scale_arap = std::sqrt(ss);
    }

    // -L on the host as CSR (assembled on the device): the matrix of both handles
    DevBuf<double> dV;
    HIPCHK(dV.upload(std::vector<double>(V, V + (size_t)nV * 3)));
    CotanSystem S;
    if (int rc = cotan_system(F, nF, nV, dV.p, 0, 0.0, -1.0, p->stream, S, false)) return rc;
    for (double& v : S.L) v = -v;
    {
        // the reduced right-hand side of the harmonic solve, -(-L)_ub u_b, for its norm alone
        std::vector<int> at((size_t)nV, -1);
        for (int r = 0; r < p->nl; r++) at[p->loop[r]] = r;
        double ss = 0.0;
        for (int i = 0; i < nV; i++) {
            if (at[i] >= 0) continue;
            double bx = 0.0, by = 0.0;
            for (int q = S.ptr[i]; q < S.ptr[i + 1]; q++)
                if (const int r = at[S.col[q]]; r >= 0) { bx -= S.L[q] * circle[r]; by -= S.L[q] * circle[(size_t)p->nl + r]; }
            ss += bx * bx + by * by;
        }
        p->scale_harmonic = std::sqrt(ss);
    }
    if (int rc = smg_precompute(p->handle[0], nV, S.ptr.data(), S.col.data(), S.L.data(), p->loop.data(), p->nl)) return rc;
    if (int rc = smg_precompute(p->handle[1], nV, S.ptr.data(), S.col.data(), S.L.data(), p->loop.data(), 1)) return rc;

    HIPCHK(p->circle.upload(circle));
    const size_t n = (size_t)nV, nf = (size_t)nF;
    HIPCHK(p->rest.alloc(6 * nf));
    HIPCHK(launch_param_rest(nF, p->F.p, dV.p, p->rest.p, p->stream));
    HIPCHK(hipStreamSynchronize(p->stream));             // dV leaves with this scope
    HIPCHK(p->R.alloc(2 * nf));
    HIPCHK(p->eterm.alloc(nf));
    HIPCHK(p->part.alloc((size_t)fixed_sum_groups(nF)));
    HIPCHK(p->B.alloc(2 * n));
    HIPCHK(p->Ua.alloc(2 * n));
    HIPCHK(p->Ub.alloc(2 * n));
    HIPCHK(p->pin.alloc(2));
    HIPCHK(p->sigma.alloc(2 * nf));
    HIPCHK(p->terms.alloc(7 * nf));
    HIPCHK(p->stats.alloc(7));
    *out = p.release();
    return SMG_OK;
}

// Ub = the harmonic map: (-L)_uu u = -(-L)_ub u_b from zero, the loop on the circle; then Ua <-> Ub
int harmonic_into_Ua(smg_param* p, const smg_solve_opts* opts, int* cycles)
{
    const size_t n = (size_t)p->nV;
    const smg_solve_opts so = opts_or_default(opts, 1e-8 * p->scale_harmonic, 50);
    HIPCHK(hipMemsetAsync(p->B.p, 0, 2 * n * sizeof(double), p->stream));
    HIPCHK(hipMemsetAsync(p->Ua.p, 0, 2 * n * sizeof(double), p->stream));
    if (int rc = inner_solve(p->handle[0], p->pcg, p->B.p, p->nV, p->circle.p, p->nl, p->Ua.p, p->nV, 2, so, p->Ub.p, p->nV, cycles)) return rc;
    std::swap(p->Ua, p->Ub);
    return SMG_OK;
}

int harmonic_impl(smg_param* p, int memspace, const smg_solve_opts* opts, double* UV, int ld_uv, int* cycles)
{
    if (!p || !UV || bad_memspace(memspace)) return fail(SMG_ERR_INVALID, "smg_param_harmonic: bad arguments");
    if (ld_uv < p->nV) return fail(SMG_ERR_INVALID, "smg_param_harmonic: a leading dimension is too small");
    DeviceScope dsc(p->device);
    if (int rc = harmonic_into_Ua(p, opts, cycles)) return rc;
    HIPCHK(copy_columns(UV, ld_uv, p->Ua.p, p->nV, p->nV, 2, copy_out(memspace), p->stream));
    HIPCHK(hipStreamSynchronize(p->stream));
    return SMG_OK;
}

int arap_impl(smg_param* p, const double* UV0, int ld_uv0, int memspace, int max_iter, double rel_tol, const smg_solve_opts* opts, double* UV,
              int ld_uv, double* energy_his, int* cycles, int* n_iter)
{
    if (!p || !UV || bad_memspace(memspace) || max_iter < 0 || !(rel_tol >= 0.0) || !std::isfinite(rel_tol))
        return fail(SMG_ERR_INVALID, "smg_param_arap: bad arguments");
    const int n = p->nV, nF = p->nF;
    if (ld_uv < n || (UV0 && ld_uv0 < n)) return fail(SMG_ERR_INVALID, "smg_param_arap: a leading dimension is too small");
    DeviceScope dsc(p->device);
    hipStream_t st = p->stream;
    const smg_solve_opts so = opts_or_default(opts, 1e-8 * p->scale_arap, 50);
    HIPCHK(p->E.ensure((size_t)max_iter + 1));
    int t_end = 0;
    if (!n_iter) n_iter = &t_end;
    *n_iter = 0;

    // the start: UV0, or the harmonic map with the same options
    if (UV0) HIPCHK(copy_columns(p->Ua.p, n, UV0, ld_uv0, n, 2, copy_in(memspace), st));
    else if (int rc = harmonic_into_Ua(p, opts, nullptr)) return rc;

    // local step: R_t from U_t, E_t = E(R_t, U_t); the right-hand side is enqueued ahead of the host's look at E_t
    auto local = [&](int t, bool with_rhs, double* E_t) -> int {
        HIPCHK(launch_param_local(nF, p->F.p, p->rest.p, p->Ua.p, n, p->R.p, p->eterm.p, st));
        HIPCHK(launch_fixed_sum(p->eterm.p, nF, p->part.p, p->E.p + t, st));
        HIPCHK(hipMemcpyAsync(E_t, p->E.p + t, sizeof(double), hipMemcpyDeviceToHost, st));
        if (with_rhs) {
            HIPCHK(launch_param_rhs(n, nF, p->m_ptr.p, p->m_idx.p, p->rest.p, p->R.p, p->B.p, n, st));
            // the pinned row: loop[0] keeps the value it has in the iterate
            HIPCHK(copy_columns(p->pin.p, 1, p->Ua.p + p->loop[0], n, 1, 2, hipMemcpyDeviceToDevice, st));
        }
        HIPCHK(hipStreamSynchronize(st));
        return SMG_OK;
    };
    // global step: (-L) U_{t+1} = rhs, loop[0] known, from U_t
    auto global = [&](int, int* entries) -> int {
        if (int rc = inner_solve(p->handle[1], p->pcg, p->B.p, n, p->pin.p, 1, p->Ua.p, n, 2, so, p->Ub.p, n, entries)) return rc;
        std::swap(p->Ua, p->Ub);
        return SMG_OK;
    };
    const int rc = local_global(max_iter, rel_tol, local, global, energy_his, cycles, n_iter);
    if (rc == LOCAL_GLOBAL_NONFINITE) return fail(SMG_ERR_NONFINITE, "smg_param_arap: non-finite energy at iteration %d", *n_iter);
    if (rc) return rc;
    HIPCHK(copy_columns(UV, ld_uv, p->Ua.p, n, n, 2, copy_out(memspace), st));
    HIPCHK(hipStreamSynchronize(st));
    return SMG_OK;
}

int distortion_impl(smg_param* p, const double* UV, int ld_uv, int memspace, double* sigma, double* stats)
{
    if (!p || !UV || !stats || bad_memspace(memspace)) return fail(SMG_ERR_INVALID, "smg_param_distortion: bad arguments");
    const int n = p->nV, nF = p->nF;
    if (ld_uv < n) return fail(SMG_ERR_INVALID, "smg_param_distortion: a leading dimension is too small");
    DeviceScope dsc(p->device);
    hipStream_t st = p->stream;
    const size_t nf = (size_t)nF;
    const double* dUV = UV;
    int ld = ld_uv;
    if (memspace == SMG_HOST) {      // the map through the right-hand side's block: no iteration is in flight between two calls
        HIPCHK(copy_columns(p->B.p, n, UV, ld_uv, n, 2, hipMemcpyHostToDevice, st));
        dUV = p->B.p;
        ld = n;
    }
    HIPCHK(launch_param_distortion(nF, p->F.p, p->rest.p, dUV, ld, nullptr, p->sigma.p, p->terms.p, st));
    for (int e = 0; e < 6; e++) HIPCHK(launch_fixed_sum(p->terms.p + e * nf, nF, p->part.p, p->stats.p + e, st));
    HIPCHK(launch_fixed_max(p->terms.p + 6 * nf, nF, p->part.p, p->stats.p + 6, st));
    double s[7];
    HIPCHK(hipMemcpyAsync(s, p->stats.p, sizeof s, hipMemcpyDeviceToHost, st));
    if (sigma) HIPCHK(hipMemcpyAsync(sigma, p->sigma.p, 2 * nf * sizeof(double), copy_out(memspace), st));
    HIPCHK(hipStreamSynchronize(st));
    stats[0] = s[0];                // flipped faces
    stats[1] = s[6];                // max sigma1 / sigma2 over the unflipped faces
    stats[2] = s[2] / s[1];         // area-weighted mean of sigma1 / sigma2
    stats[3] = s[3] / s[1];         // area-weighted mean of sigma1 sigma2
    stats[4] = s[4] / s[5];         // symmetric Dirichlet, area-weighted mean over the unflipped faces
    stats[5] = s[1];                // the rest area
    return SMG_OK;
}

}  // namespace

extern "C" int smg_param_create(const smg_hierarchy* h, const double* V, int nV, const int* F, int nF, smg_param** out)
{
    return guarded("smg_param_create", [&]() { return create_impl(h, V, nV, F, nF, out); });
}

extern "C" void smg_param_destroy(smg_param* p) { delete p; }

extern "C" int smg_param_set_solver(smg_param* p, int pcg)
{
    if (!p) return fail(SMG_ERR_INVALID, "null param object");
    latch_solver(p->pcg, pcg);
    return SMG_OK;
}

extern "C" long long smg_param_device_bytes(const smg_param* p)
{
    return p ? device_bytes(*p, p->F, p->m_ptr, p->m_idx, p->rest, p->circle, p->R, p->eterm, p->part, p->E, p->B, p->Ua, p->Ub, p->pin, p->sigma, p->terms,
                            p->stats)
             : 0;
}

extern "C" int smg_param_boundary(const smg_param* p, int* n_loop, int* loop)
{
    if (!p || (!n_loop && !loop)) return fail(SMG_ERR_INVALID, "smg_param_boundary: bad arguments");
    if (n_loop) *n_loop = p->nl;
    if (loop) std::copy(p->loop.begin(), p->loop.end(), loop);
    return SMG_OK;
}

extern "C" int smg_param_harmonic(smg_param* p, int memspace, const smg_solve_opts* opts, double* UV, int ld_uv, int* cycles)
{
    return guarded("smg_param_harmonic", [&]() { return harmonic_impl(p, memspace, opts, UV, ld_uv, cycles); });
}

extern "C" int smg_param_arap(smg_param* p, const double* UV0, int ld_uv0, int memspace, int max_iter, double rel_tol, const smg_solve_opts* opts,
                              double* UV, int ld_uv, double* energy_his, int* cycles, int* n_iter)
{
    return guarded("smg_param_arap", [&]() { return arap_impl(p, UV0, ld_uv0, memspace, max_iter, rel_tol, opts, UV, ld_uv, energy_his, cycles, n_iter); });
}

extern "C" int smg_param_distortion(smg_param* p, const double* UV, int ld_uv, int memspace, double* sigma, double* stats)
{
    return guarded("smg_param_distortion", [&]() { return distortion_impl(p, UV, ld_uv, memspace, sigma, stats); });
}
