// smg_emd.cpp -- the earth mover's (1-Wasserstein) distance between distributions on a mesh with geodesic ground cost, its transport flow and its
// Kantorovich potential (include/smg.h: smg_emd_*; Solomon, Rustamov, Guibas, Butscher 2014 in Beckmann form), by ADMM.
// The object owns one handle built from the caller's prolongations and precomputed once with -L (vertex 0 known), the geometry the kernels read
// (csrc/smg_emd_device.hip) -- faces, corner lists, positions, the gradient basis in the faces' frames, the areas -- and the state of the last
// query: Z and U per (face, column) and phi per (vertex, column).  An iteration is one vertex kernel (the right-hand side), ONE k-column solve
// warm-started from the previous phi, and one face kernel (J, the relaxation, the shrink, the terms of the bounds), all enqueued on the object's
// stream, which the handle uses too.  The host reads nothing between checks beside the solve's own history; at every check_every-th iteration and
// the last it reads upper, lower and gmax^2 of all columns in one copy.  Checks, stream, handle, the cotangent system and the inner solve:
// smg_mesh_object.hpp.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <memory>
#include <utility>
#include <vector>

#include "smg_device.hpp"
#include "smg_emd_inl.hpp"
#include "smg_mesh.hpp"
#include "smg_mesh_object.hpp"

using namespace smg;

struct smg_emd : MeshObject {              // handle[0]: -L, vertex 0 known
    int nV = 0, nF = 0;
    int pcg = 1;                           // the inner solver: 1 smg_solve_pcg, 0 smg_solve
    smg_emd_params p;
    double area = 0.0;                     // the fixed-order sum of the face areas
    size_t kcap = 0;                       // the columns the query blocks hold
    int k_state = 0, cur = 0;              // the columns of the kept state (0: none); which of phi[2] holds it
    DevBuf<int> F, m_ptr, m_idx;           // faces, corner lists per vertex
    DevBuf<double> V, W2, Af;              // positions (xyz rows), the gradient basis in the frames (6 per face), face areas
    DevBuf<double> Fs;                     // staging of a host call's flow
    DevBuf<double> B, R, phi[2], pot;      // column-major n x k: b, the right-hand side, phi and the solve's output, the potential
    DevBuf<double> ZU, J2, up, gq;         // the state (4 per (face, column)), J in the frames (2), the planes A |J| and rho^2 |grad phi|^2
    DevBuf<double> vterm, part, red;       // k planes of n (b potential; the residual's squares), the chunk sums, 4 k reductions
    DevBuf<double> rho, zero;              // k penalties; k zeros, the known values
    ~smg_emd() { quiesce(); }
};

namespace smg {

int emd_check_operands(const char* who, int op, int nV, int nF, int k, const int* F, const double* V, const double* b, const double* phi, const double* state,
                       const double* rho, const double* out)
{
    if (op < SMG_EMD_GEOMETRY || op > SMG_EMD_RESIDUAL || nV < 1 || nF < 1 || !F || !V || !out) return fail(SMG_ERR_INVALID, "%s: bad arguments", who);
    const bool needs_b = op == SMG_EMD_RHS || op == SMG_EMD_DUAL || op == SMG_EMD_RESIDUAL, needs_phi = op == SMG_EMD_UPDATE || op == SMG_EMD_DUAL;
    const bool needs_state = op != SMG_EMD_GEOMETRY, needs_rho = needs_phi;
    if ((needs_b && !b) || (needs_phi && !phi) || (needs_state && !state) || (needs_rho && !rho))
        return fail(SMG_ERR_INVALID, "%s: op %d misses an operand", who, op);
    if (k < 1) return fail(SMG_ERR_INVALID, "%s: k = %d, at least one column is needed", who, k);
    return check_faces(who, F, nF, nV);
}

}  // namespace smg

namespace {

int check_params(const char* who, const smg_emd_params& p)
{
    if (!std::isfinite(p.gap_tol) || !(p.gap_tol > 0.0)) return fail(SMG_ERR_INVALID, "%s: gap_tol = %g, a finite value > 0 is needed", who, p.gap_tol);
    if (p.max_iter < 0) return fail(SMG_ERR_INVALID, "%s: max_iter = %d, at least 0 is needed", who, p.max_iter);
    if (p.check_every < 1) return fail(SMG_ERR_INVALID, "%s: check_every = %d, at least 1 is needed", who, p.check_every);
    if (!(p.alpha > 0.0) || !(p.alpha < 2.0)) return fail(SMG_ERR_INVALID, "%s: alpha = %g, a value inside (0, 2) is needed", who, p.alpha);
    if (!std::isfinite(p.rho_scale) || !(p.rho_scale > 0.0)) return fail(SMG_ERR_INVALID, "%s: rho_scale = %g, a finite value > 0 is needed", who, p.rho_scale);
    if (!std::isfinite(p.inner_rel_tol) || !(p.inner_rel_tol > 0.0))
        return fail(SMG_ERR_INVALID, "%s: inner_rel_tol = %g, a finite value > 0 is needed", who, p.inner_rel_tol);
    return SMG_OK;
}

int create_impl(const smg_hierarchy* h, const double* V, int nV, const int* F, int nF, const smg_emd_params* p, smg_emd** out)
{
    if (out) *out = nullptr;
    const char* who = "smg_emd_create";
    if (!h || !V || !F || !p || !out || nV <= 0 || nF <= 0) return fail(SMG_ERR_INVALID, "%s: bad arguments", who);
    if (int rc = check_hierarchy(who, h, 1, nV)) return rc;
    if (int rc = check_mesh(who, V, nV, F, nF, true)) return rc;
    if (int rc = check_params(who, *p)) return rc;

    std::unique_ptr<smg_emd> g(new smg_emd());
    g->nV = nV; g->nF = nF; g->p = *p;
    if (int rc = g->open(who)) return rc;
    if (int rc = g->clone(who, h, 0)) return rc;

    // the geometry of a query and the total area, then -L with vertex 0 known: precomputed once
    HIPCHK(g->V.upload(std::vector<double>(V, V + (size_t)nV * 3)));
    if (int rc = upload_faces(F, nF, nV, g->F, g->m_ptr, g->m_idx)) return rc;
    HIPCHK(g->W2.alloc((size_t)nF * 6));
    HIPCHK(g->Af.alloc((size_t)nF));
    HIPCHK(g->part.alloc((size_t)fixed_sum_groups(std::max(nV, nF))));
    HIPCHK(g->red.alloc(4));
    HIPCHK(launch_emd_geometry(g->V.p, g->F.p, nF, g->W2.p, g->Af.p, g->stream));
    HIPCHK(launch_fixed_sum(g->Af.p, nF, g->part.p, g->red.p, g->stream));
    HIPCHK(hipMemcpyAsync(&g->area, g->red.p, sizeof(double), hipMemcpyDeviceToHost, g->stream));
    CotanSystem S;
    if (int rc = cotan_system(F, nF, nV, g->V.p, 0, 0.0, -1.0, g->stream, S, false)) return rc;   // synchronises: the area has arrived
    for (double& x : S.L) x = -x;
    const int pin = 0;
    if (int rc = smg_precompute(g->handle[0], nV, S.ptr.data(), S.col.data(), S.L.data(), &pin, 1)) return rc;
    *out = g.release();
    return SMG_OK;
}

// the blocks of a k-column query; they grow with the largest k seen and are kept.  Growing drops the kept state.
int ensure_columns(smg_emd* g, int k)
{
    const size_t n = (size_t)g->nV, nf = (size_t)g->nF, kk = (size_t)k;
    if (g->kcap >= kk) return SMG_OK;
    HIPCHK(hipStreamSynchronize(g->stream));
    g->k_state = 0;
    HIPCHK(g->B.alloc(n * kk));
    HIPCHK(g->R.alloc(n * kk));
    HIPCHK(g->phi[0].alloc(n * kk));
    HIPCHK(g->phi[1].alloc(n * kk));
    HIPCHK(g->pot.alloc(n * kk));
    HIPCHK(g->ZU.alloc(4 * nf * kk));
    HIPCHK(g->J2.alloc(2 * nf * kk));
    HIPCHK(g->up.alloc(nf * kk));
    HIPCHK(g->gq.alloc(nf * kk));
    HIPCHK(g->vterm.alloc(n * kk));
    HIPCHK(g->red.alloc(4 * kk));
    HIPCHK(g->rho.alloc(kk));
    HIPCHK(g->zero.alloc(kk));
    HIPCHK(hipMemsetAsync(g->zero.p, 0, kk * sizeof(double), g->stream));
    g->kcap = kk;
    return SMG_OK;
}

int solve_impl(smg_emd* g, const double* mu0, int ld0, const double* mu1, int ld1, int k, int memspace, const smg_solve_opts* opts, int warm,
               double* upper, double* lower, int* n_iter, double* residual, double* potential, int ld_p, double* flow)
{
    const char* who = "smg_emd_solve";
    if (!g || !mu0 || !mu1 || !upper || !lower) return fail(SMG_ERR_INVALID, "%s: bad arguments", who);
    if (k < 1) return fail(SMG_ERR_INVALID, "%s: k = %d, at least one column is needed", who, k);
    if ((long long)g->nV * k > INT_MAX || 4LL * g->nF * k > INT_MAX)
        return fail(SMG_ERR_INVALID, "%s: k = %d columns of %d vertices and %d faces exceed the index range", who, k, g->nV, g->nF);
    if (bad_memspace(memspace)) return fail(SMG_ERR_INVALID, "%s: memspace must be SMG_HOST or SMG_DEVICE", who);
    if (ld0 < g->nV || ld1 < g->nV || (potential && ld_p < g->nV)) return fail(SMG_ERR_INVALID, "%s: a leading dimension is too small", who);
    DeviceScope dsc(g->device);
    const int n = g->nV, nF = g->nF;
    const size_t nk = (size_t)n * k, fk = (size_t)nF * k, D = sizeof(double);
    hipStream_t st = g->stream;

    // b = mu1 - mu0 on the host: the refusals, the penalties and the norms are formed from it, the sums in index order
    std::vector<double> m0(nk), m1(nk), b(nk), m((size_t)k), rho((size_t)k), nb((size_t)k);
    if (memspace == SMG_HOST) {
        for (int c = 0; c < k; c++)
            for (int i = 0; i < n; i++) {
                m0[(size_t)c * n + i] = mu0[(size_t)c * ld0 + i];
                m1[(size_t)c * n + i] = mu1[(size_t)c * ld1 + i];
            }
    } else {
        HIPCHK(copy_columns(m0.data(), n, mu0, ld0, n, k, hipMemcpyDeviceToHost, st));
        HIPCHK(copy_columns(m1.data(), n, mu1, ld1, n, k, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
    }
    double bss = 0.0;
    for (int c = 0; c < k; c++) {
        double s = 0.0, comp = 0.0, a = 0.0, ss = 0.0;                 // s: Neumaier's compensated sum, so that the refusal does not depend on n
        for (int i = 0; i < n; i++) {
            const double x0 = m0[(size_t)c * n + i], x1 = m1[(size_t)c * n + i];
            if (!std::isfinite(x0) || !std::isfinite(x1)) return fail(SMG_ERR_INVALID, "%s: the mass of vertex %d in column %d is not finite", who, i, c);
            const double d = x1 - x0, t = s + d;
            b[(size_t)c * n + i] = d;
            comp += std::fabs(s) >= std::fabs(d) ? (s - t) + d : (d - t) + s;
            s = t;
            a += std::fabs(d);
            ss += d * d;
        }
        s += comp;
        if (!std::isfinite(a) || std::fabs(s) > 1e-12 * a)
            return fail(SMG_ERR_INVALID, "%s: masses differ in column %d: sum (mu1 - mu0) = %g against sum |mu1 - mu0| = %g", who, c, s, a);
        m[(size_t)c] = 0.5 * a;
        nb[(size_t)c] = std::sqrt(ss);
        rho[(size_t)c] = m[(size_t)c] > 0.0 ? g->p.rho_scale * std::sqrt(g->area) / m[(size_t)c] : 1.0;
        bss += ss;
    }

    if (int rc = ensure_columns(g, k)) return rc;
    if (flow && memspace == SMG_HOST) HIPCHK(g->Fs.ensure(3 * fk));
    const bool keep = warm != 0 && g->k_state == k;
    g->k_state = 0;                                                     // until this call has ended well
    if (!keep) {
        g->cur = 0;
        HIPCHK(hipMemsetAsync(g->ZU.p, 0, 4 * fk * D, st));
        HIPCHK(hipMemsetAsync(g->phi[0].p, 0, nk * D, st));
    }
    const int max_iter = bss > 0.0 ? g->p.max_iter : 0;                 // every column zero: nothing to iterate
    if (max_iter == 0) {
        HIPCHK(hipMemsetAsync(g->pot.p, 0, nk * D, st));
        HIPCHK(hipMemsetAsync(g->J2.p, 0, 2 * fk * D, st));
    }
    HIPCHK(hipMemcpyAsync(g->B.p, b.data(), nk * D, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(g->rho.p, rho.data(), (size_t)k * D, hipMemcpyHostToDevice, st));

    const smg_solve_opts so = opts_or_default(opts, g->p.inner_rel_tol * std::sqrt(bss), 100);
    std::vector<double> red(4 * (size_t)k, 0.0);
    double* d_up = g->red.p;
    double* d_lo = g->red.p + k;
    double* d_gm = g->red.p + 2 * (size_t)k;
    double* d_rs = g->red.p + 3 * (size_t)k;
    int t = 0;
    for (t = 1; t <= max_iter; t++) {
        HIPCHK(launch_emd_rhs(n, k, nF, g->m_ptr.p, g->m_idx.p, g->W2.p, g->Af.p, g->ZU.p, true, g->B.p, n, g->R.p, n, nullptr, st));
        if (int rc = inner_solve(g->handle[0], g->pcg, g->R.p, n, g->zero.p, 1, g->phi[g->cur].p, n, k, so, g->phi[1 - g->cur].p, n, nullptr)) return rc;
        g->cur = 1 - g->cur;
        const double* phi = g->phi[g->cur].p;
        const bool check = t % g->p.check_every == 0 || t == max_iter;
        HIPCHK(launch_emd_update(nF, k, g->F.p, g->W2.p, g->Af.p, phi, n, g->ZU.p, g->rho.p, g->p.alpha, check ? g->J2.p : nullptr, g->up.p, g->gq.p, st));
        if (!check) continue;
        for (int c = 0; c < k; c++) {
            HIPCHK(launch_fixed_sum(g->up.p + (size_t)c * nF, nF, g->part.p, d_up + c, st));
            HIPCHK(launch_fixed_max(g->gq.p + (size_t)c * nF, nF, g->part.p, d_gm + c, st));
        }
        HIPCHK(launch_emd_dual(n, k, g->B.p, n, phi, n, g->rho.p, d_gm, g->pot.p, n, g->vterm.p, st));
        for (int c = 0; c < k; c++) HIPCHK(launch_fixed_sum(g->vterm.p + (size_t)c * n, n, g->part.p, d_lo + c, st));
        HIPCHK(hipMemcpyAsync(red.data(), g->red.p, 3 * (size_t)k * D, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        bool all_done = true;
        for (int c = 0; c < k; c++) {
            const double u = red[(size_t)c], l = red[(size_t)k + c];
            if (!std::isfinite(u) || !std::isfinite(l)) return fail(SMG_ERR_NONFINITE, "%s: non-finite bounds at iteration %d", who, t);
            all_done = all_done && (!(m[(size_t)c] > 0.0) || u - l <= g->p.gap_tol * u);
        }
        if (all_done) break;
    }
    const int iterations = std::min(t, max_iter);

    if (iterations > 0) {   // the last solve's residual: the weak divergence of J minus b over the unknown rows
        HIPCHK(launch_emd_rhs(n, k, nF, g->m_ptr.p, g->m_idx.p, g->W2.p, g->Af.p, g->J2.p, false, g->B.p, n, g->R.p, n, g->vterm.p, st));
        for (int c = 0; c < k; c++) HIPCHK(launch_fixed_sum(g->vterm.p + (size_t)c * n, n, g->part.p, d_rs + c, st));
        HIPCHK(hipMemcpyAsync(red.data() + 3 * (size_t)k, d_rs, (size_t)k * D, hipMemcpyDeviceToHost, st));
    }
    if (potential) HIPCHK(copy_columns(potential, ld_p, g->pot.p, n, n, k, copy_out(memspace), st));
    if (flow) {
        double* dJ = memspace == SMG_HOST ? g->Fs.p : flow;
        HIPCHK(launch_emd_flow(nF, k, g->V.p, g->F.p, g->J2.p, dJ, st));
        if (memspace == SMG_HOST) HIPCHK(hipMemcpyAsync(flow, dJ, 3 * fk * D, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(hipStreamSynchronize(st));
    for (int c = 0; c < k; c++) {
        const bool live = m[(size_t)c] > 0.0;
        upper[c] = !live ? 0.0 : iterations > 0 ? red[(size_t)c] : HUGE_VAL;
        lower[c] = live && iterations > 0 ? red[(size_t)k + c] : 0.0;
        if (residual) residual[c] = live && iterations > 0 ? std::sqrt(red[3 * (size_t)k + c]) / nb[(size_t)c] : 0.0;
    }
    if (n_iter) *n_iter = iterations;
    g->k_state = k;
    return SMG_OK;
}

}  // namespace

extern "C" smg_emd_params smg_emd_params_default(void)
{
    smg_emd_params p;
    p.gap_tol = 1e-2; p.max_iter = 2000; p.check_every = 10; p.alpha = 1.7; p.rho_scale = 0.1; p.inner_rel_tol = 1e-8;
    return p;
}

extern "C" int smg_emd_create(const smg_hierarchy* h, const double* V, int nV, const int* F, int nF, const smg_emd_params* p, smg_emd** out)
{
    return guarded("smg_emd_create", [&]() { return create_impl(h, V, nV, F, nF, p, out); });
}

extern "C" void smg_emd_destroy(smg_emd* g) { delete g; }

extern "C" int smg_emd_set_params(smg_emd* g, const smg_emd_params* p)
{
    const char* who = "smg_emd_set_params";
    if (!g || !p) return fail(SMG_ERR_INVALID, "%s: bad arguments", who);
    if (int rc = check_params(who, *p)) return rc;
    g->p = *p;
    return SMG_OK;
}

extern "C" int smg_emd_set_solver(smg_emd* g, int pcg)
{
    if (!g) return fail(SMG_ERR_INVALID, "smg_emd_set_solver: null object");
    latch_solver(g->pcg, pcg);
    return SMG_OK;
}

extern "C" long long smg_emd_device_bytes(const smg_emd* g)
{
    if (!g) return 0;   // one list: every DevBuf of the struct
    return device_bytes(*g, g->F, g->m_ptr, g->m_idx, g->V, g->W2, g->Af, g->Fs, g->B, g->R, g->phi[0], g->phi[1], g->pot, g->ZU, g->J2, g->up, g->gq,
                        g->vterm, g->part, g->red, g->rho, g->zero);
}

extern "C" int smg_emd_solve(smg_emd* g, const double* mu0, int ld0, const double* mu1, int ld1, int k, int memspace, const smg_solve_opts* opts, int warm,
                             double* upper, double* lower, int* n_iter, double* residual, double* potential, int ld_p, double* flow)
{
    return guarded("smg_emd_solve", [&]() {
        return solve_impl(g, mu0, ld0, mu1, ld1, k, memspace, opts, warm, upper, lower, n_iter, residual, potential, ld_p, flow);
    });
}

extern "C" int smg_emd_host(int op, int nV, int nF, int k, const int* F, const double* V, const double* b, const double* phi, const double* state,
                            const double* rho, double alpha, double* out)
{
    return guarded("smg_emd_host", [&]() -> int {
        const char* who = "smg_emd_host";
        if (int rc = emd_check_operands(who, op, nV, nF, k, F, V, b, phi, state, rho, out)) return rc;
        const size_t f = (size_t)nF, nk = (size_t)nV * k, fk = f * (size_t)k;
        std::vector<double> W2(6 * f), A(f);
        emd_host_geometry(nF, F, V, W2.data(), A.data());
        std::vector<int> mp, mi;
        if (op == SMG_EMD_RHS || op == SMG_EMD_RESIDUAL) vertex_corner_lists(std::vector<int>(F, F + 3 * f), nV, mp, mi);
        switch (op) {
            case SMG_EMD_GEOMETRY:
                std::copy(W2.begin(), W2.end(), out);
                std::copy(A.begin(), A.end(), out + 6 * f);
                out[7 * f] = flow_host_sum(A.data(), nF);
                break;
            case SMG_EMD_RHS: emd_host_divergence(nV, nF, k, W2.data(), A.data(), mp.data(), mi.data(), b, state, 4, out, nullptr); break;
            case SMG_EMD_UPDATE:
                emd_host_update(nV, nF, k, F, W2.data(), A.data(), phi, state, rho, alpha, out, out + 4 * fk, out + 6 * fk, out + 7 * fk);
                for (int c = 0; c < k; c++) {
                    out[8 * fk + c] = flow_host_sum(out + 6 * fk + (size_t)c * f, nF);
                    out[8 * fk + k + c] = flow_host_max(out + 7 * fk + (size_t)c * f, nF);
                }
                break;
            case SMG_EMD_DUAL:
                emd_host_dual(nV, k, b, phi, rho, state, out, out + nk);
                for (int c = 0; c < k; c++) out[2 * nk + c] = flow_host_sum(out + nk + (size_t)c * nV, nV);
                break;
            case SMG_EMD_FLOW: emd_host_flow(nF, k, F, V, state, out); break;
            default:
                emd_host_divergence(nV, nF, k, W2.data(), A.data(), mp.data(), mi.data(), b, state, 2, out, out + nk);
                for (int c = 0; c < k; c++) out[2 * nk + c] = flow_host_sum(out + nk + (size_t)c * nV, nV);
                break;
        }
        return SMG_OK;
    });
}
