// smg_conformal.cpp -- discrete conformal metrics with prescribed angle sums on the scalar V-cycle (include/smg.h: smg_conformal_*; DESIGN.md
// section 29): Springborn, Schroeder and Pinkall 2008.  One log scale factor u_i per vertex; the convex energy's gradient is the angle defect
// g = (angle sum) - Theta and its Hessian half the cotangent matrix of the current metric, so a Newton step is (-L~)_uu d = g_u, u += t d.  The
// object owns one handle built from the caller's prolongations: one pattern-setting smg_precompute at create (-L of the rest mesh, the fixed
// vertices known), then per Newton step one face kernel, one row kernel, smg_precompute_values_device and a 1-column solve.  Every value of the
// matrix changes at every step.  Kernels: csrc/smg_conformal_device.hip.  Checks, stream, handle, the cotangent system and the inner solve:
// smg_mesh_object.hpp; the sums: launch_fixed_sum / launch_fixed_max.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cmath>
#include <memory>
#include <vector>

#include "smg_conformal_inl.hpp"
#include "smg_device.hpp"
#include "smg_mesh.hpp"
#include "smg_mesh_object.hpp"

using namespace smg;

struct smg_conformal : MeshObject {        // handle[0]: -L~ with the fixed rows known, re-precomputed by values on every Newton step
    int nV = 0, nF = 0, nnz = 0, n_fixed = 0;
    int pcg = 1;                           // the inner solver: 1 smg_solve_pcg, 0 smg_solve
    double broken_last = 0.0, broken_max = 0.0;   // the broken faces of the last accepted iterate's evaluation; the maximum over the last solve
    smg_conformal_params p;
    DevBuf<int> F, m_ptr, m_idx, rowptr, l_ptr, l_idx, fixed_list, fixed_mask;
    DevBuf<signed char> l_sgn;
    DevBuf<double> l0, area2, u, ut, s, d, g, sum, Theta;   // rest lengths (nF x 3) and double areas (nF); the state, the trial, the scales, the step, the gradient, the angle sums
    DevBuf<double> ang, hc, broken, lt;    // nF x 3, nF x 3, nF, nF x 3
    DevBuf<double> val, zero;              // the values of -L~; nV zeros: the inner start and the known values of the step
    DevBuf<double> gsq, gabs, part, red;   // the planes of terms, the chunk sums, the three reduced doubles
    ~smg_conformal() { quiesce(); }
};

namespace smg {

int conformal_check_params(const char* who, const smg_conformal_params& p)
{
    if (!std::isfinite(p.grad_tol) || !(p.grad_tol > 0.0)) return fail(SMG_ERR_INVALID, "%s: grad_tol = %g, a finite value > 0 is needed", who, p.grad_tol);
    if (p.max_newton < 0) return fail(SMG_ERR_INVALID, "%s: max_newton = %d, at least 0 is needed", who, p.max_newton);
    if (!std::isfinite(p.inner_rel_tol) || !(p.inner_rel_tol > 0.0))
        return fail(SMG_ERR_INVALID, "%s: inner_rel_tol = %g, a finite value > 0 is needed", who, p.inner_rel_tol);
    return SMG_OK;
}

int conformal_check_fixed(const char* who, const int* fixed, int n_fixed, int nV, bool may_be_empty)
{
    if (n_fixed < 0 || (n_fixed > 0 && !fixed) || (n_fixed == 0 && !may_be_empty))
        return fail(SMG_ERR_INVALID, "%s: n_fixed = %d, a list of at least one fixed vertex is needed", who, n_fixed);
    std::vector<char> seen((size_t)nV, 0);
    for (int i = 0; i < n_fixed; i++) {
        if (fixed[i] < 0 || fixed[i] >= nV) return fail(SMG_ERR_INVALID, "%s: fixed vertex %d is out of range", who, fixed[i]);
        if (seen[(size_t)fixed[i]]) return fail(SMG_ERR_INVALID, "%s: fixed vertex %d is listed twice", who, fixed[i]);
        seen[(size_t)fixed[i]] = 1;
    }
    return SMG_OK;
}

int conformal_check_operands(const char* who, int op, int nV, int nF, const int* F, const double* l0, const double* area2, const double* u, const double* d, double t,
                             const double* s, const double* Theta, const int* fixed, int n_fixed, const double* out)
{
    if (op < SMG_CONFORMAL_SCALE || op > SMG_CONFORMAL_ROWS || nV < 1 || nF < 1 || !F || !out) return fail(SMG_ERR_INVALID, "%s: bad arguments", who);
    if ((op == SMG_CONFORMAL_SCALE && !u) || (op != SMG_CONFORMAL_SCALE && (!l0 || !area2 || !s)) || (op == SMG_CONFORMAL_ROWS && !Theta))
        return fail(SMG_ERR_INVALID, "%s: op %d misses an operand", who, op);
    if (int rc = check_faces(who, F, nF, nV)) return rc;
    if (op == SMG_CONFORMAL_SCALE && d && !std::isfinite(t)) return fail(SMG_ERR_INVALID, "%s: t = %g, a finite step is needed", who, t);
    if (op == SMG_CONFORMAL_ROWS)
        if (int rc = conformal_check_fixed(who, fixed, n_fixed, nV, true)) return rc;
    return SMG_OK;
}

}  // namespace smg

namespace {

int create_impl(const smg_hierarchy* h, const double* V, int nV, const int* F, int nF, const int* fixed, int n_fixed, const smg_conformal_params* p,
                smg_conformal** out)
{
    if (out) *out = nullptr;
    const char* who = "smg_conformal_create";
    if (!h || !V || !F || !p || !out || nV <= 0 || nF <= 0) return fail(SMG_ERR_INVALID, "%s: bad arguments", who);
    if (int rc = check_hierarchy(who, h, 1, nV)) return rc;
    if (h->n_levels < 2) return fail(SMG_ERR_INVALID, "%s: a hierarchy of at least two levels is needed: every Newton step re-precomputes by values", who);
    if (int rc = check_mesh(who, V, nV, F, nF, true)) return rc;
    if (int rc = conformal_check_fixed(who, fixed, n_fixed, nV, false)) return rc;
    if (n_fixed >= nV) return fail(SMG_ERR_INVALID, "%s: no free vertex: all %d vertices are fixed", who, nV);
    if (int rc = conformal_check_params(who, *p)) return rc;

    std::unique_ptr<smg_conformal> m(new smg_conformal());
    m->nV = nV; m->nF = nF; m->n_fixed = n_fixed; m->p = *p;
    if (int rc = m->open(who)) return rc;
    if (int rc = m->clone(who, h, 0)) return rc;
    hipStream_t st = m->stream;
    const size_t n = (size_t)nV, nf = (size_t)nF;

    if (int rc = upload_faces(F, nF, nV, m->F, m->m_ptr, m->m_idx)) return rc;
    std::vector<double> l0(3 * nf), area2(nf);
    for (size_t f = 0; f < nf; f++) {
        conformal_rest_lengths(V, F, f, &l0[3 * f]);
        area2[f] = conformal_rest_area2(V, F, f);
    }
    std::vector<int> sorted(fixed, fixed + n_fixed), mask(n, 0);
    std::sort(sorted.begin(), sorted.end());
    for (int v : sorted) mask[(size_t)v] = 1;
    HIPCHK(m->l0.upload(l0));
    HIPCHK(m->area2.upload(area2));
    HIPCHK(m->fixed_list.upload(std::vector<int>(fixed, fixed + n_fixed)));
    HIPCHK(m->fixed_mask.upload(mask));
    for (DevBuf<double>* b : {&m->u, &m->ut, &m->s, &m->d, &m->g, &m->sum, &m->Theta, &m->zero, &m->gsq, &m->gabs}) HIPCHK(b->alloc(n));
    for (DevBuf<double>* b : {&m->ang, &m->hc, &m->lt}) HIPCHK(b->alloc(3 * nf));
    HIPCHK(m->broken.alloc(nf));
    HIPCHK(m->part.alloc((size_t)fixed_sum_groups(std::max(nF, nV))));
    HIPCHK(m->red.alloc(3));
    for (DevBuf<double>* b : {&m->u, &m->Theta, &m->zero}) HIPCHK(hipMemsetAsync(b->p, 0, n * sizeof(double), st));

    // -L of the rest mesh (u = 0) sets the handle's pattern, the fixed vertices known; the recipe of its entries stays for the row kernel
    const AssemblyPlan plan = make_assembly_plan(std::vector<int>(F, F + 3 * nf), nV);
    DevBuf<double> rows;
    HIPCHK(rows.upload(std::vector<double>(V, V + 3 * n)));
    CotanSystem S;
    if (int rc = cotan_system(F, nF, nV, rows.p, 0, 0.0, -1.0, st, S, true)) return rc;
    if (S.ptr.size() != plan.pattern.ptr.size() || S.col.size() != plan.pattern.col.size() ||
        !std::equal(S.ptr.begin(), S.ptr.end(), plan.pattern.ptr.begin()) || !std::equal(S.col.begin(), S.col.end(), plan.pattern.col.begin()))
        return fail(SMG_ERR_INVALID, "%s: the assembler's pattern is not the plan's", who);
    m->nnz = (int)S.col.size();
    HIPCHK(m->rowptr.upload(plan.pattern.ptr));
    HIPCHK(m->l_ptr.upload(plan.l_ptr));
    HIPCHK(m->l_idx.upload(plan.l_idx));
    HIPCHK(m->l_sgn.upload(plan.l_sgn));
    HIPCHK(m->val.alloc((size_t)m->nnz));
    if (int rc = smg_precompute(m->handle[0], nV, S.ptr.data(), S.col.data(), S.val.data(), sorted.data(), n_fixed)) return rc;
    HIPCHK(hipStreamSynchronize(st));
    *out = m.release();
    return SMG_OK;
}

// one evaluation at u + t d (d == nullptr: at u): ut, s, the faces, the rows (with the values of -L~ when asked) and the three reductions;
// r[0] = |g|_2, r[1] = max |g|, r[2] = the broken faces.  One 24-byte copy reaches the host.
int evaluate(smg_conformal* m, const double* d, double t, bool values, double* r)
{
    hipStream_t st = m->stream;
    HIPCHK(launch_conformal_scale(m->nV, m->u.p, d, t, m->ut.p, m->s.p, st));
    HIPCHK(launch_conformal_faces(m->nF, m->F.p, m->l0.p, m->area2.p, m->s.p, m->ang.p, m->hc.p, m->broken.p, st));
    HIPCHK(launch_conformal_rows(m->nV, m->nF, m->ang.p, m->hc.p, m->broken.p, m->m_ptr.p, m->m_idx.p, m->Theta.p, m->fixed_mask.p, m->rowptr.p, m->l_ptr.p,
                                 m->l_idx.p, m->l_sgn.p, m->sum.p, m->g.p, m->gsq.p, m->gabs.p, values ? m->val.p : nullptr, m->part.p, m->red.p, st));
    HIPCHK(hipMemcpyAsync(r, m->red.p, 3 * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    r[0] = std::sqrt(r[0]);
    return SMG_OK;
}

int solve_impl(smg_conformal* m, const double* Theta, const double* u_fixed, int memspace, const smg_solve_opts* opts, double* grad_his, double* step_his,
               int* cycles, int* n_newton, int* converged)
{
    const char* who = "smg_conformal_solve";
    if (n_newton) *n_newton = 0;
    if (converged) *converged = 0;
    if (!m || !Theta) return fail(SMG_ERR_INVALID, "%s: bad arguments", who);
    if (bad_memspace(memspace)) return fail(SMG_ERR_INVALID, "%s: memspace must be SMG_HOST or SMG_DEVICE", who);
    const int n = m->nV;
    if (memspace == SMG_HOST) {
        for (int i = 0; i < n; i++)
            if (!std::isfinite(Theta[i])) return fail(SMG_ERR_INVALID, "%s: Theta[%d] is not finite", who, i);
        for (int i = 0; u_fixed && i < m->n_fixed; i++)
            if (!std::isfinite(u_fixed[i])) return fail(SMG_ERR_INVALID, "%s: u_fixed[%d] is not finite", who, i);
    }
    DeviceScope dsc(m->device);
    hipStream_t st = m->stream;
    int t_end = 0, conv = 0;
    if (!n_newton) n_newton = &t_end;
    if (!converged) converged = &conv;

    HIPCHK(hipMemcpyAsync(m->Theta.p, Theta, (size_t)n * sizeof(double), copy_in(memspace), st));
    const double* uf = u_fixed;
    if (u_fixed && memspace == SMG_HOST) {                                      // staged in d, which the first solve overwrites
        HIPCHK(hipMemcpyAsync(m->d.p, u_fixed, (size_t)m->n_fixed * sizeof(double), hipMemcpyHostToDevice, st));
        uf = m->d.p;
    }
    HIPCHK(launch_conformal_fix(m->n_fixed, m->fixed_list.p, uf, m->u.p, st));

    double r[3];
    if (int rc = evaluate(m, nullptr, 0.0, true, r)) return rc;
    m->broken_last = m->broken_max = r[2];
    for (int t = 0;; t++) {
        *n_newton = t;
        if (grad_his) grad_his[t] = r[1];
        if (!std::isfinite(r[0])) return fail(SMG_ERR_NONFINITE, "%s: non-finite gradient norm at Newton step %d", who, t);
        if (r[1] <= m->p.grad_tol) { *converged = 1; return SMG_OK; }
        if (t >= m->p.max_newton) return SMG_OK;
        if (int rc = smg_precompute_values_device(m->handle[0], m->val.p)) return rc;
        const smg_solve_opts so = opts_or_default(opts, m->p.inner_rel_tol * r[0], 100);
        int entries = 0;
        if (int rc = inner_solve(m->handle[0], m->pcg, m->g.p, n, m->zero.p, m->n_fixed, m->zero.p, n, 1, so, m->d.p, n, &entries)) return rc;
        if (cycles) cycles[t] = entries;
        // the line search on the gradient norm: t = 1, 1/2, 1/4, ...; a trial's evaluation leaves the state alone
        double step = 1.0, q[3];
        for (;;) {
            if (step < 0x1p-20) return SMG_OK;                                  // no step reduces the gradient: u stays the last accepted iterate
            if (int rc = evaluate(m, m->d.p, step, false, q)) return rc;
            m->broken_max = std::max(m->broken_max, q[2]);
            if (q[0] <= (1.0 - 1e-4 * step) * r[0]) break;
            step *= 0.5;
        }
        std::swap(m->u, m->ut);                                                 // the trial's own bits become the state
        // the accepted trial's angles and cotangents are still in place: its rows once more, now with the values of -L~
        HIPCHK(launch_conformal_rows(n, m->nF, m->ang.p, m->hc.p, m->broken.p, m->m_ptr.p, m->m_idx.p, m->Theta.p, m->fixed_mask.p, m->rowptr.p, m->l_ptr.p,
                                     m->l_idx.p, m->l_sgn.p, m->sum.p, m->g.p, m->gsq.p, m->gabs.p, m->val.p, m->part.p, nullptr, st));
        if (step_his) step_his[t] = step;
        m->broken_last = q[2];
        r[0] = q[0]; r[1] = q[1]; r[2] = q[2];
    }
}

int vector_impl(const char* who, smg_conformal* m, int memspace, double* out, const double* in)
{
    if (!m || !(in ? (const void*)in : (const void*)out)) return fail(SMG_ERR_INVALID, "%s: bad arguments", who);
    if (bad_memspace(memspace)) return fail(SMG_ERR_INVALID, "%s: memspace must be SMG_HOST or SMG_DEVICE", who);
    DeviceScope dsc(m->device);
    const size_t bytes = (size_t)m->nV * sizeof(double);
    if (in) HIPCHK(hipMemcpyAsync(m->u.p, in, bytes, copy_in(memspace), m->stream));
    else HIPCHK(hipMemcpyAsync(out, m->u.p, bytes, copy_out(memspace), m->stream));
    HIPCHK(hipStreamSynchronize(m->stream));
    return SMG_OK;
}

// the angle sums (lengths == false) or the lengths l~ (true) of the current u
int query_impl(const char* who, smg_conformal* m, int memspace, double* out, bool lengths)
{
    if (!m || !out) return fail(SMG_ERR_INVALID, "%s: bad arguments", who);
    if (bad_memspace(memspace)) return fail(SMG_ERR_INVALID, "%s: memspace must be SMG_HOST or SMG_DEVICE", who);
    DeviceScope dsc(m->device);
    hipStream_t st = m->stream;
    if (lengths) {
        HIPCHK(launch_conformal_scale(m->nV, m->u.p, nullptr, 0.0, m->ut.p, m->s.p, st));
        HIPCHK(launch_conformal_lengths(m->nF, m->F.p, m->l0.p, m->s.p, m->lt.p, st));
        HIPCHK(hipMemcpyAsync(out, m->lt.p, 3 * (size_t)m->nF * sizeof(double), copy_out(memspace), st));
    } else {
        double r[3];
        if (int rc = evaluate(m, nullptr, 0.0, false, r)) return rc;
        m->broken_last = r[2];
        HIPCHK(hipMemcpyAsync(out, m->sum.p, (size_t)m->nV * sizeof(double), copy_out(memspace), st));
    }
    HIPCHK(hipStreamSynchronize(st));
    return SMG_OK;
}

}  // namespace

extern "C" smg_conformal_params smg_conformal_params_default(void)
{
    smg_conformal_params p;
    p.grad_tol = 1e-10; p.max_newton = 50; p.inner_rel_tol = 1e-6;
    return p;
}

extern "C" int smg_conformal_create(const smg_hierarchy* h, const double* V, int nV, const int* F, int nF, const int* fixed, int n_fixed,
                                    const smg_conformal_params* p, smg_conformal** out)
{
    return guarded("smg_conformal_create", [&]() { return create_impl(h, V, nV, F, nF, fixed, n_fixed, p, out); });
}

extern "C" void smg_conformal_destroy(smg_conformal* c) { delete c; }

extern "C" int smg_conformal_set_params(smg_conformal* c, const smg_conformal_params* p)
{
    const char* who = "smg_conformal_set_params";
    if (!c || !p) return fail(SMG_ERR_INVALID, "%s: bad arguments", who);
    if (int rc = conformal_check_params(who, *p)) return rc;
    c->p = *p;
    return SMG_OK;
}

extern "C" int smg_conformal_set_solver(smg_conformal* c, int pcg)
{
    if (!c) return fail(SMG_ERR_INVALID, "smg_conformal_set_solver: null object");
    latch_solver(c->pcg, pcg);
    return SMG_OK;
}

extern "C" long long smg_conformal_device_bytes(const smg_conformal* c)
{
    if (!c) return 0;   // one list: every DevBuf of the struct
    return device_bytes(*c, c->F, c->m_ptr, c->m_idx, c->rowptr, c->l_ptr, c->l_idx, c->fixed_list, c->fixed_mask, c->l_sgn, c->l0, c->area2, c->u, c->ut, c->s, c->d,
                        c->g, c->sum, c->Theta, c->ang, c->hc, c->broken, c->lt, c->val, c->zero, c->gsq, c->gabs, c->part, c->red);
}

extern "C" int smg_conformal_reset(smg_conformal* c)
{
    return guarded("smg_conformal_reset", [&]() -> int {
        if (!c) return fail(SMG_ERR_INVALID, "smg_conformal_reset: null object");
        DeviceScope dsc(c->device);
        HIPCHK(hipMemsetAsync(c->u.p, 0, (size_t)c->nV * sizeof(double), c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        return SMG_OK;
    });
}

extern "C" int smg_conformal_set_u(smg_conformal* c, const double* u, int memspace)
{
    return guarded("smg_conformal_set_u", [&]() { return vector_impl("smg_conformal_set_u", c, memspace, nullptr, u); });
}

extern "C" int smg_conformal_u(smg_conformal* c, int memspace, double* u)
{
    return guarded("smg_conformal_u", [&]() { return vector_impl("smg_conformal_u", c, memspace, u, nullptr); });
}

extern "C" int smg_conformal_solve(smg_conformal* c, const double* Theta, const double* u_fixed, int memspace, const smg_solve_opts* opts,
                                   double* grad_his, double* step_his, int* cycles, int* n_newton, int* converged)
{
    return guarded("smg_conformal_solve", [&]() { return solve_impl(c, Theta, u_fixed, memspace, opts, grad_his, step_his, cycles, n_newton, converged); });
}

extern "C" int smg_conformal_angle_sums(smg_conformal* c, int memspace, double* sums)
{
    return guarded("smg_conformal_angle_sums", [&]() { return query_impl("smg_conformal_angle_sums", c, memspace, sums, false); });
}

extern "C" int smg_conformal_lengths(smg_conformal* c, int memspace, double* len)
{
    return guarded("smg_conformal_lengths", [&]() { return query_impl("smg_conformal_lengths", c, memspace, len, true); });
}

extern "C" int smg_conformal_stats(const smg_conformal* c, double* stats)
{
    if (!c || !stats) return fail(SMG_ERR_INVALID, "smg_conformal_stats: bad arguments");
    stats[0] = c->broken_last;
    stats[1] = c->broken_max;
    return SMG_OK;
}

extern "C" int smg_conformal_host(int op, int nV, int nF, const int* F, const double* l0, const double* area2, const double* u, const double* d, double t,
                                  const double* s, const double* Theta, const int* fixed, int n_fixed, double* out)
{
    return guarded("smg_conformal_host", [&]() -> int {
        const char* who = "smg_conformal_host";
        if (int rc = conformal_check_operands(who, op, nV, nF, F, l0, area2, u, d, t, s, Theta, fixed, n_fixed, out)) return rc;
        const size_t n = (size_t)nV, nf = (size_t)nF;
        if (op == SMG_CONFORMAL_SCALE) {
            conformal_host_scale(nV, u, d, t, out, out + n);
            return SMG_OK;
        }
        if (op == SMG_CONFORMAL_FACES) {
            conformal_host_faces(nF, F, l0, area2, s, out, out + 3 * nf, out + 6 * nf, out + 7 * nf);
            return SMG_OK;
        }
        const AssemblyPlan plan = make_assembly_plan(std::vector<int>(F, F + 3 * nf), nV);
        std::vector<int> mask(n, 0);
        for (int i = 0; i < n_fixed; i++) mask[(size_t)fixed[i]] = 1;
        std::vector<double> ang(3 * nf), hc(3 * nf), broken(nf);
        conformal_host_faces(nF, F, l0, area2, s, ang.data(), hc.data(), broken.data(), nullptr);
        conformal_host_rows(nV, ang.data(), hc.data(), plan.m_ptr.data(), plan.m_idx.data(), Theta, mask.data(), plan.pattern.ptr.data(), plan.l_ptr.data(),
                            plan.l_idx.data(), plan.l_sgn.data(), out, out + n, out + 2 * n, out + 3 * n, out + 4 * n + 3);
        double* red = out + 4 * n;
        red[0] = flow_host_sum(out + 2 * n, nV);
        red[1] = flow_host_max(out + 3 * n, nV);
        red[2] = flow_host_sum(broken.data(), nF);
        return SMG_OK;
    });
}
