// smg_sinkhorn_inl.hpp -- the per-vertex arithmetic of heat-kernel optimal transport on a mesh, in registers (smg_sinkhorn_host; include/smg.h;
// DESIGN.md section 35), written as the sibling *_inl.hpp files are, so that kernels can compile the same text.  Blocks are column-major nV x k;
// planes of per-vertex terms are planes of nV; m is the barycentric mass, A its fixed-order sum.
//
//   effective  y_eff = max(y, 0) + (floor sr) / A, sr the fixed-order sum of the block column the kernel was applied to
//   scale      err = |r y_eff - mu|;  r' = mu / y_eff (0 where mu == 0);  r'^2
//   substep    r' = m y;  r'^2
//   value      ln v = ln(r_v / m), ln w = ln(r_w / m) (-inf where the mass is 0);  term = mu0 ln v + mu1 ln w, a product with a zero mass left out
//   geomean    per column c of a group:  d_c = (r_v,c / m) z_eff,c;  acc = acc + alpha_c ln d_c over the columns with alpha_c > 0, in order;
//              mu = exp(acc) (0 where such a d_c is not > 0);  b = m mu;  |b - previous|;  r_v,c' = b / z_eff,c;  r_v,c'^2
// scale and substep are +, -, *, /, fmax and fabs alone (the library is built with -ffp-contract=off): tests/sinkhorn_np.py is matched bit for
// bit there; log and exp are the C library's.  The sums are flow_host_sum (smg_flow_inl.hpp), the order of launch_fixed_sum; the masses are
// fluid_host_mass (smg_fluid_inl.hpp), the expression of k_fluid_mass.
#pragma once
#include <cmath>
#include <cstddef>
#include <limits>

#include "smg_fluid_inl.hpp"

namespace smg {

SMG_ARAP_HD double sinkhorn_effective(double y, double sr, double floor, double A) { return fmax(y, 0.0) + (floor * sr) / A; }

// *err = |r y_eff - mu|; returns r'
SMG_ARAP_HD double sinkhorn_scale(double y, double r, double mu, double sr, double floor, double A, double* err)
{
    const double ye = sinkhorn_effective(y, sr, floor, A);
    *err = fabs(r * ye - mu);
    return mu == 0.0 ? 0.0 : mu / ye;
}

// *lv, *lw: the log scalings; returns the term
SMG_ARAP_HD double sinkhorn_value(double mu0, double mu1, double rv, double rw, double m, double* lv, double* lw)
{
    const double ninf = -HUGE_VAL;
    double t0 = 0.0, t1 = 0.0;
    *lv = ninf;
    *lw = ninf;
    if (mu0 != 0.0) { *lv = log(rv / m); t0 = mu0 * *lv; }
    if (mu1 != 0.0) { *lw = log(rw / m); t1 = mu1 * *lw; }
    return t0 + t1;
}

// one column's share of a group's exponent: acc and dead (a d that is not > 0 under a positive alpha) in place
SMG_ARAP_HD void sinkhorn_geomean_term(double alpha, double rv, double m, double ze, double* acc, bool* dead)
{
    if (!(alpha > 0.0)) return;
    const double d = (rv / m) * ze;
    if (d > 0.0)
        *acc = *acc + alpha * log(d);
    else
        *dead = true;
}

SMG_ARAP_HD double sinkhorn_geomean_mass(double acc, bool dead, double m) { return m * (dead ? 0.0 : exp(acc)); }

// ---- smg_sinkhorn_host: the loops on caller arrays, with the layouts of include/smg.h -------------------------------------------------------
// y, r (nV x k), mu (nV x mu_cols; column c reads c % mu_cols), sr (k) -> rn (nV x k), err and rsq (k planes of nV each)
inline void sinkhorn_host_scale(int nV, int k, int mu_cols, const double* y, const double* r, const double* mu, const double* sr, double floor, double A,
                                double* rn, double* err, double* rsq)
{
    const size_t n = (size_t)nV;
    for (int c = 0; c < k; c++)
        for (size_t i = 0; i < n; i++) {
            const size_t e = (size_t)c * n + i;
            const double x = sinkhorn_scale(y[e], r[e], mu[(size_t)(c % mu_cols) * n + i], sr[c], floor, A, err + e);
            rn[e] = x;
            rsq[e] = x * x;
        }
}

inline void sinkhorn_host_substep(int nV, int k, const double* m, const double* y, double* rn, double* rsq)
{
    const size_t n = (size_t)nV;
    for (int c = 0; c < k; c++)
        for (size_t i = 0; i < n; i++) {
            const size_t e = (size_t)c * n + i;
            const double x = m[i] * y[e];
            rn[e] = x;
            rsq[e] = x * x;
        }
}

// terms (k planes of nV), lv, lw (nV x k)
inline void sinkhorn_host_value(int nV, int k, const double* m, const double* mu0, const double* mu1, const double* rv, const double* rw, double* terms,
                                double* lv, double* lw)
{
    const size_t n = (size_t)nV;
    for (int c = 0; c < k; c++)
        for (size_t i = 0; i < n; i++) {
            const size_t e = (size_t)c * n + i;
            terms[e] = sinkhorn_value(mu0[e], mu1[e], rv[e], rw[e], m[i], lv + e, lw + e);
        }
}

// z, rv (nV x G k_in), prev (nV x G), sr (G k_in), alphas (G x k_in row-major) -> rn (nV x G k_in), bary (nV x G), chg (G planes), rsq (G k_in planes)
inline void sinkhorn_host_geomean(int nV, int G, int k_in, const double* m, const double* z, const double* rv, const double* prev, const double* sr,
                                  const double* alphas, double floor, double A, double* rn, double* bary, double* chg, double* rsq)
{
    const size_t n = (size_t)nV;
    for (int g = 0; g < G; g++)
        for (size_t i = 0; i < n; i++) {
            double acc = 0.0;
            bool dead = false;
            for (int c = 0; c < k_in; c++) {
                const size_t e = ((size_t)g * k_in + c) * n + i;
                sinkhorn_geomean_term(alphas[(size_t)g * k_in + c], rv[e], m[i], sinkhorn_effective(z[e], sr[(size_t)g * k_in + c], floor, A), &acc, &dead);
            }
            const double b = sinkhorn_geomean_mass(acc, dead, m[i]);
            bary[(size_t)g * n + i] = b;
            chg[(size_t)g * n + i] = fabs(b - prev[(size_t)g * n + i]);
            for (int c = 0; c < k_in; c++) {
                const size_t e = ((size_t)g * k_in + c) * n + i;
                const double x = b / sinkhorn_effective(z[e], sr[(size_t)g * k_in + c], floor, A);
                rn[e] = x;
                rsq[e] = x * x;
            }
        }
}

}  // namespace smg
