// smg_rd_inl.hpp -- the per-vertex arithmetic of two-species reaction-diffusion on a surface, in registers (csrc/smg_rd_device.hip, smg_rd_host;
// include/smg.h: smg_rd_*).  The state is a column-major nV x 2k block: columns [0, k) are u, columns [k, 2k) are v, one
// pair per simulation; per-vertex term planes are planes of nV; the coefficient table is k x 20 row-major: column c's R_u at 20 c, its R_v at
// 20 c + 10, each over the monomials 1, u, v, u^2, uv, v^2, u^3, u^2 v, u v^2, v^3 in this order.
//
//   cubic     uu = u u; uv = u v; vv = v v;  r = c0;  r = r + c1 u;  r = r + c2 v;  r = r + c3 uu;  r = r + c4 uv;  r = r + c5 vv;
//             r = r + c6 (uu u);  r = r + c7 (uu v);  r = r + c8 (u vv);  r = r + c9 (vv v)
//   react     `substeps` times:  ru = cubic(R_u; u, v);  rv = cubic(R_v; u, v);  u = u + h ru;  v = v + h rv  (both rates from the same u, v);
//             then the right-hand sides m u*, m v* and their squares
//   close     the terms m u', m v' and max(|u' - u|, |v' - v|)
// Only +, -, *, max and fabs occur; host and device compile the same text (the library is built with -ffp-contract=off), so the two agree bit
// for bit.  The host twin's sums are flow_host_sum / flow_host_max (smg_flow_inl.hpp), the order of launch_fixed_sum / launch_fixed_max; the
// masses are fluid_host_mass (smg_fluid_inl.hpp), the expression of k_fluid_mass.
#pragma once
#include <cmath>
#include <cstddef>

#include "smg_fluid_inl.hpp"

namespace smg {

constexpr int RD_COEFFS = 20;   // per column: 10 of R_u, then 10 of R_v

SMG_ARAP_HD double rd_cubic(const double* c, double u, double v)
{
    const double uu = u * u, uv = u * v, vv = v * v;
    double r = c[0];
    r = r + c[1] * u;
    r = r + c[2] * v;
    r = r + c[3] * uu;
    r = r + c[4] * uv;
    r = r + c[5] * vv;
    r = r + c[6] * (uu * u);
    r = r + c[7] * (uu * v);
    r = r + c[8] * (u * vv);
    r = r + c[9] * (vv * v);
    return r;
}

// `substeps` explicit Euler steps of length h of the reaction alone
SMG_ARAP_HD void rd_react(const double* coef, double h, int substeps, double* u, double* v)
{
    double a = *u, b = *v;
    for (int s = 0; s < substeps; s++) {
        const double ru = rd_cubic(coef, a, b);
        const double rv = rd_cubic(coef + 10, a, b);
        a = a + h * ru;
        b = b + h * rv;
    }
    *u = a;
    *v = b;
}

SMG_ARAP_HD double rd_change(double u0, double v0, double u1, double v1) { return fmax(fabs(u1 - u0), fabs(v1 - v0)); }

// ---- the host twin (smg_rd_host): the kernels' loops on caller arrays, with the layouts of smg_debug_rd (include/smg.h) -------------------------
// S (nV x 2k column-major: u then v); R (nV x 2k: m u*, m v*), rsq (2k planes of nV), vs (nV x k: v*)
inline void rd_host_react(int nV, int k, const double* m, const double* S, const double* coef, double h, int substeps, double* R, double* rsq, double* vs)
{
    const size_t n = (size_t)nV, nk = n * (size_t)k;
    for (int c = 0; c < k; c++)
        for (size_t i = 0; i < n; i++) {
            const size_t e = (size_t)c * n + i;
            double u = S[e], v = S[nk + e];
            rd_react(coef + (size_t)c * RD_COEFFS, h, substeps, &u, &v);
            const double bu = m[i] * u, bv = m[i] * v;
            R[e] = bu;
            R[nk + e] = bv;
            rsq[e] = bu * bu;
            rsq[nk + e] = bv * bv;
            vs[e] = v;
        }
}

// S0, S1 (nV x 2k: the step's start and its end); mt (2k planes of nV: m u', m v'), chg (k planes of nV)
inline void rd_host_close(int nV, int k, const double* m, const double* S0, const double* S1, double* mt, double* chg)
{
    const size_t n = (size_t)nV, nk = n * (size_t)k;
    for (int c = 0; c < k; c++)
        for (size_t i = 0; i < n; i++) {
            const size_t e = (size_t)c * n + i;
            mt[e] = m[i] * S1[e];
            mt[nk + e] = m[i] * S1[nk + e];
            chg[e] = rd_change(S0[e], S0[nk + e], S1[e], S1[nk + e]);
        }
}

}  // namespace smg
