// smg_wave_inl.hpp -- the per-vertex arithmetic of the wave equation on a surface, in registers (csrc/smg_wave_device.hip, smg_wave_host;
// include/smg.h: smg_wave_*).  u, v, the right-hand side b, the warm start z and the solve's answer w are column-major
// nV x k blocks with a leading dimension, one column per experiment; per-vertex planes (mt, s2, the known mask) have nV entries, term planes k
// planes of nV.  mt_i = m_i / speed_i^2 and s2_i = 2.0 + sigma_i dt are formed once on the host; dt, a = 0.25 dt dt and q2 = 2.0 / dt are host
// doubles.
//
//   rhs       b = mt (s2 u + dt v);  rsq = b b (0.0 on a known row);  z = 2.0 u + dt v
//   sources   b = b + a (sig0 + sig1);  rsq = b b             at the source's vertex, one column at a time
//   advance   u' = w - u;  d = u' - u;  v' = q2 d - v;  ke = 0.5 ((mt v') v');  then, where asked, rhs of (u', v')
//   record    trace = u' at the receiver's vertex
// Only +, - and * occur; host and device compile the same text (the library is built with -ffp-contract=off), so the two agree bit for bit.
// The host twin's sums are flow_host_sum (smg_flow_inl.hpp), the order of launch_fixed_sum; the masses are fluid_host_mass and the potential
// energy's terms fluid_host_velocity (smg_fluid_inl.hpp), the expressions of k_fluid_mass and k_fluid_velocity.
#pragma once
#include <cmath>
#include <cstddef>

#include "smg_fluid_inl.hpp"

namespace smg {

SMG_ARAP_HD void wave_rhs(double mt, double s2, double dt, double u, double v, double* b, double* z)
{
    *b = mt * (s2 * u + dt * v);
    *z = 2.0 * u + dt * v;
}

SMG_ARAP_HD double wave_source(double b, double a, double sig0, double sig1) { return b + a * (sig0 + sig1); }

SMG_ARAP_HD void wave_advance(double mt, double q2, double w, double u, double v, double* un, double* vn, double* ke)
{
    const double u1 = w - u;
    const double d = u1 - u;
    const double v1 = q2 * d - v;
    *un = u1;
    *vn = v1;
    *ke = 0.5 * ((mt * v1) * v1);
}

// ---- the host twin (smg_wave_host): the kernels' loops on caller arrays, with the layouts of smg_debug_wave (include/smg.h) --------------------
// mt (nV) = m / (speed speed) (speed nullptr: m); s2 (nV) = 2.0 + sigma dt (sigma nullptr: 2.0)
inline void wave_host_planes(int nV, const double* m, const double* speed, const double* sigma, double dt, double* mt, double* s2)
{
    for (size_t i = 0; i < (size_t)nV; i++) {
        mt[i] = speed ? m[i] / (speed[i] * speed[i]) : m[i];
        s2[i] = sigma ? 2.0 + sigma[i] * dt : 2.0;
    }
}

// u, v (nV x k); b, z (nV x k), rsq (k planes of nV); known (nV, nullptr ok): 1 on the clamped rows
inline void wave_host_rhs(int nV, int k, const double* mt, const double* s2, const int* known, double dt, const double* u, const double* v, double* b,
                          double* rsq, double* z)
{
    const size_t n = (size_t)nV;
    for (int c = 0; c < k; c++)
        for (size_t i = 0; i < n; i++) {
            const size_t e = (size_t)c * n + i;
            wave_rhs(mt[i], s2[i], dt, u[e], v[e], b + e, z + e);
            rsq[e] = known && known[i] ? 0.0 : b[e] * b[e];
        }
}

// idx (n_src vertices, each at most once), sig0, sig1 (n_src x k row-major)
inline void wave_host_sources(int nV, int k, int n_src, const int* idx, const double* sig0, const double* sig1, double a, double* b, double* rsq)
{
    for (int j = 0; j < n_src; j++)
        for (int c = 0; c < k; c++) {
            const size_t e = (size_t)c * (size_t)nV + (size_t)idx[j], s = (size_t)j * (size_t)k + (size_t)c;
            const double x = wave_source(b[e], a, sig0[s], sig1[s]);
            b[e] = x;
            rsq[e] = x * x;
        }
}

// w, u, v (nV x k) -> un, vn (nV x k), ke (k planes of nV); bn != nullptr: the right-hand side, its squares and the warm start of (un, vn)
inline void wave_host_advance(int nV, int k, const double* mt, const double* s2, const int* known, double dt, double q2, const double* w, const double* u,
                              const double* v, double* un, double* vn, double* ke, double* bn, double* rsqn, double* zn)
{
    const size_t n = (size_t)nV;
    for (int c = 0; c < k; c++)
        for (size_t i = 0; i < n; i++) {
            const size_t e = (size_t)c * n + i;
            wave_advance(mt[i], q2, w[e], u[e], v[e], un + e, vn + e, ke + e);
            if (bn) {
                wave_rhs(mt[i], s2[i], dt, un[e], vn[e], bn + e, zn + e);
                rsqn[e] = known && known[i] ? 0.0 : bn[e] * bn[e];
            }
        }
}

// out (n_rec x k row-major) = u at the receivers
inline void wave_host_record(int nV, int k, int n_rec, const int* idx, const double* u, double* out)
{
    for (int j = 0; j < n_rec; j++)
        for (int c = 0; c < k; c++) out[(size_t)j * (size_t)k + (size_t)c] = u[(size_t)c * (size_t)nV + (size_t)idx[j]];
}

}  // namespace smg
