// smg_wave_adjoint_inl.hpp -- the per-entry arithmetic of the wave object's adjoint pass, in registers (csrc/smg_wave_adjoint_device.hip,
// smg_wave_adjoint_host; include/smg.h: smg_wave_gradient).  Layouts as in smg_wave_inl.hpp: vertex blocks are column-major
// nV x k, planes have nV entries, term planes are k planes; a trace row is (receiver slot) x column, a signal row (source) x column.
//
//   keep      e = dt v - (0.5 s2) (u' - u)                          of a forward step from (u, v) to u'
//   residual  rho = trace - observed (observed missing: trace);  sq = rho rho   in k planes of (rows x slots)
//   inject    p = p + (rho[s_0] + rho[s_1] + ...)                    the slots of one vertex in ascending order, none on a known row
//   rhs       g = p + q2 q;  gsq = g g                               both 0.0 on a known row
//   advance   G = G + y e;  t = mt y;  p' = (s2 t - p) - (2.0 q2) q;  q' = dt t - q      (p' and q' from the old p and q)
//   signal    x = a y;  gs0 = gs0 + x;  gs1 = gs1 + x                at the source's vertex
//   scale     out = fac G,  fac = (-2.0 mt) / speed formed on the host
// Only +, - and * occur; host and device compile the same text (the library is built with -ffp-contract=off), so the two agree bit for bit.
#pragma once
#include <cstddef>
#include <vector>

#include "smg_wave_inl.hpp"

namespace smg {

SMG_ARAP_HD double wave_adj_keep(double s2, double dt, double u, double v, double u1)
{
    const double d = u1 - u;
    return dt * v - (0.5 * s2) * d;
}

SMG_ARAP_HD double wave_adj_rhs(double q2, double p, double q) { return p + q2 * q; }

SMG_ARAP_HD void wave_adj_advance(double mt, double s2, double dt, double q2, double y, double e, double p, double q, double G, double* pn, double* qn,
                                  double* Gn)
{
    *Gn = G + y * e;
    const double t = mt * y;
    *pn = (s2 * t - p) - (2.0 * q2) * q;
    *qn = dt * t - q;
}

// ---- the host twin (smg_wave_adjoint_host): the kernels' loops on caller arrays, with the layouts of smg_debug_wave_adjoint (include/smg.h) ---------
// the receivers by vertex: grp_v the distinct vertices in ascending order, none on a known row; the slots of group j, ascending, are
// grp_slot[grp_ptr[j] .. grp_ptr[j + 1])
inline void wave_group_receivers(int nV, int n_rec, const int* idx, const int* known, std::vector<int>& grp_v, std::vector<int>& grp_ptr,
                                 std::vector<int>& grp_slot)
{
    std::vector<int> count((size_t)nV + 1, 0);
    for (int j = 0; j < n_rec; j++)
        if (!(known && known[idx[j]])) count[(size_t)idx[j] + 1]++;
    grp_v.clear();
    grp_ptr.assign(1, 0);
    std::vector<int> at((size_t)nV, -1);
    for (int i = 0; i < nV; i++)
        if (count[(size_t)i + 1] > 0) {
            at[(size_t)i] = (int)grp_v.size();
            grp_v.push_back(i);
            grp_ptr.push_back(grp_ptr.back() + count[(size_t)i + 1]);
        }
    grp_slot.assign((size_t)grp_ptr.back(), 0);
    std::vector<int> fill(grp_ptr.begin(), grp_ptr.end() - 1);
    for (int j = 0; j < n_rec; j++)
        if (at[(size_t)idx[j]] >= 0) grp_slot[(size_t)fill[(size_t)at[(size_t)idx[j]]]++] = j;
}

inline void wave_adj_host_planes(int nV, const double* mt, const double* speed, double* fac)
{
    for (size_t i = 0; i < (size_t)nV; i++) fac[i] = (-2.0 * mt[i]) / (speed ? speed[i] : 1.0);
}

// u, v, u1 (nV x k) -> e (nV x k)
inline void wave_adj_host_keep(int nV, int k, const double* s2, double dt, const double* u, const double* v, const double* u1, double* e)
{
    const size_t n = (size_t)nV;
    for (int c = 0; c < k; c++)
        for (size_t i = 0; i < n; i++) e[(size_t)c * n + i] = wave_adj_keep(s2[i], dt, u[(size_t)c * n + i], v[(size_t)c * n + i], u1[(size_t)c * n + i]);
}

// trace, observed (rows x slots x k row-major; observed nullptr: zeros) -> rho (the same layout), sq (k planes of rows x slots)
inline void wave_adj_host_residual(int k, size_t entries, const double* trace, const double* observed, double* rho, double* sq)
{
    for (size_t j = 0; j < entries; j++)
        for (int c = 0; c < k; c++) {
            const size_t t = j * (size_t)k + (size_t)c;
            const double r = observed ? trace[t] - observed[t] : trace[t];
            rho[t] = r;
            sq[(size_t)c * entries + j] = r * r;
        }
}

// rho: one trace row (slots x k); p (nV x k) in place
inline void wave_adj_host_inject(int nV, int k, int n_grp, const int* grp_v, const int* grp_ptr, const int* grp_slot, const double* rho, double* p)
{
    for (int j = 0; j < n_grp; j++)
        for (int c = 0; c < k; c++) {
            double x = rho[(size_t)grp_slot[grp_ptr[j]] * (size_t)k + (size_t)c];
            for (int s = grp_ptr[j] + 1; s < grp_ptr[j + 1]; s++) x = x + rho[(size_t)grp_slot[s] * (size_t)k + (size_t)c];
            const size_t e = (size_t)c * (size_t)nV + (size_t)grp_v[j];
            p[e] = p[e] + x;
        }
}

// p, q (nV x k) -> g (nV x k), gsq (k planes of nV)
inline void wave_adj_host_rhs(int nV, int k, const int* known, double q2, const double* p, const double* q, double* g, double* gsq)
{
    const size_t n = (size_t)nV;
    for (int c = 0; c < k; c++)
        for (size_t i = 0; i < n; i++) {
            const size_t e = (size_t)c * n + i;
            const double x = known && known[i] ? 0.0 : wave_adj_rhs(q2, p[e], q[e]);
            g[e] = x;
            gsq[e] = x * x;
        }
}

// y, e (nV x k); p, q, G (nV x k) in place
inline void wave_adj_host_advance(int nV, int k, const double* mt, const double* s2, double dt, double q2, const double* y, const double* e, double* p,
                                  double* q, double* G)
{
    const size_t n = (size_t)nV;
    for (int c = 0; c < k; c++)
        for (size_t i = 0; i < n; i++) {
            const size_t o = (size_t)c * n + i;
            wave_adj_advance(mt[i], s2[i], dt, q2, y[o], e[o], p[o], q[o], G[o], p + o, q + o, G + o);
        }
}

// idx (n_src vertices, each at most once), y (nV x k); gs0, gs1 (n_src x k row-major) in place
inline void wave_adj_host_signal(int nV, int k, int n_src, const int* idx, double a, const double* y, double* gs0, double* gs1)
{
    for (int j = 0; j < n_src; j++)
        for (int c = 0; c < k; c++) {
            const size_t s = (size_t)j * (size_t)k + (size_t)c;
            const double x = a * y[(size_t)c * (size_t)nV + (size_t)idx[j]];
            gs0[s] = gs0[s] + x;
            gs1[s] = gs1[s] + x;
        }
}

// G (nV x k) -> out (nV x k)
inline void wave_adj_host_scale(int nV, int k, const double* fac, const double* G, double* out)
{
    const size_t n = (size_t)nV;
    for (int c = 0; c < k; c++)
        for (size_t i = 0; i < n; i++) out[(size_t)c * n + i] = fac[i] * G[(size_t)c * n + i];
}

}  // namespace smg
