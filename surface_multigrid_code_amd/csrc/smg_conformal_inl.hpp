// smg_conformal_inl.hpp -- the arithmetic of the discrete conformal metric, in registers (csrc/smg_conformal_device.hip, smg_conformal_host;
// include/smg.h: smg_conformal_*).  Springborn, Schroeder, Pinkall 2008: one log scale factor u_i per vertex, the metric
// l~_ij = l_ij exp((u_i + u_j) / 2).
//
//   rest      l0[3 f + c] = the length of the edge opposite corner c: the expressions of k_face_terms (smg_device.hip) for l0, l1, l2;
//             area2[f] = twice the rest area, its dA
//   scale     s_i = exp(-u_i / 2), of u or of the trial u + t d: the only exp of the method
//   face      a_c = l0[3 f + c] s_{F[f][c]}: the face's lengths divided by its common factor exp((u_i + u_j + u_k) / 2); angles and cotangents
//             depend on ratios alone.  S = a + b + c, s0 = b + c - a, s1 = a + c - b, s2 = a + b - c;
//             angle 0 = 2 atan2(sqrt(s1 s2), sqrt(S s0)), half cotangent 0 = (b b + c c - a a) / sqrt(S s0 s1 s2) / 2, cyclically.
//             The quotient is formed as (b b + c c - a a) / (dA0 r) / 4 with dA0 twice the rest area as smg_mesh_cotmatrix forms it (the cross
//             product) and r = sqrt(S s0 s1 s2) / sqrt(S' s0' s1' s2') the ratio of Heron's root to the same root of the rest lengths: dA0 r is
//             sqrt(S s0 s1 s2) / 2, and at s = 1 the ratio is x / x = 1 exactly, so the values at u = 0 are smg_mesh_cotmatrix's bit for bit.
//             A face with some s_c <= 0 is broken: the angle opposite the too-long edge is pi, the others 0, the half cotangents 0.
//   length    l~ of the edge opposite corner c = l0[3 f + c] / (s_j s_k), j and k the other two corners
//   row       the angle sum over the corner list (faces ascending), g = sum - Theta (0 on a fixed row), and the row's values of -L~ from the
//             half cotangents in smg_mesh_cotmatrix's term order (AssemblyPlan: l_ptr, l_idx, l_sgn)
// Apart from exp and atan2 only +, -, *, / and sqrt occur; host and device compile the same text (the library is built with -ffp-contract=off),
// so given the same s the half cotangents, flags, lengths and matrix values agree bit for bit.  The host twin's sums are flow_host_sum / _max.
#pragma once
#include <cmath>
#include <cstddef>
#include <vector>

#include "smg_flow_inl.hpp"

namespace smg {

constexpr double CONFORMAL_PI = 3.14159265358979323846;

// twice the rest area of face f of a mesh given as xyz rows: the expression of k_face_terms and smg_mesh_cotmatrix (the cross product)
SMG_ARAP_HD double conformal_rest_area2(const double* V, const int* F, size_t f)
{
    const double* a = V + 3 * (size_t)F[3 * f];
    const double* b = V + 3 * (size_t)F[3 * f + 1];
    const double* c = V + 3 * (size_t)F[3 * f + 2];
    const double ux = b[0] - a[0], uy = b[1] - a[1], uz = b[2] - a[2];
    const double vx = c[0] - a[0], vy = c[1] - a[1], vz = c[2] - a[2];
    const double wx = uy * vz - uz * vy, wy = uz * vx - ux * vz, wz = ux * vy - uy * vx;
    return sqrt(wx * wx + wy * wy + wz * wz);
}

// the three rest lengths of face f of a mesh given as xyz rows
SMG_ARAP_HD void conformal_rest_lengths(const double* V, const int* F, size_t f, double* l)
{
    const double* a = V + 3 * (size_t)F[3 * f];
    const double* b = V + 3 * (size_t)F[3 * f + 1];
    const double* c = V + 3 * (size_t)F[3 * f + 2];
    const double d0x = b[0] - c[0], d0y = b[1] - c[1], d0z = b[2] - c[2];
    const double d1x = c[0] - a[0], d1y = c[1] - a[1], d1z = c[2] - a[2];
    const double d2x = a[0] - b[0], d2y = a[1] - b[1], d2z = a[2] - b[2];
    l[0] = sqrt(d0x * d0x + d0y * d0y + d0z * d0z);
    l[1] = sqrt(d1x * d1x + d1y * d1y + d1z * d1z);
    l[2] = sqrt(d2x * d2x + d2y * d2y + d2z * d2z);
}

// the trial u + t d (d == nullptr: u itself) and its scale
SMG_ARAP_HD double conformal_trial(const double* u, const double* d, double t, size_t i) { return d ? u[i] + t * d[i] : u[i]; }
SMG_ARAP_HD double conformal_scale(double u) { return exp((0.0 - u) / 2.0); }

// Heron's root sqrt(S s0 s1 s2) = four times the area of a triangle with lengths a, b, c
SMG_ARAP_HD double conformal_heron(double a, double b, double c)
{
    const double S = a + b + c, s0 = b + c - a, s1 = a + c - b, s2 = a + b - c;
    return sqrt(S * s0 * s1 * s2);
}

// the angles and half cotangents of a face with scaled lengths a, b, c (opposite corners 0, 1, 2); q0 = Heron's root of the rest lengths,
// dA0 = twice the rest area; returns 1.0 for a broken face
SMG_ARAP_HD double conformal_face(double a, double b, double c, double q0, double dA0, double* ang, double* hc)
{
    const double S = a + b + c, s0 = b + c - a, s1 = a + c - b, s2 = a + b - c;
    if (s0 <= 0.0 || s1 <= 0.0 || s2 <= 0.0) {
        const int big = s0 <= 0.0 ? 0 : s1 <= 0.0 ? 1 : 2;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            ang[k] = k == big ? CONFORMAL_PI : 0.0;
            hc[k] = 0.0;
        }
        return 1.0;
    }
    ang[0] = 2.0 * atan2(sqrt(s1 * s2), sqrt(S * s0));
    ang[1] = 2.0 * atan2(sqrt(s2 * s0), sqrt(S * s1));
    ang[2] = 2.0 * atan2(sqrt(s0 * s1), sqrt(S * s2));
    const double dA = dA0 * (sqrt(S * s0 * s1 * s2) / q0);
    hc[0] = (b * b + c * c - a * a) / dA / 4.0;
    hc[1] = (c * c + a * a - b * b) / dA / 4.0;
    hc[2] = (a * a + b * b - c * c) / dA / 4.0;
    return 0.0;
}

// face f from the rest lengths and the per-vertex scales
SMG_ARAP_HD double conformal_face_at(const int* F, const double* l0, const double* area2, const double* s, size_t f, double* ang, double* hc)
{
    const double a = l0[3 * f] * s[F[3 * f]], b = l0[3 * f + 1] * s[F[3 * f + 1]], c = l0[3 * f + 2] * s[F[3 * f + 2]];
    return conformal_face(a, b, c, conformal_heron(l0[3 * f], l0[3 * f + 1], l0[3 * f + 2]), area2[f], ang, hc);
}

SMG_ARAP_HD void conformal_lengths_at(const int* F, const double* l0, const double* s, size_t f, double* lt)
{
    const double s0 = s[F[3 * f]], s1 = s[F[3 * f + 1]], s2 = s[F[3 * f + 2]];
    lt[0] = l0[3 * f] / (s1 * s2);
    lt[1] = l0[3 * f + 1] / (s2 * s0);
    lt[2] = l0[3 * f + 2] / (s0 * s1);
}

// the angle sum of vertex v: its corners t = 3 f + c in list order, one accumulator from 0
SMG_ARAP_HD double conformal_angle_sum(const double* ang, const int* m_ptr, const int* m_idx, int v)
{
    double sum = 0.0;
    const int p1 = m_ptr[v + 1];
    for (int p = m_ptr[v]; p < p1; p++) sum += ang[m_idx[p]];
    return sum;
}

// entry e of -L~: the terms of the cotangent matrix's entry in cotmatrix()'s order (first term assigns), times -1: k_assemble_vals with
// mass_coef = 0 and lap_coef = -1
SMG_ARAP_HD double conformal_entry(const double* hc, const int* l_ptr, const int* l_idx, const signed char* l_sgn, int e)
{
    const int b = l_ptr[e], en = l_ptr[e + 1];
    double L = 0.0;
    if (b < en) {
        L = l_sgn[b] > 0 ? hc[l_idx[b]] : -hc[l_idx[b]];
        for (int t = b + 1; t < en; t++) L += l_sgn[t] > 0 ? hc[l_idx[t]] : -hc[l_idx[t]];
    }
    return -1.0 * L;
}

// ---- the host twin: the kernels' loops on caller arrays ---------------------------------------------------------------------------------------
// k_conformal_scale: s (nV), then the trial u + t d (nV)
inline void conformal_host_scale(int nV, const double* u, const double* d, double t, double* s, double* ut)
{
    for (size_t i = 0; i < (size_t)nV; i++) {
        const double x = conformal_trial(u, d, t, i);
        ut[i] = x;
        s[i] = conformal_scale(x);
    }
}

// k_conformal_faces and k_conformal_lengths: ang, hc (nF x 3 each), broken (nF), lt (nF x 3; nullptr: not wanted)
inline void conformal_host_faces(int nF, const int* F, const double* l0, const double* area2, const double* s, double* ang, double* hc, double* broken,
                                 double* lt)
{
    for (size_t f = 0; f < (size_t)nF; f++) {
        broken[f] = conformal_face_at(F, l0, area2, s, f, ang + 3 * f, hc + 3 * f);
        if (lt) conformal_lengths_at(F, l0, s, f, lt + 3 * f);
    }
}

// k_conformal_rows: sum, g, g^2, |g| (nV each), val (the CSR's entries; nullptr: the form without values)
inline void conformal_host_rows(int nV, const double* ang, const double* hc, const int* m_ptr, const int* m_idx, const double* Theta, const int* fixed,
                                const int* rowptr, const int* l_ptr, const int* l_idx, const signed char* l_sgn, double* sum, double* g, double* gsq,
                                double* gabs, double* val)
{
    for (int v = 0; v < nV; v++) {
        const double a = conformal_angle_sum(ang, m_ptr, m_idx, v);
        const double gv = fixed[v] ? 0.0 : a - Theta[v];
        sum[v] = a;
        g[v] = gv;
        gsq[v] = gv * gv;
        gabs[v] = std::fabs(gv);
        if (val)
            for (int e = rowptr[v]; e < rowptr[v + 1]; e++) val[e] = conformal_entry(hc, l_ptr, l_idx, l_sgn, e);
    }
}

}  // namespace smg
