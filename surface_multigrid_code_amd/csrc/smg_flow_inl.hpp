// smg_flow_inl.hpp -- the arithmetic of the conformalized mean-curvature flow and its sphere map, in registers (csrc/smg_flow_device.hip,
// smg_flow_host; include/smg.h: smg_flow_*).  Positions are column-major nV x 3 blocks (coordinate d of vertex i at
// [d * ld + i]), the layout of the solver's blocks.
//
//   darea     twice the area of a face: the expression of k_face_terms (smg_device.hip), operation by operation
//   mass      the barycentric mass of a vertex: the sum over its corner list, faces ascending, of darea / 6 (k_mass_diag's order)
//   entry     a value of M_t - delta L_0: (-delta) L0[j], the mass added on the diagonal slot
//   radius    |U_i - c|
//   sigma     the singular values of the 3 x 2 Jacobian that takes a rest face to its image: with the rest face laid into the plane as
//             (0, 0), (x1, 0), (x2, y2), x1 = |e1|, x2 = e1 . e2 / x1, y2 = darea / x1, the Jacobian's columns are j1 = s1 / x1 and
//             j2 = (s2 - x2 j1) / y2;  E = j1 . j1, G = j2 . j2, Fm = j1 . j2;  sigma1 = sqrt((E + G) / 2 + sqrt(((E - G) / 2)^2 + Fm^2)),
//             sigma2 = |j1 x j2| / sigma1 (the product of the two is the ratio of the areas, which the cross product gives without cancellation)
//   flipped   n . centroid <= 0 for the image face on the sphere (n = s1 x s2, the centroid taken as the corners' sum)
// Only +, -, *, / and sqrt occur; host and device compile the same text (the library is built with -ffp-contract=off), so the two agree bit for
// bit.  The host twin's sums restate launch_fixed_sum / launch_fixed_max (smg_fixed_sum_device.hip) in their order.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <vector>

#include "smg_arap_inl.hpp"

namespace smg {

SMG_ARAP_HD double flow_darea(const double* a, const double* b, const double* c)
{
    const double ux = b[0] - a[0], uy = b[1] - a[1], uz = b[2] - a[2];
    const double vx = c[0] - a[0], vy = c[1] - a[1], vz = c[2] - a[2];
    const double wx = uy * vz - uz * vy, wy = uz * vx - ux * vz, wz = ux * vy - uy * vx;
    return sqrt(wx * wx + wy * wy + wz * wz);
}

// the three corners of face f from a column-major block
SMG_ARAP_HD void flow_corners(const double* U, size_t ld, const int* F, size_t f, double* a, double* b, double* c)
{
    const size_t i0 = (size_t)F[3 * f], i1 = (size_t)F[3 * f + 1], i2 = (size_t)F[3 * f + 2];
#pragma unroll
    for (int d = 0; d < 3; d++) {
        a[d] = U[d * ld + i0];
        b[d] = U[d * ld + i1];
        c[d] = U[d * ld + i2];
    }
}

SMG_ARAP_HD double flow_face_darea(const double* U, size_t ld, const int* F, size_t f)
{
    double a[3], b[3], c[3];
    flow_corners(U, ld, F, f, a, b, c);
    return flow_darea(a, b, c);
}

// the barycentric mass of vertex v: its corners t = 3 f + i in list order, one accumulator from 0
SMG_ARAP_HD double flow_mass(const double* U, size_t ld, const int* F, const int* m_ptr, const int* m_idx, int v)
{
    double s = 0.0;
    const int p1 = m_ptr[v + 1];
    for (int p = m_ptr[v]; p < p1; p++) s += flow_face_darea(U, ld, F, (size_t)(m_idx[p] / 3)) / 6.0;
    return s;
}

SMG_ARAP_HD double flow_entry(double neg_delta, double L0, double mass, bool diagonal)
{
    const double x = neg_delta * L0;
    return diagonal ? mass + x : x;
}

SMG_ARAP_HD double flow_radius(double x, double y, double z, double cx, double cy, double cz)
{
    const double dx = x - cx, dy = y - cy, dz = z - cz;
    return sqrt(dx * dx + dy * dy + dz * dz);
}

// (a, b, c): the rest face, (p, q, r): its image.  sig[0] >= sig[1]; *flipped = 1.0 or 0.0
SMG_ARAP_HD void flow_sigma(const double* a, const double* b, const double* c, const double* p, const double* q, const double* r, double* sig,
                            double* flipped)
{
    const double e1[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, e2[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
    const double s1[3] = {q[0] - p[0], q[1] - p[1], q[2] - p[2]}, s2[3] = {r[0] - p[0], r[1] - p[1], r[2] - p[2]};
    const double x1 = sqrt(e1[0] * e1[0] + e1[1] * e1[1] + e1[2] * e1[2]);
    const double x2 = (e1[0] * e2[0] + e1[1] * e2[1] + e1[2] * e2[2]) / x1;
    const double y2 = flow_darea(a, b, c) / x1;
    double j1[3], j2[3];
#pragma unroll
    for (int d = 0; d < 3; d++) {
        j1[d] = s1[d] / x1;
        j2[d] = (s2[d] - x2 * j1[d]) / y2;
    }
    const double E = j1[0] * j1[0] + j1[1] * j1[1] + j1[2] * j1[2];
    const double G = j2[0] * j2[0] + j2[1] * j2[1] + j2[2] * j2[2];
    const double Fm = j1[0] * j2[0] + j1[1] * j2[1] + j1[2] * j2[2];
    const double h = (E + G) * 0.5, g = (E - G) * 0.5;
    const double cx = j1[1] * j2[2] - j1[2] * j2[1], cy = j1[2] * j2[0] - j1[0] * j2[2], cz = j1[0] * j2[1] - j1[1] * j2[0];
    sig[0] = sqrt(h + sqrt(g * g + Fm * Fm));
    sig[1] = sqrt(cx * cx + cy * cy + cz * cz) / sig[0];
    const double nx = s1[1] * s2[2] - s1[2] * s2[1], ny = s1[2] * s2[0] - s1[0] * s2[2], nz = s1[0] * s2[1] - s1[1] * s2[0];
    const double mx = (p[0] + q[0]) + r[0], my = (p[1] + q[1]) + r[1], mz = (p[2] + q[2]) + r[2];
    *flipped = (nx * mx + ny * my + nz * mz <= 0.0) ? 1.0 : 0.0;
}

// ---- the host twin: the kernels' loops on caller arrays, the sums in launch_fixed_sum's order ---------------------------------------------------
enum { FLOW_SUM_THREADS = 256, FLOW_SUM_ROWS = 8, FLOW_SUM_MAX_GROUPS = 1024 };

inline int flow_host_groups(int n)
{
    const long want = ((long)n + (long)FLOW_SUM_THREADS * FLOW_SUM_ROWS - 1) / ((long)FLOW_SUM_THREADS * FLOW_SUM_ROWS);
    return (int)std::max(1L, std::min(want, (long)FLOW_SUM_MAX_GROUPS));
}

// MAX == false: the sum; true: the maximum through the same tree (a NaN loses against a number, as fmax has it)
template <bool MAX>
inline double flow_host_reduce(const double* term, int n)
{
    auto comb = [](double a, double b) { return MAX ? std::fmax(a, b) : a + b; };
    const double id = MAX ? -HUGE_VAL : 0.0;
    const int groups = flow_host_groups(n), rpc = (n + groups - 1) / groups;
    std::vector<double> part((size_t)groups);
    double red[FLOW_SUM_THREADS];
    for (int g = 0; g < groups; g++) {
        const int r0 = g * rpc, r1 = std::min(n, r0 + rpc);
        for (int t = 0; t < FLOW_SUM_THREADS; t++) {
            double acc = id;
            for (int r = r0 + t; r < r1; r += FLOW_SUM_THREADS) acc = comb(acc, term[r]);
            red[t] = acc;
        }
        for (int half = FLOW_SUM_THREADS / 2; half > 0; half >>= 1)
            for (int t = 0; t < half; t++) red[t] = comb(red[t], red[t + half]);
        part[(size_t)g] = red[0];
    }
    double v[64];
    for (int l = 0; l < 64; l++) {
        double acc = id;
        for (int g = l; g < groups; g += 64) acc = comb(acc, part[(size_t)g]);
        v[l] = acc;
    }
    for (int o = 32; o > 0; o >>= 1)
        for (int l = 0; l < o; l++) v[l] = comb(v[l], v[l + o]);
    return v[0];
}
inline double flow_host_sum(const double* term, int n) { return flow_host_reduce<false>(term, n); }
inline double flow_host_max(const double* term, int n) { return flow_host_reduce<true>(term, n); }

// k_flow_system: mass (nV), B (nV x 3 column-major), val (the CSR's entries)
inline void flow_host_system(int nV, const int* F, const int* m_ptr, const int* m_idx, const double* U, const int* rowptr, const int* col,
                             const double* L0, double delta, double* mass, double* B, double* val)
{
    const size_t n = (size_t)nV;
    const double nd = -delta;
    for (int v = 0; v < nV; v++) {
        const double m = flow_mass(U, n, F, m_ptr, m_idx, v);
        mass[v] = m;
        for (int d = 0; d < 3; d++) B[d * n + v] = m * U[d * n + v];
        for (int j = rowptr[v]; j < rowptr[v + 1]; j++) val[j] = flow_entry(nd, L0[j], m, col[j] == v);
    }
}

// k_flow_normalize: out = U / sqrt(sum of double areas / 2), then x and y minus their means and z minus its minimum
inline void flow_host_normalize(int nV, int nF, const int* F, const double* U, double* out)
{
    const size_t n = (size_t)nV;
    std::vector<double> term((size_t)std::max(nF, nV));
    for (int f = 0; f < nF; f++) term[(size_t)f] = flow_face_darea(U, n, F, (size_t)f);
    const double scale = std::sqrt(flow_host_sum(term.data(), nF) / 2.0);
    for (size_t i = 0; i < 3 * n; i++) out[i] = U[i] / scale;
    for (size_t i = 0; i < n; i++) term[i] = 0.0 - out[2 * n + i];
    const double mx = flow_host_sum(out, nV) / (double)nV, my = flow_host_sum(out + n, nV) / (double)nV;
    const double zmin = 0.0 - flow_host_max(term.data(), nV);
    for (size_t i = 0; i < n; i++) {
        out[i] = out[i] - mx;
        out[n + i] = out[n + i] - my;
        out[2 * n + i] = out[2 * n + i] - zmin;
    }
}

// k_flow_sphericity: s[0] = the sphericity, s[1] = sum a, s[2 .. 4] = sum a U, s[5] = sum a r, s[6] = sum a (r - rbar)^2
inline void flow_host_sphericity(int nV, const int* F, const int* m_ptr, const int* m_idx, const double* U, double* s)
{
    const size_t n = (size_t)nV;
    std::vector<double> a(n), r(n), term(n);
    for (int v = 0; v < nV; v++) a[(size_t)v] = flow_mass(U, n, F, m_ptr, m_idx, v);
    s[1] = flow_host_sum(a.data(), nV);
    for (int d = 0; d < 3; d++) {
        for (size_t i = 0; i < n; i++) term[i] = a[i] * U[d * n + i];
        s[2 + d] = flow_host_sum(term.data(), nV);
    }
    const double cx = s[2] / s[1], cy = s[3] / s[1], cz = s[4] / s[1];
    for (size_t i = 0; i < n; i++) {
        r[i] = flow_radius(U[i], U[n + i], U[2 * n + i], cx, cy, cz);
        term[i] = a[i] * r[i];
    }
    s[5] = flow_host_sum(term.data(), nV);
    const double rbar = s[5] / s[1];
    for (size_t i = 0; i < n; i++) {
        const double d = r[i] - rbar;
        term[i] = a[i] * (d * d);
    }
    s[6] = flow_host_sum(term.data(), nV);
    s[0] = std::sqrt(s[6] / s[1]) / rbar;
}

// k_flow_sphere_*: S (nV x 3 column-major), sigma (2 planes of nF), terms (4 planes of nF: A_f sigma1 / sigma2, A_f, sigma1 / sigma2, flipped),
// stats (4: the area-weighted mean of sigma1 / sigma2, its maximum, the flipped count, the sphericity)
inline void flow_host_sphere(int nV, int nF, const int* F, const int* m_ptr, const int* m_idx, const double* U, const double* V0, double* S,
                             double* sigma, double* terms, double* stats)
{
    const size_t n = (size_t)nV, nf = (size_t)nF;
    double s[7];
    flow_host_sphericity(nV, F, m_ptr, m_idx, U, s);
    const double cx = s[2] / s[1], cy = s[3] / s[1], cz = s[4] / s[1];
    for (size_t i = 0; i < n; i++) {
        const double r = flow_radius(U[i], U[n + i], U[2 * n + i], cx, cy, cz);
        S[i] = (U[i] - cx) / r;
        S[n + i] = (U[n + i] - cy) / r;
        S[2 * n + i] = (U[2 * n + i] - cz) / r;
    }
    for (size_t f = 0; f < nf; f++) {
        double a[3], b[3], c[3], p[3], q[3], r[3], sg[2], fl;
        flow_corners(V0, n, F, f, a, b, c);
        flow_corners(S, n, F, f, p, q, r);
        flow_sigma(a, b, c, p, q, r, sg, &fl);
        const double A = flow_darea(a, b, c) * 0.5, ratio = sg[0] / sg[1];
        sigma[f] = sg[0];
        sigma[nf + f] = sg[1];
        terms[f] = A * ratio;
        terms[nf + f] = A;
        terms[2 * nf + f] = ratio;
        terms[3 * nf + f] = fl;
    }
    stats[0] = flow_host_sum(terms, nF) / flow_host_sum(terms + nf, nF);
    stats[1] = flow_host_max(terms + 2 * nf, nF);
    stats[2] = flow_host_sum(terms + 3 * nf, nF);
    stats[3] = s[0];
}
}  // namespace smg
