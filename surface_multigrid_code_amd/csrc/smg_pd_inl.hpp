// smg_pd_inl.hpp -- the per-face maths of the projective-dynamics membrane step (smg_pd_*, include/smg.h; kernels in csrc/smg_pd_device.hip, host
// side in smg_pd.cpp; Bouaziz, Martin, Liu, Kavan, Pauly 2014, triangle-strain constraints).
//
// Rest pose V, faces F.  Face f has corners p0, p1, p2 in F's order, e1 = p1 - p0, e2 = p2 - p0.
//   rest frame        a = |e1|, b = e1 . e2 / a, c = |e1 x e2| / a (the rest triangle of smg_param_inl.hpp), Dm = [[a, b], [0, c]], A_f = a c / 2;
//                     the four rest constants are r = {a, b, c, A_f}
//   hat gradients     g_1 = (1 / a, -b / (a c)), g_2 = (0, 1 / c), g_0 = -g_1 - g_2 in that frame
//   deformation       of a pose q (3 x 2, columns f1, f2): d1 = q1 - q0, d2 = q2 - q0, f1 = d1 / a, f2 = (d2 - b f1) / c; stored as
//                     Fg = {f1x, f1y, f1z, f2x, f2y, f2z}
//   projection        C = F^T F = [[c11, c12], [c12, c22]], each entry one accumulator over x, y, z in that order.
//                     m = (c11 + c22) / 2, d = (c11 - c22) / 2, r = sqrt(d^2 + c12^2); lambda1 = m + r, lambda2 = max(m - r, 0), sigma_i = sqrt(lambda_i).
//                     Right singular vectors without a trigonometric call: (x, y) = (r + d, c12) when d >= 0, else (c12, r - d) -- the one of
//                     the two eigenvector formulas of lambda1 that adds two numbers of one sign --, n = sqrt(x^2 + y^2), v1 = (x, y) / n,
//                     v1 = (1, 0) when n == 0 (C is a multiple of the identity), v2 = (-v1y, v1x).
//                     Left vectors u_i = (F v_i) / sigma_i, F v_i = f1 v_ix + f2 v_iy.
//                     T_f = sum_i clamp(sigma_i, sigma_min, sigma_max) u_i v_i^T, stored like Fg.  sigma_min = sigma_max = 1: the polar factor.
//   guards            both deterministic, both reported by the return value (1, else 0):
//                     lambda1 == 0: T_f has the columns (t, 0, 0) and (0, t, 0), t = clamp(0, sigma_min, sigma_max);
//                     lambda2 <= 2^-80 lambda1: u2 = the normalised component orthogonal to u1 of the coordinate axis j with the smallest |u1_j|
//                     (the lowest j on a tie).
//   energy term       (k A_f / 2) |F - T|_F^2, one accumulator over the six entries in Fg's order
//   corner shares     k A_f (T_f g_i), i = 0, 1, 2: what corner i adds to the right-hand side of the global step
// A non-finite pose gives non-finite results and no guard; the energy of the same pass is then not finite either, and the step reports it.
// Every expression is written operation by operation; host and device compile the same text with contraction off (-ffp-contract=off) and
// correctly rounded / and sqrt, and tests/pd_np.py restates it in numpy in the same order.
//
// Not covered: bending, collisions, per-face stiffness or thickness, volume constraints, several components, union / block / sharded forms,
// Chebyshev or other acceleration of the outer iteration.
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define SMG_PD_HD __host__ __device__ __forceinline__
#else
#define SMG_PD_HD inline
#endif

namespace smg {

constexpr double PD_RANK_GUARD = 8.271806125530277e-25;   // 2^-80

// r = {a, b, c, A_f} from the corners (xyz each)
SMG_PD_HD void pd_rest(const double* p0, const double* p1, const double* p2, double (&r)[4])
{
    const double e1x = p1[0] - p0[0], e1y = p1[1] - p0[1], e1z = p1[2] - p0[2];
    const double e2x = p2[0] - p0[0], e2y = p2[1] - p0[1], e2z = p2[2] - p0[2];
    const double a = sqrt(e1x * e1x + e1y * e1y + e1z * e1z);
    const double dot = e1x * e2x + e1y * e2y + e1z * e2z;
    const double wx = e1y * e2z - e1z * e2y, wy = e1z * e2x - e1x * e2z, wz = e1x * e2y - e1y * e2x;
    const double b = dot / a, c = sqrt(wx * wx + wy * wy + wz * wz) / a;
    r[0] = a; r[1] = b; r[2] = c;
    r[3] = 0.5 * (a * c);
}

// Fg of the pose with corners q0, q1, q2 (xyz each)
SMG_PD_HD void pd_gradient(const double (&r)[4], const double* q0, const double* q1, const double* q2, double (&Fg)[6])
{
#pragma unroll
    for (int l = 0; l < 3; l++) {
        const double d1 = q1[l] - q0[l], d2 = q2[l] - q0[l];
        Fg[l] = d1 / r[0];
        Fg[3 + l] = (d2 - r[1] * Fg[l]) / r[2];
    }
}

SMG_PD_HD double pd_clamp(double s, double lo, double hi) { return s < lo ? lo : (s > hi ? hi : s); }

// sigma = {sigma1, sigma2} and T (the layout of Fg) of Fg; returns 1 when a guard fired
SMG_PD_HD int pd_project(const double (&Fg)[6], double smin, double smax, double (&sigma)[2], double (&T)[6])
{
    const double c11 = (Fg[0] * Fg[0] + Fg[1] * Fg[1]) + Fg[2] * Fg[2];
    const double c12 = (Fg[0] * Fg[3] + Fg[1] * Fg[4]) + Fg[2] * Fg[5];
    const double c22 = (Fg[3] * Fg[3] + Fg[4] * Fg[4]) + Fg[5] * Fg[5];
    const double m = 0.5 * (c11 + c22), d = 0.5 * (c11 - c22);
    const double r = sqrt(d * d + c12 * c12);
    const double l1 = m + r, l2 = fmax(m - r, 0.0);
    sigma[0] = sqrt(l1);
    sigma[1] = sqrt(l2);
    const double t1 = pd_clamp(sigma[0], smin, smax), t2 = pd_clamp(sigma[1], smin, smax);
    if (l1 == 0.0) {
        T[0] = t1; T[1] = 0.0; T[2] = 0.0;
        T[3] = 0.0; T[4] = t1; T[5] = 0.0;
        return 1;
    }
    const double x = d >= 0.0 ? r + d : c12, y = d >= 0.0 ? c12 : r - d;
    const double n = sqrt(x * x + y * y);
    double v1x = 1.0, v1y = 0.0;
    if (n > 0.0) { v1x = x / n; v1y = y / n; }
    const double v2x = 0.0 - v1y, v2y = v1x;
    double u1[3], u2[3];
#pragma unroll
    for (int l = 0; l < 3; l++) u1[l] = (Fg[l] * v1x + Fg[3 + l] * v1y) / sigma[0];
    int guard = 0;
    if (l2 <= PD_RANK_GUARD * l1) {
        guard = 1;
        const double a0 = fabs(u1[0]), a1 = fabs(u1[1]), a2 = fabs(u1[2]);
        const int j = (a0 <= a1 && a0 <= a2) ? 0 : (a1 <= a2 ? 1 : 2);
        const double uj = j == 0 ? u1[0] : j == 1 ? u1[1] : u1[2];
        const double w0 = (j == 0 ? 1.0 : 0.0) - uj * u1[0], w1 = (j == 1 ? 1.0 : 0.0) - uj * u1[1], w2 = (j == 2 ? 1.0 : 0.0) - uj * u1[2];
        const double len = sqrt((w0 * w0 + w1 * w1) + w2 * w2);
        u2[0] = w0 / len; u2[1] = w1 / len; u2[2] = w2 / len;
    } else {
#pragma unroll
        for (int l = 0; l < 3; l++) u2[l] = (Fg[l] * v2x + Fg[3 + l] * v2y) / sigma[1];
    }
    const double s1x = t1 * v1x, s1y = t1 * v1y, s2x = t2 * v2x, s2y = t2 * v2y;
#pragma unroll
    for (int l = 0; l < 3; l++) {
        T[l] = s1x * u1[l] + s2x * u2[l];
        T[3 + l] = s1y * u1[l] + s2y * u2[l];
    }
    return guard;
}

// |F - T|_F^2
SMG_PD_HD double pd_distance2(const double (&Fg)[6], const double (&T)[6])
{
    double acc = 0.0;
#pragma unroll
    for (int e = 0; e < 6; e++) {
        const double x = Fg[e] - T[e];
        acc += x * x;
    }
    return acc;
}

// the face's term of E: (k A_f / 2) |F - T|_F^2
SMG_PD_HD double pd_face_energy(const double (&r)[4], double k, const double (&Fg)[6], const double (&T)[6])
{
    return 0.5 * ((k * r[3]) * pd_distance2(Fg, T));
}

// the corner shares k A_f (T g_i) as s[3 i + l]
SMG_PD_HD void pd_corner_shares(const double (&r)[4], double k, const double (&T)[6], double (&s)[9])
{
    const double kA = k * r[3];
    const double g1x = 1.0 / r[0], g1y = 0.0 - r[1] / (r[0] * r[2]), g2y = 1.0 / r[2];
#pragma unroll
    for (int l = 0; l < 3; l++) {
        const double t1 = T[l] * g1x + T[3 + l] * g1y, t2 = T[3 + l] * g2y;
        s[l] = kA * ((0.0 - t1) - t2);
        s[3 + l] = kA * t1;
        s[6 + l] = kA * t2;
    }
}

}  // namespace smg
