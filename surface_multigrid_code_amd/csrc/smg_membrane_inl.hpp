// smg_membrane_inl.hpp -- the membrane energy of one triangle (neo-Hookean; StVK and tension-field StVK further down), its gradient, its
// Hessian and the Hessian's eigenvalue fix, in registers (k_membrane_faces, k_membrane_faces_mat, csrc/smg_membrane_device.hip;
// smg_membrane_faces_host, smg_membrane_faces_host_material); and what smg_membrane.cpp shares with the kernel hooks:
// the Lame parameters and the lists of the matrix kernel.
//
// Corners q0, q1, q2, e1 = q1 - q0, e2 = q2 - q0, a = [[e1.e1, e1.e2], [e1.e2, e2.e2]], abar = a of the rest pose:
//   lnJ = log(det a / det abar) / 2,   W = coeff (beta (tr(abar^-1 a) - 2 - 2 lnJ) + alpha lnJ^2),   coeff = h sqrt(det abar) / 4.
// The derivative of vec(a) has the rows r0 = [-2 e1, 2 e1, 0], r1 = r2 = [-(e1 + e2), e2, e1], r3 = [-2 e2, 0, 2 e2], so for a symmetric 2 x 2
// c the combination c00 r0 + 2 c01 r1 + c11 r3 is 2 [-(u + v), u, v] with u = c00 e1 + c01 e2, v = c01 e1 + c11 e2.  With t1 = alpha lnJ - beta,
// T = beta abar^-1 + t1 a^-1 and p the combination of a^-1:
//   G = coeff comb(T)
//   H = coeff ((alpha / 2 - t1) p p^T + (t1 / det a) (r3 r0^T + r0 r3^T - 2 r1 r1^T) + S (x) I_3),     S from the four constant second
//   derivatives of a:  S11 = 2 T00, S22 = 2 T11, S12 = 2 T01, S01 = -2 (T00 + T01), S02 = -2 (T01 + T11), S00 = 2 (T00 + 2 T01 + T11).
// H is stored as its upper triangle, row by row (entry (r, c), r <= c, at mem_tri(r, c); 45 doubles).
//
// The eigenvalue fix (every eigenvalue below `floor` becomes `value`) uses the structure of H: it annihilates the three translations, so with
// the orthonormal basis B = [c1 (x) I_3, c2 (x) I_3], c1 = (1, -1, 0) / sqrt 2, c2 = (1, 1, -2) / sqrt 6, of their complement
//   H' = B fix(B^T H B) B^T + value (1/3) (1 1^T (x) I_3),
// which is Q fix(Lambda) Q^T of the 9 x 9 whenever its three translation eigenvalues (zero up to rounding) are below the floor.  B^T H B is
// 6 x 6; its eigen-decomposition is a cyclic Jacobi whose 15 rotations per sweep are unrolled over compile-time index pairs, so every array
// lives in registers (a run-time index would send it to scratch).  A pair is rotated while |a_pq| > eps |A|_F; the sweeps end when one of
// them rotates nothing, after MEM_SWEEP_CAP at the latest.
// Host and device compile the same text (the library is built with -ffp-contract=off).
#pragma once
#include <cmath>
#include <vector>

#include "../../include/smg.h"

#if defined(__HIPCC__)
#define SMG_MEM_HD __host__ __device__ __forceinline__
#else
#define SMG_MEM_HD inline
#endif

namespace smg {

constexpr int MEM_SWEEP_CAP = 12;
constexpr double MEM_EPS = 2.220446049250313e-16;
constexpr double MEM_S = 0.70710678118654752440;     // 1 / sqrt 2
constexpr double MEM_T = 0.40824829046386301637;     // 1 / sqrt 6

SMG_MEM_HD constexpr int mem_tri(int r, int c) { return r * 9 - r * (r - 1) / 2 + (c - r); }
SMG_MEM_HD constexpr int mem_sym(int r, int c) { return r <= c ? mem_tri(r, c) : mem_tri(c, r); }
// entry j of c_a
SMG_MEM_HD constexpr double mem_basis(int a, int j) { return a == 0 ? (j == 0 ? MEM_S : j == 1 ? -MEM_S : 0.0) : (j == 2 ? -2.0 * MEM_T : MEM_T); }

// 2 [-(u + v), u, v], u = c00 e1 + c01 e2, v = c01 e1 + c11 e2
SMG_MEM_HD void mem_comb(const double (&e1)[3], const double (&e2)[3], double c00, double c01, double c11, double (&out)[9])
{
#pragma unroll
    for (int d = 0; d < 3; d++) {
        const double u = 2.0 * (c00 * e1[d] + c01 * e2[d]), v = 2.0 * (c01 * e1[d] + c11 * e2[d]);
        out[d] = -(u + v);
        out[3 + d] = u;
        out[6 + d] = v;
    }
}

// the Lame parameters of the material (the reference's main.cpp:63-67)
inline void lame(const smg_membrane_params& p, double& alpha, double& beta)
{
    alpha = p.young * p.poisson / (1.0 - p.poisson * p.poisson);
    beta = p.young / 2.0 / (1.0 + p.poisson);
}

// q: the corners (q0, q1, q2), 9 doubles.  rest: (abar^-1)00, 01, 11, det abar, coeff.  Returns W (+inf where det a <= 0 or is not a
// number); with DERIVS also G (9) and the upper triangle of the unfixed H (45).
template <bool DERIVS>
SMG_MEM_HD double membrane_face(const double (&q)[9], const double (&rest)[5], double alpha, double beta, double (&G)[9], double (&H)[45])
{
    double e1[3], e2[3];
#pragma unroll
    for (int d = 0; d < 3; d++) { e1[d] = q[3 + d] - q[d]; e2[d] = q[6 + d] - q[d]; }
    const double a00 = (e1[0] * e1[0] + e1[1] * e1[1]) + e1[2] * e1[2];
    const double a01 = (e1[0] * e2[0] + e1[1] * e2[1]) + e1[2] * e2[2];
    const double a11 = (e2[0] * e2[0] + e2[1] * e2[1]) + e2[2] * e2[2];
    const double det = a00 * a11 - a01 * a01;
    const double coeff = rest[4];
    const double lnJ = log(det / rest[3]) / 2.0;
    const double tr = (rest[0] * a00 + 2.0 * (rest[1] * a01)) + rest[2] * a11;
    double W = coeff * (beta * ((tr - 2.0) - 2.0 * lnJ) + alpha * (lnJ * lnJ));
    if (!(det > 0.0)) W = INFINITY;
    if (!DERIVS) return W;

    const double t1 = alpha * lnJ - beta;
    const double i00 = a11 / det, i01 = -a01 / det, i11 = a00 / det;
    const double T00 = beta * rest[0] + t1 * i00, T01 = beta * rest[1] + t1 * i01, T11 = beta * rest[2] + t1 * i11;
    double g[9], p[9], r0[9], r1[9], r3[9];
    mem_comb(e1, e2, T00, T01, T11, g);
    mem_comb(e1, e2, i00, i01, i11, p);
#pragma unroll
    for (int d = 0; d < 3; d++) {
        G[d] = coeff * g[d]; G[3 + d] = coeff * g[3 + d]; G[6 + d] = coeff * g[6 + d];
        r0[d] = -2.0 * e1[d]; r0[3 + d] = 2.0 * e1[d]; r0[6 + d] = 0.0;
        r1[d] = -(e1[d] + e2[d]); r1[3 + d] = e2[d]; r1[6 + d] = e1[d];
        r3[d] = -2.0 * e2[d]; r3[3 + d] = 0.0; r3[6 + d] = 2.0 * e2[d];
    }
    const double k1 = 0.5 * alpha - t1, k2 = t1 / det;
    const double S2[3][3] = {{2.0 * ((T00 + 2.0 * T01) + T11), -2.0 * (T00 + T01), -2.0 * (T01 + T11)},
                             {-2.0 * (T00 + T01), 2.0 * T00, 2.0 * T01},
                             {-2.0 * (T01 + T11), 2.0 * T01, 2.0 * T11}};
#pragma unroll
    for (int r = 0; r < 9; r++)
#pragma unroll
        for (int c = r; c < 9; c++) {
            double h = k1 * (p[r] * p[c]) + k2 * ((r3[r] * r0[c] + r0[r] * r3[c]) - 2.0 * (r1[r] * r1[c]));
            if (r % 3 == c % 3) h += S2[r / 3][c / 3];
            H[mem_tri(r, c)] = coeff * h;
        }
    return W;
}

// ---- the StVK and tension-field StVK materials (smg_membrane_set_material 1, 2; the reference's StVKMaterial.cpp:11-60 and
// TensionFieldStVKMaterial.cpp:11-171).  Both are functions psi(a00, a01, a11) of the first fundamental form, so with t = d psi / d a
// (symmetric 2 x 2) and the symmetric table of second derivatives over (r0, r1, r3)
//   G = comb(t),   H = c00 r0 r0^T + c11 r1 r1^T + c33 r3 r3^T + c01 (r0 r1^T + r1 r0^T) + c03 (r0 r3^T + r3 r0^T) + c13 (r1 r3^T + r3 r1^T) + S(t) (x) I_3
// with the S of the header.  A material supplies W, t (3) and the table (6); one tail builds G and the 45 entries.
// With B = abar^-1, M = B (a - abar), tr = tr M, c = thickness sqrt(det abar) / 8 (= coeff / 2):
//   StVK:  W = c (alpha / 2 tr^2 + beta tr(M^2)),  t = c (alpha tr B + 2 beta M B),  and the table is constant per face:
//          c00 = c k B00^2, c33 = c k B11^2, c01 = 2 c k B00 B01, c13 = 2 c k B01 B11, k = alpha + 2 beta,
//          c03 = c (alpha B00 B11 + 2 beta B01^2), c11 = 4 c (alpha B01^2 + beta (B01^2 + B00 B11)).
//   tension field:  l1, l2 = tr / 2 +- sqrt(max(0, tr^2 / 4 - det M)), k1 = thickness alpha / 8, k2 = thickness beta / 4, tc = -k1 / (k1 + k2).
//          l1 >= 0 and l2 >= tc l1: StVK (pure tension);  else l1 < 0: W = 0, t = 0, table 0 (slack);  else (wrinkled), with
//          K = (k1 + k2 - k1^2 / (k1 + k2)) sqrt(det abar) / 2, den = sqrt(tr^2 / 4 - det M), adj = the adjugate of (a - abar),
//          I = tr / 4 B - det B / 2 adj, m = B / 2 + (sign / den) I, s = sign l1 / den:
//          W = K l1^2,  t = 2 K l1 m,  table = 2 K (m m^T + s / 4 B B^T - s / den^2 I I^T + s det B / 2 (2 r1 r1^T - r0 r3^T - r3 r0^T) in the places
//          of the table), where x x^T of a symmetric 2 x 2 x stands for comb(x) comb(x)^T.
// The comparisons are the reference's, >= included: at the rest pose M is exactly zero (a - abar is, abar being passed in exactly and not
// recovered from B) and the face is in pure tension.  W is finite for inverted faces: there is no +inf rule.
// rest: (abar^-1)00, 01, 11, det abar, coeff, abar00, abar01, abar11 (mem_rest_consts).
SMG_MEM_HD void mem_rest_consts(const double (&q0)[9], double thickness, double (&rest)[8])
{
    double e1[3], e2[3];
#pragma unroll
    for (int d = 0; d < 3; d++) { e1[d] = q0[3 + d] - q0[d]; e2[d] = q0[6 + d] - q0[d]; }
    const double a00 = (e1[0] * e1[0] + e1[1] * e1[1]) + e1[2] * e1[2];
    const double a01 = (e1[0] * e2[0] + e1[1] * e2[1]) + e1[2] * e2[2];
    const double a11 = (e2[0] * e2[0] + e2[1] * e2[1]) + e2[2] * e2[2];
    const double det = a00 * a11 - a01 * a01;
    rest[0] = a11 / det; rest[1] = -a01 / det; rest[2] = a00 / det; rest[3] = det; rest[4] = thickness * sqrt(det) / 4.0;
    rest[5] = a00; rest[6] = a01; rest[7] = a11;
}

// MAT 1: StVK, 2: tension-field StVK.  Returns W; with DERIVS also G (9) and the upper triangle of the unfixed H (45).
template <int MAT, bool DERIVS>
SMG_MEM_HD double membrane_face_mat(const double (&q)[9], const double (&rest)[8], double thickness, double alpha, double beta, double (&G)[9],
                                    double (&H)[45])
{
    double e1[3], e2[3];
#pragma unroll
    for (int d = 0; d < 3; d++) { e1[d] = q[3 + d] - q[d]; e2[d] = q[6 + d] - q[d]; }
    const double a00 = (e1[0] * e1[0] + e1[1] * e1[1]) + e1[2] * e1[2];
    const double a01 = (e1[0] * e2[0] + e1[1] * e2[1]) + e1[2] * e2[2];
    const double a11 = (e2[0] * e2[0] + e2[1] * e2[1]) + e2[2] * e2[2];
    const double b00 = rest[0], b01 = rest[1], b11 = rest[2];
    const double d00 = a00 - rest[5], d01 = a01 - rest[6], d11 = a11 - rest[7];
    const double M00 = b00 * d00 + b01 * d01, M01 = b00 * d01 + b01 * d11, M10 = b01 * d00 + b11 * d01, M11 = b01 * d01 + b11 * d11;
    const double tr = M00 + M11;
    const double c = 0.5 * rest[4];
    double W = c * ((0.5 * alpha) * (tr * tr) + beta * ((M00 * M00 + 2.0 * (M01 * M10)) + M11 * M11));
    double t00 = 0.0, t01 = 0.0, t11 = 0.0, c00 = 0.0, c01 = 0.0, c03 = 0.0, c11 = 0.0, c13 = 0.0, c33 = 0.0;
    if (DERIVS) {
        const double at = alpha * tr, k = alpha + 2.0 * beta;
        t00 = c * (at * b00 + (2.0 * beta) * (M00 * b00 + M01 * b01));
        t01 = c * (at * b01 + (2.0 * beta) * (M00 * b01 + M01 * b11));
        t11 = c * (at * b11 + (2.0 * beta) * (M10 * b01 + M11 * b11));
        c00 = c * (k * (b00 * b00));
        c33 = c * (k * (b11 * b11));
        c01 = c * ((2.0 * k) * (b00 * b01));
        c13 = c * ((2.0 * k) * (b01 * b11));
        c03 = c * (alpha * (b00 * b11) + (2.0 * beta) * (b01 * b01));
        c11 = c * (4.0 * (alpha * (b01 * b01) + beta * (b01 * b01 + b00 * b11)));
    }
    if (MAT == 2) {
        const double D = M00 * M11 - M01 * M10;
        const double disc = tr * tr / 4.0 - D;
        const double root = sqrt(fmax(0.0, disc));
        double l1 = tr / 2.0 + root, l2 = tr / 2.0 - root, sign = 1.0;
        if (l2 > l1) { const double x = l1; l1 = l2; l2 = x; sign = -1.0; }
        const double k1 = 0.5 * (thickness / 4.0) * alpha, k2 = (thickness / 4.0) * beta;
        const double tc = -k1 / (k1 + k2);
        if (!(l1 >= 0.0 && l2 >= tc * l1)) {
            if (l1 < 0.0) {
                W = 0.0;
                t00 = t01 = t11 = c00 = c01 = c03 = c11 = c13 = c33 = 0.0;
            } else {
                // wrinkled: disc > 0 here (disc <= 0 gives l1 == l2, which with l1 >= 0 and tc < 1 is pure tension), so den is the root above
                const double K = ((k1 + k2) - k1 * k1 / (k1 + k2)) * (0.5 * sqrt(rest[3]));
                W = (K * l1) * l1;
                if (DERIVS) {
                    const double den = root, detB = b00 * b11 - b01 * b01;
                    const double i00 = (tr / 4.0) * b00 - (0.5 * detB) * d11, i01 = (tr / 4.0) * b01 + (0.5 * detB) * d01,
                                 i11 = (tr / 4.0) * b11 - (0.5 * detB) * d00;
                    const double sd = sign / den, s = sign * l1 / den, s4 = s / 4.0, s3 = s / (den * den), K2 = 2.0 * K, sB = s * detB;
                    const double m00 = 0.5 * b00 + sd * i00, m01 = 0.5 * b01 + sd * i01, m11 = 0.5 * b11 + sd * i11;
                    const double Kl = K2 * l1;
                    t00 = Kl * m00; t01 = Kl * m01; t11 = Kl * m11;
                    c00 = K2 * ((m00 * m00 + s4 * (b00 * b00)) - s3 * (i00 * i00));
                    c33 = K2 * ((m11 * m11 + s4 * (b11 * b11)) - s3 * (i11 * i11));
                    c03 = K2 * (((m00 * m11 + s4 * (b00 * b11)) - s3 * (i00 * i11)) - 0.5 * sB);
                    c01 = K2 * (2.0 * ((m00 * m01 + s4 * (b00 * b01)) - s3 * (i00 * i01)));
                    c13 = K2 * (2.0 * ((m01 * m11 + s4 * (b01 * b11)) - s3 * (i01 * i11)));
                    c11 = K2 * (4.0 * ((m01 * m01 + s4 * (b01 * b01)) - s3 * (i01 * i01)) + sB);
                }
            }
        }
    }
    if (!DERIVS) return W;

    mem_comb(e1, e2, t00, t01, t11, G);
    double r0[9], r1[9], r3[9];
#pragma unroll
    for (int d = 0; d < 3; d++) {
        r0[d] = -2.0 * e1[d]; r0[3 + d] = 2.0 * e1[d]; r0[6 + d] = 0.0;
        r1[d] = -(e1[d] + e2[d]); r1[3 + d] = e2[d]; r1[6 + d] = e1[d];
        r3[d] = -2.0 * e2[d]; r3[3 + d] = 0.0; r3[6 + d] = 2.0 * e2[d];
    }
    const double S2[3][3] = {{2.0 * ((t00 + 2.0 * t01) + t11), -2.0 * (t00 + t01), -2.0 * (t01 + t11)},
                             {-2.0 * (t00 + t01), 2.0 * t00, 2.0 * t01},
                             {-2.0 * (t01 + t11), 2.0 * t01, 2.0 * t11}};
#pragma unroll
    for (int cc = 0; cc < 9; cc++) {
        // column cc of the table applied to the rows: y_k = sum_l c_kl r_l[cc]
        const double y0 = (c00 * r0[cc] + c01 * r1[cc]) + c03 * r3[cc];
        const double y1 = (c01 * r0[cc] + c11 * r1[cc]) + c13 * r3[cc];
        const double y3 = (c03 * r0[cc] + c13 * r1[cc]) + c33 * r3[cc];
#pragma unroll
        for (int r = 0; r <= cc; r++) {
            double h = (r0[r] * y0 + r1[r] * y1) + r3[r] * y3;
            if (r % 3 == cc % 3) h += S2[r / 3][cc / 3];
            H[mem_tri(r, cc)] = h;
        }
    }
    return W;
}

// the rotation of the plane (P, Q), P < Q, that zeroes a_pq; A holds its upper triangle (A[i][j], i <= j), the columns of V the eigenvectors
template <int P, int Q>
SMG_MEM_HD bool mem_jacobi_pair(double (&A)[6][6], double (&V)[6][6], double thresh)
{
    const double apq = A[P][Q];
    if (fabs(apq) <= thresh) return false;
    const double theta = (A[Q][Q] - A[P][P]) / (2.0 * apq);
    const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(1.0 + theta * theta));
    const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
#pragma unroll
    for (int k = 0; k < 6; k++) {
        if (k != P && k != Q) {
            double& xp = k < P ? A[k][P] : A[P][k];
            double& xq = k < Q ? A[k][Q] : A[Q][k];
            const double akp = xp, akq = xq;
            xp = c * akp - s * akq;
            xq = s * akp + c * akq;
        }
        const double vkp = V[k][P], vkq = V[k][Q];
        V[k][P] = c * vkp - s * vkq;
        V[k][Q] = s * vkp + c * vkq;
    }
    A[P][P] -= t * apq;
    A[Q][Q] += t * apq;
    A[P][Q] = 0.0;
    return true;
}

template <int P>
SMG_MEM_HD bool mem_jacobi_row(double (&A)[6][6], double (&V)[6][6], double thresh)
{
    bool rotated = false;
    if constexpr (P < 1) rotated = mem_jacobi_pair<P, 1>(A, V, thresh) || rotated;
    if constexpr (P < 2) rotated = mem_jacobi_pair<P, 2>(A, V, thresh) || rotated;
    if constexpr (P < 3) rotated = mem_jacobi_pair<P, 3>(A, V, thresh) || rotated;
    if constexpr (P < 4) rotated = mem_jacobi_pair<P, 4>(A, V, thresh) || rotated;
    if constexpr (P < 5) rotated = mem_jacobi_pair<P, 5>(A, V, thresh) || rotated;
    return rotated;
}

// H (upper triangle, 45) <- the fixed H'
SMG_MEM_HD void membrane_fix(double (&H)[45], double floor, double value)
{
    double A[6][6], V[6][6];
    double norm2 = 0.0;
    // A = B^T H B, upper triangle
#pragma unroll
    for (int i = 0; i < 6; i++)
#pragma unroll
        for (int j = 0; j < 6; j++) {
            V[i][j] = i == j ? 1.0 : 0.0;
            if (j < i) { A[i][j] = 0.0; continue; }
            const int a = i / 3, l = i % 3, b = j / 3, m = j % 3;
            double acc = 0.0;
#pragma unroll
            for (int cj = 0; cj < 3; cj++)
#pragma unroll
                for (int ck = 0; ck < 3; ck++) {
                    const double w = mem_basis(a, cj) * mem_basis(b, ck);
                    if (w != 0.0) acc += w * H[mem_sym(3 * cj + l, 3 * ck + m)];
                }
            A[i][j] = acc;
            norm2 += (i == j ? 1.0 : 2.0) * (acc * acc);
        }
    const double thresh = MEM_EPS * sqrt(norm2);
    for (int sweep = 0; sweep < MEM_SWEEP_CAP; sweep++) {
        bool rotated = mem_jacobi_row<0>(A, V, thresh);
        rotated = mem_jacobi_row<1>(A, V, thresh) || rotated;
        rotated = mem_jacobi_row<2>(A, V, thresh) || rotated;
        rotated = mem_jacobi_row<3>(A, V, thresh) || rotated;
        rotated = mem_jacobi_row<4>(A, V, thresh) || rotated;
        if (!rotated) break;
    }
    double lam[6];
#pragma unroll
    for (int k = 0; k < 6; k++) lam[k] = A[k][k] < floor ? value : A[k][k];
    // A <- V fix(Lambda) V^T, upper triangle
#pragma unroll
    for (int i = 0; i < 6; i++)
#pragma unroll
        for (int j = i; j < 6; j++) {
            double acc = 0.0;
#pragma unroll
            for (int k = 0; k < 6; k++) acc += (V[i][k] * lam[k]) * V[j][k];
            A[i][j] = acc;
        }
    // H' = B A B^T + value / 3 on the diagonals of the nine 3 x 3 blocks
    const double third = value / 3.0;
#pragma unroll
    for (int r = 0; r < 9; r++)
#pragma unroll
        for (int c = r; c < 9; c++) {
            const int cj = r / 3, l = r % 3, ck = c / 3, m = c % 3;
            double acc = 0.0;
#pragma unroll
            for (int a = 0; a < 2; a++)
#pragma unroll
                for (int b = 0; b < 2; b++) {
                    const double w = mem_basis(a, cj) * mem_basis(b, ck);
                    const int i = 3 * a + l, j = 3 * b + m;
                    if (w != 0.0) acc += w * (i <= j ? A[i][j] : A[j][i]);
                }
            H[mem_tri(r, c)] = l == m ? acc + third : acc;
        }
}

// the membrane's lists (smg_membrane.cpp): the block CSR of (adjacency + I), columns ascending, the block row of every block, and per block
// the face sub-blocks 9 f + 3 a + b that k_membrane_matrix sums, faces ascending
struct MembraneLists { std::vector<int> bptr, bcol, brow, c_ptr, c_src; };
void membrane_lists(const int* F, int nF, int nV, MembraneLists& L);

}  // namespace smg
