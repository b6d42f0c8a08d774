// smg_morph_inl.hpp -- the per-face arithmetic of gradient-domain morphing, in registers (csrc/smg_morph_device.hip, smg_morph_faces_host;
// include/smg.h: smg_morph_*).  3 x 3 matrices are row-major (entry (a, b) at 3a + b); a symmetric one is stored as its
// six entries 00, 01, 02, 11, 12, 22.
//
//   basis     W_fi = (n x e_i) / (2A), n, 2A of a rest face: the expressions of k_geo_basis (smg_geodesics_device.hip), operation by operation
//   gradient  J = T + N n^T,  T = sum_i x_i W_fi^T (i = 0, 1, 2 in order),  N = the pose face's unit normal (0 where its area is 0)
//   polar     J = R S: R^T = arap_closest_rotation(J) (smg_arap_inl.hpp: the rotation that maximises tr(R^T J), its determinant rule on the
//             smallest singular value), S = (M + M^T) / 2 with M = R^T J
//   log       R as a unit quaternion by Shepperd's branch on the largest of the trace and the diagonal entries, w >= 0, theta = 2 atan2(|v|, w),
//             omega = (theta / |v|) v, or 0 when |v| == 0
//   interp    J(t) = R(t) S(t): R(t) = Rodrigues' formula for t omega = cos(th) I + (1 - cos(th)) a a^T + sin(th) [a]x, th = |t omega|,
//             a = t omega / th (I when th == 0);  S(t) = I + t (S - I)
//   share     A (J W_j): a corner's term of the right-hand side
// Host and device compile the same text (the library is built with -ffp-contract=off); sin, cos and atan2 are the only calls whose bits may differ
// between the two, and only morph_log and morph_interp make them.
#pragma once
#include <cmath>

#include "smg_arap_inl.hpp"

namespace smg {

// a, b, c: the three corners (3 doubles each).  W[3i + d], nrm[3], *dA = twice the area
SMG_ARAP_HD void morph_basis(const double* a, const double* b, const double* c, double* W, double* nrm, double* dA2)
{
    const double ux = b[0] - a[0], uy = b[1] - a[1], uz = b[2] - a[2];
    const double vx = c[0] - a[0], vy = c[1] - a[1], vz = c[2] - a[2];
    const double wx = uy * vz - uz * vy, wy = uz * vx - ux * vz, wz = ux * vy - uy * vx;
    const double dA = sqrt(wx * wx + wy * wy + wz * wz);
    const double nx = wx / dA, ny = wy / dA, nz = wz / dA;
    const double e[3][3] = {{c[0] - b[0], c[1] - b[1], c[2] - b[2]}, {a[0] - c[0], a[1] - c[1], a[2] - c[2]}, {b[0] - a[0], b[1] - a[1], b[2] - a[2]}};
#pragma unroll
    for (int i = 0; i < 3; i++) {
        W[3 * i + 0] = (ny * e[i][2] - nz * e[i][1]) / dA;
        W[3 * i + 1] = (nz * e[i][0] - nx * e[i][2]) / dA;
        W[3 * i + 2] = (nx * e[i][1] - ny * e[i][0]) / dA;
    }
    nrm[0] = nx; nrm[1] = ny; nrm[2] = nz;
    *dA2 = dA;
}

// x0, x1, x2: the pose's corners; W, nrm: the rest face's basis and normal
SMG_ARAP_HD void morph_gradient(const double* x0, const double* x1, const double* x2, const double* W, const double* nrm, double* J)
{
    const double ux = x1[0] - x0[0], uy = x1[1] - x0[1], uz = x1[2] - x0[2];
    const double vx = x2[0] - x0[0], vy = x2[1] - x0[1], vz = x2[2] - x0[2];
    const double wx = uy * vz - uz * vy, wy = uz * vx - ux * vz, wz = ux * vy - uy * vx;
    const double d = sqrt(wx * wx + wy * wy + wz * wz);
    double N[3] = {0.0, 0.0, 0.0};
    if (d > 0.0) { N[0] = wx / d; N[1] = wy / d; N[2] = wz / d; }
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
        for (int b = 0; b < 3; b++) {
            const double T = x0[a] * W[b] + x1[a] * W[3 + b] + x2[a] * W[6 + b];
            J[3 * a + b] = T + N[a] * nrm[b];
        }
}

SMG_ARAP_HD void morph_polar(const double* J, double* R, double* S6)
{
    double Rt[9];
    arap_closest_rotation(J, Rt);
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
        for (int b = 0; b < 3; b++) R[3 * a + b] = Rt[3 * b + a];
    double M[9];
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
        for (int b = 0; b < 3; b++) M[3 * a + b] = Rt[3 * a] * J[b] + Rt[3 * a + 1] * J[3 + b] + Rt[3 * a + 2] * J[6 + b];
    S6[0] = M[0];
    S6[1] = 0.5 * (M[1] + M[3]);
    S6[2] = 0.5 * (M[2] + M[6]);
    S6[3] = M[4];
    S6[4] = 0.5 * (M[5] + M[7]);
    S6[5] = M[8];
}

SMG_ARAP_HD void morph_log(const double* R, double* omega)
{
    const double tr = R[0] + R[4] + R[8];
    double w, x, y, z, t;
    if (tr >= R[0] && tr >= R[4] && tr >= R[8]) {
        t = 1.0 + tr;
        w = t; x = R[7] - R[5]; y = R[2] - R[6]; z = R[3] - R[1];
    } else if (R[0] >= R[4] && R[0] >= R[8]) {
        t = ((1.0 + R[0]) - R[4]) - R[8];
        w = R[7] - R[5]; x = t; y = R[1] + R[3]; z = R[2] + R[6];
    } else if (R[4] >= R[8]) {
        t = ((1.0 - R[0]) + R[4]) - R[8];
        w = R[2] - R[6]; x = R[1] + R[3]; y = t; z = R[5] + R[7];
    } else {
        t = ((1.0 - R[0]) - R[4]) + R[8];
        w = R[3] - R[1]; x = R[2] + R[6]; y = R[5] + R[7]; z = t;
    }
    const double h = 0.5 / sqrt(t);
    w *= h; x *= h; y *= h; z *= h;
    if (w < 0.0) { w = -w; x = -x; y = -y; z = -z; }
    const double vn = sqrt(x * x + y * y + z * z);
    if (!(vn > 0.0)) { omega[0] = 0.0; omega[1] = 0.0; omega[2] = 0.0; return; }
    const double g = (2.0 * atan2(vn, w)) / vn;
    omega[0] = g * x; omega[1] = g * y; omega[2] = g * z;
}

SMG_ARAP_HD void morph_interp(const double* omega, const double* S6, double t, double* J)
{
    const double ax = t * omega[0], ay = t * omega[1], az = t * omega[2];
    const double th = sqrt(ax * ax + ay * ay + az * az);
    double R[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
    if (th > 0.0) {
        const double kx = ax / th, ky = ay / th, kz = az / th;
        const double s = sin(th), c = cos(th), v = 1.0 - c;
        R[0] = c + v * (kx * kx); R[1] = v * (kx * ky) - s * kz; R[2] = v * (kx * kz) + s * ky;
        R[3] = v * (kx * ky) + s * kz; R[4] = c + v * (ky * ky); R[5] = v * (ky * kz) - s * kx;
        R[6] = v * (kx * kz) - s * ky; R[7] = v * (ky * kz) + s * kx; R[8] = c + v * (kz * kz);
    }
    const double s00 = 1.0 + t * (S6[0] - 1.0), s01 = t * S6[1], s02 = t * S6[2];
    const double s11 = 1.0 + t * (S6[3] - 1.0), s12 = t * S6[4], s22 = 1.0 + t * (S6[5] - 1.0);
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const double r0 = R[3 * a], r1 = R[3 * a + 1], r2 = R[3 * a + 2];
        J[3 * a + 0] = r0 * s00 + r1 * s01 + r2 * s02;
        J[3 * a + 1] = r0 * s01 + r1 * s11 + r2 * s12;
        J[3 * a + 2] = r0 * s02 + r1 * s12 + r2 * s22;
    }
}

// acc_a += A (J_a0 w_0 + J_a1 w_1 + J_a2 w_2): corner j's share, w = W + 3 j
SMG_ARAP_HD void morph_share(const double* J, const double* w, double A, double* acc)
{
#pragma unroll
    for (int a = 0; a < 3; a++) acc[a] += A * (J[3 * a] * w[0] + J[3 * a + 1] * w[1] + J[3 * a + 2] * w[2]);
}

// ---- the host twin (smg_morph_faces_host): the loops of the kernels over caller arrays, with the layouts of smg_debug_morph (include/smg.h).
// V0, X: xyz rows; mp / mi: the corner lists t = 3 f + i of every vertex, faces ascending ---------------------------------------------------
inline void morph_host_face_basis(const int* F, const double* V0, int f, double* W, double* nrm, double* dA)
{
    morph_basis(V0 + 3 * (size_t)F[3 * (size_t)f], V0 + 3 * (size_t)F[3 * (size_t)f + 1], V0 + 3 * (size_t)F[3 * (size_t)f + 2], W, nrm, dA);
}

// J (k sets of nF x 9) of the k poses X (k sets of nV x 3)
inline void morph_host_gradient(int nV, int nF, int k, const int* F, const double* V0, const double* X, double* J)
{
    for (int c = 0; c < k; c++)
        for (int f = 0; f < nF; f++) {
            double W[9], nrm[3], dA;
            morph_host_face_basis(F, V0, f, W, nrm, &dA);
            const double* x = X + (size_t)c * nV * 3;
            morph_gradient(x + 3 * (size_t)F[3 * (size_t)f], x + 3 * (size_t)F[3 * (size_t)f + 1], x + 3 * (size_t)F[3 * (size_t)f + 2], W, nrm,
                           J + ((size_t)c * nF + f) * 9);
        }
}

inline void morph_host_polar(int nF, const int* F, const double* V0, const double* X, double* R, double* omega, double* S)
{
    for (int f = 0; f < nF; f++) {
        double W[9], nrm[3], dA, J[9];
        morph_host_face_basis(F, V0, f, W, nrm, &dA);
        morph_gradient(X + 3 * (size_t)F[3 * (size_t)f], X + 3 * (size_t)F[3 * (size_t)f + 1], X + 3 * (size_t)F[3 * (size_t)f + 2], W, nrm, J);
        morph_polar(J, R + 9 * (size_t)f, S + 6 * (size_t)f);
        morph_log(R + 9 * (size_t)f, omega + 3 * (size_t)f);
    }
}

// B (nV x 3k column-major, leading dimension nV) and bsq (k nV) from J (t == nullptr) or from omega, S and t
inline void morph_host_rhs(int nV, int nF, int k, const int* F, const double* V0, const int* mp, const int* mi, const double* J, const double* omega,
                           const double* S, const double* t, double* B, double* bsq)
{
    for (int c = 0; c < k; c++)
        for (int v = 0; v < nV; v++) {
            double acc[3] = {0.0, 0.0, 0.0};
            for (int p = mp[v]; p < mp[v + 1]; p++) {
                const int f = mi[p] / 3, j = mi[p] - 3 * f;
                double W[9], nrm[3], dA, Jf[9];
                morph_host_face_basis(F, V0, f, W, nrm, &dA);
                if (t) morph_interp(omega + 3 * (size_t)f, S + 6 * (size_t)f, t[c], Jf);
                else for (int e = 0; e < 9; e++) Jf[e] = J[((size_t)c * nF + f) * 9 + e];
                morph_share(Jf, W + 3 * j, dA * 0.5, acc);
            }
            for (int d = 0; d < 3; d++) B[(size_t)(3 * c + d) * nV + v] = acc[d];
            bsq[(size_t)c * nV + v] = acc[0] * acc[0] + acc[1] * acc[1] + acc[2] * acc[2];
        }
}

// hp (nh x 3k column-major) = the pins' default positions, U (nV x 3k column-major) = the default start with the pinned rows from hp
inline void morph_host_pins(int nV, int k, const double* V0, const double* X, const double* t, const int* pins, int nh, double* hp, double* U)
{
    for (int c = 0; c < k; c++)
        for (int d = 0; d < 3; d++) {
            double* u = U + (size_t)(3 * c + d) * nV;
            for (int i = 0; i < nV; i++) u[i] = X ? (1.0 - t[c]) * V0[3 * (size_t)i + d] + t[c] * X[3 * (size_t)i + d] : V0[3 * (size_t)i + d];
            for (int r = 0; r < nh; r++) {
                const size_t i = (size_t)pins[r];
                const double p = X ? (1.0 - t[c]) * V0[3 * i + d] + t[c] * X[3 * i + d] : V0[3 * i + d];
                hp[(size_t)(3 * c + d) * nh + r] = p;
                u[i] = p;
            }
        }
}

}  // namespace smg
