// smg_arap_inl.hpp -- the closest rotation of a 3 x 3 covariance, in registers (k_arap_rotations, csrc/smg_arap_device.hip).
//
// S = U Sigma V^T;  R = argmax over rotations of tr(R S) = V D U^T, D = diag(1, 1, det(V U^T)) on the smallest singular value.
// Method: one-sided (Hestenes) Jacobi on the ROWS of S.  The rows b_0, b_1, b_2 of S are rotated in pairs until they are mutually orthogonal:
// W^T S = diag(sigma) Q^T with W the product of the plane rotations (det W = +1), so S = W Sigma Q^T, U = W, V = Q, and the rows end as
// b_k = sigma_k q_k.  The rows are then ordered by norm with quarter turns (det stays +1), q_0 = b_0 / sigma_0, q_1 = b_1 / sigma_1, and the
// third direction is ALWAYS q_2 = q_0 x q_1, never b_2 / sigma_2: [q_0 q_1 q_2] is then right-handed, equal to V with its last column
// multiplied by det(V U^T), and R = [q_0 q_1 q_2] W^T is V D U^T.  The reflection case needs no branch, and a rank-2 covariance needs no
// division by a small number.  No product S^T S is formed: the condition number is not squared.
// A row of S that is zero (a flat rest pose: every rest edge has a zero component) is never rotated -- its dot products are exact zeros -- so
// sigma_2 == 0 exactly there.  sigma_0 == 0 (S == 0) gives the identity exactly; sigma_1 == 0 (rank 1) completes q_1 with a unit vector
// perpendicular to q_0.
// Every lane runs whole sweeps over the pairs (0,1), (0,2), (1,2) until a sweep rotates nothing, at most ARAP_SWEEP_CAP of them.
// Host and device compile the same text (the library is built with -ffp-contract=off).
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define SMG_ARAP_HD __host__ __device__ __forceinline__
#else
#define SMG_ARAP_HD inline
#endif

namespace smg {

constexpr int ARAP_SWEEP_CAP = 12;
constexpr double ARAP_EPS = 2.220446049250313e-16;   // a pair counts as orthogonal when |b_p . b_q| <= eps |b_p| |b_q|

SMG_ARAP_HD double arap_dot3(const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

// rows P, Q of b and w: [x_p x_q] <- [x_p x_q] [[c, s], [-s, c]] with the angle that makes b_p . b_q = 0; false: already orthogonal
template <int P, int Q>
SMG_ARAP_HD bool arap_jacobi_pair(double (&b)[3][3], double (&w)[3][3])
{
    const double alpha = arap_dot3(b[P], b[P]), beta = arap_dot3(b[Q], b[Q]), gamma = arap_dot3(b[P], b[Q]);
    if (gamma * gamma <= (ARAP_EPS * ARAP_EPS) * (alpha * beta)) return false;
    const double zeta = (beta - alpha) / (2.0 * gamma);
    const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
    const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
#pragma unroll
    for (int d = 0; d < 3; d++) {
        const double bp = b[P][d], bq = b[Q][d], wp = w[P][d], wq = w[Q][d];
        b[P][d] = c * bp - s * bq;
        b[Q][d] = s * bp + c * bq;
        w[P][d] = c * wp - s * wq;
        w[Q][d] = s * wp + c * wq;
    }
    return true;
}

// a quarter turn in the plane (P, Q) where row Q is the longer one: (x_p, x_q) <- (x_q, -x_p)
template <int P, int Q>
SMG_ARAP_HD void arap_order_pair(double (&b)[3][3], double (&w)[3][3], double (&nn)[3])
{
    if (nn[Q] > nn[P]) {
        const double t = nn[P]; nn[P] = nn[Q]; nn[Q] = t;
#pragma unroll
        for (int d = 0; d < 3; d++) {
            const double bp = b[P][d], wp = w[P][d];
            b[P][d] = b[Q][d]; b[Q][d] = -bp;
            w[P][d] = w[Q][d]; w[Q][d] = -wp;
        }
    }
}

// S, R: row-major 3 x 3 (entry (a, c) at 3a + c)
SMG_ARAP_HD void arap_closest_rotation(const double* S, double* R)
{
    double b[3][3], w[3][3];
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
        for (int c = 0; c < 3; c++) { b[a][c] = S[3 * a + c]; w[a][c] = a == c ? 1.0 : 0.0; }
    for (int sweep = 0; sweep < ARAP_SWEEP_CAP; sweep++) {
        bool rotated = arap_jacobi_pair<0, 1>(b, w);
        rotated = arap_jacobi_pair<0, 2>(b, w) || rotated;
        rotated = arap_jacobi_pair<1, 2>(b, w) || rotated;
        if (!rotated) break;
    }
    double nn[3] = {arap_dot3(b[0], b[0]), arap_dot3(b[1], b[1]), arap_dot3(b[2], b[2])};
    arap_order_pair<0, 1>(b, w, nn);
    arap_order_pair<0, 2>(b, w, nn);
    arap_order_pair<1, 2>(b, w, nn);
    const double s0 = sqrt(nn[0]), s1 = sqrt(nn[1]);
    if (!(s0 > 0.0)) {      // S == 0 (or not finite: the energy of the same pass is then not finite either, and the solve reports it)
#pragma unroll
        for (int e = 0; e < 9; e++) R[e] = (e == 0 || e == 4 || e == 8) ? 1.0 : 0.0;
        return;
    }
    double q0[3] = {b[0][0] / s0, b[0][1] / s0, b[0][2] / s0}, q1[3];
    if (s1 > 0.0) {
        q1[0] = b[1][0] / s1; q1[1] = b[1][1] / s1; q1[2] = b[1][2] / s1;
    } else {                // rank 1: q_1 = (q_0 x e) / |q_0 x e|, e the axis on which q_0 is shortest
        const double ax = fabs(q0[0]), ay = fabs(q0[1]), az = fabs(q0[2]);
        const double ex = (ax <= ay && ax <= az) ? 1.0 : 0.0, ey = (ex == 0.0 && ay <= az) ? 1.0 : 0.0, ez = (ex == 0.0 && ey == 0.0) ? 1.0 : 0.0;
        const double cx = q0[1] * ez - q0[2] * ey, cy = q0[2] * ex - q0[0] * ez, cz = q0[0] * ey - q0[1] * ex;
        const double cn = sqrt(cx * cx + cy * cy + cz * cz);
        q1[0] = cx / cn; q1[1] = cy / cn; q1[2] = cz / cn;
    }
    const double q2[3] = {q0[1] * q1[2] - q0[2] * q1[1], q0[2] * q1[0] - q0[0] * q1[2], q0[0] * q1[1] - q0[1] * q1[0]};
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
        for (int c = 0; c < 3; c++) R[3 * a + c] = q0[a] * w[0][c] + q1[a] * w[1][c] + q2[a] * w[2][c];
}

}  // namespace smg
