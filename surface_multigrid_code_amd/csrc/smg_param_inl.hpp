// smg_param_inl.hpp -- the per-face maths of the disk parameterization (smg_param_*, include/smg.h; kernels in csrc/smg_param_device.hip, host
// side in smg_param.cpp).  A face with corners p0, p1, p2 has the isometric rest triangle x0 = (0, 0), x1 = (a, 0),
// x2 = (b, c) in the plane; its six rest constants are r = {a, b, c, c0, c1, c2}, c_i the cotangent of the angle opposite edge (i, i + 1).
// d_i = x_i - x_{i+1} are the rest edges, g_i = u_i - u_{i+1} the edges of the map u (three corners, two coordinates each).
// Every sum is one accumulator in the order i = 0, 1, 2 and every expression is written operation by operation; host and device compile the
// same text (the library is built with -ffp-contract=off), and tests/test_param_host.py restates it in numpy in the same order.
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define SMG_PARAM_HD __host__ __device__ __forceinline__
#else
#define SMG_PARAM_HD inline
#endif

namespace smg {

// r = {a, b, c, c0, c1, c2} from the corners (xyz each): a = |e1|, b = e1 . e2 / a, c = |e1 x e2| / a, e1 = p1 - p0, e2 = p2 - p0
SMG_PARAM_HD void param_rest(const double* p0, const double* p1, const double* p2, double (&r)[6])
{
    const double e1x = p1[0] - p0[0], e1y = p1[1] - p0[1], e1z = p1[2] - p0[2];
    const double e2x = p2[0] - p0[0], e2y = p2[1] - p0[1], e2z = p2[2] - p0[2];
    const double a = sqrt(e1x * e1x + e1y * e1y + e1z * e1z);
    const double dot = e1x * e2x + e1y * e2y + e1z * e2z;
    const double wx = e1y * e2z - e1z * e2y, wy = e1z * e2x - e1x * e2z, wz = e1x * e2y - e1y * e2x;
    const double b = dot / a, c = sqrt(wx * wx + wy * wy + wz * wz) / a;
    const double dA = a * c;                      // twice the area of the rest triangle
    r[0] = a; r[1] = b; r[2] = c;
    r[3] = (b * (b - a) + c * c) / dA;            // the angle at x2: (x0 - x2) . (x1 - x2) / dA
    r[4] = (a * b) / dA;                          // the angle at x0: x1 . x2 / dA
    r[5] = (a * (a - b)) / dA;                    // the angle at x1: (x0 - x1) . (x2 - x1) / dA
}

// the rest edges d_i = x_i - x_{i+1}
SMG_PARAM_HD void param_edges(const double (&r)[6], double (&dx)[3], double (&dy)[3])
{
    dx[0] = 0.0 - r[0]; dy[0] = 0.0;
    dx[1] = r[0] - r[1]; dy[1] = 0.0 - r[2];
    dx[2] = r[1]; dy[2] = r[2];
}

// the map's edges g_i = u_i - u_{i+1}; u[i] = {u, v} of corner i
SMG_PARAM_HD void param_map_edges(const double (&u)[3][2], double (&gx)[3], double (&gy)[3])
{
    gx[0] = u[0][0] - u[1][0]; gy[0] = u[0][1] - u[1][1];
    gx[1] = u[1][0] - u[2][0]; gy[1] = u[1][1] - u[2][1];
    gx[2] = u[2][0] - u[0][0]; gy[2] = u[2][1] - u[0][1];
}

// S = sum_i c_i g_i d_i^T as {S00, S01, S10, S11}: entry (p, q) += (c_i g_i,p) d_i,q
SMG_PARAM_HD void param_covariance(const double (&r)[6], const double (&u)[3][2], double (&S)[4])
{
    double dx[3], dy[3], gx[3], gy[3];
    param_edges(r, dx, dy);
    param_map_edges(u, gx, gy);
    S[0] = S[1] = S[2] = S[3] = 0.0;
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const double wx = r[3 + i] * gx[i], wy = r[3 + i] * gy[i];
        S[0] += wx * dx[i]; S[1] += wx * dy[i];
        S[2] += wy * dx[i]; S[3] += wy * dy[i];
    }
}

// R = [[cs, -sn], [sn, cs]], the rotation closest to S: (cs, sn) = (a, b) / h, a = S00 + S11, b = S10 - S01, h = sqrt(a^2 + b^2); the identity
// when h == 0 (or not finite: the energy of the same pass is then not finite either, and the solve reports it)
SMG_PARAM_HD void param_rotation(const double (&S)[4], double& cs, double& sn)
{
    const double a = S[0] + S[3], b = S[2] - S[1];
    const double h = sqrt(a * a + b * b);
    if (h > 0.0) { cs = a / h; sn = b / h; }
    else { cs = 1.0; sn = 0.0; }
}

// the face's term of E: (1/2) sum_i c_i |g_i - R d_i|^2
SMG_PARAM_HD double param_face_energy(const double (&r)[6], const double (&u)[3][2], double cs, double sn)
{
    double dx[3], dy[3], gx[3], gy[3];
    param_edges(r, dx, dy);
    param_map_edges(u, gx, gy);
    double acc = 0.0;
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const double ex = gx[i] - (cs * dx[i] - sn * dy[i]);
        const double ey = gy[i] - (sn * dx[i] + cs * dy[i]);
        acc += r[3 + i] * (ex * ex + ey * ey);
    }
    return 0.5 * acc;
}

// corner i's share of the right-hand side: (1/2) R (c_i (x_i - x_{i+1}) + c_{i-1} (x_i - x_{i-1})), x_i - x_{i-1} = -d_{i-1}
SMG_PARAM_HD void param_corner_rhs(const double (&r)[6], int i, double cs, double sn, double& bx, double& by)
{
    double dx[3], dy[3];
    param_edges(r, dx, dy);
    const int m = i == 0 ? 2 : i - 1;
    const double ci = i == 0 ? r[3] : i == 1 ? r[4] : r[5], cm = m == 0 ? r[3] : m == 1 ? r[4] : r[5];
    const double dix = i == 0 ? dx[0] : i == 1 ? dx[1] : dx[2], diy = i == 0 ? dy[0] : i == 1 ? dy[1] : dy[2];
    const double dmx = m == 0 ? dx[0] : m == 1 ? dx[1] : dx[2], dmy = m == 0 ? dy[0] : m == 1 ? dy[1] : dy[2];
    const double mx = ci * dix - cm * dmx, my = ci * diy - cm * dmy;
    bx = 0.5 * (cs * mx - sn * my);
    by = 0.5 * (sn * mx + cs * my);
}

// the bound of |corner i's share| over all rotations: (1/2) (|c_i| |d_i| + |c_{i-1}| |d_{i-1}|)
SMG_PARAM_HD double param_corner_bound(const double (&r)[6], int i)
{
    double dx[3], dy[3];
    param_edges(r, dx, dy);
    const int m = i == 0 ? 2 : i - 1;
    return 0.5 * (fabs(r[3 + i]) * sqrt(dx[i] * dx[i] + dy[i] * dy[i]) + fabs(r[3 + m]) * sqrt(dx[m] * dx[m] + dy[m] * dy[m]));
}

// J = [u1 - u0, u2 - u0] [x1, x2]^-1 (column 0 = q1 / a, column 1 = (q2 - column 0 * b) / c), det J and the singular values in closed form
SMG_PARAM_HD void param_distortion(const double (&r)[6], const double (&u)[3][2], double& det, double& s1, double& s2)
{
    const double q1x = u[1][0] - u[0][0], q1y = u[1][1] - u[0][1];
    const double q2x = u[2][0] - u[0][0], q2y = u[2][1] - u[0][1];
    const double j00 = q1x / r[0], j10 = q1y / r[0];
    const double j01 = (q2x - j00 * r[1]) / r[2], j11 = (q2y - j10 * r[1]) / r[2];
    det = j00 * j11 - j01 * j10;
    const double pa = j00 + j11, pb = j10 - j01, ma = j00 - j11, mb = j10 + j01;
    const double Q = 0.5 * sqrt(pa * pa + pb * pb), T = 0.5 * sqrt(ma * ma + mb * mb);
    s1 = Q + T;
    s2 = fabs(Q - T);
}

}  // namespace smg
