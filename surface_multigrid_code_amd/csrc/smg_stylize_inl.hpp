// smg_stylize_inl.hpp -- the per-vertex maths of cubic and normal-driven stylization (k_stylize_local, csrc/smg_stylize_device.hip; the host twin
// smg_stylize_local_host).  Host and device compile the same text (the library is built with -ffp-contract=off), written
// operation by operation: tests/stylize_np.py restates it in numpy in the same order.
//
// Rest data of vertex i: n_i the unit area-weighted normal, a_i the barycentric area, both sums over the vertex's corner list (faces ascending);
// S_i = sum_j w_ij e_ij e'_ij^T over the off-diagonal entries of row i of L in stored order, as in smg_arap.  Q: the frame, row-major 3 x 3.
// Cubic mode, one ADMM iteration from the state (z, u, rho), la = lambda_i a_i:
//     M = S + rho n (Q^T (z - u))^T;  R = arap_closest_rotation(M);  y = Q R n;  z_old = z;  z = shrink(y + u, la / rho);  u += y - z;
//     r = |z - y|;  s = rho |z - z_old|;  r > mu s: rho *= tau, u /= tau;  else s > mu r: rho /= tau, u *= tau;
//     stop when r < sqrt(3) abs_tol + rel_tol max(|y|, |z|) and s < sqrt(3) abs_tol + rel_tol rho |u| (the updated rho, u).
// Normal-driven mode: R = arap_closest_rotation(S + (2 la) n t^T), one fit.
// Energy term of the vertex: (1/2) sum_j w_ij |e'_ij - R e_ij|^2 + la |Q R n|_1 (cubic) or + la |R n - t|^2 (normal-driven).
// The state of a vertex is 7 doubles -- z (3), u (3), rho -- kept as 7 planes of n (plane k of vertex i at k * n + i).
#pragma once
#include <cmath>
#include <vector>

#include "smg_arap_inl.hpp"

namespace smg {

struct StyParams { double lambda, rho0, abs_tol, rel_tol, mu, tau; int admm_iters; };   // smg_stylize_params, field by field
struct StyFrame { double q[9]; };                                                       // Q, row-major

constexpr int STY_STATE = 7;
enum { STY_CUBIC = 0, STY_TARGETS = 1, STY_ENERGY = 2 };    // the modes of k_stylize_local

SMG_ARAP_HD double sty_norm3(const double* a) { return sqrt(arap_dot3(a, a)); }
SMG_ARAP_HD double sty_shrink(double x, double k) { return x > k ? x - k : (x < -k ? x + k : 0.0); }

// n_i = the normalised sum of (p1 - p0) x (p2 - p0) over the corner list of vertex i (t = 3 f + corner, faces ascending), a_i = the sum of
// the double areas over 6, in the same order; a zero sum leaves n_i = 0
SMG_ARAP_HD void sty_vertex_normal_area(int i, const int* F, const int* mp, const int* mi, const double* V, double* nrm, double* area)
{
    double sum[3] = {0.0, 0.0, 0.0}, dbl = 0.0;
    const int q1 = mp[i + 1];
    for (int q = mp[i]; q < q1; q++) {
        const int f = mi[q] / 3;
        const double* p0 = V + 3 * (size_t)F[3 * (size_t)f];
        const double* p1 = V + 3 * (size_t)F[3 * (size_t)f + 1];
        const double* p2 = V + 3 * (size_t)F[3 * (size_t)f + 2];
        const double a[3] = {p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2]}, b[3] = {p2[0] - p0[0], p2[1] - p0[1], p2[2] - p0[2]};
        const double c[3] = {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]};
        sum[0] += c[0]; sum[1] += c[1]; sum[2] += c[2];
        dbl += sty_norm3(c);
    }
    const double len = sty_norm3(sum);
#pragma unroll
    for (int d = 0; d < 3; d++) nrm[3 * (size_t)i + d] = len > 0.0 ? sum[d] / len : 0.0;
    area[i] = dbl / 6.0;
}

// S_i = sum_j w_ij e_ij e'_ij^T (entry (a, c) = sum_j (w_ij e_a) e'_c), row i walked once in stored order: k_arap_rotations' covariance
SMG_ARAP_HD void sty_covariance(int i, const int* rowptr, const int* col, const double* w, const double* P0, const double* P, double* S)
{
#pragma unroll
    for (int e = 0; e < 9; e++) S[e] = 0.0;
    const double p0x = P0[3 * (size_t)i], p0y = P0[3 * (size_t)i + 1], p0z = P0[3 * (size_t)i + 2];
    const double px = P[3 * (size_t)i], py = P[3 * (size_t)i + 1], pz = P[3 * (size_t)i + 2];
    const int q1 = rowptr[i + 1];
    for (int q = rowptr[i]; q < q1; q++) {
        const int j = col[q];
        if (j == i) continue;
        const double wij = w[q];
        const double* r0 = P0 + 3 * (size_t)j;
        const double* r1 = P + 3 * (size_t)j;
        const double e[3] = {p0x - r0[0], p0y - r0[1], p0z - r0[2]};
        const double d[3] = {px - r1[0], py - r1[1], pz - r1[2]};
#pragma unroll
        for (int a = 0; a < 3; a++) {
            const double we = wij * e[a];
#pragma unroll
            for (int c = 0; c < 3; c++) S[3 * a + c] += we * d[c];
        }
    }
}

// sum_j w_ij |e'_ij - R e_ij|^2, row i walked once in stored order: k_arap_rotations' energy term
SMG_ARAP_HD double sty_arap_energy(int i, const int* rowptr, const int* col, const double* w, const double* P0, const double* P, const double* R)
{
    const double p0x = P0[3 * (size_t)i], p0y = P0[3 * (size_t)i + 1], p0z = P0[3 * (size_t)i + 2];
    const double px = P[3 * (size_t)i], py = P[3 * (size_t)i + 1], pz = P[3 * (size_t)i + 2];
    double acc = 0.0;
    const int q1 = rowptr[i + 1];
    for (int q = rowptr[i]; q < q1; q++) {
        const int j = col[q];
        if (j == i) continue;
        const double* r0 = P0 + 3 * (size_t)j;
        const double* r1 = P + 3 * (size_t)j;
        const double ex = p0x - r0[0], ey = p0y - r0[1], ez = p0z - r0[2];
        const double dx = (px - r1[0]) - (R[0] * ex + R[1] * ey + R[2] * ez);
        const double dy = (py - r1[1]) - (R[3] * ex + R[4] * ey + R[5] * ez);
        const double dz = (pz - r1[2]) - (R[6] * ex + R[7] * ey + R[8] * ez);
        acc += w[q] * (dx * dx + dy * dy + dz * dz);
    }
    return acc;
}

// y = Q (R n)
SMG_ARAP_HD void sty_rotated_normal(const double* Q, const double* R, const double* n, double* y)
{
    const double rn[3] = {arap_dot3(R, n), arap_dot3(R + 3, n), arap_dot3(R + 6, n)};
#pragma unroll
    for (int a = 0; a < 3; a++) y[a] = arap_dot3(Q + 3 * a, rn);
}

// one ADMM iteration; true: the stopping test holds
SMG_ARAP_HD bool sty_admm_one(const double* S, const double* n, const double* Q, double la, const StyParams& p, double* z, double* u, double& rho,
                              double* R, double* y)
{
    const double d[3] = {z[0] - u[0], z[1] - u[1], z[2] - u[2]};
    double M[9];
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const double v = Q[c] * d[0] + Q[3 + c] * d[1] + Q[6 + c] * d[2];     // (Q^T (z - u))_c
#pragma unroll
        for (int a = 0; a < 3; a++) M[3 * a + c] = S[3 * a + c] + (rho * n[a]) * v;
    }
    arap_closest_rotation(M, R);
    sty_rotated_normal(Q, R, n, y);
    const double k = la / rho;
    double dz[3], res[3];
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const double z_old = z[a];
        z[a] = sty_shrink(y[a] + u[a], k);
        u[a] = u[a] + (y[a] - z[a]);
        res[a] = z[a] - y[a];
        dz[a] = z[a] - z_old;
    }
    const double r = sty_norm3(res), s = rho * sty_norm3(dz);
    if (r > p.mu * s) {
        rho = rho * p.tau;
#pragma unroll
        for (int a = 0; a < 3; a++) u[a] = u[a] / p.tau;
    } else if (s > p.mu * r) {
        rho = rho / p.tau;
#pragma unroll
        for (int a = 0; a < 3; a++) u[a] = u[a] * p.tau;
    }
    const double floor_ = sqrt(3.0) * p.abs_tol, ny = sty_norm3(y), nz = sty_norm3(z);
    return r < floor_ + p.rel_tol * (ny > nz ? ny : nz) && s < floor_ + p.rel_tol * (rho * sty_norm3(u));
}

// The local step of vertex i.  MODE STY_CUBIC: at most p.admm_iters iterations from the state (fresh: z = u = 0, rho = p.rho0, nothing read),
// the state written back, iters[i] = the iterations used.  STY_TARGETS: one fit against tgt, iters[i] = 0.  STY_ENERGY: R is read, not written.
// Every mode ends with eterm[i]; in STY_ENERGY tgt != nullptr selects the normal-driven term.  lam == nullptr: the uniform p.lambda.
template <int MODE>
SMG_ARAP_HD void sty_local_vertex(int i, int n, const int* rowptr, const int* col, const double* w, const double* P0, const double* P, const double* nrm,
                                  const double* area, const double* lam, const StyFrame& Q, const double* tgt, const StyParams& p, int fresh,
                                  double* state, double* R_io, double* eterm, int* iters)
{
    const double nv[3] = {nrm[3 * (size_t)i], nrm[3 * (size_t)i + 1], nrm[3 * (size_t)i + 2]};
    const double la = (lam ? lam[i] : p.lambda) * area[i];
    double R[9], y[3];
    if (MODE == STY_ENERGY) {
#pragma unroll
        for (int e = 0; e < 9; e++) R[e] = R_io[9 * (size_t)i + e];
        sty_rotated_normal(Q.q, R, nv, y);
    } else {
        double S[9];
        sty_covariance(i, rowptr, col, w, P0, P, S);
        if (MODE == STY_CUBIC) {
            double z[3] = {0.0, 0.0, 0.0}, u[3] = {0.0, 0.0, 0.0}, rho = p.rho0;
            if (!fresh) {
#pragma unroll
                for (int a = 0; a < 3; a++) { z[a] = state[(size_t)a * n + i]; u[a] = state[(size_t)(3 + a) * n + i]; }
                rho = state[(size_t)6 * n + i];
            }
            int used = 0;
            while (used < p.admm_iters) {
                used++;
                if (sty_admm_one(S, nv, Q.q, la, p, z, u, rho, R, y)) break;
            }
#pragma unroll
            for (int a = 0; a < 3; a++) { state[(size_t)a * n + i] = z[a]; state[(size_t)(3 + a) * n + i] = u[a]; }
            state[(size_t)6 * n + i] = rho;
            iters[i] = used;
        } else {
            const double two_la = 2.0 * la;
#pragma unroll
            for (int a = 0; a < 3; a++) {
                const double c = two_la * nv[a];
#pragma unroll
                for (int b = 0; b < 3; b++) S[3 * a + b] = S[3 * a + b] + c * tgt[3 * (size_t)i + b];
            }
            arap_closest_rotation(S, R);
            iters[i] = 0;
        }
#pragma unroll
        for (int e = 0; e < 9; e++) R_io[9 * (size_t)i + e] = R[e];
    }
    double penalty;
    if (MODE == STY_TARGETS || (MODE == STY_ENERGY && tgt)) {        // the target lives in the mesh's own axes: R n, not Q R n
        const double rn[3] = {arap_dot3(R, nv), arap_dot3(R + 3, nv), arap_dot3(R + 6, nv)};
        const double d[3] = {rn[0] - tgt[3 * (size_t)i], rn[1] - tgt[3 * (size_t)i + 1], rn[2] - tgt[3 * (size_t)i + 2]};
        penalty = la * arap_dot3(d, d);
    } else {
        penalty = la * ((fabs(y[0]) + fabs(y[1])) + fabs(y[2]));
    }
    eterm[i] = 0.5 * sty_arap_energy(i, rowptr, col, w, P0, P, R) + penalty;
}

// The host twin of the hook's ops (smg_stylize_local_host after its checks; include/smg.h lays out `out`): 0 normals and areas, 1 one ADMM
// iteration, 2 the cubic local step, 3 the normal-driven local step, 4 the energy terms of given rotations.  mp, mi: the corner lists.
inline void sty_local_host(int op, int n, const int* F, const int* mp, const int* mi, const int* rowptr, const int* col, const double* w, const double* V0,
                           const double* P, const double* lam, const StyFrame& Q, const double* tgt, const double* state_in, const double* R_in,
                           StyParams p, double* out, int* iters)
{
    const size_t nn = (size_t)n;
    if (op == 0) {
        for (int i = 0; i < n; i++) sty_vertex_normal_area(i, F, mp, mi, V0, out, out + 3 * nn);
        return;
    }
    std::vector<double> nrm(3 * nn), area(nn);
    for (int i = 0; i < n; i++) sty_vertex_normal_area(i, F, mp, mi, V0, nrm.data(), area.data());
    if (op == 1) p.admm_iters = 1;
    if (op == 1 || op == 2) {
        double* state = out + 10 * nn;
        if (state_in) for (size_t e = 0; e < STY_STATE * nn; e++) state[e] = state_in[e];
        for (int i = 0; i < n; i++)
            sty_local_vertex<STY_CUBIC>(i, n, rowptr, col, w, V0, P, nrm.data(), area.data(), lam, Q, nullptr, p, state_in ? 0 : 1, state, out, out + 9 * nn, iters);
    } else if (op == 3) {
        for (int i = 0; i < n; i++)
            sty_local_vertex<STY_TARGETS>(i, n, rowptr, col, w, V0, P, nrm.data(), area.data(), lam, Q, tgt, p, 0, nullptr, out, out + 9 * nn, iters);
    } else {
        for (int i = 0; i < n; i++)
            sty_local_vertex<STY_ENERGY>(i, n, rowptr, col, w, V0, P, nrm.data(), area.data(), lam, Q, tgt, p, 0, nullptr, const_cast<double*>(R_in), out, nullptr);
    }
}

}  // namespace smg
