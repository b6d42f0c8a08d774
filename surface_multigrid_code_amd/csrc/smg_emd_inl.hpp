// smg_emd_inl.hpp -- the per-face, per-corner and per-vertex arithmetic of the earth mover's distance on a mesh, in registers
// (csrc/smg_emd_device.hip, smg_emd_host; include/smg.h: smg_emd_*).  Positions are xyz rows; masses and potentials are
// column-major nV x k blocks with a leading dimension; the state is 4 doubles per (face, column) -- Z then U -- and column c follows column c - 1
// (at c * 4 nF); a field in the faces' frames is 2 doubles per (face, column) (column c at c * 2 nF).
//
//   frame     t1 = (p1 - p0) / |p1 - p0|,  t2 = n x t1,  with n and W_fi = (n x e_i) / (2A) of morph_basis (smg_morph_inl.hpp)
//   geometry  W2_fi = (W_fi . t1, W_fi . t2), each ((a0 b0 + a1 b1) + a2 b2);  A = (2A) / 2
//   corner    corner (f, i)'s term of a weak divergence: A (W2_fi[0] X[0] + W2_fi[1] X[1])
//   update    Y = Z - U;  g = (phi0 W2_f0 + phi1 W2_f1) + phi2 W2_f2;  J = Y - g;  T = (alpha J + (1 - alpha) Z) + U;
//             s = max(0, 1 - (1 / rho) / |T|) (0 where |T| = 0);  Z = s T;  U = T - Z;  A |J|;  (rho rho) |g|^2
//   dual      potential = (-rho / max(1, sqrt(gmax2))) phi;  term = b potential
//   flow      J[0] t1 + J[1] t2
// Only +, -, *, /, sqrt and max occur; host and device compile the same text (the library is built with -ffp-contract=off), so the two agree bit
// for bit.  The host twin's sums are flow_host_sum / flow_host_max (smg_flow_inl.hpp), the order of launch_fixed_sum / launch_fixed_max.
#pragma once
#include <cmath>
#include <cstddef>
#include <vector>

#include "smg_hodge_inl.hpp"

namespace smg {

// t1, t2 (3 each), W (9), *dA2 = twice the area
SMG_ARAP_HD void emd_frame(const double* a, const double* b, const double* c, double* t1, double* t2, double* W, double* dA2)
{
    double nrm[3], e[3];
    morph_basis(a, b, c, W, nrm, dA2);
    hodge_edge(b, a, e);
    const double len = sqrt(hodge_dot(e, e));
    t1[0] = e[0] / len; t1[1] = e[1] / len; t1[2] = e[2] / len;
    hodge_cross(nrm, t1, t2);
}

// W2 (6: W2[2 i + d]), *A
SMG_ARAP_HD void emd_geometry(const double* a, const double* b, const double* c, double* W2, double* A)
{
    double t1[3], t2[3], W[9], dA;
    emd_frame(a, b, c, t1, t2, W, &dA);
#pragma unroll
    for (int i = 0; i < 3; i++) {
        W2[2 * i] = hodge_dot(W + 3 * i, t1);
        W2[2 * i + 1] = hodge_dot(W + 3 * i, t2);
    }
    *A = dA * 0.5;
}

SMG_ARAP_HD double emd_corner(double A, const double* w2, double x0, double x1) { return A * (w2[0] * x0 + w2[1] * x1); }

// zu (4, in place): Z then U.  J (2), *up = A |J|, *gq = rho^2 |grad phi|^2
SMG_ARAP_HD void emd_update(const double* W2, double A, double p0, double p1, double p2, double rho, double alpha, double* zu, double* J, double* up,
                            double* gq)
{
    const double oma = 1.0 - alpha, inv_rho = 1.0 / rho;
    double g[2], T[2];
#pragma unroll
    for (int d = 0; d < 2; d++) {
        const double y = zu[d] - zu[2 + d];
        g[d] = (p0 * W2[d] + p1 * W2[2 + d]) + p2 * W2[4 + d];
        J[d] = y - g[d];
        T[d] = (alpha * J[d] + oma * zu[d]) + zu[2 + d];
    }
    const double nT = sqrt(T[0] * T[0] + T[1] * T[1]);
    double s = 0.0;
    if (nT > 0.0) s = fmax(0.0, 1.0 - inv_rho / nT);
#pragma unroll
    for (int d = 0; d < 2; d++) {
        zu[d] = s * T[d];
        zu[2 + d] = T[d] - zu[d];
    }
    *up = A * sqrt(J[0] * J[0] + J[1] * J[1]);
    *gq = (rho * rho) * (g[0] * g[0] + g[1] * g[1]);
}

SMG_ARAP_HD double emd_dual_scale(double rho, double gmax2) { return -rho / fmax(1.0, sqrt(gmax2)); }

// ---- the host twin (smg_emd_host): the kernels' loops on caller arrays, with the layouts of smg_debug_emd (include/smg.h).  mp / mi: the corner
// lists t = 3 f + i of every vertex, faces ascending ------------------------------------------------------------------------------------------------
// W2 (nF x 6), A (nF)
inline void emd_host_geometry(int nF, const int* F, const double* V, double* W2, double* A)
{
    for (size_t f = 0; f < (size_t)nF; f++)
        emd_geometry(V + 3 * (size_t)F[3 * f], V + 3 * (size_t)F[3 * f + 1], V + 3 * (size_t)F[3 * f + 2], W2 + 6 * f, A + f);
}

// out (nV x k column-major) = the weak divergence of X minus b; X: the state (stride 4: Y = Z - U is formed) or a frame field (stride 2);
// dsq (optional, k planes of nV): the squares, row 0's zero
inline void emd_host_divergence(int nV, int nF, int k, const double* W2, const double* A, const int* mp, const int* mi, const double* b, const double* X,
                                int stride, double* out, double* dsq)
{
    const size_t n = (size_t)nV;
    for (int s = 0; s < k; s++)
        for (int v = 0; v < nV; v++) {
            double acc = 0.0;
            for (int p = mp[v]; p < mp[v + 1]; p++) {
                const size_t f = (size_t)(mi[p] / 3);
                const int i = mi[p] - 3 * (int)f;
                const double* x = X + ((size_t)s * nF + f) * stride;
                const double x0 = stride == 4 ? x[0] - x[2] : x[0], x1 = stride == 4 ? x[1] - x[3] : x[1];
                acc += emd_corner(A[f], W2 + 6 * f + 2 * i, x0, x1);
            }
            const double r = acc - b[(size_t)s * n + v];
            out[(size_t)s * n + v] = r;
            if (dsq) dsq[(size_t)s * n + v] = v == 0 ? 0.0 : r * r;
        }
}

// ZU (k sets of nF x 4, out), J (k sets of nF x 2), up and gq (k planes of nF each)
inline void emd_host_update(int nV, int nF, int k, const int* F, const double* W2, const double* A, const double* phi, const double* ZU_in,
                            const double* rho, double alpha, double* ZU, double* J, double* up, double* gq)
{
    const size_t n = (size_t)nV, nf = (size_t)nF;
    for (int s = 0; s < k; s++)
        for (size_t f = 0; f < nf; f++) {
            const double* pc = phi + (size_t)s * n;
            double* zu = ZU + ((size_t)s * nf + f) * 4;
            for (int e = 0; e < 4; e++) zu[e] = ZU_in[((size_t)s * nf + f) * 4 + e];
            emd_update(W2 + 6 * f, A[f], pc[F[3 * f]], pc[F[3 * f + 1]], pc[F[3 * f + 2]], rho[s], alpha, zu, J + ((size_t)s * nf + f) * 2,
                       up + (size_t)s * nf + f, gq + (size_t)s * nf + f);
        }
}

// pot (nV x k column-major), terms (k planes of nV)
inline void emd_host_dual(int nV, int k, const double* b, const double* phi, const double* rho, const double* gmax2, double* pot, double* terms)
{
    const size_t n = (size_t)nV;
    for (int s = 0; s < k; s++) {
        const double sc = emd_dual_scale(rho[s], gmax2[s]);
        for (size_t v = 0; v < n; v++) {
            pot[(size_t)s * n + v] = sc * phi[(size_t)s * n + v];
            terms[(size_t)s * n + v] = b[(size_t)s * n + v] * pot[(size_t)s * n + v];
        }
    }
}

// out (k sets of nF x 3)
inline void emd_host_flow(int nF, int k, const int* F, const double* V, const double* J, double* out)
{
    const size_t nf = (size_t)nF;
    for (int s = 0; s < k; s++)
        for (size_t f = 0; f < nf; f++) {
            double t1[3], t2[3], W[9], dA;
            emd_frame(V + 3 * (size_t)F[3 * f], V + 3 * (size_t)F[3 * f + 1], V + 3 * (size_t)F[3 * f + 2], t1, t2, W, &dA);
            const double* j = J + ((size_t)s * nf + f) * 2;
            for (int d = 0; d < 3; d++) out[((size_t)s * nf + f) * 3 + d] = j[0] * t1[d] + j[1] * t2[d];
        }
}

}  // namespace smg
