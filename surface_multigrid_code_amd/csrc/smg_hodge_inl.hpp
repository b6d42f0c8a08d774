// smg_hodge_inl.hpp -- the per-face and per-corner arithmetic of the Helmholtz-Hodge decomposition, in registers (csrc/smg_hodge_device.hip,
// smg_hodge_host; include/smg.h: smg_hodge_*).  Positions are xyz rows (nV x 3 row-major, as every create takes them); a
// field is nF x 3 row-major and set c follows set c - 1 (at c * 3 nF); potentials are column-major nV x k blocks with a leading dimension.
//
//   basis     W_fi = (n x e_i) / (2A), n, 2A: morph_basis (smg_morph_inl.hpp), the expressions of k_geo_basis operation by operation
//   edge      e_j = p_{j+2} - p_{j+1} (indices mod 3): the edge opposite corner j, from the two vertices alone
//   corner    corner (f, j)'s terms of the two right-hand sides: (n x e_j) . X_f and e_j . X_f, each ((a0 b0 + a1 b1) + a2 b2)
//   grad      sum_i a_i W_fi, i = 0, 1, 2 in order: the gradient of a piece-wise linear function
//   parts     Xt = X - (X . n) n,  G = grad u,  R = n x grad v,  H = (Xt - G) - R
//   terms     A |Xt|^2, A |G|^2, A |R|^2, A |H|^2, each A ((a0^2 + a1^2) + a2^2)
//   field     grad u + n x grad v
// Only +, -, *, / and sqrt occur; host and device compile the same text (the library is built with -ffp-contract=off), so the two agree bit for
// bit.  The host twin's sums are flow_host_sum (smg_flow_inl.hpp), the order of launch_fixed_sum.
#pragma once
#include <cmath>
#include <cstddef>

#include "smg_flow_inl.hpp"
#include "smg_morph_inl.hpp"

namespace smg {

// e = a - b: the edge opposite corner j of a face runs from vertex j + 1 (b) to vertex j + 2 (a), indices mod 3
SMG_ARAP_HD void hodge_edge(const double* a, const double* b, double* e)
{
    e[0] = a[0] - b[0]; e[1] = a[1] - b[1]; e[2] = a[2] - b[2];
}

SMG_ARAP_HD double hodge_dot(const double* a, const double* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

SMG_ARAP_HD void hodge_cross(const double* a, const double* b, double* c)
{
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}

// *tb = (n x e) . X, *tc = e . X
SMG_ARAP_HD void hodge_corner(const double* nrm, const double* e, const double* X, double* tb, double* tc)
{
    double ne[3];
    hodge_cross(nrm, e, ne);
    *tb = hodge_dot(ne, X);
    *tc = hodge_dot(e, X);
}

// g = a0 W_f0 + a1 W_f1 + a2 W_f2
SMG_ARAP_HD void hodge_grad(const double* W, double a0, double a1, double a2, double* g)
{
#pragma unroll
    for (int d = 0; d < 3; d++) g[d] = (a0 * W[d] + a1 * W[3 + d]) + a2 * W[6 + d];
}

// P = G (3), R (3), H (3); Xt (3)
SMG_ARAP_HD void hodge_parts(const double* W, const double* nrm, const double* X, const double* u, const double* v, double* Xt, double* P)
{
    const double xn = hodge_dot(X, nrm);
    double gv[3];
#pragma unroll
    for (int d = 0; d < 3; d++) Xt[d] = X[d] - xn * nrm[d];
    hodge_grad(W, u[0], u[1], u[2], P);
    hodge_grad(W, v[0], v[1], v[2], gv);
    hodge_cross(nrm, gv, P + 3);
#pragma unroll
    for (int d = 0; d < 3; d++) P[6 + d] = (Xt[d] - P[d]) - P[3 + d];
}

SMG_ARAP_HD double hodge_term(double A, const double* a) { return A * hodge_dot(a, a); }

SMG_ARAP_HD void hodge_field(const double* W, const double* nrm, const double* u, const double* v, double* X)
{
    double gu[3], gv[3], r[3];
    hodge_grad(W, u[0], u[1], u[2], gu);
    hodge_grad(W, v[0], v[1], v[2], gv);
    hodge_cross(nrm, gv, r);
#pragma unroll
    for (int d = 0; d < 3; d++) X[d] = gu[d] + r[d];
}

// ---- the host twin (smg_hodge_host): the kernels' loops on caller arrays, with the layouts of smg_debug_hodge (include/smg.h).  mp / mi: the
// corner lists t = 3 f + i of every vertex, faces ascending -----------------------------------------------------------------------------------
inline void hodge_host_face(const int* F, const double* V, size_t f, double* W, double* nrm, double* A)
{
    double dA;
    morph_basis(V + 3 * (size_t)F[3 * f], V + 3 * (size_t)F[3 * f + 1], V + 3 * (size_t)F[3 * f + 2], W, nrm, &dA);
    *A = dA * 0.5;
}

// b, c (nV x k column-major, leading dimension nV) and bsq (2 planes of k nV: b^2 then c^2)
inline void hodge_host_rhs(int nV, int nF, int k, const int* F, const double* V, const int* mp, const int* mi, const double* X, double* b, double* c,
                           double* bsq)
{
    const size_t n = (size_t)nV;
    for (int s = 0; s < k; s++)
        for (int v = 0; v < nV; v++) {
            double accb = 0.0, accc = 0.0;
            for (int p = mp[v]; p < mp[v + 1]; p++) {
                const size_t f = (size_t)(mi[p] / 3);
                const int j = mi[p] - 3 * (int)f;
                double W[9], nrm[3], A, e[3], tb, tc;
                hodge_host_face(F, V, f, W, nrm, &A);
                hodge_edge(V + 3 * (size_t)F[3 * f + (j + 2) % 3], V + 3 * (size_t)F[3 * f + (j + 1) % 3], e);
                hodge_corner(nrm, e, X + ((size_t)s * nF + f) * 3, &tb, &tc);
                accb += tb;
                accc += tc;
            }
            const double bv = 0.5 * accb, cv = -0.5 * accc;
            b[(size_t)s * n + v] = bv;
            c[(size_t)s * n + v] = cv;
            bsq[(size_t)s * n + v] = bv * bv;
            bsq[((size_t)k + s) * n + v] = cv * cv;
        }
}

// parts (k sets of nF x 9), terms (4 k planes of nF: plane 4 s + e), energy (4 k)
inline void hodge_host_parts(int nV, int nF, int k, const int* F, const double* V, const double* X, const double* u, const double* v, double* parts,
                             double* terms, double* energy)
{
    const size_t n = (size_t)nV, nf = (size_t)nF;
    for (int s = 0; s < k; s++) {
        for (size_t f = 0; f < nf; f++) {
            double W[9], nrm[3], A, Xt[3], P[9];
            hodge_host_face(F, V, f, W, nrm, &A);
            const size_t i0 = (size_t)F[3 * f], i1 = (size_t)F[3 * f + 1], i2 = (size_t)F[3 * f + 2];
            const double uf[3] = {u[(size_t)s * n + i0], u[(size_t)s * n + i1], u[(size_t)s * n + i2]};
            const double vf[3] = {v[(size_t)s * n + i0], v[(size_t)s * n + i1], v[(size_t)s * n + i2]};
            hodge_parts(W, nrm, X + ((size_t)s * nf + f) * 3, uf, vf, Xt, P);
            for (int e = 0; e < 9; e++) parts[((size_t)s * nf + f) * 9 + e] = P[e];
            terms[(4 * (size_t)s + 0) * nf + f] = hodge_term(A, Xt);
            terms[(4 * (size_t)s + 1) * nf + f] = hodge_term(A, P);
            terms[(4 * (size_t)s + 2) * nf + f] = hodge_term(A, P + 3);
            terms[(4 * (size_t)s + 3) * nf + f] = hodge_term(A, P + 6);
        }
        for (int e = 0; e < 4; e++) energy[4 * s + e] = flow_host_sum(terms + (4 * (size_t)s + e) * nf, nF);
    }
}

// X (k sets of nF x 3)
inline void hodge_host_field(int nV, int nF, int k, const int* F, const double* V, const double* u, const double* v, double* X)
{
    const size_t n = (size_t)nV, nf = (size_t)nF;
    for (int s = 0; s < k; s++)
        for (size_t f = 0; f < nf; f++) {
            double W[9], nrm[3], A;
            hodge_host_face(F, V, f, W, nrm, &A);
            const size_t i0 = (size_t)F[3 * f], i1 = (size_t)F[3 * f + 1], i2 = (size_t)F[3 * f + 2];
            const double uf[3] = {u[(size_t)s * n + i0], u[(size_t)s * n + i1], u[(size_t)s * n + i2]};
            const double vf[3] = {v[(size_t)s * n + i0], v[(size_t)s * n + i1], v[(size_t)s * n + i2]};
            hodge_field(W, nrm, uf, vf, X + ((size_t)s * nf + f) * 3);
        }
}

}  // namespace smg
