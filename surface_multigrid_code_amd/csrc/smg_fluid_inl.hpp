// smg_fluid_inl.hpp -- the per-corner, per-vertex and per-face arithmetic of incompressible flow on a surface in vorticity form, in registers
// (csrc/smg_fluid_device.hip, smg_fluid_host; include/smg.h: smg_fluid_*).  Positions are xyz rows; vorticity, stream
// function and right-hand sides are column-major nV x k blocks with a leading dimension, one column per simulation; per-vertex term planes are k
// planes of nV; a velocity is 3 doubles per (face, column), column c at c * 3 nF.
//
//   mass      m_i = (sum of A_f over i's corners, in list order) / 3.0, A_f = (2A) / 2 of morph_basis (smg_morph_inl.hpp)
//   rhs       r_i = 0.0 - m_i (w_i - wbar);  wbar = (sum m w) / (sum m) on a closed mesh, 0.0 with boundary;  r_i^2, 0 on a known row
//   corner    corner of vertex i in face (i, j, k): c = ((psi_i + psi_j) + psi_k) / 3.0;  Phi_ij = 0.5 (psi_i + psi_j) - c;
//             Phi_ik = c - 0.5 (psi_i + psi_k);  acc += (0.5 (Phi - theta |Phi|)) (w_nbr - w_i), ij then ik;  racc += max(Phi, 0.0), ij then ik
//   vertex    adv = 0.0 - acc / m_i;  rate = racc / m_i;  out = a wn_i + b (w_i + dt adv);  the term m_i out
//   dt        dt = cfl / rmax (0.0 where rmax is not > 0);  a step's cfl = dt max over its stages of rmax
//   velocity  g = sum_i psi_i W_fi (hodge_grad);  u = n x g;  the term 0.5 (A |g|^2)
//   diag      the terms m w and 0.5 ((m w) w)
// Only +, -, *, /, max and fabs occur; host and device compile the same text (the library is built with -ffp-contract=off), so the two agree bit
// for bit.  The host twin's sums are flow_host_sum / flow_host_max (smg_flow_inl.hpp), the order of launch_fixed_sum / launch_fixed_max.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <vector>

#include "smg_hodge_inl.hpp"
#include "smg_mesh.hpp"

namespace smg {

SMG_ARAP_HD double fluid_rhs(double m, double w, double wbar) { return 0.0 - m * (w - wbar); }

// the two dual-cell segments of one corner: psi and w at the corner's own vertex (i) and at the face's next (j) and previous (k) vertices
SMG_ARAP_HD void fluid_corner(double pi, double pj, double pk, double wi, double wj, double wk, double theta, double* acc, double* racc)
{
    const double c = ((pi + pj) + pk) / 3.0;
    const double fij = 0.5 * (pi + pj) - c;
    const double fik = c - 0.5 * (pi + pk);
    *acc += (0.5 * (fij - theta * fabs(fij))) * (wj - wi);
    *acc += (0.5 * (fik - theta * fabs(fik))) * (wk - wi);
    *racc += fmax(fij, 0.0);
    *racc += fmax(fik, 0.0);
}

// the fluxes alone, for the rates-only launch
SMG_ARAP_HD void fluid_corner_rate(double pi, double pj, double pk, double* racc)
{
    const double c = ((pi + pj) + pk) / 3.0;
    const double fij = 0.5 * (pi + pj) - c;
    const double fik = c - 0.5 * (pi + pk);
    *racc += fmax(fij, 0.0);
    *racc += fmax(fik, 0.0);
}

SMG_ARAP_HD double fluid_stage(double a, double b, double wn, double wi, double dt, double acc, double m)
{
    const double adv = 0.0 - acc / m;
    return a * wn + b * (wi + dt * adv);
}

SMG_ARAP_HD double fluid_dt(double cfl, double rmax) { return rmax > 0.0 ? cfl / rmax : 0.0; }

// u (3), *term = 0.5 (A |grad psi|^2)
SMG_ARAP_HD void fluid_velocity(const double* W, const double* nrm, double A, double p0, double p1, double p2, double* u, double* term)
{
    double g[3];
    hodge_grad(W, p0, p1, p2, g);
    hodge_cross(nrm, g, u);
    *term = 0.5 * hodge_term(A, g);
}

SMG_ARAP_HD void fluid_diag(double m, double w, double* mw, double* ew)
{
    *mw = m * w;
    *ew = 0.5 * (*mw * w);
}

// ---- the host twin (smg_fluid_host): the kernels' loops on caller arrays, with the layouts of smg_debug_fluid (include/smg.h).  mp / mi: the
// corner lists t = 3 f + i of every vertex, faces ascending ------------------------------------------------------------------------------------
// known (nV): 1 on the rows whose psi is given -- boundary_vertices (smg_mesh.hpp), or vertex 0 on a closed mesh.  Returns
// the number of boundary vertices (0: closed)
inline int fluid_known_rows(int nV, int nF, const int* F, std::vector<int>& known)
{
    const std::vector<int> bnd = boundary_vertices(F, nF, nV);
    known.assign((size_t)nV, 0);
    for (int v : bnd) known[(size_t)v] = 1;
    if (bnd.empty()) known[0] = 1;
    return (int)bnd.size();
}

// A (nF), m (nV)
inline void fluid_host_mass(int nV, int nF, const int* F, const double* V, const int* mp, const int* mi, double* A, double* m)
{
    for (size_t f = 0; f < (size_t)nF; f++) {
        double W[9], nrm[3];
        hodge_host_face(F, V, f, W, nrm, A + f);
    }
    for (int v = 0; v < nV; v++) {
        double acc = 0.0;
        for (int p = mp[v]; p < mp[v + 1]; p++) acc += A[mi[p] / 3];
        m[v] = acc / 3.0;
    }
}

// R (nV x k column-major), rsq (k planes of nV); mwsum (k; nullptr: wbar = 0.0)
inline void fluid_host_rhs(int nV, int k, const double* m, const int* known, const double* w, const double* mwsum, double msum, double* R, double* rsq)
{
    const size_t n = (size_t)nV;
    for (int s = 0; s < k; s++) {
        const double wbar = mwsum ? mwsum[s] / msum : 0.0;
        for (size_t v = 0; v < n; v++) {
            const double r = fluid_rhs(m[v], w[(size_t)s * n + v], wbar);
            R[(size_t)s * n + v] = r;
            rsq[(size_t)s * n + v] = known && known[v] ? 0.0 : r * r;
        }
    }
}

// out, mw (nV x k column-major; both nullptr: rates only), rate (k planes of nV)
inline void fluid_host_advect(int nV, int k, const int* F, const int* mp, const int* mi, const double* m, const double* psi, const double* w,
                              const double* wn, double a, double b, const double* dt, double theta, double* out, double* rate, double* mw)
{
    const size_t n = (size_t)nV;
    for (int s = 0; s < k; s++) {
        const double* pc = psi + (size_t)s * n;
        const double* wc = w ? w + (size_t)s * n : nullptr;
        for (int v = 0; v < nV; v++) {
            double acc = 0.0, racc = 0.0;
            for (int p = mp[v]; p < mp[v + 1]; p++) {
                const size_t f = (size_t)(mi[p] / 3);
                const int i = mi[p] - 3 * (int)f;
                const size_t vj = (size_t)F[3 * f + (i + 1) % 3], vk = (size_t)F[3 * f + (i + 2) % 3];
                if (out)
                    fluid_corner(pc[v], pc[vj], pc[vk], wc[v], wc[vj], wc[vk], theta, &acc, &racc);
                else
                    fluid_corner_rate(pc[v], pc[vj], pc[vk], &racc);
            }
            rate[(size_t)s * n + v] = racc / m[v];
            if (out) {
                const double o = fluid_stage(a, b, wn[(size_t)s * n + v], wc[v], dt[s], acc, m[v]);
                out[(size_t)s * n + v] = o;
                mw[(size_t)s * n + v] = m[v] * o;
            }
        }
    }
}

// U (k sets of nF x 3), terms (k planes of nF)
inline void fluid_host_velocity(int nV, int nF, int k, const int* F, const double* V, const double* psi, double* U, double* terms)
{
    const size_t n = (size_t)nV, nf = (size_t)nF;
    for (int s = 0; s < k; s++)
        for (size_t f = 0; f < nf; f++) {
            double W[9], nrm[3], A;
            hodge_host_face(F, V, f, W, nrm, &A);
            const double* pc = psi + (size_t)s * n;
            fluid_velocity(W, nrm, A, pc[F[3 * f]], pc[F[3 * f + 1]], pc[F[3 * f + 2]], U + ((size_t)s * nf + f) * 3, terms + (size_t)s * nf + f);
        }
}

// mw, ew (k planes of nV each)
inline void fluid_host_diag(int nV, int k, const double* m, const double* w, double* mw, double* ew)
{
    const size_t n = (size_t)nV;
    for (int s = 0; s < k; s++)
        for (size_t v = 0; v < n; v++) fluid_diag(m[v], w[(size_t)s * n + v], mw + (size_t)s * n + v, ew + (size_t)s * n + v);
}

// one step's closing arithmetic: dt0 = cfl / rmax of the first stage; cfl_step = dt0 max over the stages; time = time_in + dt0
inline void fluid_host_dt(int k, int stages, double cfl, const double* rmax, const double* time_in, double* dt0, double* cfl_step, double* time)
{
    for (int c = 0; c < k; c++) {
        dt0[c] = fluid_dt(cfl, rmax[c]);
        double r = rmax[c];
        for (int s = 1; s < stages; s++) r = fmax(r, rmax[(size_t)s * k + c]);
        cfl_step[c] = dt0[c] * r;
        time[c] = time_in[c] + dt0[c];
    }
}

}  // namespace smg
