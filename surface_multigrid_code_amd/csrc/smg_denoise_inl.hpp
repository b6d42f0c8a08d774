// smg_denoise_inl.hpp -- the per-face maths of feature-preserving mesh denoising (smg_denoise_*, include/smg.h; kernels in
// csrc/smg_denoise_device.hip, host side in smg_denoise.cpp; the normal filter is the local scheme of Zheng, Fu, Au, Tai 2011).
//
// Input mesh V, faces F.  Face f has corners p0, p1, p2 in F's order, e1 = p1 - p0, e2 = p2 - p0, N = e1 x e2.
//   rest constants    the ten numbers r = {n_x, n_y, n_z, A, c_x, c_y, c_z, w_0, w_1, w_2}: n = N / |N|, A = |N| / 2,
//                     c = ((p0 + p1) + p2) / 3, and w_k = half the cotangent of the angle at corner k, the weight of the edge opposite corner k,
//                     by the expression of smg_mesh_cotmatrix: with l2_k the squared length of that edge,
//                     w_0 = ((l2_1 + l2_2) - l2_0) / |N| / 4 and cyclic
//   filter            one neighbour g of face f adds  (A_g exp(0 - (|c_f - c_g|^2 / (2 sigma_s^2) + |m_f - m_g|^2 / (2 sigma_r^2)))) m_g  to s_f:
//                     the product of the two Gaussians as ONE exponential of the summed arguments; every |.|^2 is one accumulator over x, y, z in
//                     that order; the neighbours are added in list order into one accumulator per coordinate from 0
//   filter, the end   m_f <- s_f / |s_f|; when |s_f| is zero or not finite m_f stays, bit for bit
//   spacing           face f adds  sum_g |c_f - c_g|  in list order: the terms of the rule sigma_s = the mean of |c_f - c_g| over the ordered pairs
//   projection        for k = 0, 1, 2 with (i, j) the two corners after k in cyclic order: d = x_i - x_j, h_k = d . m_f (one accumulator over
//                     x, y, z), t_k = d - h_k m_f; the face's energy term (1/2) ((w_0 h_0^2 + w_1 h_1^2) + w_2 h_2^2); the corner shares
//                     corner 0: w_2 t_2 - w_1 t_1, corner 1: w_0 t_0 - w_2 t_2, corner 2: w_1 t_1 - w_0 t_0  (+ where the corner is i, - where it is j)
// A non-finite pose gives a non-finite energy term, and the update reports it.
// Every expression is written operation by operation; host and device compile the same text with contraction off (-ffp-contract=off) and
// correctly rounded / and sqrt.  exp is the one call whose bits may differ between the host's libm and the device's; tests/denoise_np.py
// restates all of it in numpy from the formulas.
//
// Not covered: collapse prevention (the energy does not resist slivers at high noise), anisotropic or guided filters, the edge-neighbour
// variant of N(f), union / block / sharded forms, moving connectivity.
#pragma once
#include <cmath>
#include <cstddef>

#if defined(__HIPCC__)
#define SMG_DN_HD __host__ __device__ __forceinline__
#else
#define SMG_DN_HD inline
#endif

namespace smg {

constexpr int DN_REST = 10;                          // planes of the rest constants: n (0..2), A (3), c (4..6), w (7..9)
constexpr double DN_DBL_MAX = 1.7976931348623157e308;

SMG_DN_HD double dn_dist2(const double (&a)[3], const double (&b)[3])
{
    const double x = a[0] - b[0], y = a[1] - b[1], z = a[2] - b[2];
    return (x * x + y * y) + z * z;
}

// r = {n, A, c, w} from the corners (xyz each)
SMG_DN_HD void dn_rest(const double* p0, const double* p1, const double* p2, double (&r)[DN_REST])
{
    const double e1x = p1[0] - p0[0], e1y = p1[1] - p0[1], e1z = p1[2] - p0[2];
    const double e2x = p2[0] - p0[0], e2y = p2[1] - p0[1], e2z = p2[2] - p0[2];
    const double Nx = e1y * e2z - e1z * e2y, Ny = e1z * e2x - e1x * e2z, Nz = e1x * e2y - e1y * e2x;
    const double dbl = sqrt((Nx * Nx + Ny * Ny) + Nz * Nz);
    r[0] = Nx / dbl; r[1] = Ny / dbl; r[2] = Nz / dbl;
    r[3] = 0.5 * dbl;
#pragma unroll
    for (int l = 0; l < 3; l++) r[4 + l] = ((p0[l] + p1[l]) + p2[l]) / 3.0;
    const double a[3] = {p1[0] - p2[0], p1[1] - p2[1], p1[2] - p2[2]};   // the edge opposite corner 0
    const double b[3] = {p2[0] - p0[0], p2[1] - p0[1], p2[2] - p0[2]};   // opposite corner 1
    const double c[3] = {p0[0] - p1[0], p0[1] - p1[1], p0[2] - p1[2]};   // opposite corner 2
    const double l0 = (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2];
    const double l1 = (b[0] * b[0] + b[1] * b[1]) + b[2] * b[2];
    const double l2 = (c[0] * c[0] + c[1] * c[1]) + c[2] * c[2];
    r[7] = ((l1 + l2) - l0) / dbl / 4.0;
    r[8] = ((l2 + l0) - l1) / dbl / 4.0;
    r[9] = ((l0 + l1) - l2) / dbl / 4.0;
}

// s += the share of neighbour g (centroid cg, area Ag, normal mg) in the filter of the face with centroid cf and normal mf
SMG_DN_HD void dn_filter_add(const double (&cf)[3], const double (&mf)[3], const double (&cg)[3], double Ag, const double (&mg)[3], double two_ss,
                             double two_rr, double (&s)[3])
{
    const double wgt = Ag * exp(0.0 - (dn_dist2(cf, cg) / two_ss + dn_dist2(mf, mg) / two_rr));
#pragma unroll
    for (int l = 0; l < 3; l++) s[l] += wgt * mg[l];
}

// out = s / |s|, or mf when |s| is zero or not finite
SMG_DN_HD void dn_filter_finish(const double (&s)[3], const double (&mf)[3], double (&out)[3])
{
    const double len = sqrt((s[0] * s[0] + s[1] * s[1]) + s[2] * s[2]);
    const bool ok = len > 0.0 && len <= DN_DBL_MAX;      // false for a NaN too
#pragma unroll
    for (int l = 0; l < 3; l++) out[l] = ok ? s[l] / len : mf[l];
}

// the pose's corners x0, x1, x2 (xyz each) against the normal m and the weights w: the nine corner shares s[3 i + l]; returns the energy term
SMG_DN_HD double dn_project(const double (&x)[3][3], const double (&m)[3], const double (&w)[3], double (&s)[9])
{
    double t[3][3], h[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const int i = (k + 1) % 3, j = (k + 2) % 3;
        const double d0 = x[i][0] - x[j][0], d1 = x[i][1] - x[j][1], d2 = x[i][2] - x[j][2];
        h[k] = (d0 * m[0] + d1 * m[1]) + d2 * m[2];
        t[k][0] = w[k] * (d0 - h[k] * m[0]);
        t[k][1] = w[k] * (d1 - h[k] * m[1]);
        t[k][2] = w[k] * (d2 - h[k] * m[2]);
    }
#pragma unroll
    for (int l = 0; l < 3; l++) {
        s[l] = t[2][l] - t[1][l];
        s[3 + l] = t[0][l] - t[2][l];
        s[6 + l] = t[1][l] - t[0][l];
    }
    return 0.5 * ((w[0] * (h[0] * h[0]) + w[1] * (h[1] * h[1])) + w[2] * (h[2] * h[2]));
}

// ---- the host twin of the per-face pieces (smg_denoise_faces_host after its argument checks; tests/denoise_asan_driver.cpp runs it under
// sanitizers): op 0 the rest constants (out: 10 planes), 1 the spacing terms (out: nF), 2 `iters` filter iterations from the normals `in` (3
// planes; out: 3 planes), 3 the projection of the pose P (xyz rows) against the normals `in` (out: the energy terms, then the 9 share planes).
// nb_ptr / nb_idx: N(f), read by ops 1 and 2 only.  Host only.
inline void dn_faces_host(int op, int nF, const int* F, const double* V0, const double* P, const double* in, double sigma_s, double sigma_r, int iters,
                          const int* nb_ptr, const int* nb_idx, double* out)
{
    const size_t nf = (size_t)nF;
    double* rest = out;
    double* own = nullptr;
    if (op != 0) rest = own = new double[DN_REST * nf];
    for (size_t f = 0; f < nf; f++) {
        double r[DN_REST];
        dn_rest(V0 + 3 * (size_t)F[3 * f], V0 + 3 * (size_t)F[3 * f + 1], V0 + 3 * (size_t)F[3 * f + 2], r);
        for (int e = 0; e < DN_REST; e++) rest[e * nf + f] = r[e];
    }
    auto load3 = [nf](const double* planes, size_t f, double (&v)[3]) { for (int l = 0; l < 3; l++) v[l] = planes[l * nf + f]; };
    const double* cen = rest + 4 * nf;
    if (op == 1) {
        for (size_t f = 0; f < nf; f++) {
            double cf[3], cg[3], acc = 0.0;
            load3(cen, f, cf);
            for (int q = nb_ptr[f]; q < nb_ptr[f + 1]; q++) {
                load3(cen, (size_t)nb_idx[q], cg);
                acc += sqrt(dn_dist2(cf, cg));
            }
            out[f] = acc;
        }
    } else if (op == 2) {
        double* pair = new double[6 * nf];
        double *a = pair, *b = pair + 3 * nf;
        for (size_t i = 0; i < 3 * nf; i++) a[i] = in[i];
        const double two_ss = 2.0 * (sigma_s * sigma_s), two_rr = 2.0 * (sigma_r * sigma_r);
        for (int it = 0; it < iters; it++) {
            for (size_t f = 0; f < nf; f++) {
                double cf[3], mf[3], cg[3], mg[3], s[3] = {0.0, 0.0, 0.0}, o[3];
                load3(cen, f, cf);
                load3(a, f, mf);
                for (int q = nb_ptr[f]; q < nb_ptr[f + 1]; q++) {
                    const size_t g = (size_t)nb_idx[q];
                    load3(cen, g, cg);
                    load3(a, g, mg);
                    dn_filter_add(cf, mf, cg, rest[3 * nf + g], mg, two_ss, two_rr, s);
                }
                dn_filter_finish(s, mf, o);
                for (int l = 0; l < 3; l++) b[l * nf + f] = o[l];
            }
            double* t = a; a = b; b = t;
        }
        for (size_t i = 0; i < 3 * nf; i++) out[i] = a[i];
        delete[] pair;
    } else if (op == 3) {
        for (size_t f = 0; f < nf; f++) {
            double x[3][3], s[9], m[3], w[3];
            for (int i = 0; i < 3; i++)
                for (int l = 0; l < 3; l++) x[i][l] = P[3 * (size_t)F[3 * f + i] + l];
            load3(in, f, m);
            load3(rest + 7 * nf, f, w);
            out[f] = dn_project(x, m, w, s);
            for (int e = 0; e < 9; e++) out[(1 + e) * nf + f] = s[e];
        }
    }
    delete[] own;
}

}  // namespace smg
