// smg_membrane_device.hip -- the kernels of the membrane time step, neo-Hookean, StVK and tension-field StVK (smg_membrane_step, include/smg.h; host side in
// smg_membrane.cpp; the per-face maths in smg_membrane_inl.hpp).
//
// Layout: positions, velocities, forces, gradients and right-hand sides are xyz rows (entry 3 v + l: the numbering of the 3-DOF system).
// Per-face results are face-major planes (plane e at out[e * nF + f]), so the stores of a wave coalesce: rest constants (5 planes),
// gradient (9), the upper triangle of the Hessian (45), pressure terms (6: e1 x e2, the three corner shares of the Voronoi mass).
//
// Determinism: no atomics.  A matrix block sums its faces' sub-blocks in the order of its contribution list (faces ascending), a vertex sums
// its corners in the order of its corner list (faces ascending), the objective is reduced over fixed chunks by a fixed tree (launch_fixed_sum).
// Expressions are written operation by operation (-ffp-contract=off): tests/test_membrane_host.py restates the sums in numpy in the same order.
#include <hip/hip_runtime.h>

#include "smg_device.hpp"
#include "smg_membrane_inl.hpp"

namespace smg {

namespace {

constexpr int MEM_THREADS = 256;
constexpr int MEM_FACE_THREADS = 64;      // k_membrane_faces holds a 9 x 9 Hessian and a 6 x 6 eigen-decomposition per lane: one wave per block

inline int mem_grid(long long n, int threads) { return (int)((n + threads - 1) / threads); }

__device__ __forceinline__ void load_corners(const int* __restrict__ F, const double* __restrict__ P, int f, double (&q)[9])
{
#pragma unroll
    for (int j = 0; j < 3; j++) {
        const double* p = P + 3 * (size_t)F[3 * (size_t)f + j];
        q[3 * j] = p[0]; q[3 * j + 1] = p[1]; q[3 * j + 2] = p[2];
    }
}

}  // namespace

// rest[e * nF + f]: (abar^-1)00, 01, 11, det abar, coeff = thickness sqrt(det abar) / 4
__global__ __launch_bounds__(MEM_THREADS) void k_membrane_rest(int nF, const int* __restrict__ F, const double* __restrict__ V0, double thickness,
                                                               double* __restrict__ rest)
{
    const int f = blockIdx.x * MEM_THREADS + threadIdx.x;
    if (f >= nF) return;
    double q[9];
    load_corners(F, V0, f, q);
    double e1[3], e2[3];
#pragma unroll
    for (int d = 0; d < 3; d++) { e1[d] = q[3 + d] - q[d]; e2[d] = q[6 + d] - q[d]; }
    const double a00 = (e1[0] * e1[0] + e1[1] * e1[1]) + e1[2] * e1[2];
    const double a01 = (e1[0] * e2[0] + e1[1] * e2[1]) + e1[2] * e2[2];
    const double a11 = (e2[0] * e2[0] + e2[1] * e2[1]) + e2[2] * e2[2];
    const double det = a00 * a11 - a01 * a01;
    rest[f] = a11 / det;
    rest[(size_t)nF + f] = -a01 / det;
    rest[2 * (size_t)nF + f] = a00 / det;
    rest[3 * (size_t)nF + f] = det;
    rest[4 * (size_t)nF + f] = thickness * sqrt(det) / 4.0;
}

// One lane per face.  MODE 0: W alone (the line search).  MODE 1: W, G and the unfixed H (the hook).  MODE 2: W, G and the fixed H'.
template <int MODE>
__global__ __launch_bounds__(MEM_FACE_THREADS) void k_membrane_faces(int nF, const int* __restrict__ F, const double* __restrict__ P,
                                                                     const double* __restrict__ rest, double alpha, double beta, double floor,
                                                                     double value, double* __restrict__ W, double* __restrict__ G,
                                                                     double* __restrict__ H)
{
    const int f = blockIdx.x * MEM_FACE_THREADS + threadIdx.x;
    if (f >= nF) return;
    double q[9], r[5], g[9], h[45];
    load_corners(F, P, f, q);
#pragma unroll
    for (int e = 0; e < 5; e++) r[e] = rest[e * (size_t)nF + f];
    W[f] = membrane_face<MODE != 0>(q, r, alpha, beta, g, h);
    if (MODE == 0) return;
#pragma unroll
    for (int e = 0; e < 9; e++) G[e * (size_t)nF + f] = g[e];
    if (MODE == 2) membrane_fix(h, floor, value);
#pragma unroll
    for (int e = 0; e < 45; e++) H[e * (size_t)nF + f] = h[e];
}

// The same for the StVK (MAT 1) and tension-field StVK (MAT 2) materials, under a name of its own: k_membrane_faces stays the neo-Hookean
// path.  The rest constants are recomputed from V0 by the expressions of k_membrane_rest, because M = abar^-1 (a - abar) needs abar itself
// (recovered from abar^-1 it would leave M = O(eps) at the rest pose, where the tension-field branch test needs exactly 0).  The three
// tension-field branches differ in ten scalars (membrane_face_mat), so the lanes of a wave diverge over those alone.
template <int MODE, int MAT>
__global__ __launch_bounds__(MEM_FACE_THREADS) void k_membrane_faces_mat(int nF, const int* __restrict__ F, const double* __restrict__ P,
                                                                         const double* __restrict__ V0, double thickness, double alpha,
                                                                         double beta, double floor, double value, double* __restrict__ W,
                                                                         double* __restrict__ G, double* __restrict__ H)
{
    const int f = blockIdx.x * MEM_FACE_THREADS + threadIdx.x;
    if (f >= nF) return;
    double q[9], r[8], g[9], h[45];
    load_corners(F, V0, f, q);
    mem_rest_consts(q, thickness, r);
    load_corners(F, P, f, q);
    W[f] = membrane_face_mat<MAT, MODE != 0>(q, r, thickness, alpha, beta, g, h);
    if (MODE == 0) return;
#pragma unroll
    for (int e = 0; e < 9; e++) G[e * (size_t)nF + f] = g[e];
    if (MODE == 2) membrane_fix(h, floor, value);
#pragma unroll
    for (int e = 0; e < 45; e++) H[e * (size_t)nF + f] = h[e];
}

// One lane per stored 3 x 3 block q of the pattern (vertex pair (i, j), i == j included).  Its nine values are dt^2 times the sum of the
// sub-blocks (corner a, corner b) of the incident faces' H' in list order (src = 9 f + 3 a + b), the vertex mass added last on the diagonal
// of a diagonal block; they go to their places in the scalar CSR of the 3 nV x 3 nV matrix, whose row 3 i + l holds, for every block of block
// row i in order, the three columns 3 j + m:  val[9 bptr[i] + l 3 cnt_i + 3 (q - bptr[i]) + m].
__global__ __launch_bounds__(MEM_THREADS) void k_membrane_matrix(int nB, const int* __restrict__ brow, const int* __restrict__ bcol,
                                                                 const int* __restrict__ bptr, const int* __restrict__ c_ptr,
                                                                 const int* __restrict__ c_src, const double* __restrict__ H, int nF, double dt2,
                                                                 const double* __restrict__ mass0, double mass_scale, double* __restrict__ val)
{
    const int q = blockIdx.x * MEM_THREADS + threadIdx.x;
    if (q >= nB) return;
    double acc[9];
#pragma unroll
    for (int e = 0; e < 9; e++) acc[e] = 0.0;
    const int t1 = c_ptr[q + 1];
    for (int t = c_ptr[q]; t < t1; t++) {
        const int src = c_src[t];
        const int f = src / 9, a = (src - 9 * f) / 3, b = src - 9 * f - 3 * a;
#pragma unroll
        for (int l = 0; l < 3; l++)
#pragma unroll
            for (int m = 0; m < 3; m++) {
                const int r = 3 * a + l, c = 3 * b + m;
                acc[3 * l + m] += H[(size_t)mem_sym(r, c) * nF + f];
            }
    }
    const int i = brow[q], first = bptr[i], cnt = bptr[i + 1] - first;
    const bool diag = bcol[q] == i;
    const double mv = mass_scale * mass0[i];
#pragma unroll
    for (int l = 0; l < 3; l++)
#pragma unroll
        for (int m = 0; m < 3; m++) {
            double v = dt2 * acc[3 * l + m];
            if (diag && l == m) v += mv;
            val[9 * (size_t)first + (size_t)l * 3 * cnt + 3 * (size_t)(q - first) + m] = v;
        }
}

// Qn[e * nF + f]: e1 x e2 (e = 0 .. 2) and the shares of corners 0 .. 2 in the face's mixed Voronoi area (e = 3 .. 5; the expressions of
// k_face_terms, smg_device.hip)
__global__ __launch_bounds__(MEM_THREADS) void k_membrane_pressure_faces(int nF, const int* __restrict__ F, const double* __restrict__ P,
                                                                         double* __restrict__ Qn)
{
    const int f = blockIdx.x * MEM_THREADS + threadIdx.x;
    if (f >= nF) return;
    double q[9];
    load_corners(F, P, f, q);
    const double* a = q;
    const double* b = q + 3;
    const double* c = q + 6;
    const double ux = b[0] - a[0], uy = b[1] - a[1], uz = b[2] - a[2];
    const double vx = c[0] - a[0], vy = c[1] - a[1], vz = c[2] - a[2];
    const double wx = uy * vz - uz * vy, wy = uz * vx - ux * vz, wz = ux * vy - uy * vx;
    const double dA = sqrt(wx * wx + wy * wy + wz * wz);
    const double d0x = b[0] - c[0], d0y = b[1] - c[1], d0z = b[2] - c[2];
    const double d1x = c[0] - a[0], d1y = c[1] - a[1], d1z = c[2] - a[2];
    const double d2x = a[0] - b[0], d2y = a[1] - b[1], d2z = a[2] - b[2];
    const double l0 = sqrt(d0x * d0x + d0y * d0y + d0z * d0z);
    const double l1 = sqrt(d1x * d1x + d1y * d1y + d1z * d1z);
    const double l2 = sqrt(d2x * d2x + d2y * d2y + d2z * d2z);
    const double cs0 = (l2 * l2 + l1 * l1 - l0 * l0) / (l1 * l2 * 2.0);
    const double cs1 = (l0 * l0 + l2 * l2 - l1 * l1) / (l2 * l0 * 2.0);
    const double cs2 = (l1 * l1 + l0 * l0 - l2 * l2) / (l0 * l1 * 2.0);
    const double b0 = cs0 * l0, b1 = cs1 * l1, b2 = cs2 * l2;
    const double bs = b0 + b1 + b2;
    const double p0 = b0 / bs * (dA * 0.5), p1 = b1 / bs * (dA * 0.5), p2 = b2 / bs * (dA * 0.5);
    double m0 = (p1 + p2) * 0.5, m1 = (p2 + p0) * 0.5, m2 = (p0 + p1) * 0.5;
    if (cs0 < 0) { m0 = 0.25 * dA; m1 = 0.125 * dA; m2 = 0.125 * dA; }
    if (cs1 < 0) { m0 = 0.125 * dA; m1 = 0.25 * dA; m2 = 0.125 * dA; }
    if (cs2 < 0) { m0 = 0.125 * dA; m1 = 0.125 * dA; m2 = 0.25 * dA; }
    Qn[f] = wx; Qn[(size_t)nF + f] = wy; Qn[2 * (size_t)nF + f] = wz;
    Qn[3 * (size_t)nF + f] = m0; Qn[4 * (size_t)nF + f] = m1; Qn[5 * (size_t)nF + f] = m2;
}

// One lane per vertex over its corner list (t = 3 f + j): m_v = the sum of its corner shares, N = the sum of e1 x e2 (the area-weighted face
// normals), fext_v = (-(pressure m_v)) (N / |N|).  mass and fext are optional outputs.
__global__ __launch_bounds__(MEM_THREADS) void k_membrane_pressure(int nV, const int* __restrict__ m_ptr, const int* __restrict__ m_idx,
                                                                   const double* __restrict__ Qn, int nF, double pressure,
                                                                   double* __restrict__ mass, double* __restrict__ fext)
{
    const int v = blockIdx.x * MEM_THREADS + threadIdx.x;
    if (v >= nV) return;
    double m = 0.0, nx = 0.0, ny = 0.0, nz = 0.0;
    const int p1 = m_ptr[v + 1];
    for (int p = m_ptr[v]; p < p1; p++) {
        const int t = m_idx[p], f = t / 3, j = t - 3 * f;
        m += Qn[(size_t)(3 + j) * nF + f];
        nx += Qn[f]; ny += Qn[(size_t)nF + f]; nz += Qn[2 * (size_t)nF + f];
    }
    if (mass) mass[v] = m;
    if (!fext) return;
    const double len = sqrt((nx * nx + ny * ny) + nz * nz);
    const double s = -(pressure * m);
    fext[3 * (size_t)v] = s * (nx / len);
    fext[3 * (size_t)v + 1] = s * (ny / len);
    fext[3 * (size_t)v + 2] = s * (nz / len);
}

// One lane per vertex over its corner list: g_v = the sum of the corners' G, b = -((M_v (qdot - qdot0) + dt g) + dt fext).  g is optional.
__global__ __launch_bounds__(MEM_THREADS) void k_membrane_gradient(int nV, const int* __restrict__ m_ptr, const int* __restrict__ m_idx,
                                                                   const double* __restrict__ G, int nF, const double* __restrict__ mass0,
                                                                   double mass_scale, double dt, const double* __restrict__ qdot,
                                                                   const double* __restrict__ qdot0, const double* __restrict__ fext,
                                                                   double* __restrict__ g, double* __restrict__ b)
{
    const int v = blockIdx.x * MEM_THREADS + threadIdx.x;
    if (v >= nV) return;
    double acc[3] = {0.0, 0.0, 0.0};
    const int p1 = m_ptr[v + 1];
    for (int p = m_ptr[v]; p < p1; p++) {
        const int t = m_idx[p], f = t / 3, j = t - 3 * f;
#pragma unroll
        for (int l = 0; l < 3; l++) acc[l] += G[(size_t)(3 * j + l) * nF + f];
    }
    const double mv = mass_scale * mass0[v];
#pragma unroll
    for (int l = 0; l < 3; l++) {
        const size_t e = 3 * (size_t)v + l;
        if (g) g[e] = acc[l];
        b[e] = -((mv * (qdot[e] - qdot0[e]) + dt * acc[l]) + dt * fext[e]);
    }
}

// One lane per vertex: the trial velocity t = qdot + step dx (dx == nullptr: t = qdot), the trial position p = pos0 + dt t, and the vertex's
// term of the objective, p . fext + (M_v |t - qdot0|^2) / 2.
__global__ __launch_bounds__(MEM_THREADS) void k_membrane_trial(int nV, const double* __restrict__ qdot, const double* __restrict__ dx, double step,
                                                                const double* __restrict__ qdot0, const double* __restrict__ pos0,
                                                                const double* __restrict__ fext, const double* __restrict__ mass0,
                                                                double mass_scale, double dt, double* __restrict__ t_out,
                                                                double* __restrict__ p_out, double* __restrict__ term)
{
    const int v = blockIdx.x * MEM_THREADS + threadIdx.x;
    if (v >= nV) return;
    double t[3], p[3], d[3], fe[3];
#pragma unroll
    for (int l = 0; l < 3; l++) {
        const size_t e = 3 * (size_t)v + l;
        t[l] = dx ? qdot[e] + step * dx[e] : qdot[e];
        p[l] = pos0[e] + dt * t[l];
        d[l] = t[l] - qdot0[e];
        fe[l] = fext[e];
        t_out[e] = t[l];
        p_out[e] = p[l];
    }
    const double work = (p[0] * fe[0] + p[1] * fe[1]) + p[2] * fe[2];
    const double d2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2];
    term[v] = work + 0.5 * ((mass_scale * mass0[v]) * d2);
}

// term[v] = a_v . b_v (xyz rows)
__global__ __launch_bounds__(MEM_THREADS) void k_membrane_dot3(int nV, const double* __restrict__ a, const double* __restrict__ b, double* __restrict__ term)
{
    const int v = blockIdx.x * MEM_THREADS + threadIdx.x;
    if (v >= nV) return;
    const size_t e = 3 * (size_t)v;
    term[v] = (a[e] * b[e] + a[e + 1] * b[e + 1]) + a[e + 2] * b[e + 2];
}

hipError_t launch_membrane_rest(int nF, const int* F, const double* V0, double thickness, double* rest, hipStream_t st)
{
    if (nF <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_membrane_rest, dim3(mem_grid(nF, MEM_THREADS)), dim3(MEM_THREADS), 0, st, nF, F, V0, thickness, rest);
    return hipGetLastError();
}

hipError_t launch_membrane_faces(int mode, int nF, const int* F, const double* P, const double* rest, double alpha, double beta, double floor,
                                 double value, double* W, double* G, double* H, hipStream_t st)
{
    if (nF <= 0) return hipSuccess;
    const dim3 grid(mem_grid(nF, MEM_FACE_THREADS)), block(MEM_FACE_THREADS);
    if (mode == 0) hipLaunchKernelGGL(k_membrane_faces<0>, grid, block, 0, st, nF, F, P, rest, alpha, beta, floor, value, W, G, H);
    else if (mode == 1) hipLaunchKernelGGL(k_membrane_faces<1>, grid, block, 0, st, nF, F, P, rest, alpha, beta, floor, value, W, G, H);
    else hipLaunchKernelGGL(k_membrane_faces<2>, grid, block, 0, st, nF, F, P, rest, alpha, beta, floor, value, W, G, H);
    return hipGetLastError();
}

template <int MAT>
static hipError_t launch_faces_mat(int mode, int nF, const int* F, const double* P, const double* V0, double thickness, double alpha, double beta,
                                   double floor, double value, double* W, double* G, double* H, hipStream_t st)
{
    const dim3 grid(mem_grid(nF, MEM_FACE_THREADS)), block(MEM_FACE_THREADS);
    if (mode == 0) hipLaunchKernelGGL((k_membrane_faces_mat<0, MAT>), grid, block, 0, st, nF, F, P, V0, thickness, alpha, beta, floor, value, W, G, H);
    else if (mode == 1) hipLaunchKernelGGL((k_membrane_faces_mat<1, MAT>), grid, block, 0, st, nF, F, P, V0, thickness, alpha, beta, floor, value, W, G, H);
    else hipLaunchKernelGGL((k_membrane_faces_mat<2, MAT>), grid, block, 0, st, nF, F, P, V0, thickness, alpha, beta, floor, value, W, G, H);
    return hipGetLastError();
}

hipError_t launch_membrane_faces_material(int material, int mode, int nF, const int* F, const double* P, const double* V0, const double* rest,
                                          double thickness, double alpha, double beta, double floor, double value, double* W, double* G, double* H,
                                          hipStream_t st)
{
    if (nF <= 0) return hipSuccess;
    if (material == 0) return launch_membrane_faces(mode, nF, F, P, rest, alpha, beta, floor, value, W, G, H, st);
    if (material == 1) return launch_faces_mat<1>(mode, nF, F, P, V0, thickness, alpha, beta, floor, value, W, G, H, st);
    if (material == 2) return launch_faces_mat<2>(mode, nF, F, P, V0, thickness, alpha, beta, floor, value, W, G, H, st);
    return hipErrorInvalidValue;      // a material without kernels is an error, never another material's path
}

hipError_t launch_membrane_matrix(int nB, const int* brow, const int* bcol, const int* bptr, const int* c_ptr, const int* c_src, const double* H,
                                  int nF, double dt2, const double* mass0, double mass_scale, double* val, hipStream_t st)
{
    if (nB <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_membrane_matrix, dim3(mem_grid(nB, MEM_THREADS)), dim3(MEM_THREADS), 0, st, nB, brow, bcol, bptr, c_ptr, c_src, H, nF, dt2,
                       mass0, mass_scale, val);
    return hipGetLastError();
}

hipError_t launch_membrane_pressure(int nV, int nF, const int* F, const double* P, const int* m_ptr, const int* m_idx, double pressure, double* Qn,
                                    double* mass, double* fext, hipStream_t st)
{
    if (nV <= 0 || nF <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_membrane_pressure_faces, dim3(mem_grid(nF, MEM_THREADS)), dim3(MEM_THREADS), 0, st, nF, F, P, Qn);
    hipLaunchKernelGGL(k_membrane_pressure, dim3(mem_grid(nV, MEM_THREADS)), dim3(MEM_THREADS), 0, st, nV, m_ptr, m_idx, Qn, nF, pressure, mass, fext);
    return hipGetLastError();
}

hipError_t launch_membrane_gradient(int nV, const int* m_ptr, const int* m_idx, const double* G, int nF, const double* mass0, double mass_scale,
                                    double dt, const double* qdot, const double* qdot0, const double* fext, double* g, double* b, hipStream_t st)
{
    if (nV <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_membrane_gradient, dim3(mem_grid(nV, MEM_THREADS)), dim3(MEM_THREADS), 0, st, nV, m_ptr, m_idx, G, nF, mass0, mass_scale, dt,
                       qdot, qdot0, fext, g, b);
    return hipGetLastError();
}

hipError_t launch_membrane_trial(int nV, const double* qdot, const double* dx, double step, const double* qdot0, const double* pos0,
                                 const double* fext, const double* mass0, double mass_scale, double dt, double* t_out, double* p_out, double* term,
                                 hipStream_t st)
{
    if (nV <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_membrane_trial, dim3(mem_grid(nV, MEM_THREADS)), dim3(MEM_THREADS), 0, st, nV, qdot, dx, step, qdot0, pos0, fext, mass0,
                       mass_scale, dt, t_out, p_out, term);
    return hipGetLastError();
}

hipError_t launch_membrane_dot3(int nV, const double* a, const double* b, double* term, hipStream_t st)
{
    if (nV <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_membrane_dot3, dim3(mem_grid(nV, MEM_THREADS)), dim3(MEM_THREADS), 0, st, nV, a, b, term);
    return hipGetLastError();
}

}  // namespace smg
