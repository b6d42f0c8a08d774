// smg_pd_device.hip -- the kernels of the projective-dynamics membrane step (smg_pd_*, include/smg.h; host side in smg_pd.cpp; the per-face
// maths in smg_pd_inl.hpp).
//
// Layout: the state (x, v), the forces and the rest pose are xyz rows (entry 3 v + l); the iterate Q, the prediction S and the right-hand side
// B are the solver's column-major nV x 3 blocks (coordinate l of vertex v at [l * ld + v]).  The face kernels read a pose through two strides
// (sv between vertices, sl between coordinates), so they serve both.  Per-face arrays are face-major planes (plane e of face f at
// [e * nF + f]), so a wave's loads and stores of one plane are contiguous: the rest constants (4 planes: a, b, c, A_f), the corner shares
// (9 planes: 3 i + l), Fg and T (6 planes each), sigma (2 planes).
//
// Determinism: no atomics.  A face's sums are one lane's terms in a fixed order; a vertex's right-hand side is one lane's sequential loop over
// its corner list (faces ascending); the energy and the strain statistics are fixed-order reductions of per-face and per-vertex terms
// (launch_fixed_sum / launch_fixed_max, smg_fixed_sum_device.hip).
#include <hip/hip_runtime.h>

#include "smg_device.hpp"
#include "smg_pd_inl.hpp"

namespace smg {

namespace {

constexpr int PD_THREADS = 64;          // one wave per block: a face's work is short, and small meshes still fill many CUs

inline int pd_grid(long long n) { return (int)((n + PD_THREADS - 1) / PD_THREADS); }

__device__ __forceinline__ void pd_load_rest(const double* __restrict__ rest, int nF, int f, double (&r)[4])
{
#pragma unroll
    for (int e = 0; e < 4; e++) r[e] = rest[(size_t)e * nF + f];
}

}  // namespace

// One lane per face: the four rest constants as planes.
__global__ __launch_bounds__(PD_THREADS) void k_pd_rest(int nF, const int* __restrict__ F, const double* __restrict__ V0, double* __restrict__ rest)
{
    const int f = blockIdx.x * PD_THREADS + threadIdx.x;
    if (f >= nF) return;
    double r[4];
    pd_rest(V0 + 3 * (size_t)F[3 * (size_t)f], V0 + 3 * (size_t)F[3 * (size_t)f + 1], V0 + 3 * (size_t)F[3 * (size_t)f + 2], r);
#pragma unroll
    for (int e = 0; e < 4; e++) rest[(size_t)e * nF + f] = r[e];
}

// One lane per face, one pass over the three gathers of the pose Q: F_f, its projection T_f, eterm[f] = the face's energy term and
// share[(3 i + l) * nF + f] = k A_f (T_f g_i)_l.  MODE 0 is the step; MODE 1 (the hook and the strain query) also stores Fg, sigma and T.
template <int MODE>
__global__ __launch_bounds__(PD_THREADS) void k_pd_faces(int nF, const int* __restrict__ F, const double* __restrict__ rest,
                                                         const double* __restrict__ Q, size_t sv, size_t sl, double k, double smin, double smax,
                                                         double* __restrict__ eterm, double* __restrict__ share, double* __restrict__ Fg_out,
                                                         double* __restrict__ sigma_out, double* __restrict__ T_out)
{
    const int f = blockIdx.x * PD_THREADS + threadIdx.x;
    if (f >= nF) return;
    double r[4], q[3][3], Fg[6], sigma[2], T[6], s[9];
    pd_load_rest(rest, nF, f, r);
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const size_t v = (size_t)F[3 * (size_t)f + i];
#pragma unroll
        for (int l = 0; l < 3; l++) q[i][l] = Q[v * sv + (size_t)l * sl];
    }
    pd_gradient(r, q[0], q[1], q[2], Fg);
    pd_project(Fg, smin, smax, sigma, T);
    eterm[f] = pd_face_energy(r, k, Fg, T);
    pd_corner_shares(r, k, T, s);
#pragma unroll
    for (int e = 0; e < 9; e++) share[(size_t)e * nF + f] = s[e];
    if (MODE == 1) {
#pragma unroll
        for (int e = 0; e < 6; e++) {
            Fg_out[(size_t)e * nF + f] = Fg[e];
            T_out[(size_t)e * nF + f] = T[e];
        }
        sigma_out[f] = sigma[0];
        sigma_out[(size_t)nF + f] = sigma[1];
    }
}

// One lane per face: the 5 planes the strain statistics reduce, from the planes of k_pd_faces<1>: sigma1, -sigma2, outside the band (0 / 1:
// sigma1 > sigma_max or sigma2 < sigma_min), A_f |F - T|_F^2, A_f.
__global__ __launch_bounds__(PD_THREADS) void k_pd_strain_terms(int nF, const double* __restrict__ rest, const double* __restrict__ Fg,
                                                                const double* __restrict__ sigma, const double* __restrict__ T, double smin,
                                                                double smax, double* __restrict__ terms)
{
    const int f = blockIdx.x * PD_THREADS + threadIdx.x;
    if (f >= nF) return;
    double a[6], t[6];
#pragma unroll
    for (int e = 0; e < 6; e++) {
        a[e] = Fg[(size_t)e * nF + f];
        t[e] = T[(size_t)e * nF + f];
    }
    const double s1 = sigma[f], s2 = sigma[(size_t)nF + f], A = rest[3 * (size_t)nF + f];
    terms[f] = s1;
    terms[(size_t)nF + f] = 0.0 - s2;
    terms[2 * (size_t)nF + f] = (s1 > smax || s2 < smin) ? 1.0 : 0.0;
    terms[3 * (size_t)nF + f] = A * pd_distance2(a, t);
    terms[4 * (size_t)nF + f] = A;
}

// One lane per vertex: the prediction S (column-major) of the step from (x, v): f_v = -fext_v + (rho m0_v) g with fext the pressure force of
// launch_membrane_pressure at x, s_v = (x_v + h v_v) + (h^2 f_v) / (rho m0_v).
__global__ __launch_bounds__(PD_THREADS) void k_pd_predict(int nV, const double* __restrict__ x, const double* __restrict__ vel,
                                                           const double* __restrict__ fext, const double* __restrict__ m0, double h, double rho,
                                                           double gx, double gy, double gz, double* __restrict__ S, int ld)
{
    const int v = blockIdx.x * PD_THREADS + threadIdx.x;
    if (v >= nV) return;
    const double rm = rho * m0[v], h2 = h * h;
    const double g[3] = {gx, gy, gz};
#pragma unroll
    for (int l = 0; l < 3; l++) {
        const double fv = (0.0 - fext[3 * (size_t)v + l]) + rm * g[l];
        S[(size_t)l * ld + v] = (x[3 * (size_t)v + l] + h * vel[3 * (size_t)v + l]) + (h2 * fv) / rm;
    }
}

// One lane per vertex over its corner list (t = 3 f + i, faces ascending): with w_v = c_mass m0_v (c_mass = rho / h^2, the coefficient the
// matrix was assembled with), B_v = w_v s_v + the sum of the corner shares in list order (one accumulator from 0), iterm[v] = (w_v / 2) |q_v - s_v|^2
// and bsq[v] = |B_v|^2.
__global__ __launch_bounds__(PD_THREADS) void k_pd_vertices(int nV, int nF, const int* __restrict__ m_ptr, const int* __restrict__ m_idx,
                                                            const double* __restrict__ share, const double* __restrict__ m0, double c_mass,
                                                            const double* __restrict__ S, const double* __restrict__ Q, int ld,
                                                            double* __restrict__ B, int ldb, double* __restrict__ iterm, double* __restrict__ bsq)
{
    const int v = blockIdx.x * PD_THREADS + threadIdx.x;
    if (v >= nV) return;
    double acc[3] = {0.0, 0.0, 0.0};
    const int p1 = m_ptr[v + 1];
    for (int p = m_ptr[v]; p < p1; p++) {
        const int t = m_idx[p], f = t / 3, i = t - 3 * f;
#pragma unroll
        for (int l = 0; l < 3; l++) acc[l] += share[(size_t)(3 * i + l) * nF + f];
    }
    const double w = c_mass * m0[v];
    double b[3], dq[3];
#pragma unroll
    for (int l = 0; l < 3; l++) {
        const double s = S[(size_t)l * ld + v];
        b[l] = w * s + acc[l];
        dq[l] = Q[(size_t)l * ld + v] - s;
        B[(size_t)l * ldb + v] = b[l];
    }
    iterm[v] = (0.5 * w) * ((dq[0] * dq[0] + dq[1] * dq[1]) + dq[2] * dq[2]);
    bsq[v] = (b[0] * b[0] + b[1] * b[1]) + b[2] * b[2];
}

// One lane per vertex: v = (q - x) / h, x = q.
__global__ __launch_bounds__(PD_THREADS) void k_pd_finish(int nV, const double* __restrict__ Q, int ld, double h, double* __restrict__ x,
                                                          double* __restrict__ vel)
{
    const int v = blockIdx.x * PD_THREADS + threadIdx.x;
    if (v >= nV) return;
#pragma unroll
    for (int l = 0; l < 3; l++) {
        const double q = Q[(size_t)l * ld + v];
        vel[3 * (size_t)v + l] = (q - x[3 * (size_t)v + l]) / h;
        x[3 * (size_t)v + l] = q;
    }
}

hipError_t launch_pd_rest(int nF, const int* F, const double* V0, double* rest, hipStream_t st)
{
    if (nF <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_pd_rest, dim3(pd_grid(nF)), dim3(PD_THREADS), 0, st, nF, F, V0, rest);
    return hipGetLastError();
}

hipError_t launch_pd_faces(int nF, const int* F, const double* rest, const double* Q, size_t sv, size_t sl, double k, double smin, double smax,
                           double* eterm, double* share, double* Fg, double* sigma, double* T, hipStream_t st)
{
    if (nF <= 0) return hipSuccess;
    if (Fg || sigma || T) {
        if (!Fg || !sigma || !T) return hipErrorInvalidValue;
        hipLaunchKernelGGL(k_pd_faces<1>, dim3(pd_grid(nF)), dim3(PD_THREADS), 0, st, nF, F, rest, Q, sv, sl, k, smin, smax, eterm, share, Fg, sigma, T);
    } else {
        hipLaunchKernelGGL(k_pd_faces<0>, dim3(pd_grid(nF)), dim3(PD_THREADS), 0, st, nF, F, rest, Q, sv, sl, k, smin, smax, eterm, share, nullptr,
                           nullptr, nullptr);
    }
    return hipGetLastError();
}

hipError_t launch_pd_strain_terms(int nF, const double* rest, const double* Fg, const double* sigma, const double* T, double smin, double smax,
                                  double* terms, hipStream_t st)
{
    if (nF <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_pd_strain_terms, dim3(pd_grid(nF)), dim3(PD_THREADS), 0, st, nF, rest, Fg, sigma, T, smin, smax, terms);
    return hipGetLastError();
}

hipError_t launch_pd_predict(int nV, const double* x, const double* vel, const double* fext, const double* m0, double h, double rho, const double* g,
                             double* S, int ld, hipStream_t st)
{
    if (nV <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_pd_predict, dim3(pd_grid(nV)), dim3(PD_THREADS), 0, st, nV, x, vel, fext, m0, h, rho, g[0], g[1], g[2], S, ld);
    return hipGetLastError();
}

hipError_t launch_pd_vertices(int nV, int nF, const int* m_ptr, const int* m_idx, const double* share, const double* m0, double c_mass, const double* S,
                              const double* Q, int ld, double* B, int ldb, double* iterm, double* bsq, hipStream_t st)
{
    if (nV <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_pd_vertices, dim3(pd_grid(nV)), dim3(PD_THREADS), 0, st, nV, nF, m_ptr, m_idx, share, m0, c_mass, S, Q, ld, B, ldb, iterm, bsq);
    return hipGetLastError();
}

hipError_t launch_pd_finish(int nV, const double* Q, int ld, double h, double* x, double* vel, hipStream_t st)
{
    if (nV <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_pd_finish, dim3(pd_grid(nV)), dim3(PD_THREADS), 0, st, nV, Q, ld, h, x, vel);
    return hipGetLastError();
}

}  // namespace smg
