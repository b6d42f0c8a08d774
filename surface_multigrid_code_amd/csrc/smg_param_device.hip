// smg_param_device.hip -- the kernels of the disk parameterization (smg_param_*, include/smg.h; host side in smg_param.cpp; the per-face
// maths in smg_param_inl.hpp).
//
// Layout: the map UV is the solver's column-major nV x 2 block (u of vertex v at UV[v], v at UV[ld + v]); per-face arrays are face-major
// planes (plane e of face f at [e * nF + f]), so a wave's loads and stores of one plane are contiguous: the rest constants (6 planes:
// a, b, c, c0, c1, c2), the rotations (2 planes: cos, sin), the covariance (4 planes), sigma (2 planes).  V0 is nV x 3 row-major.
//
// Determinism: no atomics.  A face's sums are one lane's three terms in corner order; a vertex's right-hand side is one lane's sequential
// loop over its corner list (faces ascending); the energy and the distortion statistics are fixed-order reductions of per-face terms
// (launch_fixed_sum / launch_fixed_max, smg_fixed_sum_device.hip).
#include <hip/hip_runtime.h>

#include "smg_device.hpp"
#include "smg_param_inl.hpp"

namespace smg {

namespace {

constexpr int PARAM_THREADS = 64;       // one wave per block: a face's work is short, and small meshes still fill many CUs

inline int param_grid(long long n) { return (int)((n + PARAM_THREADS - 1) / PARAM_THREADS); }

__device__ __forceinline__ void param_load_rest(const double* __restrict__ rest, int nF, int f, double (&r)[6])
{
#pragma unroll
    for (int e = 0; e < 6; e++) r[e] = rest[(size_t)e * nF + f];
}

__device__ __forceinline__ void param_gather_uv(const int* __restrict__ F, int f, const double* __restrict__ UV, int ld, double (&u)[3][2])
{
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const int v = F[3 * (size_t)f + i];
        u[i][0] = UV[v];
        u[i][1] = UV[(size_t)ld + v];
    }
}

}  // namespace

// One lane per face: the six rest constants as planes.
__global__ __launch_bounds__(PARAM_THREADS) void k_param_rest(int nF, const int* __restrict__ F, const double* __restrict__ V0, double* __restrict__ rest)
{
    const int f = blockIdx.x * PARAM_THREADS + threadIdx.x;
    if (f >= nF) return;
    double r[6];
    param_rest(V0 + 3 * (size_t)F[3 * (size_t)f], V0 + 3 * (size_t)F[3 * (size_t)f + 1], V0 + 3 * (size_t)F[3 * (size_t)f + 2], r);
#pragma unroll
    for (int e = 0; e < 6; e++) rest[(size_t)e * nF + f] = r[e];
}

// One lane per face, one pass over the three UV gathers.  MODE 0: out = S_f (4 planes; the hook's covariance op).  MODE 1 (k_param_local
// proper): out = R_f (2 planes: cos, sin), the rotation closest to S_f, and eterm[f] = the face's energy term with that rotation.  MODE 2:
// eterm[f] with the given rotations R_in (the hook's energy ops).
template <int MODE>
__global__ __launch_bounds__(PARAM_THREADS) void k_param_local(int nF, const int* __restrict__ F, const double* __restrict__ rest,
                                                               const double* __restrict__ UV, int ld, const double* __restrict__ R_in,
                                                               double* __restrict__ out, double* __restrict__ eterm)
{
    const int f = blockIdx.x * PARAM_THREADS + threadIdx.x;
    if (f >= nF) return;
    double r[6], u[3][2], cs, sn;
    param_load_rest(rest, nF, f, r);
    param_gather_uv(F, f, UV, ld, u);
    if (MODE == 2) {
        cs = R_in[f];
        sn = R_in[(size_t)nF + f];
    } else {
        double S[4];
        param_covariance(r, u, S);
        if (MODE == 0) {
#pragma unroll
            for (int e = 0; e < 4; e++) out[(size_t)e * nF + f] = S[e];
            return;
        }
        param_rotation(S, cs, sn);
        out[f] = cs;
        out[(size_t)nF + f] = sn;
    }
    eterm[f] = param_face_energy(r, u, cs, sn);
}

// One lane per vertex: B[v] (column-major nV x 2) = the sum over v's corners t = 3 f + i, in list order, of corner i's share of face f.
__global__ __launch_bounds__(PARAM_THREADS) void k_param_rhs(int nV, int nF, const int* __restrict__ m_ptr, const int* __restrict__ m_idx,
                                                             const double* __restrict__ rest, const double* __restrict__ R,
                                                             double* __restrict__ B, int ldb)
{
    const int v = blockIdx.x * PARAM_THREADS + threadIdx.x;
    if (v >= nV) return;
    double bx = 0.0, by = 0.0;
    const int q1 = m_ptr[v + 1];
    for (int q = m_ptr[v]; q < q1; q++) {
        const int t = m_idx[q], f = t / 3, i = t - 3 * f;
        double r[6], sx, sy;
        param_load_rest(rest, nF, f, r);
        param_corner_rhs(r, i, R[f], R[(size_t)nF + f], sx, sy);
        bx += sx;
        by += sy;
    }
    B[v] = bx;
    B[(size_t)ldb + v] = by;
}

// One lane per face: det J and the singular values of the map's Jacobian; out3 (optional, the hook's op) = det J, sigma1, sigma2 as planes;
// sigma (optional) = sigma1, sigma2 as planes; terms (optional) = the 7 planes the statistics reduce, with A the rest area, q = sigma1 / sigma2
// and ok = det J > 0: flipped (0 / 1), A, A q, A sigma1 sigma2, ok ? A (sigma1^2 + sigma2^2 + sigma1^-2 + sigma2^-2) : 0, ok ? A : 0, ok ? q : 0.
__global__ __launch_bounds__(PARAM_THREADS) void k_param_distortion(int nF, const int* __restrict__ F, const double* __restrict__ rest,
                                                                    const double* __restrict__ UV, int ld, double* __restrict__ out3,
                                                                    double* __restrict__ sigma, double* __restrict__ terms)
{
    const int f = blockIdx.x * PARAM_THREADS + threadIdx.x;
    if (f >= nF) return;
    double r[6], u[3][2], det, s1, s2;
    param_load_rest(rest, nF, f, r);
    param_gather_uv(F, f, UV, ld, u);
    param_distortion(r, u, det, s1, s2);
    if (out3) {
        out3[f] = det;
        out3[(size_t)nF + f] = s1;
        out3[2 * (size_t)nF + f] = s2;
    }
    if (sigma) {
        sigma[f] = s1;
        sigma[(size_t)nF + f] = s2;
    }
    if (terms) {
        const bool ok = det > 0.0;
        const double A = 0.5 * (r[0] * r[2]), q = s1 / s2;
        const double a1 = s1 * s1, a2 = s2 * s2;
        const double sd = ((a1 + a2) + 1.0 / a1) + 1.0 / a2;
        terms[f] = ok ? 0.0 : 1.0;
        terms[(size_t)nF + f] = A;
        terms[2 * (size_t)nF + f] = A * q;
        terms[3 * (size_t)nF + f] = A * (s1 * s2);
        terms[4 * (size_t)nF + f] = ok ? A * sd : 0.0;
        terms[5 * (size_t)nF + f] = ok ? A : 0.0;
        terms[6 * (size_t)nF + f] = ok ? q : 0.0;
    }
}

hipError_t launch_param_rest(int nF, const int* F, const double* V0, double* rest, hipStream_t st)
{
    if (nF <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_param_rest, dim3(param_grid(nF)), dim3(PARAM_THREADS), 0, st, nF, F, V0, rest);
    return hipGetLastError();
}

hipError_t launch_param_covariance(int nF, const int* F, const double* rest, const double* UV, int ld, double* S, hipStream_t st)
{
    if (nF <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_param_local<0>, dim3(param_grid(nF)), dim3(PARAM_THREADS), 0, st, nF, F, rest, UV, ld, nullptr, S, nullptr);
    return hipGetLastError();
}

hipError_t launch_param_local(int nF, const int* F, const double* rest, const double* UV, int ld, double* R, double* eterm, hipStream_t st)
{
    if (nF <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_param_local<1>, dim3(param_grid(nF)), dim3(PARAM_THREADS), 0, st, nF, F, rest, UV, ld, nullptr, R, eterm);
    return hipGetLastError();
}

hipError_t launch_param_face_energy(int nF, const int* F, const double* rest, const double* UV, int ld, const double* R, double* eterm, hipStream_t st)
{
    if (nF <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_param_local<2>, dim3(param_grid(nF)), dim3(PARAM_THREADS), 0, st, nF, F, rest, UV, ld, R, nullptr, eterm);
    return hipGetLastError();
}

hipError_t launch_param_rhs(int nV, int nF, const int* m_ptr, const int* m_idx, const double* rest, const double* R, double* B, int ldb, hipStream_t st)
{
    if (nV <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_param_rhs, dim3(param_grid(nV)), dim3(PARAM_THREADS), 0, st, nV, nF, m_ptr, m_idx, rest, R, B, ldb);
    return hipGetLastError();
}

hipError_t launch_param_distortion(int nF, const int* F, const double* rest, const double* UV, int ld, double* out3, double* sigma, double* terms,
                                   hipStream_t st)
{
    if (nF <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_param_distortion, dim3(param_grid(nF)), dim3(PARAM_THREADS), 0, st, nF, F, rest, UV, ld, out3, sigma, terms);
    return hipGetLastError();
}

}  // namespace smg
