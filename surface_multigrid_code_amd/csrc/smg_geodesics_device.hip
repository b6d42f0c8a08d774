// smg_geodesics_device.hip -- the three small kernels of the heat-method geodesic distance (smg_geodesics_solve, include/smg.h; host side in
// smg_geodesics.cpp) and the per-face gradient basis its create step builds.  Blocks are the caller's layout: column-major n x k with a
// leading dimension, column c of vertex i at c * ld + i.
//
// Determinism: no atomics.  The divergence sums a vertex's incident corners in the order of the corner list (AssemblyPlan::m_ptr / m_idx:
// faces ascending), the shift sums a column's sources in list order; every sum is one lane's sequential loop, so the same inputs give the
// same bits.  Expressions are written operation by operation (the library is built with -ffp-contract=off): tests/test_geodesics_host.py
// restates them in numpy in the same order.
#include <hip/hip_runtime.h>

#include "smg_device.hpp"

namespace smg {

namespace {

constexpr int GEO_THREADS = 256;

inline int geo_grid(long long n) { return (int)((n + GEO_THREADS - 1) / GEO_THREADS); }

}  // namespace

// W[9f + 3i + d] = d-th component of (n x e_i) / (2A), the gradient of the hat function of corner i on face f; Af[f] = A.
// e_i is the edge opposite corner i, counter-clockwise (e_0 = x_2 - x_1, e_1 = x_0 - x_2, e_2 = x_1 - x_0), n the unit normal.
__global__ __launch_bounds__(GEO_THREADS) void k_geo_basis(const double* __restrict__ V, const int* __restrict__ F, int nF, double* __restrict__ W,
                                                           double* __restrict__ Af)
{
    const int f = blockIdx.x * GEO_THREADS + threadIdx.x;
    if (f >= nF) return;
    const double* a = V + 3 * (size_t)F[3 * (size_t)f];
    const double* b = V + 3 * (size_t)F[3 * (size_t)f + 1];
    const double* c = V + 3 * (size_t)F[3 * (size_t)f + 2];
    const double ux = b[0] - a[0], uy = b[1] - a[1], uz = b[2] - a[2];
    const double vx = c[0] - a[0], vy = c[1] - a[1], vz = c[2] - a[2];
    const double wx = uy * vz - uz * vy, wy = uz * vx - ux * vz, wz = ux * vy - uy * vx;
    const double dA = sqrt(wx * wx + wy * wy + wz * wz);
    const double nx = wx / dA, ny = wy / dA, nz = wz / dA;
    const double e[3][3] = {{c[0] - b[0], c[1] - b[1], c[2] - b[2]}, {a[0] - c[0], a[1] - c[1], a[2] - c[2]}, {b[0] - a[0], b[1] - a[1], b[2] - a[2]}};
    double* w = W + 9 * (size_t)f;
#pragma unroll
    for (int i = 0; i < 3; i++) {
        w[3 * i + 0] = (ny * e[i][2] - nz * e[i][1]) / dA;
        w[3 * i + 1] = (nz * e[i][0] - nx * e[i][2]) / dA;
        w[3 * i + 2] = (nx * e[i][1] - ny * e[i][0]) / dA;
    }
    Af[f] = dA * 0.5;
}

// B[c * ldb + i] = 0 for i < n, c < k
__global__ __launch_bounds__(GEO_THREADS) void k_geo_clear(double* __restrict__ B, int n, int k, int ldb)
{
    const long long g = (long long)blockIdx.x * GEO_THREADS + threadIdx.x;
    if (g >= (long long)n * k) return;
    const int c = (int)(g / n), i = (int)(g - (long long)c * n);
    B[(size_t)c * ldb + i] = 0.0;
}

// one block per column: B[c * ldb + src[p]] = 1 for p in [src_ptr[c], src_ptr[c + 1])  (a repeated source writes the same 1)
__global__ __launch_bounds__(GEO_THREADS) void k_geo_sources(double* __restrict__ B, int ldb, const int* __restrict__ src_ptr, const int* __restrict__ src)
{
    const int c = blockIdx.x;
    for (int p = src_ptr[c] + (int)threadIdx.x; p < src_ptr[c + 1]; p += GEO_THREADS) B[(size_t)c * ldb + src[p]] = 1.0;
}

// One lane per (vertex v, column c).  For every corner t = 3f + j of v, in corner-list order: the face gradient g = sum_i u_i W_fi
// (i = 0, 1, 2 in order), X = -g / |g| (0 where |g| == 0), and the term A_f (W_fj . X).  out[c * ldo + v] = the sum of the terms =
// -(integrated divergence of X) at v, the right-hand side of -L phi = -div X.  The X field is never stored.
// Block order: the k blocks of one vertex block are adjacent in the grid (blockIdx.x = vb * k + c), so a vertex block's geometry
// (corner lists, faces, basis) is read for all columns while it is still in cache.
__global__ __launch_bounds__(GEO_THREADS) void k_geo_divergence(int n, int k, const int* __restrict__ F, const double* __restrict__ W,
                                                                const double* __restrict__ Af, const int* __restrict__ m_ptr,
                                                                const int* __restrict__ m_idx, const double* __restrict__ U, int ldu,
                                                                double* __restrict__ out, int ldo)
{
    const int c = (int)(blockIdx.x % (unsigned)k);
    const int v = (int)(blockIdx.x / (unsigned)k) * GEO_THREADS + (int)threadIdx.x;
    if (v >= n) return;
    const double* u = U + (size_t)c * ldu;
    double acc = 0.0;
    const int p1 = m_ptr[v + 1];
    for (int p = m_ptr[v]; p < p1; p++) {
        const int t = m_idx[p];
        const int f = t / 3, j = t - 3 * f;
        const double* w = W + 9 * (size_t)f;
        const double u0 = u[F[3 * (size_t)f]], u1 = u[F[3 * (size_t)f + 1]], u2 = u[F[3 * (size_t)f + 2]];
        const double gx = u0 * w[0] + u1 * w[3] + u2 * w[6];
        const double gy = u0 * w[1] + u1 * w[4] + u2 * w[7];
        const double gz = u0 * w[2] + u1 * w[5] + u2 * w[8];
        const double nrm = sqrt(gx * gx + gy * gy + gz * gz);
        double Xx = 0.0, Xy = 0.0, Xz = 0.0;
        if (nrm > 0.0) { Xx = -gx / nrm; Xy = -gy / nrm; Xz = -gz / nrm; }
        const double dot = w[3 * j] * Xx + w[3 * j + 1] * Xy + w[3 * j + 2] * Xz;
        acc += Af[f] * dot;
    }
    out[(size_t)c * ldo + v] = acc;
}

// mean[c] = (sum of phi[c * ldp + src[p]] over the column's sources, in list order) / (their count)
__global__ __launch_bounds__(64) void k_geo_source_mean(int k, const double* __restrict__ phi, int ldp, const int* __restrict__ src_ptr,
                                                        const int* __restrict__ src, double* __restrict__ mean)
{
    const int c = blockIdx.x * 64 + threadIdx.x;
    if (c >= k) return;
    const double* ph = phi + (size_t)c * ldp;
    double s = 0.0;
    const int p0 = src_ptr[c], p1 = src_ptr[c + 1];
    for (int p = p0; p < p1; p++) s += ph[src[p]];
    mean[c] = s / (double)(p1 - p0);
}

// D[c * ldd + i] = phi[c * ldp + i] - mean[c]
__global__ __launch_bounds__(GEO_THREADS) void k_geo_shift(int n, int k, const double* __restrict__ phi, int ldp, const double* __restrict__ mean,
                                                           double* __restrict__ D, int ldd)
{
    const long long g = (long long)blockIdx.x * GEO_THREADS + threadIdx.x;
    if (g >= (long long)n * k) return;
    const int c = (int)(g / n), i = (int)(g - (long long)c * n);
    D[(size_t)c * ldd + i] = phi[(size_t)c * ldp + i] - mean[c];
}

hipError_t launch_geo_basis(const double* V, const int* F, int nF, double* W, double* Af, hipStream_t st)
{
    if (nF <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_geo_basis, dim3(geo_grid(nF)), dim3(GEO_THREADS), 0, st, V, F, nF, W, Af);
    return hipGetLastError();
}

hipError_t launch_geo_scatter(int n, int k, const int* src_ptr, const int* src, double* B, int ldb, hipStream_t st)
{
    if (n <= 0 || k <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_geo_clear, dim3(geo_grid((long long)n * k)), dim3(GEO_THREADS), 0, st, B, n, k, ldb);
    hipLaunchKernelGGL(k_geo_sources, dim3(k), dim3(GEO_THREADS), 0, st, B, ldb, src_ptr, src);
    return hipGetLastError();
}

hipError_t launch_geo_divergence(int n, int k, const int* F, const double* W, const double* Af, const int* m_ptr, const int* m_idx,
                                 const double* U, int ldu, double* out, int ldo, hipStream_t st)
{
    if (n <= 0 || k <= 0) return hipSuccess;
    const long long blocks = (long long)geo_grid(n) * k;
    if (blocks > 0x7fffffffLL) return hipErrorInvalidConfiguration;
    hipLaunchKernelGGL(k_geo_divergence, dim3((unsigned)blocks), dim3(GEO_THREADS), 0, st, n, k, F, W, Af, m_ptr, m_idx, U, ldu, out, ldo);
    return hipGetLastError();
}

hipError_t launch_geo_shift(int n, int k, const int* src_ptr, const int* src, const double* phi, int ldp, double* mean, double* D, int ldd,
                            hipStream_t st)
{
    if (n <= 0 || k <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_geo_source_mean, dim3((k + 63) / 64), dim3(64), 0, st, k, phi, ldp, src_ptr, src, mean);
    hipLaunchKernelGGL(k_geo_shift, dim3(geo_grid((long long)n * k)), dim3(GEO_THREADS), 0, st, n, k, phi, ldp, mean, D, ldd);
    return hipGetLastError();
}

}  // namespace smg
