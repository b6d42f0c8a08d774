// smg_arap_device.hip -- the local step of as-rigid-as-possible deformation (smg_arap_solve, include/smg.h; host side in smg_arap.cpp;
// DESIGN.md section 19).  The matrix is the CSR of the rest pose's cotangent matrix L (diagonal included and skipped: N(i) = the
// off-diagonal entries of row i in stored order, w_ij = L_ij).
//
// Layout: rest positions P0 and current positions P are xyz rows (3 doubles per vertex), rotations are 9 contiguous doubles per vertex
// (row-major), so a neighbour costs one gather per array.  The solver's blocks are column-major n x 3 (column c of vertex i at c * ld + i);
// k_arap_rhs writes one, k_arap_rows / k_arap_columns convert between the two as plain streams.
//
// Determinism: no atomics.  Every per-vertex sum is one lane's sequential loop in the row's stored order; the energy is the fixed-order sum
// of the vertices' terms (launch_fixed_sum, smg_fixed_sum_device.hip).  Expressions are written
// operation by operation (-ffp-contract=off): tests/test_arap_host.py restates them in numpy in the same order.
#include <hip/hip_runtime.h>

#include "smg_arap_inl.hpp"
#include "smg_device.hpp"

namespace smg {

namespace {

constexpr int ARAP_THREADS = 256;

inline int arap_grid(long long n) { return (int)((n + ARAP_THREADS - 1) / ARAP_THREADS); }

// S_i = sum_j w_ij e_ij e'_ij^T (entry (a, c) = sum_j (w_ij e_a) e'_c), row i walked once in stored order
__device__ __forceinline__ void arap_covariance(int i, const int* __restrict__ rowptr, const int* __restrict__ col, const double* __restrict__ w,
                                                const double* __restrict__ P0, const double* __restrict__ P, double (&S)[9])
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

// sum_j w_ij |e'_ij - R e_ij|^2, row i walked once in stored order
__device__ __forceinline__ double arap_vertex_energy(int i, const int* __restrict__ rowptr, const int* __restrict__ col, const double* __restrict__ w,
                                                     const double* __restrict__ P0, const double* __restrict__ P, const double (&R)[9])
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

}  // namespace

// One lane per vertex.  MODE 0: out9 = S_i (the hook's covariance op).  MODE 1 (k_arap_rotations proper): out9 = R_i, the closest rotation of
// S_i, and eterm[i] = the vertex's energy term with that rotation.  MODE 2: eterm[i] from the given rotations R_in (the hook's energy op).
template <int MODE>
__global__ __launch_bounds__(ARAP_THREADS) void k_arap_rotations(int n, const int* __restrict__ rowptr, const int* __restrict__ col,
                                                                 const double* __restrict__ w, const double* __restrict__ P0,
                                                                 const double* __restrict__ P, const double* __restrict__ R_in,
                                                                 double* __restrict__ out9, double* __restrict__ eterm)
{
    const int i = blockIdx.x * ARAP_THREADS + threadIdx.x;
    if (i >= n) return;
    double R[9];
    if (MODE == 2) {
#pragma unroll
        for (int e = 0; e < 9; e++) R[e] = R_in[9 * (size_t)i + e];
    } else {
        double S[9];
        arap_covariance(i, rowptr, col, w, P0, P, S);
        if (MODE == 0) {
#pragma unroll
            for (int e = 0; e < 9; e++) out9[9 * (size_t)i + e] = S[e];
            return;
        }
        arap_closest_rotation(S, R);
#pragma unroll
        for (int e = 0; e < 9; e++) out9[9 * (size_t)i + e] = R[e];
    }
    eterm[i] = arap_vertex_energy(i, rowptr, col, w, P0, P, R);
}

// b_i = sum_j (w_ij / 2) (R_i + R_j) e_ij in stored order, written as the column-major n x 3 block the solve reads
__global__ __launch_bounds__(ARAP_THREADS) void k_arap_rhs(int n, const int* __restrict__ rowptr, const int* __restrict__ col,
                                                           const double* __restrict__ w, const double* __restrict__ P0,
                                                           const double* __restrict__ R, double* __restrict__ B, int ldb)
{
    const int i = blockIdx.x * ARAP_THREADS + threadIdx.x;
    if (i >= n) return;
    double Ri[9];
#pragma unroll
    for (int e = 0; e < 9; e++) Ri[e] = R[9 * (size_t)i + e];
    const double p0x = P0[3 * (size_t)i], p0y = P0[3 * (size_t)i + 1], p0z = P0[3 * (size_t)i + 2];
    double bx = 0.0, by = 0.0, bz = 0.0;
    const int q1 = rowptr[i + 1];
    for (int q = rowptr[i]; q < q1; q++) {
        const int j = col[q];
        if (j == i) continue;
        const double* r0 = P0 + 3 * (size_t)j;
        const double* Rj = R + 9 * (size_t)j;
        const double ex = p0x - r0[0], ey = p0y - r0[1], ez = p0z - r0[2];
        const double h = w[q] * 0.5;
        bx += h * ((Ri[0] + Rj[0]) * ex + (Ri[1] + Rj[1]) * ey + (Ri[2] + Rj[2]) * ez);
        by += h * ((Ri[3] + Rj[3]) * ex + (Ri[4] + Rj[4]) * ey + (Ri[5] + Rj[5]) * ez);
        bz += h * ((Ri[6] + Rj[6]) * ex + (Ri[7] + Rj[7]) * ey + (Ri[8] + Rj[8]) * ez);
    }
    B[i] = bx;
    B[(size_t)ldb + i] = by;
    B[2 * (size_t)ldb + i] = bz;
}

// P (xyz rows) = U (column-major n x 3)
__global__ __launch_bounds__(ARAP_THREADS) void k_arap_rows(int n, const double* __restrict__ U, int ldu, double* __restrict__ P)
{
    const int i = blockIdx.x * ARAP_THREADS + threadIdx.x;
    if (i >= n) return;
    P[3 * (size_t)i] = U[i];
    P[3 * (size_t)i + 1] = U[(size_t)ldu + i];
    P[3 * (size_t)i + 2] = U[2 * (size_t)ldu + i];
}

// U (column-major n x 3) = P (xyz rows)
__global__ __launch_bounds__(ARAP_THREADS) void k_arap_columns(int n, const double* __restrict__ P, double* __restrict__ U, int ldu)
{
    const int i = blockIdx.x * ARAP_THREADS + threadIdx.x;
    if (i >= n) return;
    U[i] = P[3 * (size_t)i];
    U[(size_t)ldu + i] = P[3 * (size_t)i + 1];
    U[2 * (size_t)ldu + i] = P[3 * (size_t)i + 2];
}

// U[c * ldu + handles[r]] = hp[c * ldh + r]: the handle rows of an iterate are the handle positions
__global__ __launch_bounds__(ARAP_THREADS) void k_arap_set_handles(int nh, const int* __restrict__ handles, const double* __restrict__ hp, int ldh,
                                                                   double* __restrict__ U, int ldu)
{
    const int g = blockIdx.x * ARAP_THREADS + threadIdx.x;
    if (g >= 3 * nh) return;
    const int c = g / nh, r = g - c * nh;
    U[(size_t)c * ldu + handles[r]] = hp[(size_t)c * ldh + r];
}

hipError_t launch_arap_covariance(int n, const int* rowptr, const int* col, const double* w, const double* P0, const double* P, double* S, hipStream_t st)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_arap_rotations<0>, dim3(arap_grid(n)), dim3(ARAP_THREADS), 0, st, n, rowptr, col, w, P0, P, nullptr, S, nullptr);
    return hipGetLastError();
}

hipError_t launch_arap_rotations(int n, const int* rowptr, const int* col, const double* w, const double* P0, const double* P, double* R, double* eterm,
                                 hipStream_t st)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_arap_rotations<1>, dim3(arap_grid(n)), dim3(ARAP_THREADS), 0, st, n, rowptr, col, w, P0, P, nullptr, R, eterm);
    return hipGetLastError();
}

hipError_t launch_arap_vertex_energy(int n, const int* rowptr, const int* col, const double* w, const double* P0, const double* P, const double* R,
                                     double* eterm, hipStream_t st)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_arap_rotations<2>, dim3(arap_grid(n)), dim3(ARAP_THREADS), 0, st, n, rowptr, col, w, P0, P, R, nullptr, eterm);
    return hipGetLastError();
}

hipError_t launch_arap_rhs(int n, const int* rowptr, const int* col, const double* w, const double* P0, const double* R, double* B, int ldb, hipStream_t st)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_arap_rhs, dim3(arap_grid(n)), dim3(ARAP_THREADS), 0, st, n, rowptr, col, w, P0, R, B, ldb);
    return hipGetLastError();
}

hipError_t launch_arap_rows(int n, const double* U, int ldu, double* P, hipStream_t st)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_arap_rows, dim3(arap_grid(n)), dim3(ARAP_THREADS), 0, st, n, U, ldu, P);
    return hipGetLastError();
}

hipError_t launch_arap_columns(int n, const double* P, double* U, int ldu, hipStream_t st)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_arap_columns, dim3(arap_grid(n)), dim3(ARAP_THREADS), 0, st, n, P, U, ldu);
    return hipGetLastError();
}

hipError_t launch_arap_set_handles(int nh, const int* handles, const double* hp, int ldh, double* U, int ldu, hipStream_t st)
{
    if (nh <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_arap_set_handles, dim3(arap_grid(3LL * nh)), dim3(ARAP_THREADS), 0, st, nh, handles, hp, ldh, U, ldu);
    return hipGetLastError();
}

}  // namespace smg
