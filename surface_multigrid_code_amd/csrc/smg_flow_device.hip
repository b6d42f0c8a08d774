// smg_flow_device.hip -- the kernels of the conformalized mean-curvature flow and its sphere map (smg_flow_*, include/smg.h; host side in
// smg_flow.cpp; the arithmetic in smg_flow_inl.hpp).
//
// Layout: positions are column-major nV x 3 blocks with a leading dimension, the solver's own layout, so the state is the solve's start and its
// result without a transpose and a lane's own three coordinates are three coalesced loads.  Per-face and per-vertex terms are planes.
//
// Determinism: no atomics.  A vertex's mass is one lane's sequential loop over its corner list (faces ascending: k_mass_diag's order, the bits of
// smg_mesh_massmatrix and of smg_assemble's diagonal); every other sum goes through launch_fixed_sum / launch_fixed_max.  A kernel that needs a
// sum reads it from the small device block `s` the sums were written to: nothing but the sphericity itself ever reaches the host.  Expressions
// are written operation by operation (-ffp-contract=off): tests/flow_np.py restates them in numpy in the same order.  Only +, -, *, / and sqrt.
//
// The block of sums, `s` (FLOW_SUMS doubles): [0] the sphericity, [1] sum a, [2..4] sum a U, [5] sum a r, [6] sum a (r - rbar)^2;
// [8] the sum of double areas, [9] sum x, [10] sum y, [11] max(-z) of the divided columns; [12..15] the four stats reductions of the sphere map.
#include <hip/hip_runtime.h>

#include "smg_device.hpp"
#include "smg_flow_inl.hpp"

namespace smg {

namespace {

constexpr int FLOW_THREADS = 256;

inline int flow_grid(int n) { return (n + FLOW_THREADS - 1) / FLOW_THREADS; }

}  // namespace

// One lane per vertex: reads U once; writes the barycentric mass, the right-hand side mass * U and the row's values of M_t - delta L_0.
// HAVE_MASS: the masses of this very U were just formed by k_flow_mass_terms (the step measures the sphericity first); they are read from
// mass_in instead of being gathered again -- the same function of the same U, so the same bits.
template <bool HAVE_MASS>
__global__ __launch_bounds__(FLOW_THREADS) void k_flow_system(int n, const double* __restrict__ U, int ldu, const int* __restrict__ F,
                                                              const int* __restrict__ m_ptr, const int* __restrict__ m_idx,
                                                              const int* __restrict__ rowptr, const int* __restrict__ diag,
                                                              const double* __restrict__ L0, double neg_delta, const double* __restrict__ mass_in,
                                                              double* __restrict__ mass, double* __restrict__ B, int ldb, double* __restrict__ val)
{
    const int v = blockIdx.x * FLOW_THREADS + threadIdx.x;
    if (v >= n) return;
    const double m = HAVE_MASS ? mass_in[v] : flow_mass(U, (size_t)ldu, F, m_ptr, m_idx, v);
    mass[v] = m;
#pragma unroll
    for (int d = 0; d < 3; d++) B[(size_t)d * ldb + v] = m * U[(size_t)d * ldu + v];
    const int j1 = rowptr[v + 1], jd = diag[v];
    for (int j = rowptr[v]; j < j1; j++) val[j] = flow_entry(neg_delta, L0[j], m, j == jd);
}

// term[f] = twice the area of face f
__global__ __launch_bounds__(FLOW_THREADS) void k_flow_face_area(int nF, const double* __restrict__ U, int ldu, const int* __restrict__ F,
                                                                 double* __restrict__ term)
{
    const int f = blockIdx.x * FLOW_THREADS + threadIdx.x;
    if (f >= nF) return;
    term[f] = flow_face_darea(U, (size_t)ldu, F, (size_t)f);
}

// out = U / sqrt(s[8] / 2); negz = 0 - the divided z
__global__ __launch_bounds__(FLOW_THREADS) void k_flow_divide(int n, const double* __restrict__ U, int ldu, const double* __restrict__ s,
                                                              double* __restrict__ out, int ldo, double* __restrict__ negz)
{
    const int i = blockIdx.x * FLOW_THREADS + threadIdx.x;
    if (i >= n) return;
    const double scale = sqrt(s[8] / 2.0);
    const double x = U[i] / scale, y = U[(size_t)ldu + i] / scale, z = U[2 * (size_t)ldu + i] / scale;
    out[i] = x;
    out[(size_t)ldo + i] = y;
    out[2 * (size_t)ldo + i] = z;
    negz[i] = 0.0 - z;
}

// out: x and y minus their means, z minus its minimum
__global__ __launch_bounds__(FLOW_THREADS) void k_flow_shift(int n, const double* __restrict__ s, double* __restrict__ out, int ldo)
{
    const int i = blockIdx.x * FLOW_THREADS + threadIdx.x;
    if (i >= n) return;
    const double mx = s[9] / (double)n, my = s[10] / (double)n, zmin = 0.0 - s[11];
    out[i] = out[i] - mx;
    out[(size_t)ldo + i] = out[(size_t)ldo + i] - my;
    out[2 * (size_t)ldo + i] = out[2 * (size_t)ldo + i] - zmin;
}

// a[v] = the barycentric mass of U; term: the three planes a U
__global__ __launch_bounds__(FLOW_THREADS) void k_flow_mass_terms(int n, const double* __restrict__ U, int ldu, const int* __restrict__ F,
                                                                  const int* __restrict__ m_ptr, const int* __restrict__ m_idx,
                                                                  double* __restrict__ a, double* __restrict__ term)
{
    const int v = blockIdx.x * FLOW_THREADS + threadIdx.x;
    if (v >= n) return;
    const double m = flow_mass(U, (size_t)ldu, F, m_ptr, m_idx, v);
    a[v] = m;
#pragma unroll
    for (int d = 0; d < 3; d++) term[(size_t)d * n + v] = m * U[(size_t)d * ldu + v];
}

// r[i] = |U_i - c|, c = s[2..4] / s[1]; term[i] = a r
__global__ __launch_bounds__(FLOW_THREADS) void k_flow_radius(int n, const double* __restrict__ U, int ldu, const double* __restrict__ a,
                                                              const double* __restrict__ s, double* __restrict__ r, double* __restrict__ term)
{
    const int i = blockIdx.x * FLOW_THREADS + threadIdx.x;
    if (i >= n) return;
    const double cx = s[2] / s[1], cy = s[3] / s[1], cz = s[4] / s[1];
    const double ri = flow_radius(U[i], U[(size_t)ldu + i], U[2 * (size_t)ldu + i], cx, cy, cz);
    r[i] = ri;
    term[i] = a[i] * ri;
}

// term[i] = a (r - rbar)^2, rbar = s[5] / s[1]
__global__ __launch_bounds__(FLOW_THREADS) void k_flow_deviation(int n, const double* __restrict__ a, const double* __restrict__ r,
                                                                 const double* __restrict__ s, double* __restrict__ term)
{
    const int i = blockIdx.x * FLOW_THREADS + threadIdx.x;
    if (i >= n) return;
    const double rbar = s[5] / s[1];
    const double d = r[i] - rbar;
    term[i] = a[i] * (d * d);
}

// s[0] = sqrt(s[6] / s[1]) / rbar
__global__ void k_flow_sphericity(double* __restrict__ s)
{
    const double rbar = s[5] / s[1];
    s[0] = sqrt(s[6] / s[1]) / rbar;
}

// S_i = (U_i - c) / r_i
__global__ __launch_bounds__(FLOW_THREADS) void k_flow_sphere_vertices(int n, const double* __restrict__ U, int ldu, const double* __restrict__ s,
                                                                       double* __restrict__ S, int lds)
{
    const int i = blockIdx.x * FLOW_THREADS + threadIdx.x;
    if (i >= n) return;
    const double cx = s[2] / s[1], cy = s[3] / s[1], cz = s[4] / s[1];
    const double x = U[i], y = U[(size_t)ldu + i], z = U[2 * (size_t)ldu + i];
    const double r = flow_radius(x, y, z, cx, cy, cz);
    S[i] = (x - cx) / r;
    S[(size_t)lds + i] = (y - cy) / r;
    S[2 * (size_t)lds + i] = (z - cz) / r;
}

// One lane per face: sigma (2 planes) of the Jacobian rest face -> sphere face; terms (4 planes): A sigma1 / sigma2, A, sigma1 / sigma2, flipped
__global__ __launch_bounds__(FLOW_THREADS) void k_flow_sphere_faces(int nF, const int* __restrict__ F, const double* __restrict__ V0, int ld0,
                                                                    const double* __restrict__ S, int lds, double* __restrict__ sigma,
                                                                    double* __restrict__ terms)
{
    const int f = blockIdx.x * FLOW_THREADS + threadIdx.x;
    if (f >= nF) return;
    double a[3], b[3], c[3], p[3], q[3], r[3], sg[2], fl;
    flow_corners(V0, (size_t)ld0, F, (size_t)f, a, b, c);
    flow_corners(S, (size_t)lds, F, (size_t)f, p, q, r);
    flow_sigma(a, b, c, p, q, r, sg, &fl);
    const double A = flow_darea(a, b, c) * 0.5, ratio = sg[0] / sg[1];
    const size_t nf = (size_t)nF;
    sigma[f] = sg[0];
    sigma[nf + f] = sg[1];
    terms[f] = A * ratio;
    terms[nf + f] = A;
    terms[2 * nf + f] = ratio;
    terms[3 * nf + f] = fl;
}

hipError_t launch_flow_system(int n, const double* U, int ldu, const int* F, const int* m_ptr, const int* m_idx, const int* rowptr, const int* diag,
                              const double* L0, double delta, const double* mass_in, double* mass, double* B, int ldb, double* val, hipStream_t st)
{
    if (n <= 0) return hipSuccess;
    if (mass_in)
        hipLaunchKernelGGL(k_flow_system<true>, dim3(flow_grid(n)), dim3(FLOW_THREADS), 0, st, n, U, ldu, F, m_ptr, m_idx, rowptr, diag, L0, -delta, mass_in,
                           mass, B, ldb, val);
    else
        hipLaunchKernelGGL(k_flow_system<false>, dim3(flow_grid(n)), dim3(FLOW_THREADS), 0, st, n, U, ldu, F, m_ptr, m_idx, rowptr, diag, L0, -delta, mass_in,
                           mass, B, ldb, val);
    return hipGetLastError();
}

hipError_t launch_flow_normalize(int n, int nF, const int* F, const double* U, int ldu, double* term, double* part, double* s, double* out, int ldo,
                                 hipStream_t st)
{
    if (n <= 0 || nF <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_flow_face_area, dim3(flow_grid(nF)), dim3(FLOW_THREADS), 0, st, nF, U, ldu, F, term);
    hipError_t e = launch_fixed_sum(term, nF, part, s + 8, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_flow_divide, dim3(flow_grid(n)), dim3(FLOW_THREADS), 0, st, n, U, ldu, s, out, ldo, term);
    if ((e = launch_fixed_sum(out, n, part, s + 9, st)) != hipSuccess) return e;
    if ((e = launch_fixed_sum(out + (size_t)ldo, n, part, s + 10, st)) != hipSuccess) return e;
    if ((e = launch_fixed_max(term, n, part, s + 11, st)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_flow_shift, dim3(flow_grid(n)), dim3(FLOW_THREADS), 0, st, n, s, out, ldo);
    return hipGetLastError();
}

hipError_t launch_flow_sphericity(int n, const double* U, int ldu, const int* F, const int* m_ptr, const int* m_idx, double* a, double* r, double* term,
                                  double* part, double* s, hipStream_t st)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_flow_mass_terms, dim3(flow_grid(n)), dim3(FLOW_THREADS), 0, st, n, U, ldu, F, m_ptr, m_idx, a, term);
    hipError_t e = launch_fixed_sum(a, n, part, s + 1, st);
    for (int d = 0; d < 3 && e == hipSuccess; d++) e = launch_fixed_sum(term + (size_t)d * n, n, part, s + 2 + d, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_flow_radius, dim3(flow_grid(n)), dim3(FLOW_THREADS), 0, st, n, U, ldu, a, s, r, term);
    if ((e = launch_fixed_sum(term, n, part, s + 5, st)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_flow_deviation, dim3(flow_grid(n)), dim3(FLOW_THREADS), 0, st, n, a, r, s, term);
    if ((e = launch_fixed_sum(term, n, part, s + 6, st)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_flow_sphericity, dim3(1), dim3(1), 0, st, s);
    return hipGetLastError();
}

hipError_t launch_flow_sphere(int n, int nF, const int* F, const double* U, int ldu, const double* V0, int ld0, const double* s_in, double* S, int lds,
                              double* sigma, double* terms, double* part, double* s_out, hipStream_t st)
{
    if (n <= 0 || nF <= 0) return hipSuccess;
    const size_t nf = (size_t)nF;
    hipLaunchKernelGGL(k_flow_sphere_vertices, dim3(flow_grid(n)), dim3(FLOW_THREADS), 0, st, n, U, ldu, s_in, S, lds);
    hipLaunchKernelGGL(k_flow_sphere_faces, dim3(flow_grid(nF)), dim3(FLOW_THREADS), 0, st, nF, F, V0, ld0, S, lds, sigma, terms);
    hipError_t e = launch_fixed_sum(terms, nF, part, s_out, st);
    if (e == hipSuccess) e = launch_fixed_sum(terms + nf, nF, part, s_out + 1, st);
    if (e == hipSuccess) e = launch_fixed_max(terms + 2 * nf, nF, part, s_out + 2, st);
    if (e == hipSuccess) e = launch_fixed_sum(terms + 3 * nf, nF, part, s_out + 3, st);
    return e;
}

}  // namespace smg
