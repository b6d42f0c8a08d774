// smg_denoise_device.hip -- the kernels of feature-preserving mesh denoising (smg_denoise_*, include/smg.h; host side in smg_denoise.cpp; the
// per-face maths in smg_denoise_inl.hpp).
//
// Layout: per-face arrays are face-major planes (plane e of face f at [e * nF + f]), so a wave's loads and stores of one plane are contiguous:
// the rest constants (10 planes: n, A, c, w), a normal field (3 planes), the corner shares (9 planes: 3 i + l).  The pose X is read through two
// strides (sv between vertices, sl between coordinates), so xyz rows and the solver's column-major blocks both serve.  N(f), the faces that
// share a vertex with f, is a CSR (nb_ptr, nb_idx) with ascending rows.
//
// The filter walks its row from global memory: a row is about 12 neighbours of 7 doubles each, the neighbours of the 64 faces of a wave overlap
// heavily (consecutive faces of a scan are close on the surface), and the planes of one iteration (7 x 8 nF bytes) are read-only while it runs,
// so the gathers are served by L2 and the vector cache; staging rows in LDS would copy each value once per reader and save no traffic.
//
// Determinism: no atomics.  A face's sums are one lane's terms in list order; the right-hand side is launch_pd_vertices' sequential loop over
// the corner list; the energy and the spacing are fixed-order reductions of per-face and per-vertex terms (launch_fixed_sum).
#include <hip/hip_runtime.h>

#include "smg_denoise_inl.hpp"
#include "smg_device.hpp"

namespace smg {

namespace {

constexpr int DN_THREADS = 64;          // one wave per block: a face's work is short, and small meshes still fill many CUs

inline int dn_grid(long long n) { return (int)((n + DN_THREADS - 1) / DN_THREADS); }

__device__ __forceinline__ void dn_load3(const double* __restrict__ planes, size_t nF, size_t f, double (&v)[3])
{
#pragma unroll
    for (int l = 0; l < 3; l++) v[l] = planes[(size_t)l * nF + f];
}

}  // namespace

// One lane per face: the ten rest constants as planes.
__global__ __launch_bounds__(DN_THREADS) void k_denoise_rest(int nF, const int* __restrict__ F, const double* __restrict__ V0, double* __restrict__ rest)
{
    const int f = blockIdx.x * DN_THREADS + threadIdx.x;
    if (f >= nF) return;
    double r[DN_REST];
    dn_rest(V0 + 3 * (size_t)F[3 * (size_t)f], V0 + 3 * (size_t)F[3 * (size_t)f + 1], V0 + 3 * (size_t)F[3 * (size_t)f + 2], r);
#pragma unroll
    for (int e = 0; e < DN_REST; e++) rest[(size_t)e * nF + f] = r[e];
}

// One lane per face over its row of N(f): term[f] = sum_g |c_f - c_g| in list order.
__global__ __launch_bounds__(DN_THREADS) void k_denoise_spacing(int nF, const int* __restrict__ nb_ptr, const int* __restrict__ nb_idx,
                                                                const double* __restrict__ rest, double* __restrict__ term)
{
    const int f = blockIdx.x * DN_THREADS + threadIdx.x;
    if (f >= nF) return;
    const double* __restrict__ cen = rest + 4 * (size_t)nF;
    double cf[3], cg[3], acc = 0.0;
    dn_load3(cen, (size_t)nF, (size_t)f, cf);
    const int p1 = nb_ptr[f + 1];
    for (int p = nb_ptr[f]; p < p1; p++) {
        dn_load3(cen, (size_t)nF, (size_t)nb_idx[p], cg);
        acc += sqrt(dn_dist2(cf, cg));
    }
    term[f] = acc;
}

// One lane per face over its row of N(f): one iteration of the normal filter, from the planes m_in into the planes m_out (another buffer: every
// face reads the old normals of its neighbours).
__global__ __launch_bounds__(DN_THREADS) void k_denoise_filter(int nF, const int* __restrict__ nb_ptr, const int* __restrict__ nb_idx,
                                                               const double* __restrict__ rest, const double* __restrict__ m_in, double two_ss,
                                                               double two_rr, double* __restrict__ m_out)
{
    const int f = blockIdx.x * DN_THREADS + threadIdx.x;
    if (f >= nF) return;
    const double* __restrict__ area = rest + 3 * (size_t)nF;
    const double* __restrict__ cen = rest + 4 * (size_t)nF;
    double cf[3], mf[3], cg[3], mg[3], s[3] = {0.0, 0.0, 0.0}, out[3];
    dn_load3(cen, (size_t)nF, (size_t)f, cf);
    dn_load3(m_in, (size_t)nF, (size_t)f, mf);
    const int p1 = nb_ptr[f + 1];
    for (int p = nb_ptr[f]; p < p1; p++) {
        const size_t g = (size_t)nb_idx[p];
        dn_load3(cen, (size_t)nF, g, cg);
        dn_load3(m_in, (size_t)nF, g, mg);
        dn_filter_add(cf, mf, cg, area[g], mg, two_ss, two_rr, s);
    }
    dn_filter_finish(s, mf, out);
#pragma unroll
    for (int l = 0; l < 3; l++) m_out[(size_t)l * nF + f] = out[l];
}

// One lane per face, one pass over the three gathers of the pose X: eterm[f] = the face's energy term, share[(3 i + l) * nF + f] = what corner i
// adds to the right-hand side of the global step.
__global__ __launch_bounds__(DN_THREADS) void k_denoise_project(int nF, const int* __restrict__ F, const double* __restrict__ rest,
                                                                const double* __restrict__ m, const double* __restrict__ X, size_t sv, size_t sl,
                                                                double* __restrict__ eterm, double* __restrict__ share)
{
    const int f = blockIdx.x * DN_THREADS + threadIdx.x;
    if (f >= nF) return;
    double x[3][3], mf[3], w[3], s[9];
    dn_load3(m, (size_t)nF, (size_t)f, mf);
    dn_load3(rest + 7 * (size_t)nF, (size_t)nF, (size_t)f, w);
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const size_t v = (size_t)F[3 * (size_t)f + i];
#pragma unroll
        for (int l = 0; l < 3; l++) x[i][l] = X[v * sv + (size_t)l * sl];
    }
    eterm[f] = dn_project(x, mf, w, s);
#pragma unroll
    for (int e = 0; e < 9; e++) share[(size_t)e * nF + f] = s[e];
}

hipError_t launch_denoise_rest(int nF, const int* F, const double* V0, double* rest, hipStream_t st)
{
    if (nF <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_denoise_rest, dim3(dn_grid(nF)), dim3(DN_THREADS), 0, st, nF, F, V0, rest);
    return hipGetLastError();
}

hipError_t launch_denoise_spacing(int nF, const int* nb_ptr, const int* nb_idx, const double* rest, double* term, hipStream_t st)
{
    if (nF <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_denoise_spacing, dim3(dn_grid(nF)), dim3(DN_THREADS), 0, st, nF, nb_ptr, nb_idx, rest, term);
    return hipGetLastError();
}

hipError_t launch_denoise_filter(int nF, const int* nb_ptr, const int* nb_idx, const double* rest, const double* m_in, double sigma_s, double sigma_r,
                                 double* m_out, hipStream_t st)
{
    if (nF <= 0) return hipSuccess;
    if (m_in == m_out) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_denoise_filter, dim3(dn_grid(nF)), dim3(DN_THREADS), 0, st, nF, nb_ptr, nb_idx, rest, m_in, 2.0 * (sigma_s * sigma_s),
                       2.0 * (sigma_r * sigma_r), m_out);
    return hipGetLastError();
}

hipError_t launch_denoise_project(int nF, const int* F, const double* rest, const double* m, const double* X, size_t sv, size_t sl, double* eterm,
                                  double* share, hipStream_t st)
{
    if (nF <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_denoise_project, dim3(dn_grid(nF)), dim3(DN_THREADS), 0, st, nF, F, rest, m, X, sv, sl, eterm, share);
    return hipGetLastError();
}

}  // namespace smg
