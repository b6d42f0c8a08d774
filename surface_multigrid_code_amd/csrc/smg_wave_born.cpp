// smg_wave_born.cpp -- Born traces and Gauss-Newton products of the wave object's trace misfit (include/smg.h: smg_wave_gauss_newton; DESIGN.md
// section 36).  With J = d traces / d speed at the linearisation point -- the run of the last smg_wave_gradient call that completed with a backward
// pass, whose history e_n the object still holds -- the call returns J d and H d = J' J d.  A speed perturbation d changes mt by fd = fac d,
// fac = (-2 mt) / speed, and the step's right-hand side by fd e_n, so the tangent run is the forward step itself (wave_forward, smg_wave.cpp) from
// the zero state, without nodal sources, with one distributed source per step (k_wave_born); J d is its traces.  The adjoint pass is linear in its
// residual and its coefficients do not depend on it: run with rho = J d (wave_backward, smg_wave_adjoint.cpp) it leaves J' J d where it leaves
// grad_speed.  The tangent run has state blocks of its own: the object's state is not touched.  It uses the forward step's right-hand side
// blocks, so the kept right-hand side is dropped; the next smg_wave_step forms it again, to the same bits.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "smg_device.hpp"
#include "smg_mesh.hpp"
#include "smg_mesh_object.hpp"
#include "smg_wave_adjoint_inl.hpp"
#include "smg_wave_born_inl.hpp"
#include "smg_wave_object.hpp"

using namespace smg;

namespace smg {

int wave_born_check_operands(const char* who, int nV, int nF, int k, int d_cols, const int* F, int clamped, const double* b, const double* e,
                             const double* fd, const double* out)
{
    if (nV < 1 || nF < 1 || !F || !out) return fail(SMG_ERR_INVALID, "%s: bad arguments", who);
    if (!b || !e || !fd) return fail(SMG_ERR_INVALID, "%s: an operand is missing", who);
    if (k < 1) return fail(SMG_ERR_INVALID, "%s: k = %d, at least one column is needed", who, k);
    if (d_cols != 1 && d_cols != k) return fail(SMG_ERR_INVALID, "%s: d_cols = %d, 1 or k = %d is needed", who, d_cols, k);
    if (clamped != 0 && clamped != 1) return fail(SMG_ERR_INVALID, "%s: clamped = %d, 0 or 1 is needed", who, clamped);
    return check_faces(who, F, nF, nV);
}

}  // namespace smg

namespace {

// the tangent state's blocks and the plane fd; they grow with the largest shape seen and are kept
int ensure_born(smg_wave* g, int d_cols)
{
    const size_t n = (size_t)g->nV;
    HIPCHK(hipStreamSynchronize(g->stream));
    for (auto& b : g->T) HIPCHK(b.ensure(2 * n * (size_t)g->k));
    HIPCHK(g->fd.ensure(n * (size_t)d_cols));
    return SMG_OK;
}

int gauss_newton_impl(smg_wave* g, const double* d, int ldd, int d_cols, const smg_solve_opts* opts, double* product, int ld, double* born_traces,
                      double* curvature, int* cycles)
{
    const char* who = "smg_wave_gauss_newton";
    if (!g) return fail(SMG_ERR_INVALID, "%s: null object", who);
    if (!g->lin_valid || g->k < 1) return fail(SMG_ERR_INVALID, "%s: no linearisation point: call smg_wave_gradient with a gradient output first", who);
    if (!d) return fail(SMG_ERR_INVALID, "%s: d is missing", who);
    const int n = g->nV, k = g->k, N = g->lin_steps, nr = g->n_rec;
    if (d_cols != 1 && d_cols != k) return fail(SMG_ERR_INVALID, "%s: d_cols = %d, 1 or k = %d is needed", who, d_cols, k);
    if (ldd < n) return fail(SMG_ERR_INVALID, "%s: ldd = %d, nV = %d at least is needed", who, ldd, n);
    for (int c = 0; c < d_cols; c++)
        for (int i = 0; i < n; i++)
            if (!std::isfinite(d[(size_t)c * (size_t)ldd + (size_t)i])) return fail(SMG_ERR_INVALID, "%s: d is not finite at vertex %d, column %d", who, i, c);
    if (!product && !born_traces && !curvature) return fail(SMG_ERR_INVALID, "%s: no output: product, born_traces and curvature are all NULL", who);
    if (product && ld < n) return fail(SMG_ERR_INVALID, "%s: a leading dimension is too small", who);
    const size_t nk = (size_t)n * k, D = sizeof(double), ent = (size_t)N * nr, ek = ent * k;
    const bool backward = product != nullptr;
    DeviceScope dsc(g->device);
    hipStream_t st = g->stream;
    if (int rc = wave_ensure_adjoint(g, N, backward, false, false)) return rc;
    if (int rc = ensure_born(g, d_cols)) return rc;

    // fd = fac d: one multiply per entry on the host, uploaded once
    std::vector<double> fac((size_t)n), fd((size_t)n * (size_t)d_cols);
    wave_adj_host_planes(n, g->mt_host.data(), g->speed_host.empty() ? nullptr : g->speed_host.data(), fac.data());
    wave_born_host_plane(n, d_cols, fac.data(), d, ldd, fd.data());
    HIPCHK(hipMemcpy(g->fd.p, fd.data(), fd.size() * D, hipMemcpyHostToDevice));

    // the tangent run: the forward loop on the tangent state from zero, its traces recorded on the device
    std::vector<int> cyc(2 * (size_t)N, 0);
    HIPCHK(hipMemsetAsync(g->T[0].p, 0, 2 * nk * D, st));
    g->rhs_valid = false;   // B, Wb and rsq hold the tangent run's from here on
    const WaveBorn born = {g->fd.p, d_cols, g->H.p};
    int cur = 0, done = 0;
    const int rcf = wave_forward(g, who, g->T, &cur, &born, N, nullptr, opts, nullptr, nullptr, true, cyc.data(), &done, nullptr);
    g->rhs_valid = false;   // what the last advance left is the tangent state's, not the state's
    if (rcf != SMG_OK || done < N) return rcf;

    // rho = J d and |J d|^2 per column
    double *rho = g->rho.p, *sq = rho + ek;
    HIPCHK(launch_wave_adj_residual(k, (long long)ent, g->trace.p, nullptr, rho, sq, st));
    for (int c = 0; c < k; c++) HIPCHK(launch_fixed_sum(sq + (size_t)c * ent, (int)ent, g->apart.p, g->ared.p + c, st));
    std::vector<double> curv((size_t)k);
    HIPCHK(hipMemcpyAsync(curv.data(), g->ared.p, (size_t)k * D, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));

    // the backward pass with rho = J d: J' J d where the gradient call leaves grad_speed
    if (backward) {
        if (int rc = wave_backward(g, who, N, rho, opts, false, cyc.data() + N)) return rc;
        HIPCHK(launch_wave_adj_scale(n, k, g->fac.p, g->G.p, n, g->G.p, n, st));
        HIPCHK(copy_columns(product, ld, g->G.p, n, n, k, hipMemcpyDeviceToHost, st));
    }
    if (born_traces) HIPCHK(hipMemcpyAsync(born_traces, g->trace.p, ek * D, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (curvature) std::copy(curv.begin(), curv.end(), curvature);
    if (cycles) std::copy(cyc.begin(), cyc.begin() + (backward ? 2 * N : N), cycles);
    return SMG_OK;
}

}  // namespace

extern "C" int smg_wave_gauss_newton(smg_wave* g, const double* d, int ldd, int d_cols, const smg_solve_opts* opts, double* product, int ld,
                                     double* born_traces, double* curvature, int* cycles)
{
    return guarded("smg_wave_gauss_newton", [&]() { return gauss_newton_impl(g, d, ldd, d_cols, opts, product, ld, born_traces, curvature, cycles); });
}

extern "C" int smg_wave_born_host(int nV, int nF, int k, int d_cols, const int* F, int clamped, const double* b, const double* e, const double* fd, double* out)
{
    return guarded("smg_wave_born_host", [&]() -> int {
        const char* who = "smg_wave_born_host";
        if (int rc = wave_born_check_operands(who, nV, nF, k, d_cols, F, clamped, b, e, fd, out)) return rc;
        const size_t nk = (size_t)nV * (size_t)k;
        std::vector<int> known;
        if (clamped) {
            known.assign((size_t)nV, 0);
            for (int v : boundary_vertices(F, nF, nV)) known[(size_t)v] = 1;
        }
        std::copy(b, b + nk, out);
        std::fill(out + nk, out + 2 * nk, 0.0);   // the squares start as k_wave_rhs leaves the known rows
        wave_born_host(nV, k, d_cols, clamped ? known.data() : nullptr, fd, e, out, out + nk);
        out[2 * nk] = flow_host_sum(out + nk, (int)nk);
        return SMG_OK;
    });
}
