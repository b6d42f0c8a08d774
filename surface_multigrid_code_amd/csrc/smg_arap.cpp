// smg_arap.cpp -- as-rigid-as-possible deformation on the V-cycle (include/smg.h: smg_arap_*).
// The object owns one handle built from the caller's prolongations and precomputed with -L of the rest pose, the handle vertices known; the
// CSR of L on the device (the weights of the local step are the system's own values), the rest positions and the buffers of an iteration.
// One iteration: rotations + energy terms (k_arap_rotations), the energy (fixed-order reduction), the right-hand side (k_arap_rhs), one
// 3-column solve warm-started at the iterate, the new iterate as xyz rows.  All of it is enqueued on the object's stream, which the handle
// uses too; per iteration the host reads one energy double beside the solve's own history.  Checks, stream, handle, the cotangent system and
// the inner solve: smg_mesh_object.hpp; the loop and its stopping rule: smg_local_global.hpp; the energy's sum: launch_fixed_sum.
#include <hip/hip_runtime_api.h>

#include <cmath>
#include <memory>
#include <vector>

#include "smg_device.hpp"
#include "smg_local_global.hpp"
#include "smg_mesh_object.hpp"

using namespace smg;

struct smg_arap : MeshObject {            // handle[0]: -L of the rest pose, the handle vertices known
    int nV = 0, nh = 0;
    int pcg = 1;                          // the inner solver: 1 smg_solve_pcg (7 - 8 loop entries per solve on C3 against 10 - 11), 0 smg_solve
    double scale = 0.0;                   // s = sqrt(sum_i (sum_j |w_ij| |e_ij|)^2) >= |b|_F for every set of rotations
    DevBuf<int> rowptr, col, handles;     // the CSR pattern of L, the handle vertices in the caller's order
    DevBuf<double> w, P0;                 // the values of L (smg_assemble's d_Lval), rest positions (xyz rows)
    DevBuf<double> P, R, eterm, part, E;  // current positions (xyz rows), rotations (9 per vertex), energy terms, their chunk sums, E_t
    DevBuf<double> B, Ua, Ub, hp;         // column-major n x 3: right-hand side, the iterate and the solve's result; handle positions (nh x 3)
    ~smg_arap() { quiesce(); }
};

namespace {

int create_impl(const smg_hierarchy* h, const double* V, int nV, const int* F, int nF, const int* handles, int n_handles, smg_arap** out)
{
    if (out) *out = nullptr;
    const char* who = "smg_arap_create";
    if (!h || !V || !F || !handles || !out || nV <= 0 || nF <= 0) return fail(SMG_ERR_INVALID, "%s: bad arguments", who);
    if (int rc = check_hierarchy(who, h, 1, nV)) return rc;
    if (int rc = check_mesh(who, V, nV, F, nF, true)) return rc;
    if (n_handles < 1) return fail(SMG_ERR_INVALID, "%s: n_handles = %d, at least one handle vertex is needed", who, n_handles);
    {
        std::vector<char> seen((size_t)nV, 0);
        for (int r = 0; r < n_handles; r++) {
            if (handles[r] < 0 || handles[r] >= nV) return fail(SMG_ERR_INVALID, "%s: handle %d out of range", who, handles[r]);
            if (seen[handles[r]]) return fail(SMG_ERR_INVALID, "%s: handle %d is repeated", who, handles[r]);
            seen[handles[r]] = 1;
        }
    }
    if (n_handles >= nV) return fail(SMG_ERR_INVALID, "%s: every vertex is a handle: nothing to solve", who);

    std::unique_ptr<smg_arap> a(new smg_arap());
    a->nV = nV; a->nh = n_handles;
    if (int rc = a->open(who)) return rc;
    if (int rc = a->clone(who, h, 0)) return rc;

    // L of the rest pose on the device: its values stay there as the weights, their negatives are the system
    HIPCHK(a->P0.upload(std::vector<double>(V, V + (size_t)nV * 3)));
    CotanSystem S;
    if (int rc = cotan_system(F, nF, nV, a->P0.p, 0, 0.0, -1.0, a->stream, S, false, &a->w)) return rc;
    double ss = 0.0;
    for (int i = 0; i < nV; i++) {
        double row = 0.0;
        for (int q = S.ptr[i]; q < S.ptr[i + 1]; q++) {
            const int j = S.col[q];
            if (j == i) continue;
            const double ex = V[3 * (size_t)i] - V[3 * (size_t)j], ey = V[3 * (size_t)i + 1] - V[3 * (size_t)j + 1], ez = V[3 * (size_t)i + 2] - V[3 * (size_t)j + 2];
            row += std::fabs(S.L[q]) * std::sqrt(ex * ex + ey * ey + ez * ez);
        }
        ss += row * row;
    }
    a->scale = std::sqrt(ss);
    for (double& v : S.L) v = -v;
    if (int rc = smg_precompute(a->handle[0], nV, S.ptr.data(), S.col.data(), S.L.data(), handles, n_handles)) return rc;

    HIPCHK(a->rowptr.upload(S.ptr));
    HIPCHK(a->col.upload(S.col));
    HIPCHK(a->handles.upload(std::vector<int>(handles, handles + n_handles)));
    const size_t n = (size_t)nV;
    HIPCHK(a->P.alloc(3 * n));
    HIPCHK(a->R.alloc(9 * n));
    HIPCHK(a->eterm.alloc(n));
    HIPCHK(a->part.alloc((size_t)fixed_sum_groups(nV)));
    HIPCHK(a->B.alloc(3 * n));
    HIPCHK(a->Ua.alloc(3 * n));
    HIPCHK(a->Ub.alloc(3 * n));
    HIPCHK(a->hp.alloc(3 * (size_t)n_handles));
    *out = a.release();
    return SMG_OK;
}

int solve_impl(smg_arap* a, const double* handle_pos, int ld_hp, const double* U0, int ld_u0, int memspace, int max_iter, double rel_tol,
               const smg_solve_opts* opts, double* U, int ld_u, double* energy_his, int* cycles, int* n_iter)
{
    if (!a || !handle_pos || !U || bad_memspace(memspace) || max_iter < 0 || !(rel_tol >= 0.0) || !std::isfinite(rel_tol))
        return fail(SMG_ERR_INVALID, "smg_arap_solve: bad arguments");
    const int n = a->nV, nh = a->nh;
    if (ld_hp < nh || ld_u < n || (U0 && ld_u0 < n)) return fail(SMG_ERR_INVALID, "smg_arap_solve: a leading dimension is too small");
    DeviceScope dsc(a->device);
    hipStream_t st = a->stream;
    const smg_solve_opts so = opts_or_default(opts, 1e-8 * a->scale, 50);
    HIPCHK(a->E.ensure((size_t)max_iter + 1));
    int t_end = 0;
    if (!n_iter) n_iter = &t_end;
    *n_iter = 0;

    // the start: U0 or the rest pose, the handle rows from handle_pos; as the solve's column-major block (Ua) and as xyz rows (P)
    HIPCHK(copy_columns(a->hp.p, nh, handle_pos, ld_hp, nh, 3, copy_in(memspace), st));
    if (U0) HIPCHK(copy_columns(a->Ua.p, n, U0, ld_u0, n, 3, copy_in(memspace), st));
    else HIPCHK(launch_arap_columns(n, a->P0.p, a->Ua.p, n, st));
    HIPCHK(launch_arap_set_handles(nh, a->handles.p, a->hp.p, nh, a->Ua.p, n, st));
    HIPCHK(launch_arap_rows(n, a->Ua.p, n, a->P.p, st));

    // local step: R_t from U_t, E_t = E(R_t, U_t); the right-hand side is enqueued ahead of the host's look at E_t
    auto local = [&](int t, bool with_rhs, double* E_t) -> int {
        HIPCHK(launch_arap_rotations(n, a->rowptr.p, a->col.p, a->w.p, a->P0.p, a->P.p, a->R.p, a->eterm.p, st));
        HIPCHK(launch_fixed_sum(a->eterm.p, n, a->part.p, a->E.p + t, st));
        HIPCHK(hipMemcpyAsync(E_t, a->E.p + t, sizeof(double), hipMemcpyDeviceToHost, st));
        if (with_rhs) HIPCHK(launch_arap_rhs(n, a->rowptr.p, a->col.p, a->w.p, a->P0.p, a->R.p, a->B.p, n, st));
        HIPCHK(hipStreamSynchronize(st));
        return SMG_OK;
    };
    // global step: (-L) U_{t+1} = b, handle rows known, from U_t
    auto global = [&](int, int* entries) -> int {
        if (int rc = inner_solve(a->handle[0], a->pcg, a->B.p, n, a->hp.p, nh, a->Ua.p, n, 3, so, a->Ub.p, n, entries)) return rc;
        std::swap(a->Ua, a->Ub);
        HIPCHK(launch_arap_rows(n, a->Ua.p, n, a->P.p, st));
        return SMG_OK;
    };
    const int rc = local_global(max_iter, rel_tol, local, global, energy_his, cycles, n_iter);
    if (rc == LOCAL_GLOBAL_NONFINITE) return fail(SMG_ERR_NONFINITE, "smg_arap_solve: non-finite energy at iteration %d", *n_iter);
    if (rc) return rc;
    HIPCHK(copy_columns(U, ld_u, a->Ua.p, n, n, 3, copy_out(memspace), st));
    HIPCHK(hipStreamSynchronize(st));
    return SMG_OK;
}

}  // namespace

extern "C" int smg_arap_create(const smg_hierarchy* h, const double* V, int nV, const int* F, int nF, const int* handles, int n_handles, smg_arap** out)
{
    return guarded("smg_arap_create", [&]() { return create_impl(h, V, nV, F, nF, handles, n_handles, out); });
}

extern "C" void smg_arap_destroy(smg_arap* a) { delete a; }

extern "C" int smg_arap_set_solver(smg_arap* a, int pcg)
{
    if (!a) return fail(SMG_ERR_INVALID, "null arap object");
    latch_solver(a->pcg, pcg);
    return SMG_OK;
}

extern "C" long long smg_arap_device_bytes(const smg_arap* a)
{
    return a ? device_bytes(*a, a->rowptr, a->col, a->handles, a->w, a->P0, a->P, a->R, a->eterm, a->part, a->E, a->B, a->Ua, a->Ub, a->hp) : 0;
}

extern "C" int smg_arap_solve(smg_arap* a, const double* handle_pos, int ld_hp, const double* U0, int ld_u0, int memspace, int max_iter,
                              double rel_tol, const smg_solve_opts* opts, double* U, int ld_u, double* energy_his, int* cycles, int* n_iter)
{
    return guarded("smg_arap_solve", [&]() {
        return solve_impl(a, handle_pos, ld_hp, U0, ld_u0, memspace, max_iter, rel_tol, opts, U, ld_u, energy_his, cycles, n_iter);
    });
}
