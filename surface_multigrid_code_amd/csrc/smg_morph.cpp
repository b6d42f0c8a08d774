// smg_morph.cpp -- gradient-domain morphing on the V-cycle (include/smg.h: smg_morph_*): Poisson reconstruction from
// prescribed per-face gradients, pose interpolation through the faces' polar factors, and deformation transfer in Botsch et al.'s Poisson form.
// The object owns one handle built from the caller's prolongations and precomputed with -L of the rest pose, the pins known, and the geometry the
// kernels read (csrc/smg_morph_device.hip): faces, corner lists, the gradient basis W, the rest normals and the areas.  A query is one or two
// face kernels, one vertex kernel that writes all 3k right-hand sides, the fixed-order sum of |b|_F^2, and ONE 3k-column solve of the constant
// matrix.  All of it is enqueued on the object's stream, which the handle uses too; beside the solve's own history the host reads one double per
// call, |b|_F^2, which sets the default tolerance and refuses non-finite input before the solve.  Checks, stream, handle, the cotangent system and
// the inner solve: smg_mesh_object.hpp.
#include <hip/hip_runtime_api.h>

#include <climits>
#include <cmath>
#include <memory>
#include <vector>

#include "smg_device.hpp"
#include "smg_mesh.hpp"
#include "smg_mesh_object.hpp"
#include "smg_morph_inl.hpp"

using namespace smg;

struct smg_morph : MeshObject {            // handle[0]: -L of the rest pose, the pins known
    int nV = 0, nF = 0, nh = 0;
    int pcg = 1;                           // the inner solver: 1 smg_solve_pcg, 0 smg_solve
    std::vector<double> h_t;               // the call's times (alive until the next call: the upload is asynchronous)
    DevBuf<int> F, m_ptr, m_idx, pins, Fs; // faces, corner lists per vertex, the pins in the caller's order; the source faces of a transfer
    DevBuf<double> V0, W, nrm, Af;         // rest positions (xyz rows), gradient basis (9 per face), rest normals (3 per face), face areas
    DevBuf<double> omega, S;               // the pose's rotation vectors (3 per face) and stretches (6 per face)
    DevBuf<double> X, J, t;                // staging of a host call's poses / gradients and the gradients of a transfer; the times
    DevBuf<double> B, Ua, Ub, hp;          // column-major n x 3k: right-hand side, start, result; pin positions (nh x 3k)
    DevBuf<double> bsq, part, sum;         // |b_v|^2 per (vertex, set), their chunk sums, |b|_F^2
    ~smg_morph() { quiesce(); }
};

namespace smg {

int morph_check_operands(const char* who, int op, int nV, int nF, int k, const int* F, const double* V0, const double* X, const double* t,
                         const double* in, const int* pins, int n_pins, const double* out)
{
    if (op < SMG_MORPH_FACE_GRADIENT || op > SMG_MORPH_PINS || nV < 1 || nF < 1 || !F || !V0 || !out) return fail(SMG_ERR_INVALID, "%s: bad arguments", who);
    const bool needs_x = op == SMG_MORPH_FACE_GRADIENT || op == SMG_MORPH_FACE_POLAR;
    const bool needs_in = op == SMG_MORPH_RHS_GRADIENT || op == SMG_MORPH_RHS_INTERP;
    const bool needs_t = op == SMG_MORPH_RHS_INTERP || (op == SMG_MORPH_PINS && X);
    if ((needs_x && !X) || (needs_in && !in) || (needs_t && !t) || (op == SMG_MORPH_PINS && (!pins || n_pins < 1)))
        return fail(SMG_ERR_INVALID, "%s: op %d misses an operand", who, op);
    if (k < 1) return fail(SMG_ERR_INVALID, "%s: k = %d, at least one set is needed", who, k);
    if (needs_t)
        for (int c = 0; c < k; c++)
            if (!std::isfinite(t[c])) return fail(SMG_ERR_INVALID, "%s: t[%d] is not finite", who, c);
    if (int rc = check_faces(who, F, nF, nV)) return rc;
    if (op == SMG_MORPH_PINS)
        for (int r = 0; r < n_pins; r++)
            if (pins[r] < 0 || pins[r] >= nV) return fail(SMG_ERR_INVALID, "%s: pin %d out of range", who, pins[r]);
    return SMG_OK;
}

}  // namespace smg

namespace {

int create_impl(const smg_hierarchy* h, const double* V, int nV, const int* F, int nF, const int* pins, int n_pins, smg_morph** out)
{
    if (out) *out = nullptr;
    const char* who = "smg_morph_create";
    if (!h || !V || !F || !pins || !out || nV <= 0 || nF <= 0) return fail(SMG_ERR_INVALID, "%s: bad arguments", who);
    if (int rc = check_hierarchy(who, h, 1, nV)) return rc;
    if (int rc = check_mesh(who, V, nV, F, nF, true)) return rc;
    if (n_pins < 1) return fail(SMG_ERR_INVALID, "%s: n_pins = %d, at least one pinned vertex is needed", who, n_pins);
    {
        std::vector<char> seen((size_t)nV, 0);
        for (int r = 0; r < n_pins; r++) {
            if (pins[r] < 0 || pins[r] >= nV) return fail(SMG_ERR_INVALID, "%s: pin %d out of range", who, pins[r]);
            if (seen[pins[r]]) return fail(SMG_ERR_INVALID, "%s: pin %d is repeated", who, pins[r]);
            seen[pins[r]] = 1;
        }
    }
    if (n_pins >= nV) return fail(SMG_ERR_INVALID, "%s: every vertex is pinned: nothing to solve", who);

    std::unique_ptr<smg_morph> m(new smg_morph());
    m->nV = nV; m->nF = nF; m->nh = n_pins;
    if (int rc = m->open(who)) return rc;
    if (int rc = m->clone(who, h, 0)) return rc;

    // the geometry of a query, then -L of the rest pose with the pinned rows known: precomputed once
    HIPCHK(m->V0.upload(std::vector<double>(V, V + (size_t)nV * 3)));
    if (int rc = upload_faces(F, nF, nV, m->F, m->m_ptr, m->m_idx)) return rc;
    HIPCHK(m->W.alloc((size_t)nF * 9));
    HIPCHK(m->nrm.alloc((size_t)nF * 3));
    HIPCHK(m->Af.alloc((size_t)nF));
    HIPCHK(m->omega.alloc((size_t)nF * 3));
    HIPCHK(m->S.alloc((size_t)nF * 6));
    HIPCHK(m->sum.alloc(1));
    HIPCHK(m->pins.upload(std::vector<int>(pins, pins + n_pins)));
    HIPCHK(launch_morph_basis(m->V0.p, m->F.p, nF, m->W.p, m->nrm.p, m->Af.p, m->stream));
    CotanSystem S;
    if (int rc = cotan_system(F, nF, nV, m->V0.p, 0, 0.0, -1.0, m->stream, S, false)) return rc;
    for (double& v : S.L) v = -v;
    if (int rc = smg_precompute(m->handle[0], nV, S.ptr.data(), S.col.data(), S.L.data(), pins, n_pins)) return rc;
    *out = m.release();
    return SMG_OK;
}

// what the three queries check alike, in this order: the object and the output, k, the memspace, the leading dimensions
int check_call(const char* who, const smg_morph* m, const void* input, int k, const double* pin_pos, int ld_pp, const double* U0, int ld_u0, int memspace,
               const double* U, int ld_u)
{
    if (!m || !input || !U) return fail(SMG_ERR_INVALID, "%s: bad arguments", who);
    if (k < 1) return fail(SMG_ERR_INVALID, "%s: k = %d, at least one set is needed", who, k);
    if ((long long)m->nV * k > INT_MAX) return fail(SMG_ERR_INVALID, "%s: k = %d sets of %d vertices exceed the index range", who, k, m->nV);
    if (bad_memspace(memspace)) return fail(SMG_ERR_INVALID, "%s: memspace must be SMG_HOST or SMG_DEVICE", who);
    if ((pin_pos && ld_pp < m->nh) || ld_u < m->nV || (U0 && ld_u0 < m->nV)) return fail(SMG_ERR_INVALID, "%s: a leading dimension is too small", who);
    return SMG_OK;
}

// the blocks of a k-set query; they grow with the largest k seen and are kept
int ensure_sets(smg_morph* m, int k)
{
    const size_t n = (size_t)m->nV, cols = 3 * (size_t)k;
    if (m->B.n >= n * cols) return SMG_OK;
    HIPCHK(hipStreamSynchronize(m->stream));
    HIPCHK(m->B.alloc(n * cols));
    HIPCHK(m->Ua.alloc(n * cols));
    HIPCHK(m->Ub.alloc(n * cols));
    HIPCHK(m->hp.alloc((size_t)m->nh * cols));
    HIPCHK(m->bsq.alloc(n * k));
    HIPCHK(m->part.alloc((size_t)fixed_sum_groups(m->nV * k)));
    HIPCHK(m->t.alloc((size_t)k));
    return SMG_OK;
}

// `count` doubles of a call's input on the device: the caller's block itself (SMG_DEVICE) or a copy in `stage`
int stage_input(smg_morph* m, DevBuf<double>& stage, const double* src, size_t count, int memspace, const double** dev)
{
    if (memspace == SMG_DEVICE) { *dev = src; return SMG_OK; }
    HIPCHK(stage.ensure(count));
    HIPCHK(hipMemcpyAsync(stage.p, src, count * sizeof(double), hipMemcpyHostToDevice, m->stream));
    *dev = stage.p;
    return SMG_OK;
}

// after the right-hand side kernel: |b|_F, the pins and the start, the solve, the copy out.  X, t (device; nullptr: the rest pose) give the defaults
int finish(const char* who, smg_morph* m, int k, const double* X, const double* t, const double* pin_pos, int ld_pp, const double* U0, int ld_u0,
           int memspace, const smg_solve_opts* opts, double* U, int ld_u, int* cycles)
{
    const int n = m->nV, nh = m->nh, cols = 3 * k;
    hipStream_t st = m->stream;
    double bb = 0.0;
    HIPCHK(launch_fixed_sum(m->bsq.p, n * k, m->part.p, m->sum.p, st));
    HIPCHK(hipMemcpyAsync(&bb, m->sum.p, sizeof(double), hipMemcpyDeviceToHost, st));
    if (pin_pos) HIPCHK(copy_columns(m->hp.p, nh, pin_pos, ld_pp, nh, cols, copy_in(memspace), st));
    else HIPCHK(launch_morph_pins(nh, k, m->pins.p, m->V0.p, X, t, m->hp.p, nh, st));
    if (U0) HIPCHK(copy_columns(m->Ua.p, n, U0, ld_u0, n, cols, copy_in(memspace), st));
    else HIPCHK(launch_morph_start(n, k, m->V0.p, X, t, m->Ua.p, n, st));
    HIPCHK(launch_morph_set_pins(nh, cols, m->pins.p, m->hp.p, nh, m->Ua.p, n, st));
    HIPCHK(hipStreamSynchronize(st));
    if (!std::isfinite(bb)) return fail(SMG_ERR_NONFINITE, "%s: the right-hand side is not finite", who);
    const smg_solve_opts so = opts_or_default(opts, 1e-10 * std::sqrt(bb), 100);
    if (int rc = inner_solve(m->handle[0], m->pcg, m->B.p, n, m->hp.p, nh, m->Ua.p, n, cols, so, m->Ub.p, n, cycles)) return rc;
    HIPCHK(copy_columns(U, ld_u, m->Ub.p, n, n, cols, copy_out(memspace), st));
    HIPCHK(hipStreamSynchronize(st));
    return SMG_OK;
}

int reconstruct_impl(smg_morph* m, const double* J, int k, const double* pin_pos, int ld_pp, const double* U0, int ld_u0, int memspace,
                     const smg_solve_opts* opts, double* U, int ld_u, int* cycles)
{
    const char* who = "smg_morph_reconstruct";
    if (int rc = check_call(who, m, J, k, pin_pos, ld_pp, U0, ld_u0, memspace, U, ld_u)) return rc;
    DeviceScope dsc(m->device);
    if (int rc = ensure_sets(m, k)) return rc;
    const double* dJ = nullptr;
    if (int rc = stage_input(m, m->J, J, (size_t)k * m->nF * 9, memspace, &dJ)) return rc;
    HIPCHK(launch_morph_rhs_gradient(m->nV, k, m->nF, m->m_ptr.p, m->m_idx.p, m->W.p, m->Af.p, dJ, m->B.p, m->nV, m->bsq.p, m->stream));
    return finish(who, m, k, nullptr, nullptr, pin_pos, ld_pp, U0, ld_u0, memspace, opts, U, ld_u, cycles);
}

int interpolate_impl(smg_morph* m, const double* X, const double* t, int k, const double* pin_pos, int ld_pp, const double* U0, int ld_u0, int memspace,
                     const smg_solve_opts* opts, double* U, int ld_u, int* cycles)
{
    const char* who = "smg_morph_interpolate";
    if (!t) return fail(SMG_ERR_INVALID, "%s: bad arguments", who);
    if (int rc = check_call(who, m, X, k, pin_pos, ld_pp, U0, ld_u0, memspace, U, ld_u)) return rc;
    for (int c = 0; c < k; c++)
        if (!std::isfinite(t[c])) return fail(SMG_ERR_INVALID, "%s: t[%d] is not finite", who, c);
    DeviceScope dsc(m->device);
    hipStream_t st = m->stream;
    if (int rc = ensure_sets(m, k)) return rc;
    HIPCHK(hipStreamSynchronize(st));            // the previous call's upload read h_t
    m->h_t.assign(t, t + k);
    HIPCHK(hipMemcpyAsync(m->t.p, m->h_t.data(), (size_t)k * sizeof(double), hipMemcpyHostToDevice, st));
    const double* dX = nullptr;
    if (int rc = stage_input(m, m->X, X, (size_t)m->nV * 3, memspace, &dX)) return rc;
    HIPCHK(launch_morph_face_polar(m->nF, m->F.p, m->W.p, m->nrm.p, dX, nullptr, m->omega.p, m->S.p, st));
    HIPCHK(launch_morph_rhs_interp(m->nV, k, m->nF, m->m_ptr.p, m->m_idx.p, m->W.p, m->Af.p, m->omega.p, m->S.p, m->t.p, m->B.p, m->nV, m->bsq.p, st));
    return finish(who, m, k, dX, m->t.p, pin_pos, ld_pp, U0, ld_u0, memspace, opts, U, ld_u, cycles);
}

int transfer_impl(smg_morph* m, const double* S0, int nVs, const int* Fs, const double* S1, int k, const double* pin_pos, int ld_pp, const double* U0,
                  int ld_u0, int memspace, const smg_solve_opts* opts, double* U, int ld_u, int* cycles)
{
    const char* who = "smg_morph_transfer";
    if (!S1 || nVs < 1) return fail(SMG_ERR_INVALID, "%s: bad arguments", who);
    if (int rc = check_call(who, m, S0, k, pin_pos, ld_pp, U0, ld_u0, memspace, U, ld_u)) return rc;
    if (!Fs && nVs != m->nV) return fail(SMG_ERR_INVALID, "%s: Fs == NULL takes the object's faces and needs nVs == nV (%d != %d)", who, nVs, m->nV);
    if (Fs)
        for (size_t i = 0; i < (size_t)m->nF * 3; i++)
            if (Fs[i] < 0 || Fs[i] >= nVs) return fail(SMG_ERR_INVALID, "%s: source face index %d out of range", who, Fs[i]);
    DeviceScope dsc(m->device);
    hipStream_t st = m->stream;
    if (int rc = ensure_sets(m, k)) return rc;
    const int* dFs = m->F.p;
    if (Fs) {
        HIPCHK(m->Fs.ensure((size_t)m->nF * 3));
        HIPCHK(hipMemcpyAsync(m->Fs.p, Fs, (size_t)m->nF * 3 * sizeof(int), hipMemcpyHostToDevice, st));
        dFs = m->Fs.p;
    }
    // the source's rest pose and its k poses: one staging block, the rest pose first
    const size_t set = (size_t)nVs * 3;
    const double *dS0 = S0, *dS1 = S1;
    if (memspace == SMG_HOST) {
        HIPCHK(m->X.ensure(set * ((size_t)k + 1)));
        HIPCHK(hipMemcpyAsync(m->X.p, S0, set * sizeof(double), hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(m->X.p + set, S1, set * k * sizeof(double), hipMemcpyHostToDevice, st));
        dS0 = m->X.p; dS1 = m->X.p + set;
    }
    HIPCHK(m->J.ensure((size_t)k * m->nF * 9));
    HIPCHK(launch_morph_face_gradient(m->nF, k, dFs, dS0, dS1, set, m->J.p, st));
    HIPCHK(launch_morph_rhs_gradient(m->nV, k, m->nF, m->m_ptr.p, m->m_idx.p, m->W.p, m->Af.p, m->J.p, m->B.p, m->nV, m->bsq.p, st));
    return finish(who, m, k, nullptr, nullptr, pin_pos, ld_pp, U0, ld_u0, memspace, opts, U, ld_u, cycles);
}

}  // namespace

extern "C" int smg_morph_create(const smg_hierarchy* h, const double* V, int nV, const int* F, int nF, const int* pins, int n_pins, smg_morph** out)
{
    return guarded("smg_morph_create", [&]() { return create_impl(h, V, nV, F, nF, pins, n_pins, out); });
}

extern "C" void smg_morph_destroy(smg_morph* m) { delete m; }

extern "C" int smg_morph_set_solver(smg_morph* m, int pcg)
{
    if (!m) return fail(SMG_ERR_INVALID, "smg_morph_set_solver: null object");
    latch_solver(m->pcg, pcg);
    return SMG_OK;
}

extern "C" long long smg_morph_device_bytes(const smg_morph* m)
{
    if (!m) return 0;   // one list: every DevBuf of the struct
    return device_bytes(*m, m->F, m->m_ptr, m->m_idx, m->pins, m->Fs, m->V0, m->W, m->nrm, m->Af, m->omega, m->S, m->X, m->J, m->t, m->B, m->Ua, m->Ub,
                        m->hp, m->bsq, m->part, m->sum);
}

extern "C" int smg_morph_reconstruct(smg_morph* m, const double* J, int k, const double* pin_pos, int ld_pp, const double* U0, int ld_u0, int memspace,
                                     const smg_solve_opts* opts, double* U, int ld_u, int* cycles)
{
    return guarded("smg_morph_reconstruct", [&]() { return reconstruct_impl(m, J, k, pin_pos, ld_pp, U0, ld_u0, memspace, opts, U, ld_u, cycles); });
}

extern "C" int smg_morph_interpolate(smg_morph* m, const double* X, const double* t, int k, const double* pin_pos, int ld_pp, const double* U0, int ld_u0,
                                     int memspace, const smg_solve_opts* opts, double* U, int ld_u, int* cycles)
{
    return guarded("smg_morph_interpolate", [&]() { return interpolate_impl(m, X, t, k, pin_pos, ld_pp, U0, ld_u0, memspace, opts, U, ld_u, cycles); });
}

extern "C" int smg_morph_transfer(smg_morph* m, const double* S0, int nVs, const int* Fs, const double* S1, int k, const double* pin_pos, int ld_pp,
                                  const double* U0, int ld_u0, int memspace, const smg_solve_opts* opts, double* U, int ld_u, int* cycles)
{
    return guarded("smg_morph_transfer", [&]() {
        return transfer_impl(m, S0, nVs, Fs, S1, k, pin_pos, ld_pp, U0, ld_u0, memspace, opts, U, ld_u, cycles);
    });
}

extern "C" int smg_morph_faces_host(int op, int nV, int nF, int k, const int* F, const double* V0, const double* X, const double* t, const double* in,
                                    const int* pins, int n_pins, double* out)
{
    return guarded("smg_morph_faces_host", [&]() -> int {
        const char* who = "smg_morph_faces_host";
        if (int rc = morph_check_operands(who, op, nV, nF, k, F, V0, X, t, in, pins, n_pins, out)) return rc;
        const size_t f = (size_t)nF, n = (size_t)nV;
        std::vector<int> mp, mi;
        if (op == SMG_MORPH_RHS_GRADIENT || op == SMG_MORPH_RHS_INTERP) vertex_corner_lists(std::vector<int>(F, F + 3 * f), nV, mp, mi);
        switch (op) {
            case SMG_MORPH_FACE_GRADIENT: morph_host_gradient(nV, nF, k, F, V0, X, out); break;
            case SMG_MORPH_FACE_POLAR: morph_host_polar(nF, F, V0, X, out, out + 9 * f, out + 12 * f); break;
            case SMG_MORPH_RHS_GRADIENT: morph_host_rhs(nV, nF, k, F, V0, mp.data(), mi.data(), in, nullptr, nullptr, nullptr, out, out + 3 * n * k); break;
            case SMG_MORPH_RHS_INTERP: morph_host_rhs(nV, nF, k, F, V0, mp.data(), mi.data(), nullptr, in, in + 3 * f, t, out, out + 3 * n * k); break;
            default: morph_host_pins(nV, k, V0, X, t, pins, n_pins, out, out + 3 * (size_t)n_pins * k); break;
        }
        return SMG_OK;
    });
}
