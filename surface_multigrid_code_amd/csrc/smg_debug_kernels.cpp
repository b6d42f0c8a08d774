// smg_debug_kernels.cpp -- handle-free test hooks of the LOBPCG and PCG block kernels (include/smg.h: smg_debug_eig_gram, smg_debug_eig_combine,
// smg_debug_eig_residual, smg_debug_krylov), of the geodesics kernels (smg_debug_geodesics), of the ARAP kernels (smg_debug_arap), of the fixed-order reduction (smg_debug_fixed_reduce), of the membrane kernels (smg_debug_membrane, smg_debug_membrane_material), of the parameterization kernels (smg_debug_param), of the projective-dynamics kernels (smg_debug_pd), of the denoising kernels (smg_debug_denoise), of the stylization kernels (smg_debug_stylize), of the morphing kernels (smg_debug_morph), of the flow kernels (smg_debug_flow), of the Hodge kernels (smg_debug_hodge), of the earth mover's kernels (smg_debug_emd), of the surface-fluid kernels (smg_debug_fluid), of the reaction-diffusion kernels (smg_debug_rd), of the wave-equation kernels (smg_debug_wave) and of the union kernels (smg_debug_union).  Each hook uploads host arrays to scratch device buffers, calls the launcher of smg_device.hpp once
// on a private stream, and copies the results back.  Every device buffer sits between two guard regions filled with a sentinel byte; a guard that
// changed is reported, so a stray write past either end of an output is seen by the caller.
#include <hip/hip_runtime_api.h>
#include <climits>

#include <algorithm>
#include <cstring>
#include <vector>

#include "smg_device.hpp"
#include "smg_fluid_inl.hpp"
#include "smg_internal.hpp"
#include "smg_membrane_inl.hpp"
#include "smg_mesh.hpp"
#include "smg_mesh_object.hpp"
#include "smg_rd_inl.hpp"
#include "smg_stylize_inl.hpp"
#include "smg_wave_adjoint_inl.hpp"
#include "smg_wave_born_inl.hpp"
#include "smg_wave_inl.hpp"
#include "smg_wave_object.hpp"

using namespace smg;

namespace {

constexpr size_t GUARD = 4096;            // bytes of sentinel in front of and behind every buffer
constexpr unsigned char SENTINEL = 0xA5;

// the scratch buffers and the stream of one hook call; freed on scope exit
class Scratch {
public:
    Scratch() = default;
    Scratch(const Scratch&) = delete;
    Scratch& operator=(const Scratch&) = delete;
    ~Scratch()
    {
        for (Buf& b : bufs_) (void)hipFree(b.base);
        if (st_) (void)hipStreamDestroy(st_);
    }
    hipError_t init() { return hipStreamCreateWithFlags(&st_, hipStreamNonBlocking); }
    hipStream_t stream() const { return st_; }

    // a device copy of src[0 .. bytes) (src == nullptr: sentinel bytes) between two guards; back != nullptr: copied there by finish()
    template <typename T>
    hipError_t add(const void* src, void* back, size_t bytes, T** dev)
    {
        Buf b;
        b.bytes = bytes;
        b.back = back;
        hipError_t e = hipMalloc((void**)&b.base, bytes + 2 * GUARD);
        if (e != hipSuccess) return e;
        bufs_.push_back(b);
        if ((e = hipMemsetAsync(b.base, SENTINEL, bytes + 2 * GUARD, st_)) != hipSuccess) return e;
        if (src && bytes && (e = hipMemcpyAsync(b.base + GUARD, src, bytes, hipMemcpyHostToDevice, st_)) != hipSuccess) return e;
        *dev = reinterpret_cast<T*>(b.base + GUARD);
        return hipSuccess;
    }

    // after the launches: the outputs back to the host; *bad = the buffers whose guards changed
    hipError_t finish(int* bad)
    {
        hipError_t e = hipStreamSynchronize(st_);
        if (e != hipSuccess) return e;
        int nbad = 0;
        std::vector<unsigned char> h;
        for (const Buf& b : bufs_) {
            h.resize(b.bytes + 2 * GUARD);
            if ((e = hipMemcpyAsync(h.data(), b.base, h.size(), hipMemcpyDeviceToHost, st_)) != hipSuccess) return e;
            if ((e = hipStreamSynchronize(st_)) != hipSuccess) return e;
            bool ok = true;
            for (size_t i = 0; i < GUARD && ok; i++) ok = h[i] == SENTINEL && h[GUARD + b.bytes + i] == SENTINEL;
            nbad += ok ? 0 : 1;
            if (b.back && b.bytes) std::memcpy(b.back, h.data() + GUARD, b.bytes);
        }
        *bad = nbad;
        return hipSuccess;
    }

private:
    struct Buf {
        unsigned char* base = nullptr;
        size_t bytes = 0;
        void* back = nullptr;
    };
    std::vector<Buf> bufs_;
    hipStream_t st_ = nullptr;
};

int need_device(const char* who)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return fail(SMG_ERR_NO_DEVICE, "%s: no HIP device: libsmg has no CPU fallback", who);
    return SMG_OK;
}

Ctrl make_ctrl(int done, double tol, double* r_his)
{
    Ctrl c;
    std::memset(&c, 0, sizeof c);
    c.done = done ? 1 : 0;
    c.sumsq = -1.0;
    c.tol = tol;
    c.r_his = r_his;
    c.his_cap = r_his ? 1 : 0;
    c.r_last = c.r_prev = -1.0;
    return c;
}

bool bad_block_shape(int n, int m, int nb) { return n < 1 || m < 1 || m > 64 || nb < 1 || nb > 3; }

}  // namespace

// which side of launch_wide_one's size gate a launch sits on (read-only: the launcher's own predicate)
extern "C" int smg_debug_wide_latency_variant(int n_slices, int kw) { return wide_latency_variant(n_slices, kw) ? 1 : 0; }

extern "C" int smg_debug_eig_gram(int n, int m, int nb_a, const double* Sa, int nb_b, const double* Sb, const double* w, int sym, int done,
                                  double* G, int* groups, int* guard_bad)
{
    return guarded("smg_debug_eig_gram", [&]() -> int {
        if (bad_block_shape(n, m, nb_a) || bad_block_shape(n, m, nb_b) || !Sa || !G || (sym ? nb_b != nb_a : !Sb))
            return fail(SMG_ERR_INVALID, "smg_debug_eig_gram: bad arguments");
        if (int rc = need_device("smg_debug_eig_gram")) return rc;
        Scratch X;
        HIPCHK(X.init());
        const size_t blk = (size_t)n * m;
        const int a = nb_a * m, b = nb_b * m, g = eig_groups(n);
        double *dSa = nullptr, *dSb = nullptr, *dw = nullptr, *dpart = nullptr, *dG = nullptr;
        Ctrl* dctrl = nullptr;
        HIPCHK(X.add(Sa, nullptr, nb_a * blk * sizeof(double), &dSa));
        if (sym) dSb = dSa;
        else HIPCHK(X.add(Sb, nullptr, nb_b * blk * sizeof(double), &dSb));
        if (w) HIPCHK(X.add(w, nullptr, (size_t)n * sizeof(double), &dw));
        HIPCHK(X.add(nullptr, nullptr, eig_gram_part_size(a, b, g) * sizeof(double), &dpart));
        HIPCHK(X.add(G, G, (size_t)a * b * sizeof(double), &dG));
        const Ctrl c = make_ctrl(done, 0.0, nullptr);
        HIPCHK(X.add(&c, nullptr, sizeof c, &dctrl));
        EigBlocks A, B;
        A.nb = nb_a;
        B.nb = nb_b;
        for (int i = 0; i < nb_a; i++) A.p[i] = dSa + i * blk;
        for (int i = 0; i < nb_b; i++) B.p[i] = dSb + i * blk;
        HIPCHK(launch_eig_gram(A, B, n, m, dw, sym != 0, dpart, g, dG, dctrl, X.stream()));
        int bad = 0;
        HIPCHK(X.finish(&bad));
        if (groups) *groups = g;
        if (guard_bad) *guard_bad = bad;
        return SMG_OK;
    });
}

extern "C" int smg_debug_eig_combine(int n, int m, int nb, const double* S, const double* AS, const double* C, int make_p, int done, double* X,
                                     double* AX, double* P, double* AP, int* guard_bad)
{
    return guarded("smg_debug_eig_combine", [&]() -> int {
        if (bad_block_shape(n, m, nb) || !S || !AS || !C || !X || !AX || (make_p && (!P || !AP)))
            return fail(SMG_ERR_INVALID, "smg_debug_eig_combine: bad arguments");
        if (int rc = need_device("smg_debug_eig_combine")) return rc;
        Scratch Z;
        HIPCHK(Z.init());
        const size_t blk = (size_t)n * m, bytes = blk * sizeof(double);
        const int q = nb * m;
        double *dS = nullptr, *dAS = nullptr, *dC = nullptr, *dX = nullptr, *dAX = nullptr, *dP = nullptr, *dAP = nullptr;
        Ctrl* dctrl = nullptr;
        HIPCHK(Z.add(S, nullptr, nb * bytes, &dS));
        HIPCHK(Z.add(AS, nullptr, nb * bytes, &dAS));
        HIPCHK(Z.add(C, nullptr, (size_t)q * 2 * m * sizeof(double), &dC));
        HIPCHK(Z.add(X, X, bytes, &dX));
        HIPCHK(Z.add(AX, AX, bytes, &dAX));
        if (make_p) {
            HIPCHK(Z.add(P, P, bytes, &dP));
            HIPCHK(Z.add(AP, AP, bytes, &dAP));
        }
        const Ctrl c = make_ctrl(done, 0.0, nullptr);
        HIPCHK(Z.add(&c, nullptr, sizeof c, &dctrl));
        EigBlocks Sb, ASb;
        Sb.nb = ASb.nb = nb;
        for (int i = 0; i < nb; i++) { Sb.p[i] = dS + i * blk; ASb.p[i] = dAS + i * blk; }
        HIPCHK(launch_eig_combine(Sb, ASb, n, m, dC, dX, dAX, dP, dAP, dctrl, Z.stream()));
        int bad = 0;
        HIPCHK(Z.finish(&bad));
        if (guard_bad) *guard_bad = bad;
        return SMG_OK;
    });
}

extern "C" int smg_debug_eig_residual(int n, int m, const double* X, const double* AX, const double* mass, const double* lam, int f32, int done,
                                      double* b0, double* u0, float* b32, float* u32, double* res, int* groups, int* guard_bad)
{
    return guarded("smg_debug_eig_residual", [&]() -> int {
        if (bad_block_shape(n, m, 1) || !X || !AX || !mass || !lam || !b0 || !u0 || !res || (f32 && (!b32 || !u32)))
            return fail(SMG_ERR_INVALID, "smg_debug_eig_residual: bad arguments");
        if (int rc = need_device("smg_debug_eig_residual")) return rc;
        Scratch Z;
        HIPCHK(Z.init());
        const size_t cnt = (size_t)n * m;
        const int g = eig_groups(n);
        double *dX = nullptr, *dAX = nullptr, *dmass = nullptr, *dlam = nullptr, *db0 = nullptr, *du0 = nullptr, *dpart = nullptr, *dres = nullptr;
        float *db32 = nullptr, *du32 = nullptr;
        Ctrl* dctrl = nullptr;
        HIPCHK(Z.add(X, nullptr, cnt * sizeof(double), &dX));
        HIPCHK(Z.add(AX, nullptr, cnt * sizeof(double), &dAX));
        HIPCHK(Z.add(mass, nullptr, (size_t)n * sizeof(double), &dmass));
        HIPCHK(Z.add(lam, nullptr, (size_t)m * sizeof(double), &dlam));
        // f32: the fp64 input buffers are handed to the launcher as well; it must leave them alone
        HIPCHK(Z.add(b0, b0, cnt * sizeof(double), &db0));
        HIPCHK(Z.add(u0, u0, cnt * sizeof(double), &du0));
        if (f32) {
            HIPCHK(Z.add(b32, b32, cnt * sizeof(float), &db32));
            HIPCHK(Z.add(u32, u32, cnt * sizeof(float), &du32));
        }
        HIPCHK(Z.add(nullptr, nullptr, (size_t)g * m * sizeof(double), &dpart));
        HIPCHK(Z.add(res, res, (size_t)m * sizeof(double), &dres));
        const Ctrl c = make_ctrl(done, 0.0, nullptr);
        HIPCHK(Z.add(&c, nullptr, sizeof c, &dctrl));
        HIPCHK(launch_eig_residual(dX, dAX, dmass, dlam, n, m, db0, du0, db32, du32, dpart, g, dres, dctrl, Z.stream()));
        int bad = 0;
        HIPCHK(Z.finish(&bad));
        if (groups) *groups = g;
        if (guard_bad) *guard_bad = bad;
        return SMG_OK;
    });
}

extern "C" int smg_debug_krylov(int op, int n, int k, double* v0, double* v1, double* v2, double* v3, float* e, double* s, int* restart, double tol,
                                int done, double* ctrl_d, int* ctrl_i, int* groups, int* guard_bad)
{
    return guarded("smg_debug_krylov", [&]() -> int {
        // the n x k operands each op reads or writes, in the order v0, v1, ...
        static const int n_vec[] = {3, 2, 2, 4, 3, 1};
        if (op < SMG_KRY_DOTS_ZR_ZQ || op > SMG_KRY_WIDEN || n < 1 || k < 1 || (long)n * k > (1L << 30))
            return fail(SMG_ERR_INVALID, "smg_debug_krylov: bad arguments");
        double* v[4] = {v0, v1, v2, v3};
        for (int i = 0; i < n_vec[op]; i++)
            if (!v[i]) return fail(SMG_ERR_INVALID, "smg_debug_krylov: operand v%d missing", i);
        if ((op <= SMG_KRY_STEP_DECIDE && !s) || (op == SMG_KRY_WIDEN && !e)) return fail(SMG_ERR_INVALID, "smg_debug_krylov: bad arguments");
        if (int rc = need_device("smg_debug_krylov")) return rc;
        Scratch Z;
        HIPCHK(Z.init());
        const size_t cnt = (size_t)n * k;
        double* dv[4] = {nullptr, nullptr, nullptr, nullptr};
        for (int i = 0; i < n_vec[op]; i++) HIPCHK(Z.add(v[i], v[i], cnt * sizeof(double), &dv[i]));
        float* de = nullptr;
        if (op == SMG_KRY_WIDEN) HIPCHK(Z.add(e, e, cnt * sizeof(float), &de));
        KryDev K;
        K.n = n;
        K.k = k;
        K.groups = kry_groups(n, k);
        const int rs0 = 0;
        HIPCHK(Z.add(nullptr, nullptr, (size_t)2 * K.groups * k * sizeof(double), &K.part));
        if (s) HIPCHK(Z.add(s, s, (size_t)KS_SLOTS * k * sizeof(double), &K.s));
        HIPCHK(Z.add(restart ? restart : &rs0, restart, sizeof(int), &K.restart));
        const double his0 = -1.0;
        double* dhis = nullptr;
        Ctrl* dctrl = nullptr;
        HIPCHK(Z.add(&his0, ctrl_d ? ctrl_d + 1 : nullptr, sizeof(double), &dhis));
        Ctrl c = make_ctrl(done, tol, dhis);
        HIPCHK(Z.add(&c, &c, sizeof c, &dctrl));
        hipStream_t st = Z.stream();
        switch (op) {
            case SMG_KRY_DOTS_ZR_ZQ: HIPCHK(launch_kry_dots_zr_zq(K, dv[0], dv[1], dv[2], dctrl, st)); break;
            case SMG_KRY_DIRECTION: HIPCHK(launch_kry_direction(K, dv[0], dv[1], dctrl, st)); break;
            case SMG_KRY_DOTS_PQ: HIPCHK(launch_kry_dots_pq(K, dv[0], dv[1], dctrl, st)); break;
            case SMG_KRY_STEP_DECIDE: HIPCHK(launch_kry_step_decide(K, dv[0], dv[1], dv[2], dv[3], dctrl, st)); break;
            case SMG_KRY_PRECOND_IN: HIPCHK(launch_kry_precond_in(dv[0], dv[1], dv[2], cnt, dctrl, st)); break;
            default: HIPCHK(launch_kry_widen(de, dv[0], cnt, dctrl, st)); break;
        }
        int bad = 0;
        HIPCHK(Z.finish(&bad));
        if (ctrl_d) ctrl_d[0] = c.sumsq;
        if (ctrl_i) { ctrl_i[0] = c.n_his; ctrl_i[1] = c.done; ctrl_i[2] = c.status; }
        if (groups) *groups = K.groups;
        if (guard_bad) *guard_bad = bad;
        return SMG_OK;
    });
}

namespace {

// the corner lists and source lists a geodesics hook is handed: in range, monotone, every source set non-empty
const char* check_geo_lists(int op, int n, int nF, int k, const int* F, const int* m_ptr, const int* m_idx, const int* src_ptr, const int* src)
{
    if (op == SMG_GEO_BASIS || op == SMG_GEO_DIVERGENCE) {
        if (!F || nF < 1) return "missing faces";
        for (size_t i = 0; i < (size_t)nF * 3; i++) if (F[i] < 0 || F[i] >= n) return "face index out of range";
    }
    if (op == SMG_GEO_DIVERGENCE) {
        if (!m_ptr || !m_idx || m_ptr[0] != 0) return "missing or bad corner lists";
        for (int v = 0; v < n; v++) if (m_ptr[v + 1] < m_ptr[v]) return "corner list pointers not monotone";
        for (int p = 0; p < m_ptr[n]; p++) if (m_idx[p] < 0 || m_idx[p] >= 3 * nF) return "corner index out of range";
    }
    if (op == SMG_GEO_SCATTER || op == SMG_GEO_SHIFT) {
        if (!src_ptr || !src || src_ptr[0] != 0) return "missing or bad source lists";
        for (int c = 0; c < k; c++) if (src_ptr[c + 1] <= src_ptr[c]) return "empty source set";
        for (int p = 0; p < src_ptr[k]; p++) if (src[p] < 0 || src[p] >= n) return "source index out of range";
    }
    return nullptr;
}

}  // namespace

extern "C" int smg_debug_geodesics(int op, int n, int nF, int k, const int* F, const int* m_ptr, const int* m_idx, const int* src_ptr,
                                   const int* src, const double* in, double* W, double* Af, double* out, int ld_out, int* guard_bad)
{
    return guarded("smg_debug_geodesics", [&]() -> int {
        if (op < SMG_GEO_BASIS || op > SMG_GEO_SHIFT || n < 1 || k < 1 || !in) return fail(SMG_ERR_INVALID, "smg_debug_geodesics: bad arguments");
        if (op == SMG_GEO_BASIS ? (!W || !Af) : (!out || ld_out < n || (op == SMG_GEO_DIVERGENCE && (!W || !Af))))
            return fail(SMG_ERR_INVALID, "smg_debug_geodesics: bad arguments");
        if (const char* why = check_geo_lists(op, n, nF, k, F, m_ptr, m_idx, src_ptr, src))
            return fail(SMG_ERR_INVALID, "smg_debug_geodesics: %s", why);
        if (int rc = need_device("smg_debug_geodesics")) return rc;
        Scratch X;
        HIPCHK(X.init());
        const size_t blk = (size_t)n * k, oblk = (size_t)ld_out * k;
        int *dF = nullptr, *dmp = nullptr, *dmi = nullptr, *dsp = nullptr, *ds = nullptr;
        double *din = nullptr, *dW = nullptr, *dAf = nullptr, *dout = nullptr, *dmean = nullptr;
        if (op == SMG_GEO_BASIS || op == SMG_GEO_DIVERGENCE) {
            HIPCHK(X.add(F, nullptr, (size_t)nF * 3 * sizeof(int), &dF));
            const bool basis = op == SMG_GEO_BASIS;   // the basis is the output of BASIS, an input of DIVERGENCE
            HIPCHK(X.add(W, basis ? W : nullptr, (size_t)nF * 9 * sizeof(double), &dW));
            HIPCHK(X.add(Af, basis ? Af : nullptr, (size_t)nF * sizeof(double), &dAf));
        }
        if (op == SMG_GEO_DIVERGENCE) {
            HIPCHK(X.add(m_ptr, nullptr, ((size_t)n + 1) * sizeof(int), &dmp));
            HIPCHK(X.add(m_idx, nullptr, (size_t)m_ptr[n] * sizeof(int), &dmi));
        }
        if (op == SMG_GEO_SCATTER || op == SMG_GEO_SHIFT) {
            HIPCHK(X.add(src_ptr, nullptr, ((size_t)k + 1) * sizeof(int), &dsp));
            HIPCHK(X.add(src, nullptr, (size_t)src_ptr[k] * sizeof(int), &ds));
        }
        if (op != SMG_GEO_SCATTER) HIPCHK(X.add(in, nullptr, (op == SMG_GEO_BASIS ? (size_t)n * 3 : blk) * sizeof(double), &din));
        if (op != SMG_GEO_BASIS) HIPCHK(X.add(out, out, oblk * sizeof(double), &dout));
        if (op == SMG_GEO_SHIFT) HIPCHK(X.add(nullptr, nullptr, (size_t)k * sizeof(double), &dmean));
        if (op == SMG_GEO_BASIS) HIPCHK(launch_geo_basis(din, dF, nF, dW, dAf, X.stream()));
        else if (op == SMG_GEO_SCATTER) HIPCHK(launch_geo_scatter(n, k, dsp, ds, dout, ld_out, X.stream()));
        else if (op == SMG_GEO_DIVERGENCE) HIPCHK(launch_geo_divergence(n, k, dF, dW, dAf, dmp, dmi, din, n, dout, ld_out, X.stream()));
        else HIPCHK(launch_geo_shift(n, k, dsp, ds, din, n, dmean, dout, ld_out, X.stream()));
        int bad = 0;
        HIPCHK(X.finish(&bad));
        if (guard_bad) *guard_bad = bad;
        return SMG_OK;
    });
}

extern "C" int smg_debug_arap(int op, int n, const int* rowptr, const int* col, const double* w, const double* P0, const double* P,
                              const double* R_in, double* out, int* guard_hits)
{
    return guarded("smg_debug_arap", [&]() -> int {
        if (op < SMG_ARAP_COVARIANCE || op > SMG_ARAP_ENERGY || n < 1 || !rowptr || !col || !w || !P0 || !out)
            return fail(SMG_ERR_INVALID, "smg_debug_arap: bad arguments");
        if ((op != SMG_ARAP_RHS && !P) || (op >= SMG_ARAP_RHS && !R_in)) return fail(SMG_ERR_INVALID, "smg_debug_arap: op %d misses an operand", op);
        if (rowptr[0] != 0) return fail(SMG_ERR_INVALID, "smg_debug_arap: rowptr[0] != 0");
        if (const char* why = check_compressed(n, n, rowptr, col)) return fail(SMG_ERR_INVALID, "smg_debug_arap: %s", why);
        if (int rc = need_device("smg_debug_arap")) return rc;
        Scratch X;
        HIPCHK(X.init());
        const size_t nnz = (size_t)rowptr[n], vec = (size_t)n * sizeof(double);
        const size_t out_bytes = op <= SMG_ARAP_ROTATIONS ? 9 * vec : op == SMG_ARAP_RHS ? 3 * vec : op == SMG_ARAP_VERTEX_ENERGY ? vec : sizeof(double);
        int *dptr = nullptr, *dcol = nullptr;
        double *dw = nullptr, *dP0 = nullptr, *dP = nullptr, *dR = nullptr, *dout = nullptr, *dterm = nullptr, *dpart = nullptr;
        HIPCHK(X.add(rowptr, nullptr, ((size_t)n + 1) * sizeof(int), &dptr));
        HIPCHK(X.add(col, nullptr, nnz * sizeof(int), &dcol));
        HIPCHK(X.add(w, nullptr, nnz * sizeof(double), &dw));
        HIPCHK(X.add(P0, nullptr, 3 * vec, &dP0));
        if (P) HIPCHK(X.add(P, nullptr, 3 * vec, &dP));
        if (op >= SMG_ARAP_RHS) HIPCHK(X.add(R_in, nullptr, 9 * vec, &dR));
        HIPCHK(X.add(out, out, out_bytes, &dout));
        if (op == SMG_ARAP_ROTATIONS || op == SMG_ARAP_ENERGY) HIPCHK(X.add(nullptr, nullptr, vec, &dterm));
        if (op == SMG_ARAP_ENERGY) HIPCHK(X.add(nullptr, nullptr, (size_t)fixed_sum_groups(n) * sizeof(double), &dpart));
        hipStream_t st = X.stream();
        switch (op) {
            case SMG_ARAP_COVARIANCE: HIPCHK(launch_arap_covariance(n, dptr, dcol, dw, dP0, dP, dout, st)); break;
            case SMG_ARAP_ROTATIONS: HIPCHK(launch_arap_rotations(n, dptr, dcol, dw, dP0, dP, dout, dterm, st)); break;
            case SMG_ARAP_RHS: HIPCHK(launch_arap_rhs(n, dptr, dcol, dw, dP0, dR, dout, n, st)); break;
            case SMG_ARAP_VERTEX_ENERGY: HIPCHK(launch_arap_vertex_energy(n, dptr, dcol, dw, dP0, dP, dR, dout, st)); break;
            default:
                HIPCHK(launch_arap_vertex_energy(n, dptr, dcol, dw, dP0, dP, dR, dterm, st));
                HIPCHK(launch_fixed_sum(dterm, n, dpart, dout, st));
                break;
        }
        int bad = 0;
        HIPCHK(X.finish(&bad));
        if (guard_hits) *guard_hits = bad;
        return SMG_OK;
    });
}

extern "C" int smg_debug_fixed_reduce(int op, int n, const double* term, double* out, int* groups, int* guard_bad)
{
    return guarded("smg_debug_fixed_reduce", [&]() -> int {
        if ((op != SMG_FIXED_SUM && op != SMG_FIXED_MAX) || n <= 0 || !term || !out) return fail(SMG_ERR_INVALID, "smg_debug_fixed_reduce: bad arguments");
        if (int rc = need_device("smg_debug_fixed_reduce")) return rc;
        Scratch X;
        HIPCHK(X.init());
        const int g = fixed_sum_groups(n);
        double *dterm = nullptr, *dpart = nullptr, *dout = nullptr;
        HIPCHK(X.add(term, nullptr, (size_t)n * sizeof(double), &dterm));
        HIPCHK(X.add(nullptr, nullptr, (size_t)g * sizeof(double), &dpart));      // exactly the chunks: one more written shows in the guard
        HIPCHK(X.add(nullptr, out, sizeof(double), &dout));
        if (op == SMG_FIXED_SUM) HIPCHK(launch_fixed_sum(dterm, n, dpart, dout, X.stream()));
        else HIPCHK(launch_fixed_max(dterm, n, dpart, dout, X.stream()));
        int bad = 0;
        HIPCHK(X.finish(&bad));
        if (groups) *groups = g;
        if (guard_bad) *guard_bad = bad;
        return SMG_OK;
    });
}

// the body of smg_debug_membrane and smg_debug_membrane_material: the face ops run the kernels of `material`
static int debug_membrane(const char* who, int material, int op, int nV, int nF, const int* F, const double* V0, const double* P, const double* in,
                          const smg_membrane_params* p, double* out, int* guard_hits)
{
    return guarded(who, [&]() -> int {
        if (material < 0 || material > 2)
            return fail(SMG_ERR_INVALID, "%s: material %d is not 0 (neo-Hookean), 1 (StVK) or 2 (tension-field StVK)", who, material);
        if (op < SMG_MEM_REST || op > SMG_MEM_OBJECTIVE || nV < 1 || nF < 1 || !F || !p || !out) return fail(SMG_ERR_INVALID, "%s: bad arguments", who);
        const bool needs_rest = op <= SMG_MEM_ENERGY || op == SMG_MEM_OBJECTIVE, needs_pose = (op >= SMG_MEM_FACES_RAW && op <= SMG_MEM_PRESSURE) || op == SMG_MEM_OBJECTIVE;
        if ((needs_rest && !V0) || (needs_pose && !P) || (op >= SMG_MEM_MATRIX && !in)) return fail(SMG_ERR_INVALID, "%s: op %d misses an operand", who, op);
        if (int rc = check_faces(who, F, nF, nV)) return rc;
        if (int rc = need_device(who)) return rc;
        double alpha, beta;
        lame(*p, alpha, beta);
        std::vector<int> Fv(F, F + 3 * (size_t)nF), mp, mi;
        vertex_corner_lists(Fv, nV, mp, mi);
        MembraneLists L;
        membrane_lists(F, nF, nV, L);
        const int nB = (int)L.bcol.size();
        const size_t D = sizeof(double), nf = (size_t)nF, nv = (size_t)nV, n3 = 3 * nv;
        const size_t out_n = op == SMG_MEM_REST ? 5 * nf : op <= SMG_MEM_FACES ? 55 * nf : op == SMG_MEM_ENERGY ? nf : op == SMG_MEM_PRESSURE ? 6 * nf + nv + n3
                             : op == SMG_MEM_MATRIX ? 9 * (size_t)nB : op == SMG_MEM_GRADIENT ? 2 * n3 : 2 * n3 + nf + nv + 1;
        const size_t in_n = op == SMG_MEM_MATRIX ? 45 * nf + nv : op == SMG_MEM_GRADIENT ? 9 * nf + nv + 3 * n3 : op == SMG_MEM_OBJECTIVE ? nv + 4 * n3 + 1 : 0;
        Scratch X;
        HIPCHK(X.init());
        hipStream_t st = X.stream();
        int *dF = nullptr, *dmp = nullptr, *dmi = nullptr, *dbrow = nullptr, *dbcol = nullptr, *dbptr = nullptr, *dcp = nullptr, *dcs = nullptr;
        double *dV0 = nullptr, *dP = nullptr, *din = nullptr, *dout = nullptr, *drest = nullptr, *dpart = nullptr;
        HIPCHK(X.add(F, nullptr, 3 * nf * sizeof(int), &dF));
        if (V0) HIPCHK(X.add(V0, nullptr, n3 * D, &dV0));
        if (P) HIPCHK(X.add(P, nullptr, n3 * D, &dP));
        if (in_n) HIPCHK(X.add(in, nullptr, in_n * D, &din));
        HIPCHK(X.add(out, out, out_n * D, &dout));
        if (needs_rest && op != SMG_MEM_REST) {
            HIPCHK(X.add(nullptr, nullptr, 5 * nf * D, &drest));
            HIPCHK(launch_membrane_rest(nF, dF, dV0, p->thickness, drest, st));
        }
        if (op == SMG_MEM_PRESSURE || op == SMG_MEM_GRADIENT) {
            HIPCHK(X.add(mp.data(), nullptr, mp.size() * sizeof(int), &dmp));
            HIPCHK(X.add(mi.data(), nullptr, mi.size() * sizeof(int), &dmi));
        }
        switch (op) {
            case SMG_MEM_REST: HIPCHK(launch_membrane_rest(nF, dF, dV0, p->thickness, dout, st)); break;
            case SMG_MEM_FACES_RAW:
            case SMG_MEM_FACES:
                HIPCHK(launch_membrane_faces_material(material, op == SMG_MEM_FACES ? 2 : 1, nF, dF, dP, dV0, drest, p->thickness, alpha, beta, p->eig_floor, p->eig_value, dout,
                                                      dout + nf, dout + 10 * nf, st));
                break;
            case SMG_MEM_ENERGY:
                HIPCHK(launch_membrane_faces_material(material, 0, nF, dF, dP, dV0, drest, p->thickness, alpha, beta, p->eig_floor, p->eig_value, dout, nullptr, nullptr, st));
                break;
            case SMG_MEM_PRESSURE:
                HIPCHK(launch_membrane_pressure(nV, nF, dF, dP, dmp, dmi, p->pressure, dout, dout + 6 * nf, dout + 6 * nf + nv, st));
                break;
            case SMG_MEM_MATRIX:
                HIPCHK(X.add(L.brow.data(), nullptr, L.brow.size() * sizeof(int), &dbrow));
                HIPCHK(X.add(L.bcol.data(), nullptr, L.bcol.size() * sizeof(int), &dbcol));
                HIPCHK(X.add(L.bptr.data(), nullptr, L.bptr.size() * sizeof(int), &dbptr));
                HIPCHK(X.add(L.c_ptr.data(), nullptr, L.c_ptr.size() * sizeof(int), &dcp));
                HIPCHK(X.add(L.c_src.data(), nullptr, L.c_src.size() * sizeof(int), &dcs));
                HIPCHK(launch_membrane_matrix(nB, dbrow, dbcol, dbptr, dcp, dcs, din, nF, p->dt * p->dt, din + 45 * nf, p->mass_scale, dout, st));
                break;
            case SMG_MEM_GRADIENT: {
                const double* mass0 = din + 9 * nf;
                HIPCHK(launch_membrane_gradient(nV, dmp, dmi, din, nF, mass0, p->mass_scale, p->dt, mass0 + nv, mass0 + nv + n3, mass0 + nv + 2 * n3, dout,
                                                dout + n3, st));
                break;
            }
            default: {
                const double *qdot = din + nv, *dx = qdot + n3, *qdot0 = dx + n3, *fext = qdot0 + n3;
                double* terms = dout + 2 * n3;
                HIPCHK(X.add(nullptr, nullptr, (size_t)fixed_sum_groups(nF + nV) * D, &dpart));
                HIPCHK(launch_membrane_trial(nV, qdot, dx, in[nv + 4 * n3], qdot0, dP, fext, din, p->mass_scale, p->dt, dout, dout + n3, terms + nf, st));
                HIPCHK(launch_membrane_faces_material(material, 0, nF, dF, dout + n3, dV0, drest, p->thickness, alpha, beta, p->eig_floor, p->eig_value, terms, nullptr, nullptr, st));
                HIPCHK(launch_fixed_sum(terms, nF + nV, dpart, terms + nf + nv, st));
                break;
            }
        }
        int bad = 0;
        HIPCHK(X.finish(&bad));
        if (guard_hits) *guard_hits = bad;
        return SMG_OK;
    });
}

extern "C" int smg_debug_membrane(int op, int nV, int nF, const int* F, const double* V0, const double* P, const double* in,
                                  const smg_membrane_params* p, double* out, int* guard_hits)
{
    return debug_membrane("smg_debug_membrane", 0, op, nV, nF, F, V0, P, in, p, out, guard_hits);
}

extern "C" int smg_debug_membrane_material(int material, int op, int nV, int nF, const int* F, const double* V0, const double* P, const double* in,
                                           const smg_membrane_params* p, double* out, int* guard_hits)
{
    return debug_membrane("smg_debug_membrane_material", material, op, nV, nF, F, V0, P, in, p, out, guard_hits);
}

extern "C" int smg_debug_param(int op, int nV, int nF, const int* F, const double* V0, const double* UV, const double* R_in, double* out,
                               int* guard_hits)
{
    return guarded("smg_debug_param", [&]() -> int {
        if (op < SMG_PARAM_REST || op > SMG_PARAM_DISTORTION || nV < 1 || nF < 1 || !F || !V0 || !out) return fail(SMG_ERR_INVALID, "smg_debug_param: bad arguments");
        const bool needs_uv = op != SMG_PARAM_REST && op != SMG_PARAM_RHS, needs_rot = op >= SMG_PARAM_RHS && op <= SMG_PARAM_ENERGY;
        if ((needs_uv && !UV) || (needs_rot && !R_in)) return fail(SMG_ERR_INVALID, "smg_debug_param: op %d misses an operand", op);
        if (int rc = check_faces("smg_debug_param", F, nF, nV)) return rc;
        if (int rc = need_device("smg_debug_param")) return rc;
        const size_t D = sizeof(double), nf = (size_t)nF, nv = (size_t)nV;
        const size_t out_n = op == SMG_PARAM_REST ? 6 * nf : op == SMG_PARAM_COVARIANCE ? 4 * nf : op == SMG_PARAM_ROTATIONS ? 2 * nf : op == SMG_PARAM_RHS ? 2 * nv
                             : op == SMG_PARAM_FACE_ENERGY ? nf : op == SMG_PARAM_ENERGY ? 1 : 3 * nf;
        Scratch X;
        HIPCHK(X.init());
        hipStream_t st = X.stream();
        int *dF = nullptr, *dmp = nullptr, *dmi = nullptr;
        double *dV0 = nullptr, *dUV = nullptr, *dR = nullptr, *dout = nullptr, *drest = nullptr, *dterm = nullptr, *dpart = nullptr;
        HIPCHK(X.add(F, nullptr, 3 * nf * sizeof(int), &dF));
        HIPCHK(X.add(V0, nullptr, 3 * nv * D, &dV0));
        if (UV) HIPCHK(X.add(UV, nullptr, 2 * nv * D, &dUV));
        if (needs_rot) HIPCHK(X.add(R_in, nullptr, 2 * nf * D, &dR));
        HIPCHK(X.add(out, out, out_n * D, &dout));
        if (op != SMG_PARAM_REST) {
            HIPCHK(X.add(nullptr, nullptr, 6 * nf * D, &drest));
            HIPCHK(launch_param_rest(nF, dF, dV0, drest, st));
        }
        if (op == SMG_PARAM_ROTATIONS || op == SMG_PARAM_ENERGY) HIPCHK(X.add(nullptr, nullptr, nf * D, &dterm));
        std::vector<int> mp, mi;
        switch (op) {
            case SMG_PARAM_REST: HIPCHK(launch_param_rest(nF, dF, dV0, dout, st)); break;
            case SMG_PARAM_COVARIANCE: HIPCHK(launch_param_covariance(nF, dF, drest, dUV, nV, dout, st)); break;
            case SMG_PARAM_ROTATIONS: HIPCHK(launch_param_local(nF, dF, drest, dUV, nV, dout, dterm, st)); break;
            case SMG_PARAM_RHS:
                vertex_corner_lists(std::vector<int>(F, F + 3 * nf), nV, mp, mi);
                HIPCHK(X.add(mp.data(), nullptr, mp.size() * sizeof(int), &dmp));
                HIPCHK(X.add(mi.data(), nullptr, mi.size() * sizeof(int), &dmi));
                HIPCHK(launch_param_rhs(nV, nF, dmp, dmi, drest, dR, dout, nV, st));
                break;
            case SMG_PARAM_FACE_ENERGY: HIPCHK(launch_param_face_energy(nF, dF, drest, dUV, nV, dR, dout, st)); break;
            case SMG_PARAM_ENERGY:
                HIPCHK(X.add(nullptr, nullptr, (size_t)fixed_sum_groups(nF) * D, &dpart));
                HIPCHK(launch_param_face_energy(nF, dF, drest, dUV, nV, dR, dterm, st));
                HIPCHK(launch_fixed_sum(dterm, nF, dpart, dout, st));
                break;
            default: HIPCHK(launch_param_distortion(nF, dF, drest, dUV, nV, dout, nullptr, nullptr, st)); break;
        }
        int bad = 0;
        HIPCHK(X.finish(&bad));
        if (guard_hits) *guard_hits = bad;
        return SMG_OK;
    });
}

extern "C" int smg_debug_pd(int op, int nV, int nF, const int* F, const double* V0, const double* P, const double* in, const smg_pd_params* p,
                            double* out, int* guard_hits)
{
    return guarded("smg_debug_pd", [&]() -> int {
        if (op < SMG_PD_REST || op > SMG_PD_STRAIN || nV < 1 || nF < 1 || !F || !p || !out) return fail(SMG_ERR_INVALID, "smg_debug_pd: bad arguments");
        const bool needs_rest = op != SMG_PD_ENERGY && op != SMG_PD_FINISH && op != SMG_PD_VERTICES;
        const bool needs_pose = op == SMG_PD_FACES || op == SMG_PD_FACES_STEP || op == SMG_PD_PREDICT || op == SMG_PD_FINISH || op == SMG_PD_STRAIN;
        const bool needs_in = op == SMG_PD_PREDICT || op == SMG_PD_VERTICES || op == SMG_PD_ENERGY || op == SMG_PD_FINISH;
        if ((needs_rest && !V0) || (needs_pose && !P) || (needs_in && !in)) return fail(SMG_ERR_INVALID, "smg_debug_pd: op %d misses an operand", op);
        if (int rc = check_faces("smg_debug_pd", F, nF, nV)) return rc;
        if (int rc = need_device("smg_debug_pd")) return rc;
        const size_t D = sizeof(double), nf = (size_t)nF, nv = (size_t)nV, n3 = 3 * nv;
        const size_t out_n = op == SMG_PD_REST ? 4 * nf : op == SMG_PD_FACES ? 24 * nf : op == SMG_PD_FACES_STEP ? 10 * nf : op == SMG_PD_MASS ? nv
                             : op == SMG_PD_PREDICT ? 2 * n3 : op == SMG_PD_VERTICES ? n3 + 2 * nv : op == SMG_PD_ENERGY ? 1 : op == SMG_PD_FINISH ? 2 * n3 : 5 * nf;
        const size_t in_n = op == SMG_PD_PREDICT ? n3 : op == SMG_PD_VERTICES ? 9 * nf + nv + 2 * n3 : op == SMG_PD_ENERGY ? nf + nv : op == SMG_PD_FINISH ? n3 : 0;
        Scratch X;
        HIPCHK(X.init());
        hipStream_t st = X.stream();
        int *dF = nullptr, *dmp = nullptr, *dmi = nullptr;
        double *dV0 = nullptr, *dP = nullptr, *din = nullptr, *dout = nullptr, *drest = nullptr, *dQ = nullptr, *dQn = nullptr, *dm0 = nullptr, *dpart = nullptr;
        HIPCHK(X.add(F, nullptr, 3 * nf * sizeof(int), &dF));
        if (V0) HIPCHK(X.add(V0, nullptr, n3 * D, &dV0));
        if (P) HIPCHK(X.add(P, nullptr, n3 * D, &dP));
        if (in_n) HIPCHK(X.add(in, nullptr, in_n * D, &din));
        HIPCHK(X.add(out, out, out_n * D, &dout));
        if (op == SMG_PD_FACES || op == SMG_PD_FACES_STEP || op == SMG_PD_STRAIN) {
            HIPCHK(X.add(nullptr, nullptr, 4 * nf * D, &drest));
            HIPCHK(launch_pd_rest(nF, dF, dV0, drest, st));
        }
        std::vector<int> mp, mi;
        if (op == SMG_PD_MASS || op == SMG_PD_PREDICT || op == SMG_PD_VERTICES) {
            vertex_corner_lists(std::vector<int>(F, F + 3 * nf), nV, mp, mi);
            HIPCHK(X.add(mp.data(), nullptr, mp.size() * sizeof(int), &dmp));
            HIPCHK(X.add(mi.data(), nullptr, mi.size() * sizeof(int), &dmi));
        }
        switch (op) {
            case SMG_PD_REST: HIPCHK(launch_pd_rest(nF, dF, dV0, dout, st)); break;
            case SMG_PD_FACES:
                HIPCHK(launch_pd_faces(nF, dF, drest, dP, 3, 1, p->stiffness, p->sigma_min, p->sigma_max, dout + 14 * nf, dout + 15 * nf, dout, dout + 6 * nf,
                                       dout + 8 * nf, st));
                break;
            case SMG_PD_FACES_STEP:
                HIPCHK(X.add(nullptr, nullptr, n3 * D, &dQ));
                HIPCHK(launch_arap_columns(nV, dP, dQ, nV, st));
                HIPCHK(launch_pd_faces(nF, dF, drest, dQ, 1, nv, p->stiffness, p->sigma_min, p->sigma_max, dout, dout + nf, nullptr, nullptr, nullptr, st));
                break;
            case SMG_PD_MASS:
                HIPCHK(X.add(nullptr, nullptr, 6 * nf * D, &dQn));
                HIPCHK(launch_membrane_pressure(nV, nF, dF, dV0, dmp, dmi, 0.0, dQn, dout, nullptr, st));
                break;
            case SMG_PD_PREDICT:
                HIPCHK(X.add(nullptr, nullptr, 6 * nf * D, &dQn));
                HIPCHK(X.add(nullptr, nullptr, nv * D, &dm0));
                HIPCHK(launch_membrane_pressure(nV, nF, dF, dV0, dmp, dmi, 0.0, dQn, dm0, nullptr, st));
                HIPCHK(launch_membrane_pressure(nV, nF, dF, dP, dmp, dmi, p->pressure, dQn, nullptr, dout, st));
                HIPCHK(launch_pd_predict(nV, dP, din, dout, dm0, p->dt, p->density, p->gravity, dout + n3, nV, st));
                break;
            case SMG_PD_VERTICES: {
                const double *m0 = din + 9 * nf, *S = m0 + nv, *Q = S + n3;
                HIPCHK(launch_pd_vertices(nV, nF, dmp, dmi, din, m0, p->density / (p->dt * p->dt), S, Q, nV, dout, nV, dout + n3, dout + n3 + nv, st));
                break;
            }
            case SMG_PD_ENERGY:
                HIPCHK(X.add(nullptr, nullptr, (size_t)fixed_sum_groups(nF + nV) * D, &dpart));
                HIPCHK(launch_fixed_sum(din, nF + nV, dpart, dout, st));
                break;
            case SMG_PD_FINISH:
                HIPCHK(hipMemcpyAsync(dout + n3, dP, n3 * D, hipMemcpyDeviceToDevice, st));
                HIPCHK(launch_pd_finish(nV, din, nV, p->dt, dout + n3, dout, st));
                break;
            default: {
                double *dFg = nullptr, *dsig = nullptr, *dT = nullptr, *det = nullptr, *dsh = nullptr;
                HIPCHK(X.add(nullptr, nullptr, 6 * nf * D, &dFg));
                HIPCHK(X.add(nullptr, nullptr, 2 * nf * D, &dsig));
                HIPCHK(X.add(nullptr, nullptr, 6 * nf * D, &dT));
                HIPCHK(X.add(nullptr, nullptr, nf * D, &det));
                HIPCHK(X.add(nullptr, nullptr, 9 * nf * D, &dsh));
                HIPCHK(launch_pd_faces(nF, dF, drest, dP, 3, 1, p->stiffness, p->sigma_min, p->sigma_max, det, dsh, dFg, dsig, dT, st));
                HIPCHK(launch_pd_strain_terms(nF, drest, dFg, dsig, dT, p->sigma_min, p->sigma_max, dout, st));
                break;
            }
        }
        int bad = 0;
        HIPCHK(X.finish(&bad));
        if (guard_hits) *guard_hits = bad;
        return SMG_OK;
    });
}

extern "C" int smg_debug_denoise(int op, int nV, int nF, const int* F, const double* V0, const double* P, const double* in, const smg_denoise_params* p,
                                 double* out, int* guard_hits)
{
    return guarded("smg_debug_denoise", [&]() -> int {
        if (op < SMG_DN_REST || op > SMG_DN_ENERGY || nV < 1 || nF < 1 || !F || !p || !out) return fail(SMG_ERR_INVALID, "smg_debug_denoise: bad arguments");
        const bool needs_rest = op != SMG_DN_ENERGY, needs_pose = op == SMG_DN_PROJECT, needs_in = op >= SMG_DN_FILTER;
        if ((needs_rest && !V0) || (needs_pose && !P) || (needs_in && !in)) return fail(SMG_ERR_INVALID, "smg_debug_denoise: op %d misses an operand", op);
        if (op == SMG_DN_FILTER && (!(p->sigma_s > 0.0) || !(p->sigma_r > 0.0) || p->normal_iters < 0))
            return fail(SMG_ERR_INVALID, "smg_debug_denoise: the filter takes sigma_s > 0, sigma_r > 0 and normal_iters >= 0");
        if (int rc = check_faces("smg_debug_denoise", F, nF, nV)) return rc;
        if (int rc = need_device("smg_debug_denoise")) return rc;
        const size_t D = sizeof(double), nf = (size_t)nF, nv = (size_t)nV, n3 = 3 * nv;
        const size_t out_n = op == SMG_DN_REST ? 10 * nf : op == SMG_DN_SPACING ? nf : op == SMG_DN_FILTER ? 3 * nf : op == SMG_DN_PROJECT ? 10 * nf
                             : op == SMG_DN_RHS ? 2 * n3 : 1;
        const size_t in_n = op == SMG_DN_FILTER || op == SMG_DN_PROJECT ? 3 * nf : op == SMG_DN_RHS ? 9 * nf + n3 : op == SMG_DN_ENERGY ? nf + nv : 0;
        Scratch X;
        HIPCHK(X.init());
        hipStream_t st = X.stream();
        int *dF = nullptr, *dmp = nullptr, *dmi = nullptr, *dnp = nullptr, *dni = nullptr;
        double *dV0 = nullptr, *dP = nullptr, *din = nullptr, *dout = nullptr, *drest = nullptr, *dQ = nullptr, *dQn = nullptr, *dm2 = nullptr, *dpart = nullptr;
        HIPCHK(X.add(F, nullptr, 3 * nf * sizeof(int), &dF));
        if (V0) HIPCHK(X.add(V0, nullptr, n3 * D, &dV0));
        if (P) HIPCHK(X.add(P, nullptr, n3 * D, &dP));
        if (in_n) HIPCHK(X.add(in, nullptr, in_n * D, &din));
        HIPCHK(X.add(out, out, out_n * D, &dout));
        if (op == SMG_DN_SPACING || op == SMG_DN_FILTER || op == SMG_DN_PROJECT) {
            HIPCHK(X.add(nullptr, nullptr, 10 * nf * D, &drest));
            HIPCHK(launch_denoise_rest(nF, dF, dV0, drest, st));
        }
        std::vector<int> mp, mi, np, ni;
        if (op == SMG_DN_SPACING || op == SMG_DN_FILTER || op == SMG_DN_RHS) {
            const std::vector<int> Fv(F, F + 3 * nf);
            vertex_corner_lists(Fv, nV, mp, mi);
            if (op == SMG_DN_RHS) {
                HIPCHK(X.add(mp.data(), nullptr, mp.size() * sizeof(int), &dmp));
                HIPCHK(X.add(mi.data(), nullptr, mi.size() * sizeof(int), &dmi));
            } else {
                if (!face_neighbours(Fv, mp, mi, np, ni)) return fail(SMG_ERR_INVALID, "smg_debug_denoise: the neighbourhoods have more than 2^31 - 1 entries");
                HIPCHK(X.add(np.data(), nullptr, np.size() * sizeof(int), &dnp));
                HIPCHK(X.add(ni.data(), nullptr, ni.size() * sizeof(int), &dni));
            }
        }
        switch (op) {
            case SMG_DN_REST: HIPCHK(launch_denoise_rest(nF, dF, dV0, dout, st)); break;
            case SMG_DN_SPACING: HIPCHK(launch_denoise_spacing(nF, dnp, dni, drest, dout, st)); break;
            case SMG_DN_FILTER: {
                // the object's ping-pong: the host swaps the pair between the launches; the result is copied into the guarded output
                double *a = din, *b = nullptr;
                HIPCHK(X.add(nullptr, nullptr, 3 * nf * D, &b));
                for (int it = 0; it < p->normal_iters; it++) {
                    HIPCHK(launch_denoise_filter(nF, dnp, dni, drest, a, p->sigma_s, p->sigma_r, b, st));
                    std::swap(a, b);
                }
                HIPCHK(hipMemcpyAsync(dout, a, 3 * nf * D, hipMemcpyDeviceToDevice, st));
                break;
            }
            case SMG_DN_PROJECT:
                HIPCHK(X.add(nullptr, nullptr, n3 * D, &dQ));
                HIPCHK(launch_arap_columns(nV, dP, dQ, nV, st));
                HIPCHK(launch_denoise_project(nF, dF, drest, din, dQ, 1, nv, dout, dout + nf, st));
                break;
            case SMG_DN_RHS: {
                HIPCHK(X.add(nullptr, nullptr, 6 * nf * D, &dQn));
                HIPCHK(X.add(nullptr, nullptr, n3 * D, &dQ));
                dm2 = dout + n3 + 2 * nv;
                HIPCHK(launch_membrane_pressure(nV, nF, dF, dV0, dmp, dmi, 0.0, dQn, dm2, nullptr, st));
                HIPCHK(launch_arap_columns(nV, dV0, dQ, nV, st));
                HIPCHK(launch_pd_vertices(nV, nF, dmp, dmi, din, dm2, p->fidelity, dQ, din + 9 * nf, nV, dout, nV, dout + n3, dout + n3 + nv, st));
                break;
            }
            default:
                HIPCHK(X.add(nullptr, nullptr, (size_t)fixed_sum_groups(nF + nV) * D, &dpart));
                HIPCHK(launch_fixed_sum(din, nF + nV, dpart, dout, st));
                break;
        }
        int bad = 0;
        HIPCHK(X.finish(&bad));
        if (guard_hits) *guard_hits = bad;
        return SMG_OK;
    });
}

extern "C" int smg_debug_stylize(int op, int nV, int nF, const int* F, const int* rowptr, const int* col, const double* w, const double* V0,
                                 const double* P, const double* lambda, const double* Q, const double* targets, const double* state_in,
                                 const double* R_in, const smg_stylize_params* p, double* out, int* iters, int* guard_hits)
{
    return guarded("smg_debug_stylize", [&]() -> int {
        const char* who = "smg_debug_stylize";
        if (int rc = stylize_check_operands(who, op, nV, nF, F, rowptr, col, w, V0, P, lambda, Q, targets, R_in, p, out, iters)) return rc;
        if (int rc = need_device(who)) return rc;
        std::vector<int> mp, mi;
        vertex_corner_lists(std::vector<int>(F, F + 3 * (size_t)nF), nV, mp, mi);
        Scratch X;
        HIPCHK(X.init());
        const size_t n = (size_t)nV, nnz = (size_t)rowptr[nV], vec = n * sizeof(double);
        const bool cubic = op == SMG_STY_ADMM_ONE || op == SMG_STY_LOCAL;
        const size_t out_bytes = op == SMG_STY_NORMALS ? 4 * vec : cubic ? (10 + STY_STATE) * vec : op == SMG_STY_LOCAL_TARGETS ? 10 * vec : vec + sizeof(double);
        int *dF = nullptr, *dmp = nullptr, *dmi = nullptr, *dptr = nullptr, *dcol = nullptr, *dit = nullptr;
        double *dw = nullptr, *dV0 = nullptr, *dP = nullptr, *dlam = nullptr, *dtgt = nullptr, *dR = nullptr, *dn = nullptr, *da = nullptr, *dout = nullptr,
               *dpart = nullptr;
        HIPCHK(X.add(F, nullptr, 3 * (size_t)nF * sizeof(int), &dF));
        HIPCHK(X.add(mp.data(), nullptr, mp.size() * sizeof(int), &dmp));
        HIPCHK(X.add(mi.data(), nullptr, mi.size() * sizeof(int), &dmi));
        HIPCHK(X.add(rowptr, nullptr, (n + 1) * sizeof(int), &dptr));
        HIPCHK(X.add(col, nullptr, nnz * sizeof(int), &dcol));
        HIPCHK(X.add(w, nullptr, nnz * sizeof(double), &dw));
        HIPCHK(X.add(V0, nullptr, 3 * vec, &dV0));
        if (P) HIPCHK(X.add(P, nullptr, 3 * vec, &dP));
        if (lambda) HIPCHK(X.add(lambda, nullptr, vec, &dlam));
        if (targets) HIPCHK(X.add(targets, nullptr, 3 * vec, &dtgt));
        if (op == SMG_STY_ENERGY) HIPCHK(X.add(R_in, nullptr, 9 * vec, &dR));
        HIPCHK(X.add(out, out, out_bytes, &dout));
        if (op != SMG_STY_NORMALS) {
            HIPCHK(X.add(nullptr, nullptr, 3 * vec, &dn));
            HIPCHK(X.add(nullptr, nullptr, vec, &da));
        }
        if (iters && op != SMG_STY_NORMALS && op != SMG_STY_ENERGY) HIPCHK(X.add(iters, iters, n * sizeof(int), &dit));
        if (op == SMG_STY_ENERGY) HIPCHK(X.add(nullptr, nullptr, (size_t)fixed_sum_groups(nV) * sizeof(double), &dpart));
        hipStream_t st = X.stream();
        StyFrame fr = {{1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0}};
        if (Q) for (int e = 0; e < 9; e++) fr.q[e] = Q[e];
        StyParams sp = sty_params(*p);
        if (op == SMG_STY_ADMM_ONE) sp.admm_iters = 1;
        if (op == SMG_STY_NORMALS) {
            HIPCHK(launch_stylize_normals(nV, dF, dmp, dmi, dV0, dout, dout + 3 * n, st));
        } else {
            HIPCHK(launch_stylize_normals(nV, dF, dmp, dmi, dV0, dn, da, st));
            if (cubic) {
                if (state_in) HIPCHK(hipMemcpyAsync(dout + 10 * n, state_in, STY_STATE * vec, hipMemcpyHostToDevice, st));
                HIPCHK(launch_stylize_cubic(nV, dptr, dcol, dw, dV0, dP, dn, da, dlam, fr, sp, state_in ? 0 : 1, dout + 10 * n, dout, dout + 9 * n, dit, st));
            } else if (op == SMG_STY_LOCAL_TARGETS) {
                HIPCHK(launch_stylize_targets(nV, dptr, dcol, dw, dV0, dP, dn, da, dlam, dtgt, sp, dout, dout + 9 * n, dit, st));
            } else {
                HIPCHK(launch_stylize_energy(nV, dptr, dcol, dw, dV0, dP, dn, da, dlam, fr, dtgt, sp, dR, dout, st));
                HIPCHK(launch_fixed_sum(dout, nV, dpart, dout + n, st));
            }
        }
        int bad = 0;
        HIPCHK(X.finish(&bad));
        if (guard_hits) *guard_hits = bad;
        return SMG_OK;
    });
}

extern "C" int smg_debug_morph(int op, int nV, int nF, int k, const int* F, const double* V0, const double* X, const double* t, const double* in,
                               const int* pins, int n_pins, double* out, int* guard_hits)
{
    return guarded("smg_debug_morph", [&]() -> int {
        const char* who = "smg_debug_morph";
        if (int rc = morph_check_operands(who, op, nV, nF, k, F, V0, X, t, in, pins, n_pins, out)) return rc;
        if (int rc = need_device(who)) return rc;
        const size_t n = (size_t)nV, f = (size_t)nF, D = sizeof(double);
        const bool rhs = op == SMG_MORPH_RHS_GRADIENT || op == SMG_MORPH_RHS_INTERP;
        std::vector<int> mp, mi;
        if (rhs) vertex_corner_lists(std::vector<int>(F, F + 3 * f), nV, mp, mi);
        Scratch S;
        HIPCHK(S.init());
        const size_t out_count = op == SMG_MORPH_FACE_GRADIENT ? 9 * f * k : op == SMG_MORPH_FACE_POLAR ? 18 * f : rhs ? 4 * n * k : 3 * (n + (size_t)n_pins) * k;
        const size_t x_count = op == SMG_MORPH_FACE_GRADIENT ? 3 * n * k : 3 * n;
        const size_t in_count = op == SMG_MORPH_RHS_GRADIENT ? 9 * f * k : 9 * f;
        int *dF = nullptr, *dmp = nullptr, *dmi = nullptr, *dpins = nullptr;
        double *dV0 = nullptr, *dX = nullptr, *dt = nullptr, *din = nullptr, *dout = nullptr, *dW = nullptr, *dn = nullptr, *dA = nullptr;
        HIPCHK(S.add(F, nullptr, 3 * f * sizeof(int), &dF));
        HIPCHK(S.add(V0, nullptr, 3 * n * D, &dV0));
        if (X && !rhs) HIPCHK(S.add(X, nullptr, x_count * D, &dX));
        if (t && (op == SMG_MORPH_RHS_INTERP || (op == SMG_MORPH_PINS && X))) HIPCHK(S.add(t, nullptr, (size_t)k * D, &dt));
        if (rhs) {
            HIPCHK(S.add(in, nullptr, in_count * D, &din));
            HIPCHK(S.add(mp.data(), nullptr, mp.size() * sizeof(int), &dmp));
            HIPCHK(S.add(mi.data(), nullptr, mi.size() * sizeof(int), &dmi));
        }
        if (rhs || op == SMG_MORPH_FACE_POLAR) {
            HIPCHK(S.add(nullptr, nullptr, 9 * f * D, &dW));
            HIPCHK(S.add(nullptr, nullptr, 3 * f * D, &dn));
            HIPCHK(S.add(nullptr, nullptr, f * D, &dA));
        }
        if (op == SMG_MORPH_PINS) HIPCHK(S.add(pins, nullptr, (size_t)n_pins * sizeof(int), &dpins));
        HIPCHK(S.add(out, out, out_count * D, &dout));
        hipStream_t st = S.stream();
        if (dW) HIPCHK(launch_morph_basis(dV0, dF, nF, dW, dn, dA, st));
        switch (op) {
            case SMG_MORPH_FACE_GRADIENT: HIPCHK(launch_morph_face_gradient(nF, k, dF, dV0, dX, 3 * n, dout, st)); break;
            case SMG_MORPH_FACE_POLAR: HIPCHK(launch_morph_face_polar(nF, dF, dW, dn, dX, dout, dout + 9 * f, dout + 12 * f, st)); break;
            case SMG_MORPH_RHS_GRADIENT: HIPCHK(launch_morph_rhs_gradient(nV, k, nF, dmp, dmi, dW, dA, din, dout, nV, dout + 3 * n * k, st)); break;
            case SMG_MORPH_RHS_INTERP:
                HIPCHK(launch_morph_rhs_interp(nV, k, nF, dmp, dmi, dW, dA, din, din + 3 * f, dt, dout, nV, dout + 3 * n * k, st));
                break;
            default: {
                double *hp = dout, *U = dout + 3 * (size_t)n_pins * k;
                HIPCHK(launch_morph_pins(n_pins, k, dpins, dV0, dX, dt, hp, n_pins, st));
                HIPCHK(launch_morph_start(nV, k, dV0, dX, dt, U, nV, st));
                HIPCHK(launch_morph_set_pins(n_pins, 3 * k, dpins, hp, n_pins, U, nV, st));
                break;
            }
        }
        int bad = 0;
        HIPCHK(S.finish(&bad));
        if (guard_hits) *guard_hits = bad;
        return SMG_OK;
    });
}

extern "C" int smg_debug_flow(int op, int nV, int nF, const int* F, const double* U, const double* V0, const int* rowptr, const int* col,
                              const double* L0, double delta, double* out, int* guard_hits)
{
    return guarded("smg_debug_flow", [&]() -> int {
        const char* who = "smg_debug_flow";
        if (int rc = flow_check_operands(who, op, nV, nF, F, U, V0, rowptr, col, L0, delta, out)) return rc;
        if (int rc = need_device(who)) return rc;
        const size_t n = (size_t)nV, f = (size_t)nF, D = sizeof(double);
        std::vector<int> mp, mi, diag;
        if (op == SMG_FLOW_SYSTEM || op == SMG_FLOW_SPHERICITY || op == SMG_FLOW_SPHERE) vertex_corner_lists(std::vector<int>(F, F + 3 * f), nV, mp, mi);
        const size_t nnz = op == SMG_FLOW_SYSTEM ? (size_t)rowptr[nV] : 0;
        if (op == SMG_FLOW_SYSTEM) flow_diagonal(nV, rowptr, col, diag);
        Scratch S;
        HIPCHK(S.init());
        const size_t out_count = op == SMG_FLOW_SYSTEM ? 4 * n + nnz : op == SMG_FLOW_NORMALIZE ? 3 * n : op == SMG_FLOW_SPHERICITY ? 7 : 3 * n + 6 * f + 4;
        int *dF = nullptr, *dmp = nullptr, *dmi = nullptr, *drp = nullptr, *ddiag = nullptr;
        double *dU = nullptr, *dV0 = nullptr, *dL0 = nullptr, *dout = nullptr, *da = nullptr, *dr = nullptr, *dterm = nullptr, *dpart = nullptr, *ds = nullptr;
        double hs[FLOW_SUMS];
        for (double& v : hs) v = 0.0;
        HIPCHK(S.add(F, nullptr, 3 * f * sizeof(int), &dF));
        HIPCHK(S.add(U, nullptr, 3 * n * D, &dU));
        if (!mp.empty()) {
            HIPCHK(S.add(mp.data(), nullptr, mp.size() * sizeof(int), &dmp));
            HIPCHK(S.add(mi.data(), nullptr, mi.size() * sizeof(int), &dmi));
        }
        if (op == SMG_FLOW_SYSTEM) {
            HIPCHK(S.add(rowptr, nullptr, (n + 1) * sizeof(int), &drp));
            HIPCHK(S.add(diag.data(), nullptr, n * sizeof(int), &ddiag));
            HIPCHK(S.add(L0, nullptr, nnz * D, &dL0));
        } else {
            HIPCHK(S.add(nullptr, nullptr, n * D, &da));
            HIPCHK(S.add(nullptr, nullptr, n * D, &dr));
            HIPCHK(S.add(nullptr, nullptr, std::max(3 * n, f) * D, &dterm));
            HIPCHK(S.add(nullptr, nullptr, (size_t)fixed_sum_groups(std::max(nV, nF)) * D, &dpart));
            HIPCHK(S.add(hs, hs, sizeof hs, &ds));
        }
        if (op == SMG_FLOW_SPHERE) HIPCHK(S.add(V0, nullptr, 3 * n * D, &dV0));
        HIPCHK(S.add(out, out, out_count * D, &dout));
        hipStream_t st = S.stream();
        switch (op) {
            case SMG_FLOW_SYSTEM:
                HIPCHK(launch_flow_system(nV, dU, nV, dF, dmp, dmi, drp, ddiag, dL0, delta, nullptr, dout, dout + n, nV, dout + 4 * n, st));
                break;
            case SMG_FLOW_NORMALIZE: HIPCHK(launch_flow_normalize(nV, nF, dF, dU, nV, dterm, dpart, ds, dout, nV, st)); break;
            case SMG_FLOW_SPHERICITY: HIPCHK(launch_flow_sphericity(nV, dU, nV, dF, dmp, dmi, da, dr, dterm, dpart, ds, st)); break;
            default:
                HIPCHK(launch_flow_sphericity(nV, dU, nV, dF, dmp, dmi, da, dr, dterm, dpart, ds, st));
                HIPCHK(launch_flow_sphere(nV, nF, dF, dU, nV, dV0, nV, ds, dout, nV, dout + 3 * n, dout + 3 * n + 2 * f, dpart, ds + 12, st));
                break;
        }
        int bad = 0;
        HIPCHK(S.finish(&bad));
        if (op == SMG_FLOW_SPHERICITY)
            for (int e = 0; e < 7; e++) out[e] = hs[e];
        if (op == SMG_FLOW_SPHERE) {
            double* stats = out + 3 * n + 6 * f;
            stats[0] = hs[12] / hs[13]; stats[1] = hs[14]; stats[2] = hs[15]; stats[3] = hs[0];
        }
        if (guard_hits) *guard_hits = bad;
        return SMG_OK;
    });
}

extern "C" int smg_debug_hodge(int op, int nV, int nF, int k, const int* F, const double* V, const double* X, const double* u, const double* v,
                               double* out, int* guard_hits)
{
    return guarded("smg_debug_hodge", [&]() -> int {
        const char* who = "smg_debug_hodge";
        if (int rc = hodge_check_operands(who, op, nV, nF, k, F, V, X, u, v, out)) return rc;
        if (int rc = need_device(who)) return rc;
        const size_t n = (size_t)nV, f = (size_t)nF, nk = n * (size_t)k, D = sizeof(double);
        if (2 * nk > (size_t)INT_MAX || 4 * f * (size_t)k > (size_t)INT_MAX) return fail(SMG_ERR_INVALID, "%s: k = %d exceeds the index range", who, k);
        std::vector<int> mp, mi;
        if (op == SMG_HODGE_RHS) vertex_corner_lists(std::vector<int>(F, F + 3 * f), nV, mp, mi);
        Scratch S;
        HIPCHK(S.init());
        const size_t out_count = op == SMG_HODGE_RHS ? 4 * nk : op == SMG_HODGE_PARTS ? 13 * f * k + 4 * (size_t)k : 3 * f * k;
        int *dF = nullptr, *dmp = nullptr, *dmi = nullptr;
        double *dV = nullptr, *dX = nullptr, *du = nullptr, *dv = nullptr, *dout = nullptr, *dW = nullptr, *dn = nullptr, *dA = nullptr, *dpart = nullptr;
        HIPCHK(S.add(F, nullptr, 3 * f * sizeof(int), &dF));
        HIPCHK(S.add(V, nullptr, 3 * n * D, &dV));
        if (op != SMG_HODGE_FIELD) HIPCHK(S.add(X, nullptr, 3 * f * k * D, &dX));
        if (op == SMG_HODGE_RHS) {
            HIPCHK(S.add(mp.data(), nullptr, mp.size() * sizeof(int), &dmp));
            HIPCHK(S.add(mi.data(), nullptr, mi.size() * sizeof(int), &dmi));
        } else {
            HIPCHK(S.add(u, nullptr, nk * D, &du));
            HIPCHK(S.add(v, nullptr, nk * D, &dv));
        }
        HIPCHK(S.add(nullptr, nullptr, 9 * f * D, &dW));
        HIPCHK(S.add(nullptr, nullptr, 3 * f * D, &dn));
        HIPCHK(S.add(nullptr, nullptr, f * D, &dA));
        if (op == SMG_HODGE_PARTS) HIPCHK(S.add(nullptr, nullptr, (size_t)fixed_sum_groups(nF) * D, &dpart));
        HIPCHK(S.add(out, out, out_count * D, &dout));
        hipStream_t st = S.stream();
        HIPCHK(launch_hodge_geometry(dV, dF, nF, dW, dn, dA, st));
        switch (op) {
            case SMG_HODGE_RHS: HIPCHK(launch_hodge_rhs(nV, k, nF, dmp, dmi, dF, dV, dn, dX, dout, dout + nk, nV, dout + 2 * nk, st)); break;
            case SMG_HODGE_PARTS: {
                double *terms = dout + 9 * f * k, *energy = dout + 13 * f * k;
                HIPCHK(launch_hodge_parts(nF, k, dF, dW, dn, dA, dX, du, nV, dv, nV, dout, terms, st));
                for (int e = 0; e < 4 * k; e++) HIPCHK(launch_fixed_sum(terms + (size_t)e * f, nF, dpart, energy + e, st));
                break;
            }
            default: HIPCHK(launch_hodge_field(nF, k, dF, dW, dn, du, nV, dv, nV, dout, st)); break;
        }
        int bad = 0;
        HIPCHK(S.finish(&bad));
        if (guard_hits) *guard_hits = bad;
        return SMG_OK;
    });
}

extern "C" int smg_debug_emd(int op, int nV, int nF, int k, const int* F, const double* V, const double* b, const double* phi, const double* state,
                             const double* rho, double alpha, double* out, int* guard_hits)
{
    return guarded("smg_debug_emd", [&]() -> int {
        const char* who = "smg_debug_emd";
        if (int rc = emd_check_operands(who, op, nV, nF, k, F, V, b, phi, state, rho, out)) return rc;
        if (int rc = need_device(who)) return rc;
        const size_t n = (size_t)nV, f = (size_t)nF, kk = (size_t)k, nk = n * kk, fk = f * kk, D = sizeof(double);
        if (nk > (size_t)INT_MAX || 4 * fk > (size_t)INT_MAX) return fail(SMG_ERR_INVALID, "%s: k = %d exceeds the index range", who, k);
        const bool corners = op == SMG_EMD_RHS || op == SMG_EMD_RESIDUAL;
        std::vector<int> mp, mi;
        if (corners) vertex_corner_lists(std::vector<int>(F, F + 3 * f), nV, mp, mi);
        Scratch S;
        HIPCHK(S.init());
        const size_t out_count = op == SMG_EMD_GEOMETRY ? 7 * f + 1 : op == SMG_EMD_RHS ? nk : op == SMG_EMD_UPDATE ? 8 * fk + 2 * kk
                                 : op == SMG_EMD_FLOW ? 3 * fk : 2 * nk + kk;
        const size_t state_count = op == SMG_EMD_RHS || op == SMG_EMD_UPDATE ? 4 * fk : op == SMG_EMD_DUAL ? kk : 2 * fk;
        int *dF = nullptr, *dmp = nullptr, *dmi = nullptr;
        double *dV = nullptr, *db = nullptr, *dphi = nullptr, *dstate = nullptr, *drho = nullptr, *dout = nullptr, *dW2 = nullptr, *dA = nullptr, *dpart = nullptr;
        HIPCHK(S.add(F, nullptr, 3 * f * sizeof(int), &dF));
        HIPCHK(S.add(V, nullptr, 3 * n * D, &dV));
        if (b) HIPCHK(S.add(b, nullptr, nk * D, &db));
        if (phi) HIPCHK(S.add(phi, nullptr, nk * D, &dphi));
        if (rho) HIPCHK(S.add(rho, nullptr, kk * D, &drho));
        if (op != SMG_EMD_GEOMETRY) HIPCHK(S.add(state, nullptr, state_count * D, &dstate));
        if (corners) {
            HIPCHK(S.add(mp.data(), nullptr, mp.size() * sizeof(int), &dmp));
            HIPCHK(S.add(mi.data(), nullptr, mi.size() * sizeof(int), &dmi));
        }
        HIPCHK(S.add(nullptr, nullptr, 6 * f * D, &dW2));
        HIPCHK(S.add(nullptr, nullptr, f * D, &dA));
        HIPCHK(S.add(nullptr, nullptr, (size_t)fixed_sum_groups(std::max(nV, nF)) * D, &dpart));
        HIPCHK(S.add(out, out, out_count * D, &dout));
        hipStream_t st = S.stream();
        HIPCHK(launch_emd_geometry(dV, dF, nF, dW2, dA, st));
        switch (op) {
            case SMG_EMD_GEOMETRY:
                HIPCHK(hipMemcpyAsync(dout, dW2, 6 * f * D, hipMemcpyDeviceToDevice, st));
                HIPCHK(hipMemcpyAsync(dout + 6 * f, dA, f * D, hipMemcpyDeviceToDevice, st));
                HIPCHK(launch_fixed_sum(dA, nF, dpart, dout + 7 * f, st));
                break;
            case SMG_EMD_RHS: HIPCHK(launch_emd_rhs(nV, k, nF, dmp, dmi, dW2, dA, dstate, true, db, nV, dout, nV, nullptr, st)); break;
            case SMG_EMD_UPDATE: {
                double *up = dout + 6 * fk, *gq = dout + 7 * fk;
                HIPCHK(hipMemcpyAsync(dout, dstate, 4 * fk * D, hipMemcpyDeviceToDevice, st));
                HIPCHK(launch_emd_update(nF, k, dF, dW2, dA, dphi, nV, dout, drho, alpha, dout + 4 * fk, up, gq, st));
                for (int c = 0; c < k; c++) {
                    HIPCHK(launch_fixed_sum(up + (size_t)c * f, nF, dpart, dout + 8 * fk + c, st));
                    HIPCHK(launch_fixed_max(gq + (size_t)c * f, nF, dpart, dout + 8 * fk + kk + c, st));
                }
                break;
            }
            case SMG_EMD_DUAL:
                HIPCHK(launch_emd_dual(nV, k, db, nV, dphi, nV, drho, dstate, dout, nV, dout + nk, st));
                for (int c = 0; c < k; c++) HIPCHK(launch_fixed_sum(dout + nk + (size_t)c * n, nV, dpart, dout + 2 * nk + c, st));
                break;
            case SMG_EMD_FLOW: HIPCHK(launch_emd_flow(nF, k, dV, dF, dstate, dout, st)); break;
            default:
                HIPCHK(launch_emd_rhs(nV, k, nF, dmp, dmi, dW2, dA, dstate, false, db, nV, dout, nV, dout + nk, st));
                for (int c = 0; c < k; c++) HIPCHK(launch_fixed_sum(dout + nk + (size_t)c * n, nV, dpart, dout + 2 * nk + c, st));
                break;
        }
        int bad = 0;
        HIPCHK(S.finish(&bad));
        if (guard_hits) *guard_hits = bad;
        return SMG_OK;
    });
}

extern "C" int smg_debug_fluid(int op, int nV, int nF, int k, const int* F, const double* V, const double* w, const double* psi, const double* wn, double a,
                               double b, const double* dt, double theta, int rates_only, double* out, int* guard_hits)
{
    return guarded("smg_debug_fluid", [&]() -> int {
        const char* who = "smg_debug_fluid";
        if (int rc = fluid_check_operands(who, op, nV, nF, k, F, V, w, psi, wn, dt, theta, rates_only, out)) return rc;
        if (int rc = need_device(who)) return rc;
        const size_t n = (size_t)nV, f = (size_t)nF, kk = (size_t)k, nk = n * kk, fk = f * kk, D = sizeof(double);
        if (nk > (size_t)INT_MAX || 3 * fk > (size_t)INT_MAX) return fail(SMG_ERR_INVALID, "%s: k = %d exceeds the index range", who, k);
        const bool full = op == SMG_FLUID_ADVECT && !rates_only;
        Scratch S;
        HIPCHK(S.init());
        hipStream_t st = S.stream();
        if (op == SMG_FLUID_DT) {
            double *drm = nullptr, *dtime = nullptr, *dout = nullptr;
            HIPCHK(S.add(w, nullptr, 3 * kk * D, &drm));
            HIPCHK(S.add(psi, nullptr, kk * D, &dtime));
            HIPCHK(S.add(out, out, 3 * kk * D, &dout));
            HIPCHK(launch_fluid_dt(0, k, 3, a, drm, dout, nullptr, nullptr, nullptr, st));
            HIPCHK(launch_fluid_dt(1, k, 3, a, drm, dout, dtime, dout + kk, dout + 2 * kk, st));
            int bad = 0;
            HIPCHK(S.finish(&bad));
            if (guard_hits) *guard_hits = bad;
            return SMG_OK;
        }
        std::vector<int> mp, mi, known;
        vertex_corner_lists(std::vector<int>(F, F + 3 * f), nV, mp, mi);
        const int nb = fluid_known_rows(nV, nF, F, known);
        const size_t out_count = op == SMG_FLUID_RHS ? n + 1 + 3 * nk + kk + 1 : op == SMG_FLUID_ADVECT ? (full ? 3 * nk + 2 * kk : nk + kk)
                                 : op == SMG_FLUID_VELOCITY ? 4 * fk + kk : 2 * nk + 2 * kk;
        int *dF = nullptr, *dmp = nullptr, *dmi = nullptr, *dknown = nullptr;
        double *dV = nullptr, *dw = nullptr, *dpsi = nullptr, *dwn = nullptr, *ddt = nullptr, *dout = nullptr, *dW = nullptr, *dn = nullptr, *dA = nullptr,
               *dm = nullptr, *dpart = nullptr, *dew = nullptr;
        HIPCHK(S.add(F, nullptr, 3 * f * sizeof(int), &dF));
        HIPCHK(S.add(V, nullptr, 3 * n * D, &dV));
        HIPCHK(S.add(mp.data(), nullptr, mp.size() * sizeof(int), &dmp));
        HIPCHK(S.add(mi.data(), nullptr, mi.size() * sizeof(int), &dmi));
        HIPCHK(S.add(known.data(), nullptr, n * sizeof(int), &dknown));
        if (w && op != SMG_FLUID_VELOCITY && (op != SMG_FLUID_ADVECT || full)) HIPCHK(S.add(w, nullptr, nk * D, &dw));
        if (psi && (op == SMG_FLUID_ADVECT || op == SMG_FLUID_VELOCITY)) HIPCHK(S.add(psi, nullptr, nk * D, &dpsi));
        if (full) {
            HIPCHK(S.add(wn, nullptr, nk * D, &dwn));
            HIPCHK(S.add(dt, nullptr, kk * D, &ddt));
        }
        HIPCHK(S.add(nullptr, nullptr, 9 * f * D, &dW));
        HIPCHK(S.add(nullptr, nullptr, 3 * f * D, &dn));
        HIPCHK(S.add(nullptr, nullptr, f * D, &dA));
        HIPCHK(S.add(nullptr, nullptr, n * D, &dm));
        HIPCHK(S.add(nullptr, nullptr, (size_t)fixed_sum_groups((int)std::max(nk, f)) * D, &dpart));
        if (op == SMG_FLUID_RHS) HIPCHK(S.add(nullptr, nullptr, nk * D, &dew));
        HIPCHK(S.add(out, out, out_count * D, &dout));
        HIPCHK(launch_hodge_geometry(dV, dF, nF, dW, dn, dA, st));
        HIPCHK(launch_fluid_mass(nV, dmp, dmi, dA, dm, st));
        switch (op) {
            case SMG_FLUID_RHS: {
                double *msum = dout + n, *mw = dout + n + 1, *mwsum = mw + nk, *R = mwsum + kk, *rsq = R + nk;
                HIPCHK(hipMemcpyAsync(dout, dm, n * D, hipMemcpyDeviceToDevice, st));
                HIPCHK(launch_fixed_sum(dm, nV, dpart, msum, st));
                HIPCHK(launch_fluid_diag(nV, k, dm, dw, nV, mw, dew, st));
                for (int c = 0; c < k; c++) HIPCHK(launch_fixed_sum(mw + (size_t)c * n, nV, dpart, mwsum + c, st));
                HIPCHK(launch_fluid_rhs(nV, k, dm, dknown, dw, nV, nb > 0 ? nullptr : mwsum, msum, R, nV, rsq, st));
                HIPCHK(launch_fixed_sum(rsq, (int)nk, dpart, rsq + nk, st));
                break;
            }
            case SMG_FLUID_ADVECT:
                if (!full) {
                    HIPCHK(launch_fluid_advect(nV, k, dF, dmp, dmi, dm, dpsi, nV, nullptr, nV, nullptr, nV, a, b, nullptr, theta, nullptr, nV, dout, nullptr,
                                               true, st));
                    for (int c = 0; c < k; c++) HIPCHK(launch_fixed_max(dout + (size_t)c * n, nV, dpart, dout + nk + c, st));
                } else {
                    double *rate = dout + nk, *mw = dout + 2 * nk;
                    HIPCHK(launch_fluid_advect(nV, k, dF, dmp, dmi, dm, dpsi, nV, dw, nV, dwn, nV, a, b, ddt, theta, dout, nV, rate, mw, false, st));
                    for (int c = 0; c < k; c++) {
                        HIPCHK(launch_fixed_max(rate + (size_t)c * n, nV, dpart, dout + 3 * nk + c, st));
                        HIPCHK(launch_fixed_sum(mw + (size_t)c * n, nV, dpart, dout + 3 * nk + kk + c, st));
                    }
                }
                break;
            case SMG_FLUID_VELOCITY:
                HIPCHK(launch_fluid_velocity(nF, k, dF, dW, dn, dA, dpsi, nV, dout, dout + 3 * fk, st));
                for (int c = 0; c < k; c++) HIPCHK(launch_fixed_sum(dout + 3 * fk + (size_t)c * f, nF, dpart, dout + 4 * fk + c, st));
                break;
            default:
                HIPCHK(launch_fluid_diag(nV, k, dm, dw, nV, dout, dout + nk, st));
                for (int c = 0; c < k; c++) {
                    HIPCHK(launch_fixed_sum(dout + (size_t)c * n, nV, dpart, dout + 2 * nk + c, st));
                    HIPCHK(launch_fixed_sum(dout + nk + (size_t)c * n, nV, dpart, dout + 2 * nk + kk + c, st));
                }
                break;
        }
        int bad = 0;
        HIPCHK(S.finish(&bad));
        if (guard_hits) *guard_hits = bad;
        return SMG_OK;
    });
}

extern "C" int smg_debug_fluid_time(int op, int nV, int nF, int k, const int* F, const double* V, int rates_only, int reps, double* ms)
{
    return guarded("smg_debug_fluid_time", [&]() -> int {
        const char* who = "smg_debug_fluid_time";
        if (op < SMG_FLUID_RHS || op > SMG_FLUID_DIAG || nV < 1 || nF < 1 || !F || !V || !ms) return fail(SMG_ERR_INVALID, "%s: bad arguments", who);
        if (k < 1 || reps < 1) return fail(SMG_ERR_INVALID, "%s: k = %d, reps = %d, at least 1 each is needed", who, k, reps);
        if (int rc = check_faces(who, F, nF, nV)) return rc;
        if (int rc = need_device(who)) return rc;
        const size_t n = (size_t)nV, f = (size_t)nF, kk = (size_t)k, nk = n * kk, fk = f * kk, D = sizeof(double);
        if (nk > (size_t)INT_MAX || 3 * fk > (size_t)INT_MAX) return fail(SMG_ERR_INVALID, "%s: k = %d exceeds the index range", who, k);
        std::vector<int> mp, mi, known;
        vertex_corner_lists(std::vector<int>(F, F + 3 * f), nV, mp, mi);
        fluid_known_rows(nV, nF, F, known);
        struct Event { hipEvent_t e = nullptr; ~Event() { if (e) (void)hipEventDestroy(e); } } t0, t1;
        Scratch S;                                                           // for its stream alone
        HIPCHK(S.init());
        hipStream_t st = S.stream();
        DevBuf<int> dF, dmp, dmi, dknown;
        DevBuf<double> dV, dW, dn, dA, dm, dsum, dk, dpart, w, psi, wn, out, rate, mw, U;
        HIPCHK(dF.upload(std::vector<int>(F, F + 3 * f)));
        HIPCHK(dmp.upload(mp));
        HIPCHK(dmi.upload(mi));
        HIPCHK(dknown.upload(known));
        HIPCHK(dV.upload(std::vector<double>(V, V + 3 * n)));
        HIPCHK(dW.alloc(9 * f));
        HIPCHK(dn.alloc(3 * f));
        HIPCHK(dA.alloc(f));
        HIPCHK(dm.alloc(n));
        HIPCHK(dsum.alloc(1));
        HIPCHK(dk.alloc(kk));
        HIPCHK(dpart.alloc((size_t)fixed_sum_groups(nV)));
        for (DevBuf<double>* b : {&w, &psi, &wn, &out, &rate, &mw}) {        // zeros: the operands' values do not change what a launch moves
            HIPCHK(b->alloc(std::max(nk, fk)));
            HIPCHK(hipMemsetAsync(b->p, 0, std::max(nk, fk) * D, st));
        }
        if (op == SMG_FLUID_VELOCITY) HIPCHK(U.alloc(3 * fk));
        HIPCHK(hipMemsetAsync(dk.p, 0, kk * D, st));
        HIPCHK(launch_hodge_geometry(dV.p, dF.p, nF, dW.p, dn.p, dA.p, st));
        HIPCHK(launch_fluid_mass(nV, dmp.p, dmi.p, dA.p, dm.p, st));
        HIPCHK(launch_fixed_sum(dm.p, nV, dpart.p, dsum.p, st));
        auto launch = [&]() -> hipError_t {
            switch (op) {
                case SMG_FLUID_RHS: return launch_fluid_rhs(nV, k, dm.p, dknown.p, w.p, nV, dk.p, dsum.p, out.p, nV, rate.p, st);
                case SMG_FLUID_ADVECT:
                    return launch_fluid_advect(nV, k, dF.p, dmp.p, dmi.p, dm.p, psi.p, nV, w.p, nV, wn.p, nV, 0.75, 0.25, dk.p, 0.0, out.p, nV, rate.p, mw.p,
                                               rates_only != 0, st);
                case SMG_FLUID_VELOCITY: return launch_fluid_velocity(nF, k, dF.p, dW.p, dn.p, dA.p, psi.p, nV, U.p, rate.p, st);
                default: return launch_fluid_diag(nV, k, dm.p, w.p, nV, out.p, mw.p, st);
            }
        };
        HIPCHK(hipEventCreate(&t0.e));
        HIPCHK(hipEventCreate(&t1.e));
        HIPCHK(launch());                                                    // one launch that is not timed
        HIPCHK(hipEventRecord(t0.e, st));
        for (int r = 0; r < reps; r++) HIPCHK(launch());
        HIPCHK(hipEventRecord(t1.e, st));
        HIPCHK(hipStreamSynchronize(st));
        float total = 0.0f;
        HIPCHK(hipEventElapsedTime(&total, t0.e, t1.e));
        *ms = (double)total / reps;
        return SMG_OK;
    });
}

extern "C" int smg_debug_rd(int op, int nV, int nF, int k, const int* F, const double* V, const double* u, const double* v, const double* coeff, double dt,
                            int substeps, const double* un, const double* vn, double* out, int* guard_hits)
{
    return guarded("smg_debug_rd", [&]() -> int {
        const char* who = "smg_debug_rd";
        if (int rc = rd_check_operands(who, op, nV, nF, k, F, V, u, v, coeff, dt, substeps, un, vn, out)) return rc;
        if (int rc = need_device(who)) return rc;
        const size_t n = (size_t)nV, f = (size_t)nF, kk = (size_t)k, nk = n * kk, D = sizeof(double);
        if (2 * nk > (size_t)INT_MAX) return fail(SMG_ERR_INVALID, "%s: k = %d exceeds the index range", who, k);
        Scratch S;
        HIPCHK(S.init());
        hipStream_t st = S.stream();
        std::vector<int> mp, mi;
        vertex_corner_lists(std::vector<int>(F, F + 3 * f), nV, mp, mi);
        const size_t out_count = op == SMG_RD_REACT ? 5 * nk + 2 : 3 * nk + 3 * kk;
        int *dF = nullptr, *dmp = nullptr, *dmi = nullptr;
        double *dV = nullptr, *du = nullptr, *dv = nullptr, *dun = nullptr, *dvn = nullptr, *dcoef = nullptr, *dout = nullptr, *dW = nullptr, *dn = nullptr,
               *dA = nullptr, *dm = nullptr, *dpart = nullptr;
        HIPCHK(S.add(F, nullptr, 3 * f * sizeof(int), &dF));
        HIPCHK(S.add(V, nullptr, 3 * n * D, &dV));
        HIPCHK(S.add(mp.data(), nullptr, mp.size() * sizeof(int), &dmp));
        HIPCHK(S.add(mi.data(), nullptr, mi.size() * sizeof(int), &dmi));
        HIPCHK(S.add(u, nullptr, nk * D, &du));
        HIPCHK(S.add(v, nullptr, nk * D, &dv));
        if (op == SMG_RD_REACT) {
            HIPCHK(S.add(coeff, nullptr, kk * RD_COEFFS * D, &dcoef));
        } else {
            HIPCHK(S.add(un, nullptr, nk * D, &dun));
            HIPCHK(S.add(vn, nullptr, nk * D, &dvn));
        }
        HIPCHK(S.add(nullptr, nullptr, 9 * f * D, &dW));
        HIPCHK(S.add(nullptr, nullptr, 3 * f * D, &dn));
        HIPCHK(S.add(nullptr, nullptr, f * D, &dA));
        HIPCHK(S.add(nullptr, nullptr, n * D, &dm));
        HIPCHK(S.add(nullptr, nullptr, (size_t)fixed_sum_groups((int)nk) * D, &dpart));
        HIPCHK(S.add(out, out, out_count * D, &dout));
        HIPCHK(launch_hodge_geometry(dV, dF, nF, dW, dn, dA, st));
        HIPCHK(launch_fluid_mass(nV, dmp, dmi, dA, dm, st));
        if (op == SMG_RD_REACT) {
            double* rsq = dout + 2 * nk;
            HIPCHK(launch_rd_react(nV, k, dm, du, dv, nV, dcoef, dt / substeps, substeps, dout, dout + nk, nV, rsq, dout + 4 * nk, nV, st));
            HIPCHK(launch_fixed_sum(rsq, (int)nk, dpart, dout + 5 * nk, st));
            HIPCHK(launch_fixed_sum(rsq + nk, (int)nk, dpart, dout + 5 * nk + 1, st));
        } else {
            double* chg = dout + 2 * nk;
            HIPCHK(launch_rd_close(nV, k, dm, du, dv, dun, dvn, nV, dout, chg, st));
            for (size_t c = 0; c < 2 * kk; c++) HIPCHK(launch_fixed_sum(dout + c * n, nV, dpart, dout + 3 * nk + c, st));
            for (size_t c = 0; c < kk; c++) HIPCHK(launch_fixed_max(chg + c * n, nV, dpart, dout + 3 * nk + 2 * kk + c, st));
        }
        int bad = 0;
        HIPCHK(S.finish(&bad));
        if (guard_hits) *guard_hits = bad;
        return SMG_OK;
    });
}

extern "C" int smg_debug_rd_time(int op, int nV, int nF, int k, const int* F, const double* V, int substeps, int reps, double* ms)
{
    return guarded("smg_debug_rd_time", [&]() -> int {
        const char* who = "smg_debug_rd_time";
        if (op < SMG_RD_REACT || op > SMG_RD_CLOSE || nV < 1 || nF < 1 || !F || !V || !ms) return fail(SMG_ERR_INVALID, "%s: bad arguments", who);
        if (k < 1 || substeps < 1 || reps < 1) return fail(SMG_ERR_INVALID, "%s: k = %d, substeps = %d, reps = %d, at least 1 each is needed", who, k, substeps, reps);
        if (int rc = check_faces(who, F, nF, nV)) return rc;
        if (int rc = need_device(who)) return rc;
        const size_t n = (size_t)nV, f = (size_t)nF, kk = (size_t)k, nk = n * kk, D = sizeof(double);
        if (2 * nk > (size_t)INT_MAX) return fail(SMG_ERR_INVALID, "%s: k = %d exceeds the index range", who, k);
        std::vector<int> mp, mi;
        vertex_corner_lists(std::vector<int>(F, F + 3 * f), nV, mp, mi);
        struct Event { hipEvent_t e = nullptr; ~Event() { if (e) (void)hipEventDestroy(e); } } t0, t1;
        Scratch S;                                                           // for its stream alone
        HIPCHK(S.init());
        hipStream_t st = S.stream();
        DevBuf<int> dF, dmp, dmi;
        DevBuf<double> dV, dW, dn, dA, dm, coef, s0, s1, R, rsq, chg;
        HIPCHK(dF.upload(std::vector<int>(F, F + 3 * f)));
        HIPCHK(dmp.upload(mp));
        HIPCHK(dmi.upload(mi));
        HIPCHK(dV.upload(std::vector<double>(V, V + 3 * n)));
        HIPCHK(dW.alloc(9 * f));
        HIPCHK(dn.alloc(3 * f));
        HIPCHK(dA.alloc(f));
        HIPCHK(dm.alloc(n));
        HIPCHK(coef.alloc(kk * RD_COEFFS));
        HIPCHK(chg.alloc(nk));
        HIPCHK(hipMemsetAsync(coef.p, 0, kk * RD_COEFFS * D, st));
        for (DevBuf<double>* b : {&s0, &s1, &R, &rsq}) {                     // zeros: the operands' values do not change what a launch moves
            HIPCHK(b->alloc(2 * nk));
            HIPCHK(hipMemsetAsync(b->p, 0, 2 * nk * D, st));
        }
        HIPCHK(launch_hodge_geometry(dV.p, dF.p, nF, dW.p, dn.p, dA.p, st));
        HIPCHK(launch_fluid_mass(nV, dmp.p, dmi.p, dA.p, dm.p, st));
        auto launch = [&]() -> hipError_t {
            if (op == SMG_RD_REACT)
                return launch_rd_react(nV, k, dm.p, s0.p, s0.p + nk, nV, coef.p, 0.5, substeps, R.p, R.p + nk, nV, rsq.p, nullptr, nV, st);
            return launch_rd_close(nV, k, dm.p, s0.p, s0.p + nk, s1.p, s1.p + nk, nV, rsq.p, chg.p, st);
        };
        HIPCHK(hipEventCreate(&t0.e));
        HIPCHK(hipEventCreate(&t1.e));
        HIPCHK(launch());                                                    // one launch that is not timed
        HIPCHK(hipEventRecord(t0.e, st));
        for (int r = 0; r < reps; r++) HIPCHK(launch());
        HIPCHK(hipEventRecord(t1.e, st));
        HIPCHK(hipStreamSynchronize(st));
        float total = 0.0f;
        HIPCHK(hipEventElapsedTime(&total, t0.e, t1.e));
        *ms = (double)total / reps;
        return SMG_OK;
    });
}

namespace {

// the geometry, the masses (on the device, then read back) and the planes mt, s2 of a wave hook; dm: n doubles of scratch
int wave_planes(hipStream_t st, int nV, int nF, const double* dV, const int* dF, const int* dmp, const int* dmi, double* dW, double* dn, double* dA, double* dm,
                const double* speed, const double* sigma, double dt, std::vector<double>& mt, std::vector<double>& s2)
{
    std::vector<double> m((size_t)nV);
    mt.resize((size_t)nV);
    s2.resize((size_t)nV);
    HIPCHK(launch_hodge_geometry(dV, dF, nF, dW, dn, dA, st));
    HIPCHK(launch_fluid_mass(nV, dmp, dmi, dA, dm, st));
    HIPCHK(hipMemcpyAsync(m.data(), dm, (size_t)nV * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    wave_host_planes(nV, m.data(), speed, sigma, dt, mt.data(), s2.data());
    return SMG_OK;
}

}  // namespace

extern "C" int smg_debug_wave(int op, int nV, int nF, int k, const int* F, const double* V, const double* speed, const double* sigma, int clamped, double dt,
                              const double* u, const double* v, const double* w, const int* idx, int n_idx, const double* sig0, const double* sig1, double* out,
                              int* guard_hits)
{
    return guarded("smg_debug_wave", [&]() -> int {
        const char* who = "smg_debug_wave";
        if (int rc = wave_check_operands(who, op, nV, nF, k, F, V, speed, sigma, clamped, dt, u, v, w, idx, n_idx, sig0, sig1, out)) return rc;
        if (int rc = need_device(who)) return rc;
        const size_t n = (size_t)nV, f = (size_t)nF, kk = (size_t)k, nk = n * kk, D = sizeof(double);
        if (2 * nk > (size_t)INT_MAX || 3 * f * kk > (size_t)INT_MAX) return fail(SMG_ERR_INVALID, "%s: k = %d exceeds the index range", who, k);
        Scratch S;
        HIPCHK(S.init());
        hipStream_t st = S.stream();
        const size_t ni = (size_t)std::max(n_idx, 0);
        const size_t out_count = op == SMG_WAVE_RECORD ? ni * kk : op == SMG_WAVE_ADVANCE ? 9 * nk + 2 * kk + 1 : 3 * nk + 1;
        double *du = nullptr, *dv = nullptr, *dw = nullptr, *dout = nullptr, *ds0 = nullptr, *ds1 = nullptr;
        int* didx = nullptr;
        HIPCHK(S.add(u, nullptr, nk * D, &du));
        if (v) HIPCHK(S.add(v, nullptr, nk * D, &dv));
        if (op == SMG_WAVE_ADVANCE) HIPCHK(S.add(w, nullptr, nk * D, &dw));
        if (op == SMG_WAVE_SOURCES || op == SMG_WAVE_RECORD) HIPCHK(S.add(idx, nullptr, ni * sizeof(int), &didx));
        if (op == SMG_WAVE_SOURCES) {
            HIPCHK(S.add(sig0, nullptr, ni * kk * D, &ds0));
            HIPCHK(S.add(sig1, nullptr, ni * kk * D, &ds1));
        }
        HIPCHK(S.add(out, out, out_count * D, &dout));
        if (op == SMG_WAVE_RECORD) {
            HIPCHK(launch_wave_record(nV, k, n_idx, didx, du, nV, dout, st));
        } else {
            std::vector<int> mp, mi, known;
            vertex_corner_lists(std::vector<int>(F, F + 3 * f), nV, mp, mi);
            int *dF = nullptr, *dmp = nullptr, *dmi = nullptr, *dknown = nullptr;
            double *dV = nullptr, *dW = nullptr, *dn = nullptr, *dA = nullptr, *dm = nullptr, *dmt = nullptr, *ds2 = nullptr, *dpart = nullptr, *dterms = nullptr;
            HIPCHK(S.add(F, nullptr, 3 * f * sizeof(int), &dF));
            HIPCHK(S.add(V, nullptr, 3 * n * D, &dV));
            HIPCHK(S.add(mp.data(), nullptr, mp.size() * sizeof(int), &dmp));
            HIPCHK(S.add(mi.data(), nullptr, mi.size() * sizeof(int), &dmi));
            HIPCHK(S.add(nullptr, nullptr, 9 * f * D, &dW));
            HIPCHK(S.add(nullptr, nullptr, 3 * f * D, &dn));
            HIPCHK(S.add(nullptr, nullptr, f * D, &dA));
            HIPCHK(S.add(nullptr, nullptr, n * D, &dm));
            HIPCHK(S.add(nullptr, nullptr, (size_t)fixed_sum_groups((int)std::max(nk, f)) * D, &dpart));
            if (clamped) {
                known.assign(n, 0);
                for (int b : boundary_vertices(F, nF, nV)) known[(size_t)b] = 1;
                HIPCHK(S.add(known.data(), nullptr, n * sizeof(int), &dknown));
            }
            std::vector<double> mt, s2;
            if (int rc = wave_planes(st, nV, nF, dV, dF, dmp, dmi, dW, dn, dA, dm, speed, sigma, dt, mt, s2)) return rc;
            HIPCHK(S.add(mt.data(), nullptr, n * D, &dmt));
            HIPCHK(S.add(s2.data(), nullptr, n * D, &ds2));
            const double a = 0.25 * dt * dt, q2 = 2.0 / dt;
            if (op == SMG_WAVE_ADVANCE) {
                HIPCHK(S.add(nullptr, nullptr, f * kk * D, &dterms));
                HIPCHK(launch_wave_advance(nV, k, dmt, ds2, dknown, dt, q2, dw, nV, du, dv, nV, dout, dout + nk, nV, dout + 2 * nk, nullptr, nullptr, nV, nullptr, st));
                double* o = dout + 3 * nk;
                HIPCHK(launch_wave_advance(nV, k, dmt, ds2, dknown, dt, q2, dw, nV, du, dv, nV, o, o + nk, nV, o + 2 * nk, o + 3 * nk, o + 5 * nk, nV, o + 4 * nk, st));
                HIPCHK(launch_fluid_velocity(nF, k, dF, dW, dn, dA, o, nV, nullptr, dterms, st));
                double* s = dout + 9 * nk;
                for (size_t c = 0; c < kk; c++) {
                    HIPCHK(launch_fixed_sum(o + 2 * nk + c * n, nV, dpart, s + c, st));
                    HIPCHK(launch_fixed_sum(dterms + c * f, nF, dpart, s + kk + c, st));
                }
                HIPCHK(launch_fixed_sum(o + 4 * nk, (int)nk, dpart, s + 2 * kk, st));
            } else {
                double *b = dout, *rsq = dout + nk, *z = dout + 2 * nk;
                HIPCHK(launch_wave_rhs(nV, k, dmt, ds2, dknown, dt, du, dv, nV, b, z, nV, rsq, st));
                if (op == SMG_WAVE_SOURCES) HIPCHK(launch_wave_sources(nV, k, n_idx, didx, ds0, ds1, a, b, nV, rsq, st));
                HIPCHK(launch_fixed_sum(rsq, (int)nk, dpart, dout + 3 * nk, st));
            }
            int bad = 0;
            HIPCHK(S.finish(&bad));   // mt, s2 and the lists live until the stream has drained
            if (guard_hits) *guard_hits = bad;
            return SMG_OK;
        }
        int bad = 0;
        HIPCHK(S.finish(&bad));
        if (guard_hits) *guard_hits = bad;
        return SMG_OK;
    });
}

extern "C" int smg_debug_wave_adjoint(int op, int nV, int nF, int k, const int* F, const double* V, const double* speed, const double* sigma, int clamped,
                                      double dt, const double* x0, const double* x1, const double* x2, const double* x3, const double* x4, const int* idx, int n_idx,
                                      int n_rows, double* out, int* guard_hits)
{
    return guarded("smg_debug_wave_adjoint", [&]() -> int {
        const char* who = "smg_debug_wave_adjoint";
        if (int rc = wave_adjoint_check_operands(who, op, nV, nF, k, F, V, speed, sigma, clamped, dt, x0, x1, x2, x3, x4, idx, n_idx, n_rows, out)) return rc;
        if (int rc = need_device(who)) return rc;
        const size_t n = (size_t)nV, f = (size_t)nF, kk = (size_t)k, nk = n * kk, D = sizeof(double);
        if (2 * nk > (size_t)INT_MAX) return fail(SMG_ERR_INVALID, "%s: k = %d exceeds the index range", who, k);
        Scratch S;
        HIPCHK(S.init());
        hipStream_t st = S.stream();
        const size_t ni = (size_t)std::max(n_idx, 0), ent = (size_t)std::max(n_rows, 0) * ni, sk = ni * kk;
        const size_t xs[7][5] = {{nk, nk, nk, 0, 0}, {ent * kk, ent * kk, 0, 0, 0}, {nk, sk, 0, 0, 0}, {nk, nk, 0, 0, 0}, {nk, nk, nk, nk, nk}, {nk, sk, sk, 0, 0},
                                 {nk, 0, 0, 0, 0}};   // the operands' extents per op
        const size_t outs[7] = {nk, 2 * ent * kk + kk, nk, 2 * nk + 1, 3 * nk, 2 * sk, nk};
        const double* x[5] = {x0, x1, x2, x3, x4};
        double *dx[5] = {nullptr, nullptr, nullptr, nullptr, nullptr}, *dout = nullptr, *dpart = nullptr;
        for (int j = 0; j < 5; j++)
            if (x[j] && xs[op][j] > 0) HIPCHK(S.add(x[j], nullptr, xs[op][j] * D, &dx[j]));
        HIPCHK(S.add(out, out, outs[op] * D, &dout));
        HIPCHK(S.add(nullptr, nullptr, (size_t)fixed_sum_groups((int)std::max(nk, ent)) * D, &dpart));
        std::vector<int> known, gv, gp, gl, mp, mi;   // they live until the stream has drained
        std::vector<double> mt, s2, fac;
        int *dknown = nullptr, *didx = nullptr;
        if (clamped) {
            known.assign(n, 0);
            for (int b : boundary_vertices(F, nF, nV)) known[(size_t)b] = 1;
            HIPCHK(S.add(known.data(), nullptr, n * sizeof(int), &dknown));
        }
        const double a = 0.25 * dt * dt, q2 = 2.0 / dt;
        if (op == SMG_WAVE_ADJ_RESIDUAL) {
            double* sq = dout + ent * kk;
            HIPCHK(launch_wave_adj_residual(k, (long long)ent, dx[0], dx[1], dout, sq, st));
            for (size_t c = 0; c < kk; c++) HIPCHK(launch_fixed_sum(sq + c * ent, (int)ent, dpart, dout + 2 * ent * kk + c, st));
        } else if (op == SMG_WAVE_ADJ_INJECT) {
            wave_group_receivers(nV, n_idx, idx, clamped ? known.data() : nullptr, gv, gp, gl);
            int *dgv = nullptr, *dgp = nullptr, *dgl = nullptr;
            if (!gv.empty()) {
                HIPCHK(S.add(gv.data(), nullptr, gv.size() * sizeof(int), &dgv));
                HIPCHK(S.add(gl.data(), nullptr, gl.size() * sizeof(int), &dgl));
            }
            HIPCHK(S.add(gp.data(), nullptr, gp.size() * sizeof(int), &dgp));
            HIPCHK(hipMemcpyAsync(dout, dx[0], nk * D, hipMemcpyDeviceToDevice, st));
            HIPCHK(launch_wave_adj_inject(nV, k, (int)gv.size(), dgv, dgp, dgl, dx[1], dout, nV, st));
        } else if (op == SMG_WAVE_ADJ_RHS) {
            HIPCHK(launch_wave_adj_rhs(nV, k, dknown, q2, dx[0], dx[1], nV, dout, nV, dout + nk, st));
            HIPCHK(launch_fixed_sum(dout + nk, (int)nk, dpart, dout + 2 * nk, st));
        } else if (op == SMG_WAVE_ADJ_SIGNAL) {
            HIPCHK(S.add(idx, nullptr, ni * sizeof(int), &didx));
            HIPCHK(hipMemcpyAsync(dout, dx[1], sk * D, hipMemcpyDeviceToDevice, st));
            HIPCHK(hipMemcpyAsync(dout + sk, dx[2], sk * D, hipMemcpyDeviceToDevice, st));
            HIPCHK(launch_wave_adj_signal(nV, k, n_idx, didx, a, dx[0], nV, dout, dout + sk, st));
        } else {
            vertex_corner_lists(std::vector<int>(F, F + 3 * f), nV, mp, mi);
            int *dF = nullptr, *dmp = nullptr, *dmi = nullptr;
            double *dV = nullptr, *dW = nullptr, *dn = nullptr, *dA = nullptr, *dm = nullptr, *dmt = nullptr, *ds2 = nullptr, *dfac = nullptr;
            HIPCHK(S.add(F, nullptr, 3 * f * sizeof(int), &dF));
            HIPCHK(S.add(V, nullptr, 3 * n * D, &dV));
            HIPCHK(S.add(mp.data(), nullptr, mp.size() * sizeof(int), &dmp));
            HIPCHK(S.add(mi.data(), nullptr, mi.size() * sizeof(int), &dmi));
            HIPCHK(S.add(nullptr, nullptr, 9 * f * D, &dW));
            HIPCHK(S.add(nullptr, nullptr, 3 * f * D, &dn));
            HIPCHK(S.add(nullptr, nullptr, f * D, &dA));
            HIPCHK(S.add(nullptr, nullptr, n * D, &dm));
            if (int rc = wave_planes(st, nV, nF, dV, dF, dmp, dmi, dW, dn, dA, dm, speed, sigma, dt, mt, s2)) return rc;
            HIPCHK(S.add(mt.data(), nullptr, n * D, &dmt));
            HIPCHK(S.add(s2.data(), nullptr, n * D, &ds2));
            if (op == SMG_WAVE_ADJ_KEEP) {
                HIPCHK(launch_wave_adj_keep(nV, k, ds2, dt, dx[0], dx[1], dx[2], nV, dout, st));
            } else if (op == SMG_WAVE_ADJ_ADVANCE) {
                HIPCHK(hipMemcpyAsync(dout, dx[1], nk * D, hipMemcpyDeviceToDevice, st));
                HIPCHK(hipMemcpyAsync(dout + nk, dx[2], nk * D, hipMemcpyDeviceToDevice, st));
                HIPCHK(hipMemcpyAsync(dout + 2 * nk, dx[4], nk * D, hipMemcpyDeviceToDevice, st));
                HIPCHK(launch_wave_adj_advance(nV, k, dmt, ds2, dt, q2, dx[0], nV, dx[3], dout, dout + nk, dout + 2 * nk, nV, st));
            } else {
                fac.resize(n);
                wave_adj_host_planes(nV, mt.data(), speed, fac.data());
                HIPCHK(S.add(fac.data(), nullptr, n * D, &dfac));
                HIPCHK(launch_wave_adj_scale(nV, k, dfac, dx[0], nV, dout, nV, st));
            }
        }
        int bad = 0;
        HIPCHK(S.finish(&bad));
        if (guard_hits) *guard_hits = bad;
        return SMG_OK;
    });
}

extern "C" int smg_debug_wave_born(int nV, int nF, int k, int d_cols, const int* F, int clamped, const double* b, const double* e, const double* fd,
                                   double* out, int* guard_hits)
{
    return guarded("smg_debug_wave_born", [&]() -> int {
        const char* who = "smg_debug_wave_born";
        if (int rc = wave_born_check_operands(who, nV, nF, k, d_cols, F, clamped, b, e, fd, out)) return rc;
        if (int rc = need_device(who)) return rc;
        const size_t n = (size_t)nV, kk = (size_t)k, nk = n * kk, D = sizeof(double);
        if (2 * nk > (size_t)INT_MAX) return fail(SMG_ERR_INVALID, "%s: k = %d exceeds the index range", who, k);
        Scratch S;
        HIPCHK(S.init());
        hipStream_t st = S.stream();
        double *db = nullptr, *de = nullptr, *dfd = nullptr, *dout = nullptr, *dpart = nullptr;
        int* dknown = nullptr;
        HIPCHK(S.add(b, nullptr, nk * D, &db));
        HIPCHK(S.add(e, nullptr, nk * D, &de));
        HIPCHK(S.add(fd, nullptr, n * (size_t)d_cols * D, &dfd));
        HIPCHK(S.add(nullptr, out, (2 * nk + 1) * D, &dout));
        HIPCHK(S.add(nullptr, nullptr, (size_t)fixed_sum_groups((int)nk) * D, &dpart));
        std::vector<int> known;   // lives until the stream has drained
        if (clamped) {
            known.assign(n, 0);
            for (int v : boundary_vertices(F, nF, nV)) known[(size_t)v] = 1;
            HIPCHK(S.add(known.data(), nullptr, n * sizeof(int), &dknown));
        }
        HIPCHK(hipMemcpyAsync(dout, db, nk * D, hipMemcpyDeviceToDevice, st));
        HIPCHK(hipMemsetAsync(dout + nk, 0, nk * D, st));   // the squares start as k_wave_rhs leaves the known rows
        HIPCHK(launch_wave_born(nV, k, d_cols, dknown, dfd, de, dout, nV, dout + nk, st));
        HIPCHK(launch_fixed_sum(dout + nk, (int)nk, dpart, dout + 2 * nk, st));
        int bad = 0;
        HIPCHK(S.finish(&bad));
        if (guard_hits) *guard_hits = bad;
        return SMG_OK;
    });
}

extern "C" int smg_debug_wave_time(int op, int nV, int nF, int k, const int* F, const double* V, int reps, double* ms)
{
    return guarded("smg_debug_wave_time", [&]() -> int {
        const char* who = "smg_debug_wave_time";
        if ((op != SMG_WAVE_RHS && op != SMG_WAVE_ADVANCE) || nV < 1 || nF < 1 || !F || !V || !ms) return fail(SMG_ERR_INVALID, "%s: bad arguments", who);
        if (k < 1 || reps < 1) return fail(SMG_ERR_INVALID, "%s: k = %d, reps = %d, at least 1 each is needed", who, k, reps);
        if (int rc = check_faces(who, F, nF, nV)) return rc;
        if (int rc = need_device(who)) return rc;
        const size_t n = (size_t)nV, f = (size_t)nF, kk = (size_t)k, nk = n * kk, D = sizeof(double);
        if (2 * nk > (size_t)INT_MAX) return fail(SMG_ERR_INVALID, "%s: k = %d exceeds the index range", who, k);
        std::vector<int> mp, mi;
        vertex_corner_lists(std::vector<int>(F, F + 3 * f), nV, mp, mi);
        struct Event { hipEvent_t e = nullptr; ~Event() { if (e) (void)hipEventDestroy(e); } } t0, t1;
        Scratch S;                                                           // for its stream alone
        HIPCHK(S.init());
        hipStream_t st = S.stream();
        DevBuf<int> dF, dmp, dmi;
        DevBuf<double> dV, dW, dn, dA, dm, dmt, ds2, s0, s1, B, Wb, rsq, ke;
        HIPCHK(dF.upload(std::vector<int>(F, F + 3 * f)));
        HIPCHK(dmp.upload(mp));
        HIPCHK(dmi.upload(mi));
        HIPCHK(dV.upload(std::vector<double>(V, V + 3 * n)));
        HIPCHK(dW.alloc(9 * f));
        HIPCHK(dn.alloc(3 * f));
        HIPCHK(dA.alloc(f));
        HIPCHK(dm.alloc(n));
        std::vector<double> mt, s2;
        if (int rc = wave_planes(st, nV, nF, dV.p, dF.p, dmp.p, dmi.p, dW.p, dn.p, dA.p, dm.p, nullptr, nullptr, 0.5, mt, s2)) return rc;
        HIPCHK(dmt.upload(mt));
        HIPCHK(ds2.upload(s2));
        for (DevBuf<double>* b : {&s0, &s1}) {                               // zeros: the operands' values do not change what a launch moves
            HIPCHK(b->alloc(2 * nk));
            HIPCHK(hipMemsetAsync(b->p, 0, 2 * nk * D, st));
        }
        for (DevBuf<double>* b : {&B, &Wb, &rsq, &ke}) {
            HIPCHK(b->alloc(nk));
            HIPCHK(hipMemsetAsync(b->p, 0, nk * D, st));
        }
        auto launch = [&]() -> hipError_t {
            if (op == SMG_WAVE_RHS) return launch_wave_rhs(nV, k, dmt.p, ds2.p, nullptr, 0.5, s0.p, s0.p + nk, nV, B.p, Wb.p, nV, rsq.p, st);
            return launch_wave_advance(nV, k, dmt.p, ds2.p, nullptr, 0.5, 4.0, Wb.p, nV, s0.p, s0.p + nk, nV, s1.p, s1.p + nk, nV, ke.p, B.p, Wb.p, nV, rsq.p, st);   // as the object: the warm start over w
        };
        HIPCHK(hipEventCreate(&t0.e));
        HIPCHK(hipEventCreate(&t1.e));
        HIPCHK(launch());                                                    // one launch that is not timed
        HIPCHK(hipEventRecord(t0.e, st));
        for (int r = 0; r < reps; r++) HIPCHK(launch());
        HIPCHK(hipEventRecord(t1.e, st));
        HIPCHK(hipStreamSynchronize(st));
        float total = 0.0f;
        HIPCHK(hipEventElapsedTime(&total, t0.e, t1.e));
        *ms = (double)total / reps;
        return SMG_OK;
    });
}

extern "C" int smg_debug_conformal(int op, int nV, int nF, const int* F, const double* l0, const double* area2, const double* u, const double* d, double t,
                                   const double* s, const double* Theta, const int* fixed, int n_fixed, double* out, int* guard_hits)
{
    return guarded("smg_debug_conformal", [&]() -> int {
        const char* who = "smg_debug_conformal";
        if (int rc = conformal_check_operands(who, op, nV, nF, F, l0, area2, u, d, t, s, Theta, fixed, n_fixed, out)) return rc;
        if (int rc = need_device(who)) return rc;
        const size_t n = (size_t)nV, f = (size_t)nF, D = sizeof(double), I = sizeof(int);
        AssemblyPlan plan;
        std::vector<int> mask;
        if (op == SMG_CONFORMAL_ROWS) {
            plan = make_assembly_plan(std::vector<int>(F, F + 3 * f), nV);
            mask.assign(n, 0);
            for (int i = 0; i < n_fixed; i++) mask[(size_t)fixed[i]] = 1;
        }
        const size_t nnz = plan.pattern.col.size();
        Scratch S;
        HIPCHK(S.init());
        const size_t out_count = op == SMG_CONFORMAL_SCALE ? 2 * n : op == SMG_CONFORMAL_FACES ? 10 * f : 4 * n + 3 + nnz;
        int *dF = nullptr, *dmp = nullptr, *dmi = nullptr, *drp = nullptr, *dlp = nullptr, *dli = nullptr, *dmask = nullptr;
        signed char* dls = nullptr;
        double *dl0 = nullptr, *da2 = nullptr, *du = nullptr, *dd = nullptr, *ds = nullptr, *dTh = nullptr, *dout = nullptr, *dang = nullptr, *dhc = nullptr, *dbr = nullptr,
               *dpart = nullptr;
        HIPCHK(S.add(F, nullptr, 3 * f * I, &dF));
        if (op == SMG_CONFORMAL_SCALE) {
            HIPCHK(S.add(u, nullptr, n * D, &du));
            if (d) HIPCHK(S.add(d, nullptr, n * D, &dd));
        } else {
            HIPCHK(S.add(l0, nullptr, 3 * f * D, &dl0));
            HIPCHK(S.add(area2, nullptr, f * D, &da2));
            HIPCHK(S.add(s, nullptr, n * D, &ds));
        }
        if (op == SMG_CONFORMAL_ROWS) {
            HIPCHK(S.add(Theta, nullptr, n * D, &dTh));
            HIPCHK(S.add(mask.data(), nullptr, n * I, &dmask));
            HIPCHK(S.add(plan.m_ptr.data(), nullptr, plan.m_ptr.size() * I, &dmp));
            HIPCHK(S.add(plan.m_idx.data(), nullptr, plan.m_idx.size() * I, &dmi));
            HIPCHK(S.add(plan.pattern.ptr.data(), nullptr, plan.pattern.ptr.size() * I, &drp));
            HIPCHK(S.add(plan.l_ptr.data(), nullptr, plan.l_ptr.size() * I, &dlp));
            HIPCHK(S.add(plan.l_idx.data(), nullptr, plan.l_idx.size() * I, &dli));
            HIPCHK(S.add(plan.l_sgn.data(), nullptr, plan.l_sgn.size(), &dls));
            HIPCHK(S.add(nullptr, nullptr, 3 * f * D, &dang));
            HIPCHK(S.add(nullptr, nullptr, 3 * f * D, &dhc));
            HIPCHK(S.add(nullptr, nullptr, f * D, &dbr));
            HIPCHK(S.add(nullptr, nullptr, (size_t)fixed_sum_groups(std::max(nV, nF)) * D, &dpart));
        }
        HIPCHK(S.add(out, out, out_count * D, &dout));
        hipStream_t st = S.stream();
        switch (op) {
            case SMG_CONFORMAL_SCALE: HIPCHK(launch_conformal_scale(nV, du, dd, t, dout + n, dout, st)); break;
            case SMG_CONFORMAL_FACES:
                HIPCHK(launch_conformal_faces(nF, dF, dl0, da2, ds, dout, dout + 3 * f, dout + 6 * f, st));
                HIPCHK(launch_conformal_lengths(nF, dF, dl0, ds, dout + 7 * f, st));
                break;
            default:
                HIPCHK(launch_conformal_faces(nF, dF, dl0, da2, ds, dang, dhc, dbr, st));
                HIPCHK(launch_conformal_rows(nV, nF, dang, dhc, dbr, dmp, dmi, dTh, dmask, drp, dlp, dli, dls, dout, dout + n, dout + 2 * n, dout + 3 * n,
                                             dout + 4 * n + 3, dpart, dout + 4 * n, st));
                break;
        }
        int bad = 0;
        HIPCHK(S.finish(&bad));
        if (guard_hits) *guard_hits = bad;
        return SMG_OK;
    });
}

namespace {

// what the union launchers index with: the level-0 row lists (SUMSQ_DECIDE, RESTORE) or the coarsest level's member blocks (COARSE)
const char* check_union_lists(int op, int m, int n, const int* rptr, const int* rows, const long long* moff, const int* mlda, const int* mrow0,
                              const int* row_member)
{
    if (op != SMG_UNION_COARSE) {
        if (!rptr || !rows || rptr[0] != 0) return "missing or bad row lists";
        for (int i = 0; i < m; i++) if (rptr[i + 1] < rptr[i]) return "row list pointers not monotone";
        if (rptr[m] > n) return "more listed rows than rows";
        std::vector<char> seen((size_t)n, 0);
        for (int p = 0; p < rptr[m]; p++) {
            if (rows[p] < 0 || rows[p] >= n) return "row index out of range";
            if (seen[(size_t)rows[p]]++) return "a row is listed twice";
        }
        return nullptr;
    }
    if (!moff || !mlda || !mrow0 || !row_member || mrow0[0] != 0 || mrow0[m] != n) return "missing or bad member blocks";
    for (int i = 0; i < m; i++) {
        const int ni = mrow0[i + 1] - mrow0[i];
        if (ni < 0) return "member rows not monotone";
        if (mlda[i] < 64 || mlda[i] % 64 != 0 || mlda[i] < ni) return "a leading dimension that is no multiple of 64 or smaller than its member";
        if (moff[i] < 0 || moff[i] % 2 != 0) return "a block offset that is negative or odd";
        for (int r = mrow0[i]; r < mrow0[i + 1]; r++) if (row_member[r] != i) return "row_member disagrees with mrow0";
    }
    return nullptr;
}

}  // namespace

extern "C" int smg_debug_union(int op, int m, int n, int k, const int* rptr, const int* rows, double* r, double* u, double* zsave, double* ss,
                               int* mdone, int* nhis, double* his, int cap, const double* Ainv, const long long* moff, const int* mlda,
                               const int* mrow0, const int* row_member, double* b, double tol, int done, double* ctrl_d, int* ctrl_i, double* r_his,
                               int* guard_hits)
{
    return guarded("smg_debug_union", [&]() -> int {
        if (op < SMG_UNION_SUMSQ_DECIDE || op > SMG_UNION_COARSE || m < 1 || m > 65535 || n < 1 || k < 1 || (long)n * k > (1L << 30) || !u)
            return fail(SMG_ERR_INVALID, "smg_debug_union: bad arguments");
        if (op != SMG_UNION_COARSE && (!zsave || !mdone)) return fail(SMG_ERR_INVALID, "smg_debug_union: op %d misses an operand", op);
        if (op == SMG_UNION_SUMSQ_DECIDE && (!r || !ss || !nhis || !his || cap < 1 || !ctrl_i || !ctrl_d || ctrl_i[2] < 0 || (ctrl_i[2] > 0 && !r_his)))
            return fail(SMG_ERR_INVALID, "smg_debug_union: op %d misses an operand", op);
        if (op == SMG_UNION_COARSE && (!Ainv || !b)) return fail(SMG_ERR_INVALID, "smg_debug_union: op %d misses an operand", op);
        if (const char* why = check_union_lists(op, m, n, rptr, rows, moff, mlda, mrow0, row_member)) return fail(SMG_ERR_INVALID, "smg_debug_union: %s", why);
        if (int rc = need_device("smg_debug_union")) return rc;
        Scratch X;
        HIPCHK(X.init());
        hipStream_t st = X.stream();
        const size_t blk = (size_t)n * k * sizeof(double), mi = (size_t)m * sizeof(int), md = (size_t)m * sizeof(double);
        UnionDev U;
        U.m = m;
        U.his_cap = cap;
        int *drptr = nullptr, *drows = nullptr, *dmlda = nullptr, *dmrow0 = nullptr, *dmember = nullptr;
        long long* dmoff = nullptr;
        double *dr = nullptr, *du = nullptr, *db = nullptr, *dAinv = nullptr, *dhis = nullptr;
        Ctrl* dctrl = nullptr;
        HIPCHK(X.add(u, u, blk, &du));
        Ctrl c = make_ctrl(done, tol, nullptr);
        if (op != SMG_UNION_COARSE) {
            HIPCHK(X.add(rptr, nullptr, ((size_t)m + 1) * sizeof(int), &drptr));
            HIPCHK(X.add(rows, nullptr, (size_t)rptr[m] * sizeof(int), &drows));
            HIPCHK(X.add(zsave, zsave, blk, &U.zsave));
            HIPCHK(X.add(mdone, mdone, mi, &U.done));
            U.rows = drows;
            U.rptr = drptr;
            for (int i = 0; i < m; i++) U.max_rows = std::max(U.max_rows, rptr[i + 1] - rptr[i]);
        }
        if (op == SMG_UNION_SUMSQ_DECIDE) {
            HIPCHK(X.add(r, r, blk, &dr));
            HIPCHK(X.add(ss, ss, md, &U.ss));
            HIPCHK(X.add(nhis, nhis, mi, &U.nhis));
            HIPCHK(X.add(his, his, (size_t)m * cap * sizeof(double), &U.his));
            HIPCHK(X.add(r_his, r_his, (size_t)ctrl_i[2] * sizeof(double), &dhis));
            c.r_his = dhis;
            c.n_his = ctrl_i[0];
            c.status = ctrl_i[1];
            c.his_cap = ctrl_i[2];
            c.r_last = ctrl_d[0];
        }
        if (op == SMG_UNION_COARSE) {
            size_t len = 0;
            for (int i = 0; i < m; i++) len = std::max(len, (size_t)moff[i] + (size_t)mlda[i] * mlda[i]);
            HIPCHK(X.add(Ainv, nullptr, len * sizeof(double), &dAinv));
            HIPCHK(X.add(moff, nullptr, (size_t)m * sizeof(long long), &dmoff));
            HIPCHK(X.add(mlda, nullptr, mi, &dmlda));
            HIPCHK(X.add(mrow0, nullptr, ((size_t)m + 1) * sizeof(int), &dmrow0));
            HIPCHK(X.add(row_member, nullptr, (size_t)n * sizeof(int), &dmember));
            HIPCHK(X.add(b, b, blk, &db));
            U.crow_member = dmember;
            U.moff = dmoff;
            U.mlda = dmlda;
            U.mrow0 = dmrow0;
        }
        HIPCHK(X.add(&c, &c, sizeof c, &dctrl));
        if (op == SMG_UNION_SUMSQ_DECIDE) HIPCHK(launch_union_sumsq_decide(U, dr, du, k, dctrl, st));
        else if (op == SMG_UNION_RESTORE) HIPCHK(launch_union_restore(U, du, k, dctrl, st));
        else HIPCHK(launch_blockdiag_gemv_add(U, dAinv, n, db, du, k, dctrl, st));
        int bad = 0;
        HIPCHK(X.finish(&bad));
        if (ctrl_d) { ctrl_d[0] = c.r_last; ctrl_d[1] = c.r_prev; ctrl_d[2] = c.sumsq; }
        if (ctrl_i) { ctrl_i[0] = c.n_his; ctrl_i[1] = c.status; ctrl_i[3] = c.done; }
        if (guard_hits) *guard_hits = bad;
        return SMG_OK;
    });
}
