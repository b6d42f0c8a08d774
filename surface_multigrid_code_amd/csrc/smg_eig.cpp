// smg_eig.cpp -- the smallest eigenpairs of A_uu x = lambda M_uu x by LOBPCG preconditioned by the V-cycle (include/smg.h: smg_eigs,
// DESIGN.md section 17), and the small dense generalized symmetric eigensolver its Rayleigh-Ritz step runs on the host.
//
// One iteration (m iterated columns, X M-orthonormal with X^T A X = Lambda):
//   W = V(R, 0);  AW = A W                                            (device: V-cycle, SpMV)
//   G_M = S^T M S,  G_A = S^T AS   for S = [X W P], AS = [AX AW AP]   (device: smg_eig_device.hip, deterministic Grams)
//   -> host: the residual norms of X and both Grams in one synchronisation; Rayleigh-Ritz on span(S) with the basis orthonormalised in the
//      small space (scaled Cholesky of G_M, columns of W and P dropped where the pivot says they add nothing new)
//   X, AX = S Cx, AS Cx;  P, AP = [W P] Cp, [AW AP] Cp                (device: one pass over S and AS)
//   R = AX - M X Lambda with its norms, and the next preconditioner input in the same pass
// M is diagonal, so M-products are never stored: the Gram kernel weights rows by the mass, the residual kernel multiplies by it.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "smg_internal.hpp"

using namespace smg;

namespace {

// ---- small dense symmetric eigenproblems (row-major n x n, n <= 192 in the loop) ---------------------------------------------------

// Householder reduction of the symmetric A to tridiagonal form, A = Q T Q^T (Golub / Van Loan, Algorithm 8.3.1).  On return A holds T and
// Z = Q (row-major).
void tridiagonalize(std::vector<double>& A, int n, std::vector<double>& Z)
{
    Z.assign((size_t)n * n, 0.0);
    for (int i = 0; i < n; i++) Z[(size_t)i * n + i] = 1.0;
    std::vector<double> v((size_t)n), p((size_t)n), w((size_t)n);
    for (int k = 0; k + 2 < n; k++) {
        const int len = n - k - 1;
        double tail = 0.0;
        for (int j = 1; j < len; j++) tail += A[(size_t)(k + 1 + j) * n + k] * A[(size_t)(k + 1 + j) * n + k];
        if (tail == 0.0) continue;            // the column is already tridiagonal
        const double x0 = A[(size_t)(k + 1) * n + k];
        const double nrm = std::sqrt(x0 * x0 + tail);
        const double alpha = x0 >= 0.0 ? -nrm : nrm;
        for (int j = 0; j < len; j++) v[j] = A[(size_t)(k + 1 + j) * n + k];
        v[0] -= alpha;
        double vv = 0.0;
        for (int j = 0; j < len; j++) vv += v[j] * v[j];
        const double beta = 2.0 / vv;
        // p = beta A22 v;  w = p - (beta / 2) (p.v) v;  A22 -= v w^T + w v^T
        for (int i = 0; i < len; i++) {
            double s = 0.0;
            const double* row = &A[(size_t)(k + 1 + i) * n + k + 1];
            for (int j = 0; j < len; j++) s += row[j] * v[j];
            p[i] = beta * s;
        }
        double pv = 0.0;
        for (int j = 0; j < len; j++) pv += p[j] * v[j];
        for (int j = 0; j < len; j++) w[j] = p[j] - 0.5 * beta * pv * v[j];
        for (int i = 0; i < len; i++) {
            double* row = &A[(size_t)(k + 1 + i) * n + k + 1];
            for (int j = 0; j < len; j++) row[j] -= v[i] * w[j] + w[i] * v[j];
        }
        A[(size_t)(k + 1) * n + k] = A[(size_t)k * n + k + 1] = alpha;
        for (int j = 1; j < len; j++) A[(size_t)(k + 1 + j) * n + k] = A[(size_t)k * n + k + 1 + j] = 0.0;
        // Z = Z (I - beta v v^T) on columns k+1 ..
        for (int i = 0; i < n; i++) {
            double* row = &Z[(size_t)i * n + k + 1];
            double s = 0.0;
            for (int j = 0; j < len; j++) s += row[j] * v[j];
            s *= beta;
            for (int j = 0; j < len; j++) row[j] -= s * v[j];
        }
    }
}

// Eigen-decomposition of the symmetric A (row-major, destroyed): ascending eigenvalues d, eigenvectors as the columns of Z (row-major).
// Householder tridiagonalisation, then implicit symmetric QR steps with the Wilkinson shift (Golub / Van Loan, Algorithm 8.3.3), the Givens
// rotations accumulated into Z.  false: no convergence.
bool sym_eig(std::vector<double>& A, int n, std::vector<double>& d, std::vector<double>& Z)
{
    tridiagonalize(A, n, Z);
    // the rotations combine two columns of Z: they run on the rows of Zt = Z^T, where those columns are contiguous
    std::vector<double> Zt((size_t)n * n);
    for (int i = 0; i < n; i++)
        for (int j = 0; j < n; j++) Zt[(size_t)j * n + i] = Z[(size_t)i * n + j];
    auto T = [&](int i, int j) -> double& { return A[(size_t)i * n + j]; };
    const double eps = 2.220446049250313e-16;
    int hi = n - 1, sweeps = 0;
    while (hi > 0) {
        for (int i = 0; i < hi; i++)
            if (std::fabs(T(i + 1, i)) <= eps * (std::fabs(T(i, i)) + std::fabs(T(i + 1, i + 1)))) T(i + 1, i) = T(i, i + 1) = 0.0;
        while (hi > 0 && T(hi, hi - 1) == 0.0) hi--;
        if (hi == 0) break;
        int lo = hi - 1;
        while (lo > 0 && T(lo, lo - 1) != 0.0) lo--;
        if (++sweeps > 60 * n) return false;
        // Wilkinson shift from the trailing 2 x 2 block
        const double a = T(hi - 1, hi - 1), b = T(hi, hi - 1), c = T(hi, hi);
        const double del = 0.5 * (a - c);
        const double den = del + (del >= 0.0 ? 1.0 : -1.0) * std::hypot(del, b);
        const double mu = c - b * b / den;
        double x = T(lo, lo) - mu, z = T(lo + 1, lo);
        for (int k = lo; k < hi; k++) {
            const double r = std::hypot(x, z);
            const double cs = r == 0.0 ? 1.0 : x / r, sn = r == 0.0 ? 0.0 : z / r;
            const int w0 = std::max(lo, k - 1), w1 = std::min(hi, k + 2);
            for (int j = w0; j <= w1; j++) {     // rows k, k+1
                const double t0 = T(k, j), t1 = T(k + 1, j);
                T(k, j) = cs * t0 + sn * t1;
                T(k + 1, j) = -sn * t0 + cs * t1;
            }
            for (int i = w0; i <= w1; i++) {     // columns k, k+1
                const double t0 = T(i, k), t1 = T(i, k + 1);
                T(i, k) = cs * t0 + sn * t1;
                T(i, k + 1) = -sn * t0 + cs * t1;
            }
            if (k > lo) T(k + 1, k - 1) = T(k - 1, k + 1) = 0.0;   // the bulge this rotation chased
            double* zk = &Zt[(size_t)k * n];
            double* zk1 = &Zt[(size_t)(k + 1) * n];
            for (int i = 0; i < n; i++) {
                const double z0 = zk[i], z1 = zk1[i];
                zk[i] = cs * z0 + sn * z1;
                zk1[i] = -sn * z0 + cs * z1;
            }
            if (k + 1 < hi) { x = T(k + 1, k); z = T(k + 2, k); }
        }
    }
    std::vector<int> ord((size_t)n);
    for (int i = 0; i < n; i++) ord[i] = i;
    std::stable_sort(ord.begin(), ord.end(), [&](int i, int j) { return T(i, i) < T(j, j); });
    d.resize((size_t)n);
    std::vector<double> Zs((size_t)n * n);
    for (int j = 0; j < n; j++) {
        d[j] = T(ord[j], ord[j]);
        for (int i = 0; i < n; i++) Zs[(size_t)i * n + j] = Zt[(size_t)ord[j] * n + i];
    }
    Z.swap(Zs);
    return true;
}

// Rayleigh-Ritz on the span of the q = nb m columns of S given G_M = S^T M S and G_A = S^T A S (row-major q x q).  The columns are scaled to
// unit M-norm and orthonormalised by a Cholesky factorisation of the scaled G_M in column order (X, then W, then P); a column whose pivot
// -- the squared M-sine of its angle to the columns kept before it -- is below `drop` is left out.  A dropped column of X is a failure.
// Out: C (q x m, row-major, rows of dropped columns 0) with S C M-orthonormal and (S C)^T A (S C) = diag(lam), lam ascending; *kept.
int rayleigh_ritz(int q, int m, const double* GM, const double* GA, double drop, std::vector<double>& C, std::vector<double>& lam, int* kept)
{
    std::vector<double> sc((size_t)q);
    std::vector<int> keep;
    std::vector<double> L;      // row-major q x q, row i = the kept column i's coefficients over the kept columns before it
    L.assign((size_t)q * q, 0.0);
    for (int j = 0; j < q; j++) {
        const double g = GM[(size_t)j * q + j];
        if (!(g > 0.0) || !std::isfinite(g)) { if (j < m) return SMG_ERR_NONFINITE; continue; }
        sc[j] = 1.0 / std::sqrt(g);
        const int r = (int)keep.size();
        double* Lj = &L[(size_t)j * q];
        double piv = 1.0;
        for (int t = 0; t < r; t++) {
            const int k = keep[t];
            double s = GM[(size_t)j * q + k] * sc[j] * sc[k];
            const double* Lk = &L[(size_t)k * q];
            for (int u = 0; u < t; u++) s -= Lj[u] * Lk[u];
            Lj[t] = s / Lk[t];
            piv -= Lj[t] * Lj[t];
        }
        if (!(piv > drop)) { if (j < m) return SMG_ERR_NONFINITE; for (int t = 0; t < r; t++) Lj[t] = 0.0; continue; }
        Lj[r] = std::sqrt(piv);
        keep.push_back(j);
    }
    const int r = (int)keep.size();
    *kept = r;
    if (r < m) return SMG_ERR_NONFINITE;
    // Ah = L^-1 (D G_A D) L^-T on the kept columns
    std::vector<double> Y((size_t)r * r), Ah((size_t)r * r);
    for (int c = 0; c < r; c++) {             // column c of Y = L^-1 (D G_A D)[:, c]
        const int kc = keep[c];
        for (int i = 0; i < r; i++) {
            const int ki = keep[i];
            double s = 0.5 * (GA[(size_t)ki * q + kc] + GA[(size_t)kc * q + ki]) * sc[ki] * sc[kc];
            for (int u = 0; u < i; u++) s -= L[(size_t)ki * q + u] * Y[(size_t)u * r + c];
            Y[(size_t)i * r + c] = s / L[(size_t)ki * q + i];
        }
    }
    for (int c = 0; c < r; c++) {             // column c of Ah = L^-1 (row c of Y)^T
        for (int i = 0; i < r; i++) {
            double s = Y[(size_t)c * r + i];
            for (int u = 0; u < i; u++) s -= L[(size_t)keep[i] * q + u] * Ah[(size_t)u * r + c];
            Ah[(size_t)i * r + c] = s / L[(size_t)keep[i] * q + i];
        }
    }
    for (int i = 0; i < r; i++)
        for (int j = 0; j < i; j++) Ah[(size_t)i * r + j] = Ah[(size_t)j * r + i] = 0.5 * (Ah[(size_t)i * r + j] + Ah[(size_t)j * r + i]);
    std::vector<double> th, Z;
    if (!sym_eig(Ah, r, th, Z)) return SMG_ERR_NONFINITE;
    // C = D L^-T Z[:, :m]
    C.assign((size_t)q * m, 0.0);
    lam.assign(th.begin(), th.begin() + m);
    std::vector<double> col((size_t)r);
    for (int c = 0; c < m; c++) {
        for (int i = r - 1; i >= 0; i--) {
            double s = Z[(size_t)i * r + c];
            for (int u = i + 1; u < r; u++) s -= L[(size_t)keep[u] * q + i] * col[u];
            col[i] = s / L[(size_t)keep[i] * q + i];
        }
        for (int i = 0; i < r; i++) C[(size_t)keep[i] * m + c] = col[i] * sc[keep[i]];
    }
    return SMG_OK;
}

// a counter-based hash of (seed, row, column) -> uniform in [-1, 1): the default start block
double start_value(unsigned long long seed, long long row, int col)
{
    unsigned long long z = seed + 0x9E3779B97F4A7C15ull * (unsigned long long)(row * 64 + col + 1);
    for (int i = 0; i < 2; i++) {     // two rounds of splitmix64's finaliser
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        z ^= z >> 31;
    }
    return (double)(z >> 11) * (2.0 / 9007199254740992.0) - 1.0;
}

int default_block(int nev)
{
    const int want = nev + std::max(2, nev / 4);
    int b = 8;
    while (b < want && b < 64) b *= 2;
    return b;
}

}  // namespace

extern "C" int smg_debug_dense_geneig_host(int n, const double* A, const double* B, double* evals, double* V)
{
    return guarded("smg_debug_dense_geneig_host", [&]() -> int {
        if (n < 1 || !A || !B || !evals || !V) return fail(SMG_ERR_INVALID, "smg_debug_dense_geneig_host: bad arguments");
        // B = L L^T (lower, row-major)
        std::vector<double> L((size_t)n * n, 0.0);
        for (int j = 0; j < n; j++) {
            for (int i = j; i < n; i++) {
                double s = B[(size_t)i + (size_t)j * n];
                for (int u = 0; u < j; u++) s -= L[(size_t)i * n + u] * L[(size_t)j * n + u];
                if (i == j) {
                    if (!(s > 0.0) || !std::isfinite(s)) return fail(SMG_ERR_INVALID, "smg_debug_dense_geneig_host: B is not positive definite");
                    L[(size_t)j * n + j] = std::sqrt(s);
                } else L[(size_t)i * n + j] = s / L[(size_t)j * n + j];
            }
        }
        // Ah = L^-1 A L^-T
        std::vector<double> Y((size_t)n * n), Ah((size_t)n * n);
        for (int c = 0; c < n; c++)
            for (int i = 0; i < n; i++) {
                double s = A[(size_t)i + (size_t)c * n];
                for (int u = 0; u < i; u++) s -= L[(size_t)i * n + u] * Y[(size_t)u * n + c];
                Y[(size_t)i * n + c] = s / L[(size_t)i * n + i];
            }
        for (int c = 0; c < n; c++)
            for (int i = 0; i < n; i++) {
                double s = Y[(size_t)c * n + i];
                for (int u = 0; u < i; u++) s -= L[(size_t)i * n + u] * Ah[(size_t)u * n + c];
                Ah[(size_t)i * n + c] = s / L[(size_t)i * n + i];
            }
        for (int i = 0; i < n; i++)
            for (int j = 0; j < i; j++) Ah[(size_t)i * n + j] = Ah[(size_t)j * n + i] = 0.5 * (Ah[(size_t)i * n + j] + Ah[(size_t)j * n + i]);
        for (double v : Ah) if (!std::isfinite(v)) return fail(SMG_ERR_NONFINITE, "smg_debug_dense_geneig_host: non-finite entry");
        std::vector<double> d, Z;
        if (!sym_eig(Ah, n, d, Z)) return fail(SMG_ERR_NONFINITE, "smg_debug_dense_geneig_host: the QR iteration did not converge");
        // V = L^-T Z (column-major out)
        for (int c = 0; c < n; c++) {
            evals[c] = d[c];
            for (int i = n - 1; i >= 0; i--) {
                double s = Z[(size_t)i * n + c];
                for (int u = i + 1; u < n; u++) s -= L[(size_t)u * n + i] * V[(size_t)u + (size_t)c * n];
                V[(size_t)i + (size_t)c * n] = s / L[(size_t)i * n + i];
            }
        }
        return SMG_OK;
    });
}

namespace {

constexpr double EIG_DROP = 1e-8;       // Rayleigh-Ritz: smallest kept pivot of the unit-scaled M-Gram

struct EigRun {
    smg_hierarchy* h;
    int n, m;
    Ctrl* ctrl;
    int cur = 0;             // which of the double buffers holds X, AX, P, AP
    bool has_p = false;
    double *GM = nullptr, *GA = nullptr, *C = nullptr, *lam = nullptr, *res = nullptr;     // device (eig_small)
    double *hGM = nullptr, *hGA = nullptr, *hC = nullptr, *hlam = nullptr, *hres = nullptr;   // pinned host mirror
    int groups = 0;
};

// the cycle's options become the handle's selection and the level vectors are ready for k unpadded internal columns; the cycle never fuses a head
int eig_prepare(smg_hierarchy* h, const smg_solve_opts& o, int k)
{
    int rc = latch_solve_opts(h, o);
    if (rc || (rc = ensure_work(h, k))) return rc;
    if (h->precision == 1 && (rc = ensure_fp32(h, k))) return rc;
    h->k = k; h->k_user = k; h->coarse_cols = 0;
    h->head_fuse = false;
    return SMG_OK;
}

int eig_buffers(smg_hierarchy* h, EigRun& R)
{
    const size_t cnt = (size_t)R.n * R.m;
    const int q = 3 * R.m;
    for (int b = 0; b < 2; b++)
        for (DevBuf<double>* d : {&h->eig_x[b], &h->eig_ax[b], &h->eig_p[b], &h->eig_ap[b]}) HIPCHK(d->ensure(cnt));
    HIPCHK(h->eig_aw.ensure(cnt));
    if (h->precision == 1) HIPCHK(h->eig_w.ensure(cnt));
    HIPCHK(h->eig_mass.ensure((size_t)R.n));
    R.groups = eig_groups(R.n);
    HIPCHK(h->eig_part.ensure(std::max(eig_gram_part_size(q, q, R.groups), (size_t)R.groups * R.m)));
    const size_t small = (size_t)2 * q * q + (size_t)q * 2 * R.m + 2 * (size_t)R.m;
    HIPCHK(h->eig_small.ensure(small));
    HIPCHK(h->eig_pin.ensure(small));
    double* d = h->eig_small.p;
    double* p = h->eig_pin.p;
    const size_t off[5] = {0, (size_t)q * q, (size_t)2 * q * q, (size_t)2 * q * q + (size_t)q * 2 * R.m, (size_t)2 * q * q + (size_t)q * 2 * R.m + R.m};
    R.GM = d + off[0]; R.GA = d + off[1]; R.C = d + off[2]; R.lam = d + off[3]; R.res = d + off[4];
    R.hGM = p + off[0]; R.hGA = p + off[1]; R.hC = p + off[2]; R.hlam = p + off[3]; R.hres = p + off[4];
    return SMG_OK;
}

// Grams of the nb blocks [X W P] against themselves (weighted by M) and against [AX AW AP], queued with their download
int eig_grams(smg_hierarchy* h, EigRun& R, const EigBlocks& S, const EigBlocks& AS)
{
    const int q = S.nb * R.m;
    ProfGuard pg(h, "EIG: Gram");
    HIPCHK(launch_eig_gram(S, S, R.n, R.m, h->eig_mass.p, true, h->eig_part.p, R.groups, R.GM, R.ctrl, h->stream));
    HIPCHK(launch_eig_gram(S, AS, R.n, R.m, nullptr, false, h->eig_part.p, R.groups, R.GA, R.ctrl, h->stream));
    HIPCHK(hipMemcpyAsync(R.hGM, R.GM, (size_t)q * q * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(R.hGA, R.GA, (size_t)q * q * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    return SMG_OK;
}

// Rayleigh-Ritz on the downloaded Grams, then X, AX (and P, AP) = the recombination, and the residual of the new X
int eig_update(smg_hierarchy* h, EigRun& R, EigBlocks S, EigBlocks AS, int* nb_used)
{
    const int m = R.m;
    int nb = S.nb, rc = SMG_ERR_NONFINITE, kept = 0;
    std::vector<double> C, lam;
    std::vector<double> gm, ga;
    for (; nb >= 1; nb--) {           // a basis the Cholesky cannot orthonormalise: drop P (restart), then W
        const int q = nb * m, q0 = S.nb * m;
        gm.resize((size_t)q * q); ga.resize((size_t)q * q);
        for (int i = 0; i < q; i++)
            for (int j = 0; j < q; j++) { gm[(size_t)i * q + j] = R.hGM[(size_t)i * q0 + j]; ga[(size_t)i * q + j] = R.hGA[(size_t)i * q0 + j]; }
        rc = rayleigh_ritz(q, m, gm.data(), ga.data(), EIG_DROP, C, lam, &kept);
        if (rc == SMG_OK) break;
    }
    if (rc) return fail(SMG_ERR_NONFINITE, "smg_eigs: the Rayleigh-Ritz basis lost rank (X is no longer M-independent)");
    *nb_used = nb;
    S.nb = AS.nb = nb;
    const int q = nb * m;
    for (int i = 0; i < q; i++)
        for (int j = 0; j < m; j++) {
            R.hC[(size_t)i * 2 * m + j] = C[(size_t)i * m + j];
            R.hC[(size_t)i * 2 * m + m + j] = i < m ? 0.0 : C[(size_t)i * m + j];
        }
    for (int j = 0; j < m; j++) R.hlam[j] = lam[j];
    HIPCHK(hipMemcpyAsync(R.C, R.hC, (size_t)q * 2 * m * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(R.lam, R.hlam, (size_t)m * sizeof(double), hipMemcpyHostToDevice, h->stream));
    const int nx = 1 - R.cur;
    const bool make_p = nb >= 2;
    {
        ProfGuard pg(h, "EIG: recombination");
        HIPCHK(launch_eig_combine(S, AS, R.n, m, R.C, h->eig_x[nx].p, h->eig_ax[nx].p, make_p ? h->eig_p[nx].p : nullptr, make_p ? h->eig_ap[nx].p : nullptr,
                                  R.ctrl, h->stream));
    }
    R.cur = nx;
    R.has_p = make_p;
    Level& L0 = h->lv[0];
    ProfGuard pg(h, "EIG: residual");
    const bool f32 = h->precision == 1;
    HIPCHK(launch_eig_residual(h->eig_x[nx].p, h->eig_ax[nx].p, h->eig_mass.p, R.lam, R.n, m, f32 ? nullptr : L0.b.p, f32 ? nullptr : L0.u.p,
                               f32 ? L0.f32.b.p : nullptr, f32 ? L0.f32.u.p : nullptr, h->eig_part.p, R.groups, R.res, R.ctrl, h->stream));
    HIPCHK(hipMemcpyAsync(R.hres, R.res, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    return SMG_OK;
}

}  // namespace

extern "C" int smg_eigs(smg_hierarchy* h, const double* mass_diag, int nev, int block, const double* X0, int ld_x0, int memspace,
                        const smg_solve_opts* opts, unsigned long long seed, double* evals, double* X, int ld_x, double* res_his, int* n_iter,
                        int* n_converged)
{
    return guarded("smg_eigs", [&]() -> int {
        int rc = check_ready(h, "smg_eigs");
        if (rc) return rc;
        if (h->union_m > 0) return fail(SMG_ERR_INVALID, "smg_eigs: a union handle is not supported");
        if (h->in_solve) return fail(SMG_ERR_INVALID, "smg_eigs: a split-phase solve is in progress (smg_solve_end)");
        smg_solve_opts o;
        smg_solve_opts_default(&o);
        if (opts) o = *opts;
        if ((rc = check_cycle_opts(o))) return rc;
        if (o.max_iter < 0 || !(o.tol >= 0.0)) return fail(SMG_ERR_INVALID, "smg_eigs: max_iter must be >= 0 and tol >= 0");
        const int n_full = h->n_full, n = h->lv[0].n;
        if (nev < 1 || nev > 64) return fail(SMG_ERR_INVALID, "smg_eigs: nev must be in 1 .. 64");
        const int m = block == 0 ? std::max(nev, std::min(default_block(nev), n)) : block;
        if (m < nev || m > 64) return fail(SMG_ERR_INVALID, "smg_eigs: block must be 0 or in nev .. 64");
        if (n < m) return fail(SMG_ERR_INVALID, "smg_eigs: %d unknowns, fewer than the block of %d", n, m);
        if (!mass_diag || !evals || !X || ld_x < n_full || (X0 && ld_x0 < n_full) || (memspace != SMG_HOST && memspace != SMG_DEVICE))
            return fail(SMG_ERR_INVALID, "smg_eigs: bad mass_diag / evals / X / ld / memspace");
        DeviceScope dsc(h->device);
        // the mass of every unknown row, checked before anything of the handle changes
        std::vector<double> mh((size_t)n_full);
        if (memspace == SMG_HOST) std::memcpy(mh.data(), mass_diag, (size_t)n_full * sizeof(double));
        else HIPCHK(hipMemcpy(mh.data(), mass_diag, (size_t)n_full * sizeof(double), hipMemcpyDeviceToHost));
        const Level& L0c = h->lv[0];
        std::vector<double> mi((size_t)n);
        for (int i = 0; i < n; i++) {
            const int p = L0c.ord.perm[(size_t)i];
            const double v = mh[(size_t)(h->has_known ? h->unknown[(size_t)p] : p)];
            if (!(v > 0.0) || !std::isfinite(v)) return fail(SMG_ERR_INVALID, "smg_eigs: the mass of an unknown row is not finite and > 0");
            mi[(size_t)i] = v;
        }
        if ((rc = eig_prepare(h, o, m))) return rc;
        EigRun R{h, n, m, h->d_ctrl.p};
        if ((rc = eig_buffers(h, R))) return rc;
        Level& L0 = h->lv[0];
        HIPCHK(hipMemcpyAsync(h->eig_mass.p, mi.data(), (size_t)n * sizeof(double), hipMemcpyHostToDevice, h->stream));
        if ((rc = reset_ctrl(h, 0))) return rc;      // not done (the kernels' early return): nothing else of the control block is used here
        // the start block, gathered into the internal numbering
        const double* src = X0;
        int ld_src = ld_x0;
        std::vector<double> gen;
        if (!X0 || memspace == SMG_HOST) {
            HIPCHK(h->eig_stage.ensure((size_t)n_full * m));
            if (!X0) {
                gen.resize((size_t)n_full * m);
                for (int c = 0; c < m; c++)
                    for (int r = 0; r < n_full; r++) gen[(size_t)c * n_full + r] = start_value(seed, r, c);
                HIPCHK(hipMemcpyAsync(h->eig_stage.p, gen.data(), gen.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
            } else
                HIPCHK(hipMemcpy2DAsync(h->eig_stage.p, (size_t)n_full * 8, X0, (size_t)ld_x0 * 8, (size_t)n_full * 8, m, hipMemcpyHostToDevice, h->stream));
            src = h->eig_stage.p; ld_src = n_full;
        }
        HIPCHK(launch_gather_in(h->eig_x[0].p, src, h->d_map0.p, n, m, m, ld_src, h->stream));
        if ((rc = apply_A(h, 0, SELL_AX, h->eig_x[0].p, nullptr, h->eig_ax[0].p, m, R.ctrl))) return rc;
        // Rayleigh-Ritz of the start: history row 0 is its residual
        EigBlocks S, AS;
        S.p[0] = h->eig_x[0].p; AS.p[0] = h->eig_ax[0].p; S.nb = AS.nb = 1;
        if ((rc = eig_grams(h, R, S, AS))) return rc;
        HIPCHK(hipStreamSynchronize(h->stream));
        int nb_used = 0;
        for (int i = 0; i < 2 * m * m; i++) if (!std::isfinite(i < m * m ? R.hGM[i] : R.hGA[i - m * m])) return fail(SMG_ERR_NONFINITE, "smg_eigs: non-finite Gram entry");
        if ((rc = eig_update(h, R, S, AS, &nb_used))) return rc;
        const bool f32 = h->precision == 1;
        const size_t cnt = (size_t)n * m;
        int it = 0, conv = 0;
        for (;; it++) {
            const bool more = it < o.max_iter;
            if (more) {
                {
                    ProfGuard pg(h, "MG: total VCycle");
                    if ((rc = enqueue_vcycle(h, m, R.ctrl, FIRST_NONE))) return rc;
                }
                const double* W = L0.u.p;
                if (f32) { HIPCHK(launch_kry_widen(L0.f32.u.p, h->eig_w.p, cnt, R.ctrl, h->stream)); W = h->eig_w.p; }
                {
                    ProfGuard pg(h, "EIG: SpMV");
                    if ((rc = apply_A(h, 0, SELL_AX, W, nullptr, h->eig_aw.p, m, R.ctrl))) return rc;
                }
                S.p[0] = h->eig_x[R.cur].p; S.p[1] = W; S.p[2] = h->eig_p[R.cur].p;
                AS.p[0] = h->eig_ax[R.cur].p; AS.p[1] = h->eig_aw.p; AS.p[2] = h->eig_ap[R.cur].p;
                S.nb = AS.nb = R.has_p ? 3 : 2;
                if ((rc = eig_grams(h, R, S, AS))) return rc;
            }
            HIPCHK(hipStreamSynchronize(h->stream));
            // the residuals of the current X: history row `it`
            conv = 0;
            bool lead = true;
            for (int j = 0; j < nev; j++) {
                const double r = R.hres[j];
                if (!std::isfinite(r)) return fail(SMG_ERR_NONFINITE, "smg_eigs: non-finite residual at iteration %d", it);
                if (res_his) res_his[(size_t)it * nev + j] = r;
                if (lead && r <= o.tol) conv++; else lead = false;
            }
            if (o.verbosity > 0) std::printf("LOBPCG iteration: %d, converged: %d, largest residual: %g\n", it, conv,
                                             *std::max_element(R.hres, R.hres + nev));
            if (conv == nev || !more) break;
            const int q = S.nb * m;
            for (int i = 0; i < q * q; i++)
                if (!std::isfinite(R.hGM[i]) || !std::isfinite(R.hGA[i])) return fail(SMG_ERR_NONFINITE, "smg_eigs: non-finite Gram entry at iteration %d", it);
            if ((rc = eig_update(h, R, S, AS, &nb_used))) return rc;
        }
        if (n_iter) *n_iter = it + 1;
        if (n_converged) *n_converged = conv;
        for (int j = 0; j < nev; j++) evals[j] = R.hlam[j];
        // X(unknown) = the first nev columns, X(known) = 0
        double* dz = X;
        int ldz = ld_x;
        if (memspace == SMG_HOST) { HIPCHK(h->eig_stage.ensure((size_t)n_full * nev)); dz = h->eig_stage.p; ldz = n_full; }
        HIPCHK(hipMemset2DAsync(dz, (size_t)ldz * 8, 0, (size_t)n_full * 8, nev, h->stream));
        HIPCHK(launch_scatter_out(dz, h->eig_x[R.cur].p, h->d_map0.p, n, nev, m, ldz, h->stream));
        if (memspace == SMG_HOST)
            HIPCHK(hipMemcpy2DAsync(X, (size_t)ld_x * 8, dz, (size_t)n_full * 8, (size_t)n_full * 8, nev, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        prof_collect(h);
        return SMG_OK;
    });
}
