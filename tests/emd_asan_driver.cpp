// emd_asan_driver.cpp -- a stand-alone program (its own main) that runs the host side of the earth mover's distance on exactly-sized heap arrays,
// so that AddressSanitizer sees any read or write past an end and UndefinedBehaviorSanitizer any undefined operation: every loop of the host twin
// (smg::emd_host_* of csrc/smg_emd_inl.hpp, what smg_emd_host runs after its argument checks), on closed double pyramids of 255, 256 and 257
// vertices -- the edges of a block of 256 lanes -- and of 2100 vertices, whose apex corner lists are the long ones, and on one open fan, k = 1 and
// 3.  The corner lists come from csrc/smg_mesh.cpp.  tests/test_emd_host.py compiles it together with csrc/smg_mesh.cpp and csrc/smg_sparse.cpp
// with -fsanitize=address,undefined and runs it directly.
#include <cmath>
#include <cstdio>
#include <memory>
#include <vector>

#include "smg_emd_inl.hpp"
#include "smg_mesh.hpp"

using namespace smg;

// a closed double pyramid: a ring of nV - 2 vertices on a wavy ellipse, one apex above and one below; open: the upper fan alone, nV - 1 vertices.
// V: xyz rows
static void make_mesh(int nV, bool open, std::vector<double>& V, std::vector<int>& F)
{
    const int ring = open ? nV - 1 : nV - 2, top = ring, bottom = ring + 1;
    V.assign(3 * (size_t)nV, 0.0);
    for (int i = 0; i < ring; i++) {
        const double a = 6.283185307179586 * i / ring;
        V[3 * (size_t)i] = 1.3 * std::cos(a); V[3 * (size_t)i + 1] = 0.8 * std::sin(a); V[3 * (size_t)i + 2] = 0.1 * std::sin(3.0 * a);
    }
    V[3 * (size_t)top + 2] = 0.9;
    if (!open) V[3 * (size_t)bottom + 2] = -0.7;
    F.clear();
    for (int i = 0; i < ring; i++) {
        const int j = (i + 1) % ring;
        F.insert(F.end(), {i, j, top});
        if (!open) F.insert(F.end(), {j, i, bottom});
    }
}

template <class T>
static std::unique_ptr<T[]> exact(const T* src, size_t n)
{
    std::unique_ptr<T[]> p(new T[n]);
    for (size_t i = 0; i < n; i++) p[i] = src[i];
    return p;
}

static bool run_case(int nV, bool open, int k)
{
    std::vector<double> Vv;
    std::vector<int> Fv, mpv, miv;
    make_mesh(nV, open, Vv, Fv);
    const int nF = (int)Fv.size() / 3;
    const size_t n = (size_t)nV, f = (size_t)nF, nk = n * (size_t)k, fk = f * (size_t)k;
    vertex_corner_lists(Fv, nV, mpv, miv);
    auto F = exact(Fv.data(), Fv.size());
    auto mp = exact(mpv.data(), mpv.size());
    auto mi = exact(miv.data(), miv.size());
    auto V = exact(Vv.data(), Vv.size());
    std::unique_ptr<double[]> W2(new double[6 * f]), A(new double[f]), b(new double[nk]), phi(new double[nk]), ZU0(new double[4 * fk]), ZU(new double[4 * fk]),
        J(new double[2 * fk]), up(new double[fk]), gq(new double[fk]), r(new double[nk]), d(new double[nk]), dsq(new double[nk]), pot(new double[nk]),
        terms(new double[nk]), J3(new double[3 * fk]), rho(new double[(size_t)k]), gmax2(new double[(size_t)k]);
    for (int s = 0; s < k; s++) {
        for (size_t i = 0; i < n; i++) {
            b[(size_t)s * n + i] = 0.0;
            phi[(size_t)s * n + i] = std::sin((3.0 + s) * V[3 * i]) + V[3 * i + 1] * V[3 * i + 2];
        }
        b[(size_t)s * n + 1] = -1.0; b[(size_t)s * n + n / 2] = 1.0;
        rho[(size_t)s] = 0.5 + s;
        for (size_t i = 0; i < 4 * f; i++) ZU0[(size_t)s * 4 * f + i] = i % 28 < 4 ? 0.0 : 0.25 * std::cos(0.37 * (double)i + s);
    }
    emd_host_geometry(nF, F.get(), V.get(), W2.get(), A.get());
    emd_host_divergence(nV, nF, k, W2.get(), A.get(), mp.get(), mi.get(), b.get(), ZU0.get(), 4, r.get(), nullptr);
    emd_host_update(nV, nF, k, F.get(), W2.get(), A.get(), phi.get(), ZU0.get(), rho.get(), 1.7, ZU.get(), J.get(), up.get(), gq.get());
    for (int s = 0; s < k; s++) gmax2[(size_t)s] = flow_host_max(gq.get() + (size_t)s * f, nF);
    emd_host_dual(nV, k, b.get(), phi.get(), rho.get(), gmax2.get(), pot.get(), terms.get());
    emd_host_flow(nF, k, F.get(), V.get(), J.get(), J3.get());
    emd_host_divergence(nV, nF, k, W2.get(), A.get(), mp.get(), mi.get(), b.get(), J.get(), 2, d.get(), dsq.get());
    bool finite = true, sums = true, split = true, lengths = true, squares = true;
    for (size_t i = 0; i < nk; i++) finite = finite && std::isfinite(r[i]) && std::isfinite(d[i]) && std::isfinite(pot[i]) && terms[i] == b[i] * pot[i];
    for (int s = 0; s < k; s++) {
        // the hat functions' gradients sum to zero on every face, and so does b: the rows of a weak divergence sum to zero
        double sr = 0.0, sd = 0.0, scale = 0.0;
        for (size_t i = 0; i < n; i++) { sr += r[(size_t)s * n + i]; sd += d[(size_t)s * n + i]; scale += std::fabs(r[(size_t)s * n + i]) + std::fabs(d[(size_t)s * n + i]); }
        sums = sums && std::fabs(sr) <= 1e-12 * scale && std::fabs(sd) <= 1e-12 * scale;
        squares = squares && dsq[(size_t)s * n] == 0.0 && dsq[(size_t)s * n + 2] == d[(size_t)s * n + 2] * d[(size_t)s * n + 2] && gmax2[(size_t)s] > 0.0;
        for (size_t q = 0; q < f; q++) {
            const double* z = ZU.get() + ((size_t)s * f + q) * 4;
            const double* j = J.get() + ((size_t)s * f + q) * 2;
            const double* j3 = J3.get() + ((size_t)s * f + q) * 3;
            const double nz = std::sqrt(z[0] * z[0] + z[1] * z[1]), nt = std::sqrt((z[0] + z[2]) * (z[0] + z[2]) + (z[1] + z[3]) * (z[1] + z[3]));
            const double nj = std::sqrt(j[0] * j[0] + j[1] * j[1]), nj3 = std::sqrt(j3[0] * j3[0] + j3[1] * j3[1] + j3[2] * j3[2]);
            // Z is T shrunk by 1 / rho or zero; the frame is orthonormal: |J| is the same in 3-D
            split = split && std::isfinite(nz) && (nz == 0.0 || std::fabs(nz - (nt - 1.0 / rho[(size_t)s])) <= 1e-12 * (1.0 + nt));
            lengths = lengths && std::fabs(nj3 - nj) <= 1e-12 * (1.0 + nj) && up[(size_t)s * f + q] == A[q] * nj;
        }
    }
    const bool ok = finite && sums && split && lengths && squares;
    std::printf("nV %d nF %d k %d %s: finite %d, rows sum to zero %d, the shrink %d, |J| in 3-D %d, squares %d: ok %d\n", nV, nF, k, open ? "open" : "closed",
                (int)finite, (int)sums, (int)split, (int)lengths, (int)squares, (int)ok);
    return ok;
}

int main()
{
    bool ok = true;
    for (int nV : {255, 256, 257})
        for (int k : {1, 3}) ok = run_case(nV, false, k) && ok;
    ok = run_case(2100, false, 1) && ok;
    for (int k : {1, 3}) ok = run_case(258, true, k) && ok;
    return ok ? 0 : 1;
}
