// hodge_asan_driver.cpp -- a stand-alone program (its own main) that runs the host side of the Hodge decomposition on exactly-sized heap arrays,
// so that AddressSanitizer sees any read or write past an end and UndefinedBehaviorSanitizer any undefined operation: every loop of the host twin
// (smg::hodge_host_* of csrc/smg_hodge_inl.hpp, what smg_hodge_host runs after its argument checks) for all three ops, on closed double pyramids
// of 255, 256 and 257 vertices -- the edges of a block of 256 lanes -- and of 2100 vertices, whose apex corner lists are the long ones, and on one
// open fan.  The corner lists come from csrc/smg_mesh.cpp.  tests/test_hodge_host.py compiles it together with csrc/smg_mesh.cpp and
// csrc/smg_sparse.cpp with -fsanitize=address,undefined and runs it directly.
#include <cmath>
#include <cstdio>
#include <memory>
#include <vector>

#include "smg_hodge_inl.hpp"
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
    std::unique_ptr<double[]> u(new double[nk]), v(new double[nk]), X(new double[3 * fk]), b(new double[nk]), c(new double[nk]), bsq(new double[2 * nk]),
        parts(new double[9 * fk]), terms(new double[4 * fk]), energy(new double[4 * (size_t)k]), X2(new double[3 * fk]), parts2(new double[9 * fk]),
        terms2(new double[4 * fk]), energy2(new double[4 * (size_t)k]);
    for (int s = 0; s < k; s++)
        for (size_t i = 0; i < n; i++) {
            u[(size_t)s * n + i] = std::sin((3.0 + s) * V[3 * i]) + V[3 * i + 1] * V[3 * i + 2];
            v[(size_t)s * n + i] = std::cos((2.0 + s) * V[3 * i + 1]) - 0.5 * V[3 * i];
        }
    // X = grad u + J grad v; its right-hand sides; its parts with the potentials it came from: H must vanish to rounding
    hodge_host_field(nV, nF, k, F.get(), V.get(), u.get(), v.get(), X.get());
    hodge_host_rhs(nV, nF, k, F.get(), V.get(), mp.get(), mi.get(), X.get(), b.get(), c.get(), bsq.get());
    hodge_host_parts(nV, nF, k, F.get(), V.get(), X.get(), u.get(), v.get(), parts.get(), terms.get(), energy.get());
    // and a field that is not tangent, with zero potentials: G = R = 0, H = Xt
    for (size_t i = 0; i < 3 * fk; i++) X2[i] = 0.25 + 0.001 * (double)(i % 97);
    for (size_t i = 0; i < nk; i++) u[i] = v[i] = 0.0;
    hodge_host_parts(nV, nF, k, F.get(), V.get(), X2.get(), u.get(), v.get(), parts2.get(), terms2.get(), energy2.get());
    bool finite = true, sums = true, nothing_left = true, zero_parts = true;
    for (size_t i = 0; i < nk; i++) finite = finite && std::isfinite(b[i]) && std::isfinite(c[i]) && bsq[i] == b[i] * b[i] && bsq[nk + i] == c[i] * c[i];
    for (size_t i = 0; i < 3 * fk; i++) finite = finite && std::isfinite(X[i]);
    for (int s = 0; s < k; s++) {
        double sb = 0.0, sc = 0.0, scale = 0.0;
        for (size_t i = 0; i < n; i++) { sb += b[(size_t)s * n + i]; sc += c[(size_t)s * n + i]; scale += std::fabs(b[(size_t)s * n + i]) + std::fabs(c[(size_t)s * n + i]); }
        if (!open) sums = sums && std::fabs(sb) <= 1e-12 * scale && std::fabs(sc) <= 1e-12 * scale;       // both right-hand sides sum to zero on a closed mesh
        nothing_left = nothing_left && energy[4 * s + 3] <= 1e-24 * energy[4 * s] && energy[4 * s] > 0.0;
        zero_parts = zero_parts && energy2[4 * s + 1] == 0.0 && energy2[4 * s + 2] == 0.0 && energy2[4 * s + 3] == energy2[4 * s];
    }
    const bool ok = finite && sums && nothing_left && zero_parts;
    std::printf("nV %d nF %d k %d %s: finite %d, sums to zero %d, H of grad u + J grad v vanishes %d, zero potentials leave H = Xt %d: ok %d\n", nV, nF, k,
                open ? "open" : "closed", (int)finite, (int)sums, (int)nothing_left, (int)zero_parts, (int)ok);
    return ok;
}

int main()
{
    bool ok = true;
    for (int nV : {255, 256, 257, 2100}) ok = run_case(nV, false, nV == 2100 ? 1 : 3) && ok;
    ok = run_case(258, true, 2) && ok;
    return ok ? 0 : 1;
}
