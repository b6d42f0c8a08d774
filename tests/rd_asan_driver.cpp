// rd_asan_driver.cpp -- a stand-alone program (its own main) that runs the host side of reaction-diffusion on a surface on exactly-sized heap
// arrays, so that AddressSanitizer sees any read or write past an end and UndefinedBehaviorSanitizer any undefined operation: every loop of the
// host twin (smg::rd_host_react and rd_host_close of csrc/smg_rd_inl.hpp with the masses of fluid_host_mass, what smg_rd_host runs after its
// argument checks), on closed double pyramids of 63, 64, 65 and 257 vertices -- the edges of a wavefront of 64 lanes and of a block of 256 -- and
// on one open fan, k = 3, with one and with three sub-steps.  The corner lists come from csrc/smg_mesh.cpp.  tests/test_rd_host.py compiles it
// together with csrc/smg_mesh.cpp and csrc/smg_sparse.cpp with -fsanitize=address,undefined and runs it directly.
#include <cmath>
#include <cstdio>
#include <memory>
#include <vector>

#include "smg_mesh.hpp"
#include "smg_rd_inl.hpp"

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
    const size_t n = (size_t)nV, f = (size_t)nF, kk = (size_t)k, nk = n * kk;
    vertex_corner_lists(Fv, nV, mpv, miv);
    auto F = exact(Fv.data(), Fv.size());
    auto mp = exact(mpv.data(), mpv.size());
    auto mi = exact(miv.data(), miv.size());
    auto V = exact(Vv.data(), Vv.size());
    std::unique_ptr<double[]> A(new double[f]), m(new double[n]), S0(new double[2 * nk]), S1(new double[2 * nk]), coef(new double[kk * RD_COEFFS]),
        R(new double[2 * nk]), rsq(new double[2 * nk]), vs(new double[nk]), R3(new double[2 * nk]), rsq3(new double[2 * nk]), vs3(new double[nk]),
        mt(new double[2 * nk]), chg(new double[nk]);
    for (int s = 0; s < k; s++) {
        for (size_t i = 0; i < n; i++) {
            S0[(size_t)s * n + i] = 1.0 - 0.5 * std::cos((2.0 + s) * V[3 * i + 1]);
            S0[nk + (size_t)s * n + i] = 0.25 + 0.2 * std::sin((3.0 + s) * V[3 * i]);
        }
        double* c = coef.get() + (size_t)s * RD_COEFFS;                       // Gray-Scott, feed 0.03 + 0.01 s, kill 0.06
        for (int j = 0; j < RD_COEFFS; j++) c[j] = 0.0;
        const double feed = 0.03 + 0.01 * s, kill = 0.06;
        c[0] = feed; c[1] = -feed; c[8] = -1.0; c[10 + 8] = 1.0; c[10 + 2] = -(feed + kill);
    }
    fluid_host_mass(nV, nF, F.get(), V.get(), mp.get(), mi.get(), A.get(), m.get());
    rd_host_react(nV, k, m.get(), S0.get(), coef.get(), 0.5, 1, R.get(), rsq.get(), vs.get());
    rd_host_react(nV, k, m.get(), S0.get(), coef.get(), 0.5 / 3, 3, R3.get(), rsq3.get(), vs3.get());
    for (size_t e = 0; e < 2 * nk; e++) S1[e] = R[e] / m[e % n];              // the step without diffusion: (u*, v*)
    rd_host_close(nV, k, m.get(), S0.get(), S1.get(), mt.get(), chg.get());
    bool finite = true, squares = true, star = true, subs = true, closing = true;
    for (size_t e = 0; e < 2 * nk; e++) {
        finite = finite && std::isfinite(R[e]) && std::isfinite(R3[e]) && std::isfinite(mt[e]);
        squares = squares && rsq[e] == R[e] * R[e] && rsq3[e] == R3[e] * R3[e];
    }
    for (size_t e = 0; e < nk; e++) {
        star = star && R[nk + e] == m[e % n] * vs[e] && R3[nk + e] == m[e % n] * vs3[e];
        // one Euler step and three sub-steps of a third agree to second order in the step: |difference| <= dt^2 |R| |R'| / 2 ~ 0.5^2 * 1 * 4 / 2
        subs = subs && std::fabs(vs3[e] - vs[e]) <= 0.5 && vs3[e] != vs[e];
        const double du = std::fabs(S1[e] - S0[e]), dv = std::fabs(S1[nk + e] - S0[nk + e]);
        closing = closing && chg[e] == std::fmax(du, dv) && chg[e] > 0.0 && std::fabs(mt[e] - R[e]) <= 4e-16 * std::fabs(R[e]);
    }
    const double ss = flow_host_sum(rsq.get(), (int)nk), mx = flow_host_max(chg.get(), nV);
    finite = finite && std::isfinite(ss) && ss > 0.0 && mx > 0.0;
    const bool ok = finite && squares && star && subs && closing;
    std::printf("nV %d nF %d k %d %s: finite %d, squares %d, v* %d, sub-steps %d, closing %d: ok %d\n", nV, nF, k, open ? "open" : "closed", (int)finite,
                (int)squares, (int)star, (int)subs, (int)closing, (int)ok);
    return ok;
}

int main()
{
    bool ok = true;
    for (int nV : {63, 64, 65, 257}) ok = run_case(nV, false, 3) && ok;
    ok = run_case(66, true, 3) && ok;
    return ok ? 0 : 1;
}
