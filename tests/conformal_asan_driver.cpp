// conformal_asan_driver.cpp -- a stand-alone program (its own main) that runs the host side of the conformal metric on exactly-sized heap arrays,
// so that AddressSanitizer sees any read or write past an end and UndefinedBehaviorSanitizer any undefined operation: every loop of the host twin
// (smg::conformal_host_* of csrc/smg_conformal_inl.hpp, what smg_conformal_host runs after its argument checks) with the assembly plan of
// csrc/smg_mesh.cpp, on closed double pyramids of 255, 256 and 257 vertices -- the edges of a block of 256 lanes -- and of 2100 vertices, which
// takes the sums through two row chunks; and smg::unfold on an open fan.  tests/test_conformal_host.py compiles it together with
// csrc/smg_mesh.cpp and csrc/smg_sparse.cpp with -fsanitize=address,undefined and runs it directly.
#include <cmath>
#include <cstdio>
#include <memory>
#include <vector>

#include "smg_conformal_inl.hpp"
#include "smg_mesh.hpp"

using namespace smg;

// a closed double pyramid: a ring of nV - 2 vertices on a wavy ellipse, one apex above and one below.  V: xyz rows
static void make_mesh(int nV, std::vector<double>& V, std::vector<int>& F)
{
    const int ring = nV - 2, top = nV - 2, bottom = nV - 1;
    V.assign(3 * (size_t)nV, 0.0);
    for (int i = 0; i < ring; i++) {
        const double a = 6.283185307179586 * i / ring;
        V[3 * (size_t)i] = 1.3 * std::cos(a); V[3 * (size_t)i + 1] = 0.8 * std::sin(a); V[3 * (size_t)i + 2] = 0.1 * std::sin(3.0 * a);
    }
    V[3 * (size_t)top + 2] = 0.9; V[3 * (size_t)bottom + 2] = -0.7;
    F.clear();
    for (int i = 0; i < ring; i++) {
        const int j = (i + 1) % ring;
        F.insert(F.end(), {i, j, top});
        F.insert(F.end(), {j, i, bottom});
    }
}

template <class T, class Vec>
static std::unique_ptr<T[]> exact(const Vec& src)
{
    std::unique_ptr<T[]> p(new T[src.size()]);
    for (size_t i = 0; i < src.size(); i++) p[i] = src[i];
    return p;
}

static bool run_case(int nV)
{
    std::vector<double> Vv;
    std::vector<int> Fv;
    make_mesh(nV, Vv, Fv);
    const int nF = (int)Fv.size() / 3;
    const size_t n = (size_t)nV, f = (size_t)nF;
    const AssemblyPlan plan = make_assembly_plan(Fv, nV);
    const size_t nnz = plan.pattern.col.size();
    auto F = exact<int>(Fv);
    auto mp = exact<int>(plan.m_ptr);
    auto mi = exact<int>(plan.m_idx);
    auto rowptr = exact<int>(plan.pattern.ptr);
    auto lp = exact<int>(plan.l_ptr);
    auto li = exact<int>(plan.l_idx);
    auto ls = exact<signed char>(plan.l_sgn);
    std::unique_ptr<double[]> l0(new double[3 * f]), area2(new double[f]), u(new double[n]), d(new double[n]), s(new double[n]), ut(new double[n]), Theta(new double[n]);
    std::unique_ptr<int[]> mask(new int[n]);
    for (size_t g = 0; g < f; g++) {
        conformal_rest_lengths(Vv.data(), F.get(), g, l0.get() + 3 * g);
        area2[g] = conformal_rest_area2(Vv.data(), F.get(), g);
    }
    for (size_t i = 0; i < n; i++) {
        u[i] = 0.2 * std::sin(0.37 * (double)i);
        d[i] = 0.1 * std::cos(0.11 * (double)i);
        Theta[i] = 6.283185307179586;
        mask[i] = i == 0 || i + 1 == n ? 1 : 0;
    }
    u[7] = 6.0;                                                                     // breaks the faces around vertex 7
    std::unique_ptr<double[]> ang(new double[3 * f]), hc(new double[3 * f]), broken(new double[f]), lt(new double[3 * f]), sum(new double[n]), g(new double[n]),
        gsq(new double[n]), gabs(new double[n]), val(new double[nnz]);
    conformal_host_scale(nV, u.get(), d.get(), 0.5, s.get(), ut.get());
    conformal_host_faces(nF, F.get(), l0.get(), area2.get(), s.get(), ang.get(), hc.get(), broken.get(), lt.get());
    conformal_host_rows(nV, ang.get(), hc.get(), mp.get(), mi.get(), Theta.get(), mask.get(), rowptr.get(), lp.get(), li.get(), ls.get(), sum.get(), g.get(),
                        gsq.get(), gabs.get(), val.get());
    conformal_host_rows(nV, ang.get(), hc.get(), mp.get(), mi.get(), Theta.get(), mask.get(), rowptr.get(), lp.get(), li.get(), ls.get(), sum.get(), g.get(),
                        gsq.get(), gabs.get(), nullptr);
    const double sumsq = flow_host_sum(gsq.get(), nV), gmax = flow_host_max(gabs.get(), nV), nbroken = flow_host_sum(broken.get(), nF);
    bool finite = std::isfinite(sumsq) && gmax >= 0.0, angles = true, rows = true;
    for (size_t t = 0; t < f; t++) {                                                // every face's angles sum to pi, broken or not
        const double a = ang[3 * t] + ang[3 * t + 1] + ang[3 * t + 2];
        angles = angles && std::fabs(a - CONFORMAL_PI) < 1e-14 && std::isfinite(lt[3 * t]) && lt[3 * t] > 0.0;
    }
    for (int v = 0; v < nV; v++) {                                                  // the rows of -L~ sum to zero
        double r = 0.0, scale = 0.0;
        for (int e = rowptr[v]; e < rowptr[v + 1]; e++) { r += val[e]; scale += std::fabs(val[e]); }
        rows = rows && std::fabs(r) <= 1e-13 * (scale + 1.0);
    }
    finite = finite && g[0] == 0.0 && g[n - 1] == 0.0;
    const bool ok = finite && angles && rows && nbroken >= 1.0;
    std::printf("nV %d nF %d: finite %d, angles sum to pi %d, rows sum to zero %d, broken faces %g: ok %d\n", nV, nF, (int)finite, (int)angles, (int)rows, nbroken,
                (int)ok);
    return ok;
}

// an open fan of k triangles around vertex 0, laid out from its own lengths
static bool run_fan(int k)
{
    std::vector<double> V(3 * (size_t)(k + 2), 0.0);
    std::vector<int> Fv;
    for (int i = 0; i <= k; i++) {
        const double a = 4.5 * i / k, r = 1.0 + 0.1 * i;
        V[3 * (size_t)(i + 1)] = r * std::cos(a); V[3 * (size_t)(i + 1) + 1] = r * std::sin(a);
    }
    for (int i = 0; i < k; i++) Fv.insert(Fv.end(), {0, i + 1, i + 2});
    const int nV = k + 2, nF = k;
    auto F = exact<int>(Fv);
    std::unique_ptr<double[]> len(new double[3 * (size_t)nF]), X(new double[2 * (size_t)nV]), stats(new double[2]);
    for (size_t g = 0; g < (size_t)nF; g++) conformal_rest_lengths(V.data(), F.get(), g, len.get() + 3 * g);
    int where = -1;
    const int rc = unfold(F.get(), nF, nV, len.get(), X.get(), stats.get(), &where);
    len[4] = 100.0;                                                                 // and a refusal: the triangle inequality
    std::unique_ptr<double[]> X2(new double[2 * (size_t)nV]), stats2(new double[2]);
    const int rc2 = unfold(F.get(), nF, nV, len.get(), X2.get(), stats2.get(), &where);
    const bool ok = rc == UNFOLD_OK && stats[0] < 1e-13 && stats[1] == 0.0 && rc2 == UNFOLD_TRIANGLE && where == 1;
    std::printf("fan of %d faces: rc %d, mismatch %.2e, flipped %g, refusal %d at face %d: ok %d\n", k, rc, stats[0], stats[1], rc2, where, (int)ok);
    return ok;
}

int main()
{
    bool ok = true;
    for (int nV : {255, 256, 257, 2100}) ok = run_case(nV) && ok;
    ok = run_fan(9) && ok;
    return ok ? 0 : 1;
}
