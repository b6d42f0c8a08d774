// sinkhorn_asan_driver.cpp -- a stand-alone program (its own main) that runs the host side of heat-kernel optimal transport on exactly-sized heap
// arrays, so that AddressSanitizer sees any read or write past an end and UndefinedBehaviorSanitizer any undefined operation: every loop of the
// host twin (smg::sinkhorn_host_* of csrc/smg_sinkhorn_inl.hpp, what smg_sinkhorn_host runs after its argument checks), on closed double pyramids
// of 255, 256 and 257 vertices -- the edges of a block of 256 lanes -- and of 2100 vertices, with k = 1 and 3 columns and a geomean of G = 2
// groups of k_in = 3 columns.  The corner lists come from csrc/smg_mesh.cpp.  tests/test_sinkhorn_host.py compiles it together with
// csrc/smg_mesh.cpp and csrc/smg_sparse.cpp with -fsanitize=address,undefined and runs it directly.
#include <cmath>
#include <cstdio>
#include <memory>
#include <vector>

#include "smg_mesh.hpp"
#include "smg_sinkhorn_inl.hpp"

using namespace smg;

// a closed double pyramid: a ring of nV - 2 vertices on a wavy ellipse, one apex above and one below.  V: xyz rows
static void make_mesh(int nV, std::vector<double>& V, std::vector<int>& F)
{
    const int ring = nV - 2, top = ring, bottom = ring + 1;
    V.assign(3 * (size_t)nV, 0.0);
    for (int i = 0; i < ring; i++) {
        const double a = 6.283185307179586 * i / ring;
        V[3 * (size_t)i] = 1.3 * std::cos(a); V[3 * (size_t)i + 1] = 0.8 * std::sin(a); V[3 * (size_t)i + 2] = 0.1 * std::sin(3.0 * a);
    }
    V[3 * (size_t)top + 2] = 0.9;
    V[3 * (size_t)bottom + 2] = -0.7;
    F.clear();
    for (int i = 0; i < ring; i++) {
        const int j = (i + 1) % ring;
        F.insert(F.end(), {i, j, top});
        F.insert(F.end(), {j, i, bottom});
    }
}

template <class T>
static std::unique_ptr<T[]> exact(const T* src, size_t n)
{
    std::unique_ptr<T[]> p(new T[n]);
    for (size_t i = 0; i < n; i++) p[i] = src[i];
    return p;
}

static std::unique_ptr<double[]> block(size_t n) { return std::unique_ptr<double[]>(new double[n]); }

static bool run_case(int nV, int k)
{
    const int G = 2, k_in = 3, K = G * k_in;
    std::vector<double> Vv;
    std::vector<int> Fv, mpv, miv;
    make_mesh(nV, Vv, Fv);
    const int nF = (int)Fv.size() / 3;
    const size_t n = (size_t)nV, f = (size_t)nF, nk = n * (size_t)k, nK = n * (size_t)K, nG = n * (size_t)G;
    vertex_corner_lists(Fv, nV, mpv, miv);
    auto F = exact(Fv.data(), Fv.size());
    auto mp = exact(mpv.data(), mpv.size());
    auto mi = exact(miv.data(), miv.size());
    auto V = exact(Vv.data(), Vv.size());
    auto Af = block(f), m = block(n);
    fluid_host_mass(nV, nF, F.get(), V.get(), mp.get(), mi.get(), Af.get(), m.get());
    const double A = flow_host_sum(m.get(), nV), floor = 1e-10;

    // distance side: y with a zero and a negative entry, masses with zeros
    auto y = block(nk), r = block(nk), mu0 = block(nk), mu1 = block(nk), sr = block((size_t)k), rn = block(nk), err = block(nk), rsq = block(nk), rs = block(nk),
         terms = block(nk), lv = block(nk), lw = block(nk);
    for (int c = 0; c < k; c++) {
        for (size_t i = 0; i < n; i++) {
            const size_t e = (size_t)c * n + i;
            y[e] = std::exp(-6.0 + 5.0 * std::sin(0.3 * (double)i + c));
            r[e] = m[i] * (1.0 + 0.5 * std::cos(0.7 * (double)i + c));
            mu0[e] = i % 5 == 1 ? 0.0 : m[i] * (2.0 + std::sin(0.11 * (double)i + c));
            mu1[e] = i % 7 == 2 ? 0.0 : m[i] * (2.0 + std::cos(0.13 * (double)i - c));
        }
        y[(size_t)c * n + 3] = 0.0;
        y[(size_t)c * n + 9] = -1e-12;
        sr[(size_t)c] = flow_host_sum(r.get() + (size_t)c * n, nV);
    }
    sinkhorn_host_scale(nV, k, k, y.get(), r.get(), mu0.get(), sr.get(), floor, A, rn.get(), err.get(), rsq.get());
    sinkhorn_host_substep(nV, k, m.get(), y.get(), rs.get(), rsq.get());
    sinkhorn_host_scale(nV, k, 1, y.get(), r.get(), mu1.get(), sr.get(), floor, A, rs.get(), err.get(), rsq.get());   // one column of masses for all
    sinkhorn_host_scale(nV, k, k, y.get(), r.get(), mu1.get(), sr.get(), floor, A, rs.get(), err.get(), rsq.get());
    sinkhorn_host_value(nV, k, m.get(), mu0.get(), mu1.get(), rn.get(), rs.get(), terms.get(), lv.get(), lw.get());
    bool scaled = true, logs = true;
    for (size_t e = 0; e < nk; e++) {
        const double ye = sinkhorn_effective(y[e], sr[e / n], floor, A);
        scaled = scaled && ye > 0.0 && (mu0[e] == 0.0 ? rn[e] == 0.0 : std::fabs(rn[e] * ye - mu0[e]) <= 4e-16 * mu0[e]) && rsq[e] == rs[e] * rs[e];
        logs = logs && std::isfinite(terms[e]) && (mu0[e] == 0.0) == (std::isinf(lv[e]) && lv[e] < 0.0) && (mu1[e] == 0.0) == (std::isinf(lw[e]) && lw[e] < 0.0);
    }

    // barycentre side: G groups of k_in columns, a zero alpha in group 0
    auto z = block(nK), rv = block(nK), prev = block(nG), srK = block((size_t)K), al = block((size_t)K), rvn = block(nK), bary = block(nG), chg = block(nG),
         rsqK = block(nK);
    for (int c = 0; c < K; c++) {
        for (size_t i = 0; i < n; i++) {
            z[(size_t)c * n + i] = std::exp(-4.0 + 3.0 * std::cos(0.2 * (double)i + c));
            rv[(size_t)c * n + i] = m[i] * (1.0 + 0.25 * std::sin(0.5 * (double)i - c));
        }
        srK[(size_t)c] = flow_host_sum(rv.get() + (size_t)c * n, nV);
        al[(size_t)c] = (1.0 + c % k_in) / 6.0;
    }
    al[0] = 0.0; al[1] = 0.4; al[2] = 0.6;
    for (size_t e = 0; e < nG; e++) prev[e] = 0.0;
    sinkhorn_host_geomean(nV, G, k_in, m.get(), z.get(), rv.get(), prev.get(), srK.get(), al.get(), floor, A, rvn.get(), bary.get(), chg.get(), rsqK.get());
    bool means = true;
    for (size_t e = 0; e < nG; e++) means = means && bary[e] > 0.0 && std::isfinite(bary[e]) && chg[e] == bary[e];
    for (size_t e = 0; e < nK; e++) means = means && std::isfinite(rvn[e]) && rsqK[e] == rvn[e] * rvn[e];
    const bool ok = scaled && logs && means;
    std::printf("nV %d nF %d k %d: the scalings %d, the logarithms %d, the means %d: ok %d\n", nV, nF, k, (int)scaled, (int)logs, (int)means, (int)ok);
    return ok;
}

int main()
{
    bool ok = true;
    for (int nV : {255, 256, 257, 2100})
        for (int k : {1, 3}) ok = run_case(nV, k) && ok;
    return ok ? 0 : 1;
}
