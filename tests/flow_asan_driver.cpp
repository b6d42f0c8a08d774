// flow_asan_driver.cpp -- a stand-alone program (its own main) that runs the host side of the flow on exactly-sized heap arrays, so that
// AddressSanitizer sees any read or write past an end and UndefinedBehaviorSanitizer any undefined operation: every loop of the host twin
// (smg::flow_host_* of csrc/smg_flow_inl.hpp, what smg_flow_host runs after its argument checks) for every op, on closed double pyramids of 255,
// 256 and 257 vertices -- the edges of a block of 256 lanes -- and of 2100 vertices, which takes the sums through two row chunks.  The corner lists
// come from csrc/smg_mesh.cpp.  tests/test_flow_host.py compiles it together with csrc/smg_mesh.cpp and csrc/smg_sparse.cpp with
// -fsanitize=address,undefined and runs it directly.
#include <cmath>
#include <cstdio>
#include <memory>
#include <vector>

#include "smg_flow_inl.hpp"
#include "smg_mesh.hpp"

using namespace smg;

// a closed double pyramid: a ring of nV - 2 vertices on a wavy ellipse, one apex above and one below.  V: column-major nV x 3
static void make_mesh(int nV, std::vector<double>& V, std::vector<int>& F)
{
    const int ring = nV - 2, top = nV - 2, bottom = nV - 1;
    const size_t n = (size_t)nV;
    V.assign(3 * n, 0.0);
    for (int i = 0; i < ring; i++) {
        const double a = 6.283185307179586 * i / ring;
        V[i] = 1.3 * std::cos(a); V[n + i] = 0.8 * std::sin(a); V[2 * n + i] = 0.1 * std::sin(3.0 * a);
    }
    V[2 * n + top] = 0.9; V[2 * n + bottom] = -0.7;
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

static bool run_case(int nV)
{
    std::vector<double> Vv;
    std::vector<int> Fv, mpv, miv;
    make_mesh(nV, Vv, Fv);
    const int nF = (int)Fv.size() / 3;
    const size_t n = (size_t)nV, f = (size_t)nF;
    vertex_corner_lists(Fv, nV, mpv, miv);
    // a CSR with the mesh's pattern: every row holds its vertex and the vertex's neighbours, ascending
    std::vector<std::vector<int>> rows(n);
    for (int v = 0; v < nV; v++) rows[(size_t)v].push_back(v);
    for (size_t g = 0; g < f; g++)
        for (int c = 0; c < 3; c++) rows[(size_t)Fv[3 * g + c]].push_back(Fv[3 * g + (c + 1) % 3]);
    std::vector<int> rp(1, 0), cl;
    for (auto& r : rows) {
        std::sort(r.begin(), r.end());
        r.erase(std::unique(r.begin(), r.end()), r.end());
        cl.insert(cl.end(), r.begin(), r.end());
        rp.push_back((int)cl.size());
    }
    const size_t nnz = cl.size();
    std::vector<double> Lv(nnz);
    for (int v = 0; v < nV; v++)
        for (int j = rp[(size_t)v]; j < rp[(size_t)v + 1]; j++) Lv[(size_t)j] = cl[(size_t)j] == v ? -(double)(rp[(size_t)v + 1] - rp[(size_t)v] - 1) : 1.0;
    auto F = exact(Fv.data(), Fv.size());
    auto mp = exact(mpv.data(), mpv.size());
    auto mi = exact(miv.data(), miv.size());
    auto V0 = exact(Vv.data(), Vv.size());
    auto rowptr = exact(rp.data(), rp.size());
    auto col = exact(cl.data(), cl.size());
    auto L0 = exact(Lv.data(), Lv.size());
    std::unique_ptr<double[]> U(new double[3 * n]);
    for (size_t i = 0; i < 3 * n; i++) U[i] = 1.5 * V0[i] + 0.25;
    std::unique_ptr<double[]> mass(new double[n]), B(new double[3 * n]), val(new double[nnz]), Un(new double[3 * n]), s(new double[7]), S(new double[3 * n]),
        sigma(new double[2 * f]), terms(new double[4 * f]), stats(new double[4]);
    flow_host_system(nV, F.get(), mp.get(), mi.get(), U.get(), rowptr.get(), col.get(), L0.get(), 0.01, mass.get(), B.get(), val.get());
    flow_host_normalize(nV, nF, F.get(), U.get(), Un.get());
    flow_host_sphericity(nV, F.get(), mp.get(), mi.get(), U.get(), s.get());
    flow_host_sphere(nV, nF, F.get(), mp.get(), mi.get(), U.get(), V0.get(), S.get(), sigma.get(), terms.get(), stats.get());
    bool finite = true, unit = true, area = true, ordered = true;
    double msum = 0.0, a2 = 0.0;
    for (size_t i = 0; i < n; i++) { finite = finite && mass[i] > 0.0; msum += mass[i]; }
    for (size_t i = 0; i < 3 * n; i++) finite = finite && std::isfinite(B[i]) && std::isfinite(Un[i]) && std::isfinite(S[i]);
    for (size_t i = 0; i < nnz; i++) finite = finite && std::isfinite(val[i]);
    for (size_t g = 0; g < f; g++) a2 += flow_face_darea(Un.get(), n, F.get(), g);
    area = std::fabs(0.5 * a2 - 1.0) < 1e-12 && std::fabs(msum - s[1]) < 1e-12 * msum;          // unit area after normalising; the masses sum to sum a
    for (size_t i = 0; i < n; i++) unit = unit && std::fabs(S[i] * S[i] + S[n + i] * S[n + i] + S[2 * n + i] * S[2 * n + i] - 1.0) < 1e-14;
    for (size_t g = 0; g < f; g++) ordered = ordered && sigma[g] >= sigma[f + g] && sigma[f + g] > 0.0;
    finite = finite && std::isfinite(s[0]) && s[0] > 0.0 && stats[0] >= 1.0 && stats[1] >= stats[0] && stats[3] == s[0];
    const bool ok = finite && unit && area && ordered;
    std::printf("nV %d nF %d: finite %d, |S| = 1 %d, unit area %d, sigma1 >= sigma2 > 0 %d, flipped %g: ok %d\n", nV, nF, (int)finite, (int)unit, (int)area,
                (int)ordered, stats[2], (int)ok);
    return ok;
}

int main()
{
    bool ok = true;
    for (int nV : {255, 256, 257, 2100}) ok = run_case(nV) && ok;
    return ok ? 0 : 1;
}
