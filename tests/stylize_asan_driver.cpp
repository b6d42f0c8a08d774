// stylize_asan_driver.cpp -- a stand-alone program (its own main) that runs the host side of the stylizer's local step on exactly-sized heap
// arrays, so that AddressSanitizer sees any read or write past an end and UndefinedBehaviorSanitizer any undefined operation: every op of the host
// twin (smg::sty_local_host of csrc/smg_stylize_inl.hpp, what smg_stylize_local_host runs after its argument checks) on flat open strips of 255,
// 256 and 257 vertices -- the edges of a block of 256 lanes, rank-2 covariances -- and on a tetrahedron.  The cotangent matrix and the corner
// lists come from csrc/smg_mesh.cpp.  tests/test_stylize_host.py compiles it together with csrc/smg_mesh.cpp and csrc/smg_sparse.cpp with
// -fsanitize=address,undefined and runs it directly.
#include <cmath>
#include <cstdio>
#include <memory>
#include <vector>

#include "smg_mesh.hpp"
#include "smg_stylize_inl.hpp"

using namespace smg;

// an open strip of nV vertices between two rows, in the plane z = 0 (tests/denoise_np.py: strip, flattened), or the tetrahedron (nV == 4)
static Mesh make_mesh(int nV)
{
    Mesh m;
    if (nV == 4) {
        m.V = {0.0, 0.0, 0.0, 1.0, 0.1, 0.0, 0.2, 0.9, 0.1, 0.3, 0.2, 0.8};
        m.F = {0, 2, 1, 0, 1, 3, 1, 2, 3, 2, 0, 3};
        return m;
    }
    const int nF = nV - 2, rows = nF / 2 + 2;
    std::vector<double> V(6 * (size_t)rows);
    for (int i = 0; i < rows; i++) {
        const double x = (double)i;
        V[3 * i] = x; V[3 * i + 1] = 0.1 * std::sin(x); V[3 * i + 2] = 0.0;
        V[3 * (rows + i)] = x + 0.4; V[3 * (rows + i) + 1] = 1.0 + 0.1 * std::cos(x); V[3 * (rows + i) + 2] = 0.0;
    }
    std::vector<int> F;
    for (int i = 0; i < rows - 1 && (int)F.size() < 3 * nF; i++) {
        F.insert(F.end(), {i, i + 1, rows + i});
        if ((int)F.size() < 3 * nF) F.insert(F.end(), {i + 1, rows + i + 1, rows + i});
    }
    std::vector<int> id(2 * (size_t)rows, -1);
    for (int v : F) id[v] = 0;
    int used = 0;
    for (int v = 0; v < 2 * rows; v++)
        if (id[v] == 0) {
            id[v] = used++;
            m.V.insert(m.V.end(), {V[3 * v], V[3 * v + 1], V[3 * v + 2]});
        }
    for (int v : F) m.F.push_back(id[v]);
    return m;
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
    const Mesh m = make_mesh(nV);
    if (m.nV() != nV) return false;
    const int nF = m.nF();
    const size_t n = (size_t)nV;
    const Csr L = cotmatrix(m);
    std::vector<int> mpv, miv;
    vertex_corner_lists(m.F, nV, mpv, miv);
    // exactly-sized copies of everything the twin reads
    auto F = exact(m.F.data(), m.F.size());
    auto mp = exact(mpv.data(), mpv.size());
    auto mi = exact(miv.data(), miv.size());
    auto ptr = exact(L.ptr.data(), L.ptr.size());
    auto col = exact(L.col.data(), L.col.size());
    auto w = exact(L.val.data(), L.val.size());
    auto V0 = exact(m.V.data(), m.V.size());
    std::unique_ptr<double[]> P(new double[3 * n]), lam(new double[n]), tgt(new double[3 * n]);
    for (size_t i = 0; i < 3 * n; i++) P[i] = V0[i] + 0.05 * std::sin(1.0 + (double)i);
    for (size_t i = 0; i < n; i++) { lam[i] = 0.3 * (double)(i % 3); tgt[3 * i] = 0.0; tgt[3 * i + 1] = 0.6; tgt[3 * i + 2] = 0.8; }
    const StyParams p = {0.2, 1e-4, 1e-5, 1e-3, 10.0, 2.0, 100};
    const StyFrame I = {{1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0}}, Q = {{0.0, 1.0, 0.0, -1.0, 0.0, 0.0, 0.0, 0.0, 1.0}};
    std::unique_ptr<double[]> na(new double[4 * n]), one(new double[17 * n]), full(new double[17 * n]), again(new double[17 * n]), tg(new double[10 * n]),
        en(new double[n]);
    std::unique_ptr<int[]> it1(new int[n]), it2(new int[n]), it3(new int[n]);
    const int *f = F.get(), *a = mp.get(), *b = mi.get(), *rp = ptr.get(), *cl = col.get();
    sty_local_host(0, nV, f, a, b, rp, cl, w.get(), V0.get(), nullptr, nullptr, I, nullptr, nullptr, nullptr, p, na.get(), nullptr);
    sty_local_host(1, nV, f, a, b, rp, cl, w.get(), V0.get(), P.get(), nullptr, I, nullptr, nullptr, nullptr, p, one.get(), it1.get());
    sty_local_host(2, nV, f, a, b, rp, cl, w.get(), V0.get(), P.get(), lam.get(), Q, nullptr, one.get() + 10 * n, nullptr, p, full.get(), it2.get());
    sty_local_host(2, nV, f, a, b, rp, cl, w.get(), V0.get(), P.get(), nullptr, I, nullptr, nullptr, nullptr, p, again.get(), it3.get());
    sty_local_host(3, nV, f, a, b, rp, cl, w.get(), V0.get(), P.get(), nullptr, I, tgt.get(), nullptr, nullptr, p, tg.get(), it1.get());
    sty_local_host(4, nV, f, a, b, rp, cl, w.get(), V0.get(), P.get(), nullptr, I, nullptr, nullptr, again.get(), p, en.get(), nullptr);
    bool finite = true, unit = true, counted = true, same = true;
    double area = 0.0;
    for (size_t i = 0; i < n; i++) {
        const double len = std::sqrt(na[3 * i] * na[3 * i] + na[3 * i + 1] * na[3 * i + 1] + na[3 * i + 2] * na[3 * i + 2]);
        unit = unit && std::fabs(len - 1.0) < 1e-15;
        area += na[3 * n + i];
        counted = counted && it2[i] >= 1 && it2[i] <= 100 && it3[i] >= 1 && it3[i] <= 100 && it1[i] == 0;
        same = same && en[i] == again[9 * n + i];            // the energy op on the step's own rotations returns the step's terms
    }
    for (size_t i = 0; i < 17 * n; i++) finite = finite && std::isfinite(full[i]) && std::isfinite(again[i]) && std::isfinite(one[i]);
    for (size_t i = 0; i < 10 * n; i++) finite = finite && std::isfinite(tg[i]);
    const bool ok = finite && unit && counted && same && area > 0.0;
    std::printf("nV %d nF %d: area %.6f, finite %d, unit %d, counted %d, same %d: ok %d\n", nV, nF, area, (int)finite, (int)unit, (int)counted, (int)same, (int)ok);
    return ok;
}

int main()
{
    bool ok = true;
    for (int nV : {255, 256, 257, 4}) ok = run_case(nV) && ok;
    return ok ? 0 : 1;
}
