// morph_asan_driver.cpp -- a stand-alone program (its own main) that runs the host side of the morpher on exactly-sized heap arrays, so that
// AddressSanitizer sees any read or write past an end and UndefinedBehaviorSanitizer any undefined operation: every loop of the host twin
// (smg::morph_host_* of csrc/smg_morph_inl.hpp, what smg_morph_faces_host runs after its argument checks) on open strips of 255, 256 and 257
// vertices -- the edges of a block of 256 lanes -- and on a tetrahedron, with k = 1, 2 and 5 sets.  The corner lists come from csrc/smg_mesh.cpp.
// tests/test_morph_host.py compiles it together with csrc/smg_mesh.cpp and csrc/smg_sparse.cpp with -fsanitize=address,undefined and runs it
// directly.
#include <cmath>
#include <cstdio>
#include <memory>
#include <vector>

#include "smg_mesh.hpp"
#include "smg_morph_inl.hpp"

using namespace smg;

// an open, gently curved strip of nV vertices between two rows, or the tetrahedron (nV == 4)
static Mesh make_mesh(int nV)
{
    Mesh m;
    if (nV == 4) {
        m.V = {0.0, 0.0, 0.0, 1.0, 0.1, 0.0, 0.2, 0.9, 0.1, 0.3, 0.2, 0.8};
        m.F = {0, 2, 1, 0, 1, 3, 1, 2, 3, 2, 0, 3};
        return m;
    }
    const int nF = nV - 2, rows = nV / 2 + 1;
    std::vector<double> V(6 * (size_t)rows);
    for (int i = 0; i < rows; i++) {
        const double x = (double)i;
        V[3 * i] = x; V[3 * i + 1] = 0.1 * std::sin(x); V[3 * i + 2] = 0.2 * std::cos(0.3 * x);
        V[3 * (rows + i)] = x + 0.4; V[3 * (rows + i) + 1] = 1.0 + 0.1 * std::cos(x); V[3 * (rows + i) + 2] = 0.2 * std::sin(0.3 * x);
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

static bool run_case(int nV, int k)
{
    const Mesh m = make_mesh(nV);
    if (m.nV() != nV) return false;
    const int nF = m.nF();
    const size_t n = (size_t)nV, f = (size_t)nF;
    std::vector<int> mpv, miv;
    vertex_corner_lists(m.F, nV, mpv, miv);
    auto F = exact(m.F.data(), m.F.size());
    auto mp = exact(mpv.data(), mpv.size());
    auto mi = exact(miv.data(), miv.size());
    auto V0 = exact(m.V.data(), m.V.size());
    // k poses: the rest pose turned about z by 0.4 (c + 1), stretched, with a ripple
    std::unique_ptr<double[]> X(new double[3 * n * k]), t(new double[k]);
    for (int c = 0; c < k; c++) {
        const double a = 0.4 * (c + 1), cs = std::cos(a), sn = std::sin(a);
        t[c] = -0.5 + 0.75 * c;
        for (size_t i = 0; i < n; i++) {
            const double x = 1.3 * V0[3 * i], y = 0.8 * V0[3 * i + 1], z = V0[3 * i + 2] + 0.05 * std::sin(1.0 + (double)i);
            double* o = X.get() + ((size_t)c * n + i) * 3;
            o[0] = cs * x - sn * y; o[1] = sn * x + cs * y; o[2] = z;
        }
    }
    const int pins[2] = {nV - 1, 0};
    auto pn = exact(pins, 2);
    std::unique_ptr<double[]> J(new double[9 * f * k]), pol(new double[18 * f]), B1(new double[3 * n * k]), q1(new double[n * k]), B2(new double[3 * n * k]),
        q2(new double[n * k]), hp(new double[6 * (size_t)k]), U(new double[3 * n * k]), hp0(new double[6 * (size_t)k]), U0(new double[3 * n * k]);
    morph_host_gradient(nV, nF, k, F.get(), V0.get(), X.get(), J.get());
    morph_host_polar(nF, F.get(), V0.get(), X.get(), pol.get(), pol.get() + 9 * f, pol.get() + 12 * f);
    morph_host_rhs(nV, nF, k, F.get(), V0.get(), mp.get(), mi.get(), J.get(), nullptr, nullptr, nullptr, B1.get(), q1.get());
    morph_host_rhs(nV, nF, k, F.get(), V0.get(), mp.get(), mi.get(), nullptr, pol.get() + 9 * f, pol.get() + 12 * f, t.get(), B2.get(), q2.get());
    morph_host_pins(nV, k, V0.get(), X.get(), t.get(), pn.get(), 2, hp.get(), U.get());
    morph_host_pins(nV, k, V0.get(), nullptr, nullptr, pn.get(), 2, hp0.get(), U0.get());
    bool finite = true, rot = true, sym = true, rest = true;
    for (size_t i = 0; i < 9 * f * k; i++) finite = finite && std::isfinite(J[i]);
    for (size_t i = 0; i < 3 * n * k; i++) finite = finite && std::isfinite(B1[i]) && std::isfinite(B2[i]) && std::isfinite(U[i]);
    for (size_t i = 0; i < n * k; i++) finite = finite && q1[i] >= 0.0 && q2[i] >= 0.0;
    for (size_t g = 0; g < f; g++) {
        const double* R = pol.get() + 9 * g;
        for (int a = 0; a < 3; a++)
            for (int b = 0; b < 3; b++) {
                const double d = R[a] * R[b] + R[3 + a] * R[3 + b] + R[6 + a] * R[6 + b] - (a == b ? 1.0 : 0.0);
                rot = rot && std::fabs(d) < 1e-14;
            }
        // J = R S for the first pose: S comes out symmetric by construction, so check the product instead
        const double* S = pol.get() + 12 * f + 6 * g;
        const double Sm[9] = {S[0], S[1], S[2], S[1], S[3], S[4], S[2], S[4], S[5]};
        for (int a = 0; a < 3; a++)
            for (int b = 0; b < 3; b++) {
                const double rs = R[3 * a] * Sm[b] + R[3 * a + 1] * Sm[3 + b] + R[3 * a + 2] * Sm[6 + b];
                sym = sym && std::fabs(rs - J[9 * g + 3 * a + b]) < 1e-13;
            }
    }
    for (int c = 0; c < k; c++)
        for (int d = 0; d < 3; d++)
            for (size_t i = 0; i < n; i++) rest = rest && U0[(size_t)(3 * c + d) * n + i] == V0[3 * i + d];
    const bool ok = finite && rot && sym && rest;
    std::printf("nV %d nF %d k %d: finite %d, rotations %d, J = R S %d, rest start %d: ok %d\n", nV, nF, k, (int)finite, (int)rot, (int)sym, (int)rest, (int)ok);
    return ok;
}

int main()
{
    bool ok = true;
    for (int nV : {255, 256, 257, 4})
        for (int k : {1, 2, 5}) ok = run_case(nV, k) && ok;
    return ok ? 0 : 1;
}
