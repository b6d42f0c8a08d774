// fluid_asan_driver.cpp -- a stand-alone program (its own main) that runs the host side of the surface fluid on exactly-sized heap arrays, so that
// AddressSanitizer sees any read or write past an end and UndefinedBehaviorSanitizer any undefined operation: every loop of the host twin
// (smg::fluid_host_* and fluid_known_rows of csrc/smg_fluid_inl.hpp, what smg_fluid_host runs after its argument checks), on closed double
// pyramids of 255, 256 and 257 vertices -- the edges of a block of 256 lanes -- and of 2100 vertices, whose apex corner lists are the long ones,
// and on one open fan, k = 2.  The corner lists come from csrc/smg_mesh.cpp.  tests/test_fluid_host.py compiles it together with csrc/smg_mesh.cpp
// and csrc/smg_sparse.cpp with -fsanitize=address,undefined and runs it directly.
#include <cmath>
#include <cstdio>
#include <memory>
#include <vector>

#include "smg_fluid_inl.hpp"
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
    std::vector<int> Fv, mpv, miv, knownv;
    make_mesh(nV, open, Vv, Fv);
    const int nF = (int)Fv.size() / 3;
    const size_t n = (size_t)nV, f = (size_t)nF, kk = (size_t)k, nk = n * kk, fk = f * kk;
    vertex_corner_lists(Fv, nV, mpv, miv);
    const int nb = fluid_known_rows(nV, nF, Fv.data(), knownv);
    auto F = exact(Fv.data(), Fv.size());
    auto mp = exact(mpv.data(), mpv.size());
    auto mi = exact(miv.data(), miv.size());
    auto V = exact(Vv.data(), Vv.size());
    auto known = exact(knownv.data(), knownv.size());
    std::unique_ptr<double[]> A(new double[f]), m(new double[n]), w(new double[nk]), psi(new double[nk]), mw(new double[nk]), ew(new double[nk]),
        mwsum(new double[kk]), R(new double[nk]), rsq(new double[nk]), out(new double[nk]), rate(new double[nk]), rate2(new double[nk]), mo(new double[nk]),
        U(new double[3 * fk]), terms(new double[fk]), dt(new double[kk]), rmax(new double[3 * kk]), t_in(new double[kk]), dt0(new double[kk]),
        cfl(new double[kk]), t_out(new double[kk]);
    for (int s = 0; s < k; s++)
        for (size_t i = 0; i < n; i++) {
            w[(size_t)s * n + i] = std::cos((2.0 + s) * V[3 * i + 1]) - 0.5 * V[3 * i] * V[3 * i + 2];
            psi[(size_t)s * n + i] = known[i] && nb > 0 ? 0.0 : std::sin((3.0 + s) * V[3 * i]) + V[3 * i + 1] * V[3 * i + 2] + 0.3 * V[3 * i + 2];
        }
    fluid_host_mass(nV, nF, F.get(), V.get(), mp.get(), mi.get(), A.get(), m.get());
    const double msum = flow_host_sum(m.get(), nV);
    fluid_host_diag(nV, k, m.get(), w.get(), mw.get(), ew.get());
    for (int s = 0; s < k; s++) mwsum[(size_t)s] = flow_host_sum(mw.get() + (size_t)s * n, nV);
    fluid_host_rhs(nV, k, m.get(), known.get(), w.get(), nb > 0 ? nullptr : mwsum.get(), msum, R.get(), rsq.get());
    fluid_host_advect(nV, k, F.get(), mp.get(), mi.get(), m.get(), psi.get(), nullptr, nullptr, 0.0, 1.0, nullptr, 0.0, nullptr, rate2.get(), nullptr);
    for (int s = 0; s < k; s++) {
        rmax[(size_t)s] = flow_host_max(rate2.get() + (size_t)s * n, nV);
        rmax[kk + (size_t)s] = 0.5 * rmax[(size_t)s];
        rmax[2 * kk + (size_t)s] = 1.25 * rmax[(size_t)s];
        t_in[(size_t)s] = 0.5 * s;
    }
    fluid_host_dt(k, 3, 0.5, rmax.get(), t_in.get(), dt0.get(), cfl.get(), t_out.get());
    for (int s = 0; s < k; s++) dt[(size_t)s] = dt0[(size_t)s];
    fluid_host_advect(nV, k, F.get(), mp.get(), mi.get(), m.get(), psi.get(), w.get(), w.get(), 0.0, 1.0, dt.get(), 1.0, out.get(), rate.get(), mo.get());
    fluid_host_velocity(nV, nF, k, F.get(), V.get(), psi.get(), U.get(), terms.get());
    bool finite = true, rates = true, circ = true, maxp = true, step = true;
    for (size_t i = 0; i < nk; i++)
        finite = finite && std::isfinite(R[i]) && std::isfinite(out[i]) && std::isfinite(mw[i]) && (known[i % n] ? rsq[i] == 0.0 : rsq[i] == R[i] * R[i]);
    for (size_t i = 0; i < 3 * fk; i++) finite = finite && std::isfinite(U[i]);
    for (size_t i = 0; i < nk; i++) rates = rates && rate[i] == rate2[i] && rate[i] >= 0.0;
    double area = 0.0;
    for (size_t q = 0; q < f; q++) area += A[q];
    finite = finite && std::fabs(msum - area) <= 1e-12 * area;
    for (int s = 0; s < k; s++) {
        // the fluxes of a vertex sum to zero (psi = 0 on a boundary): a stage keeps sum m w; upwind at dt rate <= 1/2 stays inside the extremes
        double before = 0.0, after = 0.0, scale = 0.0, lo = w[(size_t)s * n], hi = lo;
        for (size_t i = 0; i < n; i++) {
            before += mw[(size_t)s * n + i]; after += mo[(size_t)s * n + i]; scale += std::fabs(mw[(size_t)s * n + i]);
            lo = std::fmin(lo, w[(size_t)s * n + i]); hi = std::fmax(hi, w[(size_t)s * n + i]);
        }
        circ = circ && std::fabs(after - before) <= 1e-11 * scale;
        for (size_t i = 0; i < n; i++) maxp = maxp && out[(size_t)s * n + i] <= hi + 1e-12 && out[(size_t)s * n + i] >= lo - 1e-12;
        step = step && rmax[(size_t)s] > 0.0 && dt0[(size_t)s] > 0.0 && std::fabs(cfl[(size_t)s] - 0.625) <= 1e-12 && t_out[(size_t)s] == t_in[(size_t)s] + dt0[(size_t)s];
    }
    const bool ok = finite && rates && circ && maxp && step;
    std::printf("nV %d nF %d k %d %s: finite %d, rates %d, circulation %d, maximum principle %d, step %d: ok %d\n", nV, nF, k, open ? "open" : "closed",
                (int)finite, (int)rates, (int)circ, (int)maxp, (int)step, (int)ok);
    return ok;
}

int main()
{
    bool ok = true;
    for (int nV : {255, 256, 257, 2100}) ok = run_case(nV, false, 2) && ok;
    ok = run_case(258, true, 2) && ok;
    return ok ? 0 : 1;
}
