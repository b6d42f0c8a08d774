// wave_asan_driver.cpp -- a stand-alone program (its own main) that runs the host side of the wave equation on a surface on exactly-sized heap
// arrays, so that AddressSanitizer sees any read or write past an end and UndefinedBehaviorSanitizer any undefined operation: every loop of the
// host twin (smg::wave_host_planes, _rhs, _sources, _advance and _record of csrc/smg_wave_inl.hpp with the masses of fluid_host_mass and the
// potential terms of fluid_host_velocity, what smg_wave_host runs after its argument checks), on closed double pyramids of 63, 64, 65 and 257
// vertices -- the edges of a wavefront of 64 lanes and of a block of 256 -- and on one open fan, free and clamped, k = 3.  The corner lists and
// the boundary come from csrc/smg_mesh.cpp.  tests/test_wave_host.py compiles it together with csrc/smg_mesh.cpp and csrc/smg_sparse.cpp with
// -fsanitize=address,undefined and runs it directly.
#include <cmath>
#include <cstdio>
#include <memory>
#include <vector>

#include "smg_mesh.hpp"
#include "smg_wave_inl.hpp"

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

static bool run_case(int nV, bool open, bool clamped, int k)
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
    std::vector<int> kv(n, 0);
    if (clamped)
        for (int b : boundary_vertices(F.get(), nF, nV)) kv[(size_t)b] = 1;
    auto known = exact(kv.data(), n);
    const int top = open ? nV - 1 : nV - 2;                                   // an interior vertex in every case
    const int n_src = 2, n_rec = 3;
    const int src_v[2] = {top, clamped ? top : 0}, rec_v[3] = {0, nV - 1, 0};
    std::unique_ptr<int[]> src(exact(src_v, clamped ? 1 : 2)), rec(exact(rec_v, 3));
    const int ns = clamped ? 1 : n_src;
    const double dt = 0.05, a = 0.25 * dt * dt, q2 = 2.0 / dt;
    std::unique_ptr<double[]> A(new double[f]), m(new double[n]), speed(new double[n]), sigma(new double[n]), mt(new double[n]), s2(new double[n]),
        u(new double[nk]), v(new double[nk]), w(new double[nk]), b(new double[nk]), rsq(new double[nk]), z(new double[nk]), b0(new double[nk]),
        sig0(new double[(size_t)ns * kk]), sig1(new double[(size_t)ns * kk]), un(new double[nk]), vn(new double[nk]), ke(new double[nk]), un2(new double[nk]),
        vn2(new double[nk]), ke2(new double[nk]), bn(new double[nk]), rsqn(new double[nk]), zn(new double[nk]), b2(new double[nk]), rsq2(new double[nk]),
        z2(new double[nk]), tr(new double[(size_t)n_rec * kk]), U(new double[3 * f * kk]), terms(new double[f * kk]);
    for (size_t i = 0; i < n; i++) {
        speed[i] = 1.0 + 0.25 * std::sin(2.0 * V[3 * i]);
        sigma[i] = 0.2 * (1.0 + std::cos(3.0 * V[3 * i + 1]));
    }
    for (int s = 0; s < k; s++)
        for (size_t i = 0; i < n; i++) {
            const bool fixed = known[i] != 0;
            u[(size_t)s * n + i] = fixed ? 0.0 : 1.0 - 0.5 * std::cos((2.0 + s) * V[3 * i + 1]);
            v[(size_t)s * n + i] = fixed ? 0.0 : 0.25 + 0.2 * std::sin((3.0 + s) * V[3 * i]);
            w[(size_t)s * n + i] = fixed ? 0.0 : 2.0 * u[(size_t)s * n + i] + 0.01 * (s + 1);
        }
    for (size_t j = 0; j < (size_t)ns * kk; j++) { sig0[j] = 0.5 + 0.1 * j; sig1[j] = -0.25 * j; }
    fluid_host_mass(nV, nF, F.get(), V.get(), mp.get(), mi.get(), A.get(), m.get());
    wave_host_planes(nV, m.get(), speed.get(), sigma.get(), dt, mt.get(), s2.get());
    wave_host_rhs(nV, k, mt.get(), s2.get(), clamped ? known.get() : nullptr, dt, u.get(), v.get(), b.get(), rsq.get(), z.get());
    for (size_t e = 0; e < nk; e++) b0[e] = b[e];
    wave_host_sources(nV, k, ns, src.get(), sig0.get(), sig1.get(), a, b.get(), rsq.get());
    wave_host_advance(nV, k, mt.get(), s2.get(), clamped ? known.get() : nullptr, dt, q2, w.get(), u.get(), v.get(), un.get(), vn.get(), ke.get(), nullptr,
                      nullptr, nullptr);
    wave_host_advance(nV, k, mt.get(), s2.get(), clamped ? known.get() : nullptr, dt, q2, w.get(), u.get(), v.get(), un2.get(), vn2.get(), ke2.get(), bn.get(),
                      rsqn.get(), zn.get());
    wave_host_rhs(nV, k, mt.get(), s2.get(), clamped ? known.get() : nullptr, dt, un.get(), vn.get(), b2.get(), rsq2.get(), z2.get());
    wave_host_record(nV, k, n_rec, rec.get(), un.get(), tr.get());
    fluid_host_velocity(nV, nF, k, F.get(), V.get(), un.get(), U.get(), terms.get());
    bool finite = true, squares = true, fused = true, zeros = true, sourced = true, traces = true;
    for (size_t e = 0; e < nk; e++) {
        const size_t i = e % n;
        finite = finite && std::isfinite(b[e]) && std::isfinite(un[e]) && std::isfinite(vn[e]) && std::isfinite(ke[e]) && ke[e] >= 0.0;
        squares = squares && rsq[e] == (known[i] ? 0.0 : b[e] * b[e]);
        fused = fused && un2[e] == un[e] && vn2[e] == vn[e] && ke2[e] == ke[e] && bn[e] == b2[e] && rsqn[e] == rsq2[e] && zn[e] == z2[e];
        if (known[i]) zeros = zeros && b[e] == 0.0 && un[e] == 0.0 && vn[e] == 0.0 && bn[e] == 0.0;
        bool is_src = false;
        for (int j = 0; j < ns; j++) is_src = is_src || (size_t)src[j] == i;
        sourced = sourced && (is_src ? b[e] != b0[e] : b[e] == b0[e]);
    }
    for (int j = 0; j < n_rec; j++)
        for (int c = 0; c < k; c++) traces = traces && tr[(size_t)j * kk + c] == un[(size_t)c * n + (size_t)rec[j]];
    double pe = 0.0;
    for (size_t c = 0; c < kk; c++) pe += flow_host_sum(terms.get() + c * f, nF);
    const double ss = flow_host_sum(rsq.get(), (int)nk), kin = flow_host_sum(ke.get(), nV);
    finite = finite && std::isfinite(ss) && ss > 0.0 && kin > 0.0 && std::isfinite(pe) && pe > 0.0;
    const bool ok = finite && squares && fused && zeros && sourced && traces;
    std::printf("nV %d nF %d k %d %s %s: finite %d, squares %d, fused %d, zeros %d, sources %d, traces %d: ok %d\n", nV, nF, k, open ? "open" : "closed",
                clamped ? "clamped" : "free", (int)finite, (int)squares, (int)fused, (int)zeros, (int)sourced, (int)traces, (int)ok);
    return ok;
}

int main()
{
    bool ok = true;
    for (int nV : {63, 64, 65, 257}) ok = run_case(nV, false, false, 3) && ok;
    ok = run_case(66, true, false, 3) && ok;
    ok = run_case(66, true, true, 3) && ok;
    return ok ? 0 : 1;
}
