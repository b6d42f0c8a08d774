// wave_gradient_asan_driver.cpp -- a stand-alone program (its own main) that runs the host side of the wave object's adjoint pass on exactly-sized heap
// arrays, so that AddressSanitizer sees any read or write past an end and UndefinedBehaviorSanitizer any undefined operation: every loop of the
// host twin (smg::wave_group_receivers, wave_adj_host_planes, _keep, _residual, _inject, _rhs, _advance, _signal and _scale of
// csrc/smg_wave_adjoint_inl.hpp, what smg_wave_adjoint_host runs after its argument checks), on closed double pyramids of 63, 64, 65 and 257 vertices
// -- the edges of a wavefront of 64 lanes and of a block of 256 -- and on one open fan, free and clamped, k = 3, with a receiver list that repeats
// vertices and holds vertex 0 and vertex nV - 1.  tests/test_wave_adjoint_host.py compiles it together with csrc/smg_mesh.cpp and
// csrc/smg_sparse.cpp with -fsanitize=address,undefined and runs it directly.
#include <cmath>
#include <cstdio>
#include <memory>
#include <vector>

#include "smg_mesh.hpp"
#include "smg_wave_adjoint_inl.hpp"

using namespace smg;

// a closed double pyramid: a ring of nV - 2 vertices on a wavy ellipse, one apex above and one below; open: the upper fan alone, nV - 1 vertices
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
    const int n_rec = 5, n_src = 1, rows = 2;
    const int rec_v[5] = {0, nV - 1, top, 0, top}, src_v[1] = {top};
    std::unique_ptr<int[]> rec(exact(rec_v, 5)), src(exact(src_v, 1));
    std::vector<int> gv, gp, gl;
    wave_group_receivers(nV, n_rec, rec.get(), clamped ? known.get() : nullptr, gv, gp, gl);
    auto grp_v = exact(gv.data(), gv.size());
    auto grp_ptr = exact(gp.data(), gp.size());
    auto grp_slot = exact(gl.data(), gl.size());
    const int n_grp = (int)gv.size();
    bool groups = gp.back() == (int)gl.size();
    for (int j = 0; j < n_grp; j++) {
        groups = groups && !known[(size_t)gv[(size_t)j]] && (j == 0 || gv[(size_t)j - 1] < gv[(size_t)j]) && gp[(size_t)j] < gp[(size_t)j + 1];
        for (int s = gp[(size_t)j]; s < gp[(size_t)j + 1]; s++)
            groups = groups && rec[(size_t)gl[(size_t)s]] == gv[(size_t)j] && (s == gp[(size_t)j] || gl[(size_t)s - 1] < gl[(size_t)s]);
    }
    const double dt = 0.05, a = 0.25 * dt * dt, q2 = 2.0 / dt;
    const size_t ent = (size_t)rows * n_rec, sk = (size_t)n_src * kk;
    std::unique_ptr<double[]> A(new double[f]), m(new double[n]), speed(new double[n]), sigma(new double[n]), mt(new double[n]), s2(new double[n]), fac(new double[n]),
        u(new double[nk]), v(new double[nk]), u1(new double[nk]), e(new double[nk]), tr(new double[ent * kk]), ob(new double[ent * kk]), rho(new double[ent * kk]),
        sq(new double[ent * kk]), rho0(new double[ent * kk]), sq0(new double[ent * kk]), p(new double[nk]), q(new double[nk]), y(new double[nk]), G(new double[nk]),
        g(new double[nk]), gsq(new double[nk]), p0(new double[nk]), gs0(new double[sk]), gs1(new double[sk]), out(new double[nk]);
    for (size_t i = 0; i < n; i++) {
        speed[i] = 1.0 + 0.25 * std::sin(2.0 * V[3 * i]);
        sigma[i] = 0.2 * (1.0 + std::cos(3.0 * V[3 * i + 1]));
    }
    for (int s = 0; s < k; s++)
        for (size_t i = 0; i < n; i++) {
            const bool fixed = known[i] != 0;
            const size_t o = (size_t)s * n + i;
            u[o] = fixed ? 0.0 : 1.0 - 0.5 * std::cos((2.0 + s) * V[3 * i + 1]);
            v[o] = fixed ? 0.0 : 0.25 + 0.2 * std::sin((3.0 + s) * V[3 * i]);
            u1[o] = fixed ? 0.0 : u[o] + 0.01 * (s + 1);
            y[o] = fixed ? 0.0 : 0.3 * std::cos((1.0 + s) * V[3 * i]);
            p[o] = 0.0; q[o] = fixed ? 0.0 : 0.1 * v[o]; G[o] = 0.0;
        }
    for (size_t j = 0; j < ent * kk; j++) { tr[j] = 0.5 + 0.1 * j; ob[j] = 0.25 * j; }
    for (size_t j = 0; j < sk; j++) { gs0[j] = 0.0; gs1[j] = 1.0; }
    fluid_host_mass(nV, nF, F.get(), V.get(), mp.get(), mi.get(), A.get(), m.get());
    wave_host_planes(nV, m.get(), speed.get(), sigma.get(), dt, mt.get(), s2.get());
    wave_adj_host_planes(nV, mt.get(), speed.get(), fac.get());
    wave_adj_host_keep(nV, k, s2.get(), dt, u.get(), v.get(), u1.get(), e.get());
    wave_adj_host_residual(k, ent, tr.get(), ob.get(), rho.get(), sq.get());
    wave_adj_host_residual(k, ent, tr.get(), nullptr, rho0.get(), sq0.get());
    wave_adj_host_inject(nV, k, n_grp, grp_v.get(), grp_ptr.get(), grp_slot.get(), rho.get() + (size_t)n_rec * kk, p.get());
    for (size_t o = 0; o < nk; o++) p0[o] = p[o];
    wave_adj_host_rhs(nV, k, clamped ? known.get() : nullptr, q2, p.get(), q.get(), g.get(), gsq.get());
    wave_adj_host_advance(nV, k, mt.get(), s2.get(), dt, q2, y.get(), e.get(), p.get(), q.get(), G.get());
    wave_adj_host_signal(nV, k, n_src, src.get(), a, y.get(), gs0.get(), gs1.get());
    wave_adj_host_scale(nV, k, fac.get(), G.get(), out.get());
    bool finite = true, squares = true, zeros = true, injected = true, signal = true;
    for (size_t o = 0; o < nk; o++) {
        const size_t i = o % n;
        finite = finite && std::isfinite(e[o]) && std::isfinite(p[o]) && std::isfinite(q[o]) && std::isfinite(G[o]) && std::isfinite(out[o]);
        squares = squares && gsq[o] == g[o] * g[o] && G[o] == 0.0 + y[o] * e[o];
        if (known[i]) zeros = zeros && g[o] == 0.0 && p[o] == 0.0 && q[o] == 0.0 && G[o] == 0.0 && out[o] == 0.0 && p0[o] == 0.0;
        bool is_rec = false;
        for (int j = 0; j < n_rec; j++) is_rec = is_rec || ((size_t)rec[j] == i && !known[i]);
        injected = injected && (is_rec ? p0[o] != 0.0 : p0[o] == 0.0);
    }
    for (size_t j = 0; j < ent * kk; j++) squares = squares && rho[j] == tr[j] - ob[j] && rho0[j] == tr[j];
    for (size_t j = 0; j < sk; j++) {
        const double x = a * y[(j % kk) * n + (size_t)top];
        signal = signal && gs0[j] == 0.0 + x && gs1[j] == 1.0 + x;
    }
    double J = 0.0;
    for (size_t c = 0; c < kk; c++) J += 0.5 * flow_host_sum(sq.get() + c * ent, (int)ent);
    finite = finite && std::isfinite(J) && J > 0.0 && flow_host_sum(gsq.get(), (int)nk) > 0.0;
    const bool ok = finite && groups && squares && zeros && injected && signal;
    std::printf("nV %d nF %d k %d %s %s: finite %d, groups %d (%d), squares %d, zeros %d, injected %d, signal %d: ok %d\n", nV, nF, k, open ? "open" : "closed",
                clamped ? "clamped" : "free", (int)finite, (int)groups, n_grp, (int)squares, (int)zeros, (int)injected, (int)signal, (int)ok);
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
