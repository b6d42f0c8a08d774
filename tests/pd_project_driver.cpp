// pd_project_driver.cpp -- a stand-alone program (its own main) that runs the host side of csrc/smg_pd_inl.hpp on exactly-sized heap arrays, so
// that AddressSanitizer sees any read or write past an end and UndefinedBehaviorSanitizer any undefined operation: a strip of faces at a
// stretched pose, then the guard faces (one collapsed to a segment, one to a point) in the last two slots.  tests/test_pd_host.py compiles it
// with -fsanitize=address,undefined and runs it directly.
#include <cmath>
#include <cstdio>
#include <memory>

#include "smg_pd_inl.hpp"

int main()
{
    using namespace smg;
    const int nF = 67, nV = 3 * nF;                                   // every face has its own three vertices
    std::unique_ptr<double[]> V0(new double[3 * nV]), P(new double[3 * nV]);
    std::unique_ptr<double[]> rest(new double[4 * nF]), Fg(new double[6 * nF]), sigma(new double[2 * nF]), T(new double[6 * nF]);
    std::unique_ptr<double[]> eterm(new double[nF]), share(new double[9 * nF]);
    for (int f = 0; f < nF; f++) {
        const double x = 0.1 * f, rest_face[9] = {x, 0.0, 0.0, x + 1.0, 0.1 * std::sin(x), 0.0, x + 0.3, 0.8, 0.05 * x};
        for (int e = 0; e < 9; e++) {
            V0[9 * f + e] = rest_face[e];
            P[9 * f + e] = rest_face[e] * (e % 3 == 0 ? 0.7 + 0.01 * f : e % 3 == 1 ? 1.3 - 0.01 * f : 1.0) + 0.01 * std::cos(3.0 * e + f);
        }
    }
    const double seg[9] = {0, 0, 0, 2, 0, 0, 0.6, 0, 0}, rest_tri[9] = {0, 0, 0, 1, 0, 0, 0.3, 0.8, 0};
    for (int e = 0; e < 9; e++) {
        V0[9 * (nF - 2) + e] = V0[9 * (nF - 1) + e] = rest_tri[e];
        P[9 * (nF - 2) + e] = seg[e];
        P[9 * (nF - 1) + e] = e % 3 == 0 ? 0.25 : e % 3 == 1 ? -1.0 : 2.0;
    }
    int guards = 0;
    double energy = 0.0;
    for (int f = 0; f < nF; f++) {
        double r[4], g[6], s[2], t[6], sh[9];
        pd_rest(&V0[9 * f], &V0[9 * f + 3], &V0[9 * f + 6], r);
        pd_gradient(r, &P[9 * f], &P[9 * f + 3], &P[9 * f + 6], g);
        guards += pd_project(g, 0.9, 1.2, s, t);
        pd_corner_shares(r, 1.0, t, sh);
        eterm[f] = pd_face_energy(r, 1.0, g, t);
        for (int e = 0; e < 4; e++) rest[e * nF + f] = r[e];
        for (int e = 0; e < 6; e++) { Fg[e * nF + f] = g[e]; T[e * nF + f] = t[e]; }
        for (int e = 0; e < 2; e++) sigma[e * nF + f] = s[e];
        for (int e = 0; e < 9; e++) share[e * nF + f] = sh[e];
        energy += eterm[f];
    }
    bool finite = std::isfinite(energy);
    for (int i = 0; i < 6 * nF; i++) finite = finite && std::isfinite(T[i]) && std::isfinite(Fg[i]);
    for (int i = 0; i < 9 * nF; i++) finite = finite && std::isfinite(share[i]);
    const bool seg_ok = T[0 * nF + nF - 2] == 1.2 && T[4 * nF + nF - 2] == 0.9 && sigma[nF - 2] == 2.0 && sigma[nF + nF - 2] == 0.0;
    const bool point_ok = T[0 * nF + nF - 1] == 0.9 && T[4 * nF + nF - 1] == 0.9 && T[1 * nF + nF - 1] == 0.0 && sigma[nF - 1] == 0.0;
    std::printf("faces %d, guard faces %d, energy %.6e, finite %d, segment %d, point %d\n", nF, guards, energy, (int)finite, (int)seg_ok, (int)point_ok);
    return (guards == 2 && finite && seg_ok && point_ok) ? 0 : 1;
}
