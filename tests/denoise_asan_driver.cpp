// denoise_asan_driver.cpp -- a stand-alone program (its own main) that runs the host side of the denoiser on exactly-sized heap arrays, so that
// AddressSanitizer sees any read or write past an end and UndefinedBehaviorSanitizer any undefined operation: the neighbourhoods
// (smg::face_neighbours of csrc/smg_mesh.cpp, what smg_mesh_face_neighbours returns) of a closed fan of 65 faces -- every row has 64 entries --
// and of a tetrahedron, then every op of the host twin (smg::dn_faces_host of csrc/smg_denoise_inl.hpp, what smg_denoise_faces_host runs after
// its argument checks) on the fan.  tests/test_denoise_host.py compiles it together with csrc/smg_mesh.cpp and csrc/smg_sparse.cpp with
// -fsanitize=address,undefined and runs it directly.
#include <cmath>
#include <cstdio>
#include <memory>
#include <vector>

#include "smg_denoise_inl.hpp"
#include "smg_mesh.hpp"

int main()
{
    using namespace smg;
    const int nF = 65, nV = nF + 1;
    std::unique_ptr<double[]> V(new double[3 * nV]), X(new double[3 * nV]);
    std::vector<int> F(3 * nF);
    V[0] = 0.05; V[1] = -0.02; V[2] = 0.4;
    for (int i = 0; i < nF; i++) {
        const double t = 2.0 * 3.14159265358979323846 * i / nF, rad = 1.0 + 0.2 * std::cos(3.0 * t);
        V[3 * (1 + i)] = rad * std::cos(t); V[3 * (1 + i) + 1] = rad * std::sin(t); V[3 * (1 + i) + 2] = 0.3 * std::sin(2.0 * t);
        F[3 * i] = 0; F[3 * i + 1] = 1 + i; F[3 * i + 2] = 1 + (i + 1) % nF;
    }
    for (int i = 0; i < 3 * nV; i++) X[i] = V[i] + 0.01 * std::sin(1.0 + i);
    std::vector<int> mp, mi, np, ni;
    vertex_corner_lists(F, nV, mp, mi);
    bool ok = face_neighbours(F, mp, mi, np, ni);
    int full = 0;
    for (int f = 0; f < nF; f++) {
        full += np[f + 1] - np[f] == nF - 1 ? 1 : 0;
        for (int q = np[f]; q < np[f + 1]; q++) ok = ok && ni[q] != f && (q == np[f] || ni[q - 1] < ni[q]);
    }
    // exactly-sized copies of the lists: the twin must not read past them
    std::unique_ptr<int[]> ptr(new int[nF + 1]), idx(new int[ni.size()]), Fx(new int[3 * nF]);
    for (int i = 0; i <= nF; i++) ptr[i] = np[i];
    for (size_t i = 0; i < ni.size(); i++) idx[i] = ni[i];
    for (int i = 0; i < 3 * nF; i++) Fx[i] = F[i];
    std::unique_ptr<double[]> rest(new double[DN_REST * nF]), sp(new double[nF]), m(new double[3 * nF]), m0(new double[3 * nF]), pr(new double[10 * nF]);
    dn_faces_host(0, nF, Fx.get(), V.get(), nullptr, nullptr, 0.0, 0.0, 0, nullptr, nullptr, rest.get());
    dn_faces_host(1, nF, Fx.get(), V.get(), nullptr, nullptr, 0.0, 0.0, 0, ptr.get(), idx.get(), sp.get());
    double pairs = 0.0;
    for (int f = 0; f < nF; f++) pairs += sp[f];
    const double sigma_s = pairs / (double)ni.size();
    dn_faces_host(2, nF, Fx.get(), V.get(), nullptr, rest.get(), sigma_s, 0.35, 0, ptr.get(), idx.get(), m0.get());
    dn_faces_host(2, nF, Fx.get(), V.get(), nullptr, rest.get(), sigma_s, 0.35, 5, ptr.get(), idx.get(), m.get());
    dn_faces_host(3, nF, Fx.get(), V.get(), X.get(), m.get(), 0.0, 0.0, 0, nullptr, nullptr, pr.get());
    bool finite = true, unit = true, same = true;
    double energy = 0.0;
    for (int f = 0; f < nF; f++) {
        const double len = std::sqrt(m[f] * m[f] + m[nF + f] * m[nF + f] + m[2 * nF + f] * m[2 * nF + f]);
        unit = unit && std::fabs(len - 1.0) < 1e-15;
        energy += pr[f];
    }
    for (int i = 0; i < 3 * nF; i++) same = same && m0[i] == rest[i];            // no iteration returns the input bits
    for (int i = 0; i < 10 * nF; i++) finite = finite && std::isfinite(pr[i]);
    // the tetrahedron: every row has 3 entries
    std::vector<int> T = {0, 2, 1, 0, 1, 3, 1, 2, 3, 2, 0, 3}, tp, ti, tnp, tni;
    vertex_corner_lists(T, 4, tp, ti);
    ok = ok && face_neighbours(T, tp, ti, tnp, tni) && tni.size() == 12;
    std::printf("rows of 64: %d, entries %zu, lists ok %d, sigma_s %.6f, energy %.6e, finite %d, unit %d, input kept %d\n", full, ni.size(), (int)ok, sigma_s,
                energy, (int)finite, (int)unit, (int)same);
    return (full == nF && ok && finite && unit && same && energy > 0.0) ? 0 : 1;
}
