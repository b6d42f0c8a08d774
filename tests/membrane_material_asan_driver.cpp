// membrane_material_asan_driver.cpp -- a stand-alone program for tests/test_membrane_materials_host.py: smg_membrane_faces_host_material on a small
// strip for the three materials, energy only, with derivatives, with the fix; built with -fsanitize=address,undefined against the sanitized host
// library and run directly.  Every array is a heap block of exactly the documented size, so a write past the 1 + 9 + 45 planes is a report.
#include <cmath>
#include <cstdio>
#include <vector>

#include "smg.h"

int main()
{
    const int n = 8, nV = 2 * n, nF = 2 * (n - 1);
    std::vector<double> V0(3 * (size_t)nV), P(3 * (size_t)nV);
    std::vector<int> F(3 * (size_t)nF);
    for (int i = 0; i < n; i++)
        for (int j = 0; j < 2; j++) {
            const int v = 2 * i + j;
            V0[3 * v] = i; V0[3 * v + 1] = j; V0[3 * v + 2] = 0.1 * std::sin(0.7 * i);
            // stretched along the strip, compressed across it, more or less from quad to quad: pure-tension, wrinkled and slack faces
            const double sx = 0.9 + 0.05 * (i % 5), sy = 0.8 + 0.09 * (i % 4);
            P[3 * v] = sx * i; P[3 * v + 1] = sy * j; P[3 * v + 2] = 0.1 * std::sin(0.7 * i) + 0.01 * j;
        }
    for (int i = 0; i + 1 < n; i++) {
        const int a = 2 * i, b = 2 * i + 1, c = 2 * i + 2, d = 2 * i + 3;
        int* f = &F[6 * (size_t)i];
        f[0] = a; f[1] = c; f[2] = b; f[3] = b; f[4] = c; f[5] = d;
    }
    smg_membrane_params prm;
    smg_membrane_params_default(&prm);
    int failures = 0;
    for (int material = 0; material < 3; material++) {
        std::vector<double> W0(nF), W1(nF), W2(nF), G(9 * (size_t)nF), G2(9 * (size_t)nF), H(45 * (size_t)nF), H2(45 * (size_t)nF);
        int rc = smg_membrane_faces_host_material(V0.data(), P.data(), nV, F.data(), nF, &prm, material, 0, W0.data(), nullptr, nullptr);
        rc |= smg_membrane_faces_host_material(V0.data(), P.data(), nV, F.data(), nF, &prm, material, 0, W1.data(), G.data(), H.data());
        rc |= smg_membrane_faces_host_material(V0.data(), P.data(), nV, F.data(), nF, &prm, material, 1, W2.data(), G2.data(), H2.data());
        if (rc != SMG_OK) { std::printf("material %d: rc %d (%s)\n", material, rc, smg_last_error()); failures++; continue; }
        int zero = 0;
        for (int f = 0; f < nF; f++) {
            if (W0[f] != W1[f] || W0[f] != W2[f]) { std::printf("material %d face %d: the energy differs between the modes\n", material, f); failures++; }
            if (!std::isfinite(W0[f])) { std::printf("material %d face %d: W is not finite\n", material, f); failures++; }
            zero += W0[f] == 0.0;
        }
        for (size_t e = 0; e < H2.size(); e++)
            if (!std::isfinite(H2[e])) { std::printf("material %d: a non-finite fixed entry\n", material); failures++; break; }
        std::printf("material %d: %d faces, %d with W == 0\n", material, nF, zero);
    }
    std::vector<double> W(nF);
    for (int bad : {-1, 3})
        if (smg_membrane_faces_host_material(V0.data(), P.data(), nV, F.data(), nF, &prm, bad, 0, W.data(), nullptr, nullptr) != SMG_ERR_INVALID) {
            std::printf("material %d was not refused\n", bad);
            failures++;
        }
    if (smg_membrane_set_material(nullptr, 1) != SMG_ERR_INVALID || smg_membrane_material(nullptr) != 0) failures++;
    std::printf(failures ? "MEMBRANE_MATERIAL_DRIVER FAILED\n" : "MEMBRANE_MATERIAL_DRIVER OK\n");
    return failures ? 1 : 0;
}
