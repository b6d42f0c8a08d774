// examples/06_balloon_sim.cpp -- the reference's 06_example_balloon_sim/main.cpp on libsmg, without the viewer: a closed neo-Hookean
// membrane inflated by a pressure force, implicit Euler in time, every Newton system solved by the surface multigrid V-cycle on the 3-DOF
// hierarchy (mg_precompute_block).  Energy, gradient, Hessian, the per-face eigenvalue fix, assembly and the line search run on the device;
// the matrix keeps its sparsity, so every precompute after the first is value-only.
//
//   ./06_balloon_sim tests/golden/meshes/bunny_15K_init.smgm [steps] [matid]      matid (main.cpp:92-101): 0 neo-Hookean (default), 1 StVK,
//                                                                               2 tension-field StVK
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../surface_multigrid_code_amd/csrc/mg_api.hpp"

int main(int argc, char* argv[])
{
    const char* path = argc > 1 ? argv[1] : "tests/golden/meshes/bunny_15K_init.smgm";
    const int steps = argc > 2 ? std::atoi(argv[2]) : 2;      // numSteps + 1 (main.cpp:109, :159)
    double* Vp = nullptr; int* Fp = nullptr; int nV = 0, nF = 0;
    if (smg_mesh_read(path, &Vp, &nV, &Fp, &nF) != SMG_OK) { std::fprintf(stderr, "%s\n", smg_last_error()); return 1; }
    smgDense origV(nV, 3); smgDenseI F(nF, 3);
    for (int i = 0; i < nV; i++) for (int c = 0; c < 3; c++) origV(i, c) = Vp[3 * i + c];
    for (int i = 0; i < nF; i++) for (int c = 0; c < 3; c++) F(i, c) = Fp[3 * i + c];
    std::printf("original mesh: |V| %d, |F|: %d\n", nV, nF);

    std::vector<mg_data> mg;
    mg_precompute_block(origV, F, mg);                          // main.cpp:171
    std::printf("numLv: %d\n", (int)mg.size());

    balloon_sim_data sim;                                       // thickness 0.1, poisson 0.5, young 6e6, M = 1000 * lumped mass, dt = 1e-3
    if (argc > 3) sim.material = std::atoi(argv[3]);
    balloon_sim_precompute(origV, F, mg, sim);
    const double mg_tolerance = 2e-1;
    smgDense curPos = origV;
    std::vector<double> qdot((size_t)nV * 3, 0.0);
    for (int j = 0; j < steps; j++) {
        std::printf("iter: %d\n", j);
        implicit_euler_mg_balloon(sim, curPos, qdot, mg_tolerance);
        for (int i = 0; i < sim.params.newton_iters; i++)
            std::printf("newton %d: objective %.15g alpha: %g cycles: %d\n", i, sim.objective[i], sim.alpha[i], sim.cycles[i]);
        double disp = 0.0;
        for (int i = 0; i < nV; i++) for (int c = 0; c < 3; c++) disp = std::fmax(disp, std::fabs(curPos(i, c) - origV(i, c)));
        std::printf("step %d: objective %.15g max displacement %.6e\n", j, sim.objective[sim.params.newton_iters], disp);
    }
    smg_free(Vp); smg_free(Fp);
    return 0;
}
