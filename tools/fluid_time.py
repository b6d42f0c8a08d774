#!/usr/bin/env python3
"""Time of a step of the device-resident surface fluid (smg_fluid_*, Python SurfaceFluid) for k = 1, 8, 32 simulations, with the default
parameters (central flux, three stages, the adaptive step at cfl = 0.5) and the default options (PCG, tol = 1e-10 |rhs|_F).

    python tools/fluid_time.py [workload] [reps]

Host clock: the median over `reps` calls of N_STEPS steps each after one call that is dropped, divided by N_STEPS; a call's fixed cost is one copy of
the histories.  The initial vorticity is z plus a column-dependent smooth field, so the columns are k different flows.

The split of a step into its solves and its own kernels comes from the same clock: with opts.max_iter = 0 every solve returns its start, so a
step is its kernels, reductions, copies and the host's round trips alone ("without solves"); the difference to the full step is the solves.

Per kernel: smg_debug_fluid_time launches one launcher alone, 20 times back to back between two events, on blocks of zeros of the same shapes;
the line gives the mean time of a launch and the launcher's algorithmic bytes over it (every operand once, from the shapes: per (vertex,
column) k_fluid_rhs reads w and writes r and its square, k_fluid_advect reads psi, w and w_n and writes out, the rate and m out -- rates only:
psi and the rate --; once per launch the corner lists (4 n + 12 nF), the faces (12 nF) and m; k_fluid_velocity reads 13 doubles and the
three indices of a face once per launch and psi once per (vertex, column), and writes 32 bytes per (face, column)).  Sets no threshold."""
import argparse
import ctypes as C
import os
import sys
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

N_STEPS = 10
KS = (1, 8, 32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("workload", nargs="?", default="C3")
    ap.add_argument("reps", nargs="?", type=int, default=5)
    args = ap.parse_args()
    import bench as B
    import surface_multigrid_code_amd as smg
    from surface_multigrid_code_amd import mesh
    mg, A, Mb, V, F, label, _ = B.build_workload(args.workload, smg, mesh)
    n, nF = V.shape[0], F.shape[0]
    L = smg._lib.load()
    Vc, Fc = np.ascontiguousarray(V, dtype=np.float64), np.ascontiguousarray(F, dtype=np.int32)

    def timed(fn):
        t0 = time.perf_counter()
        out = fn()
        return time.perf_counter() - t0, out

    t_create, obj = timed(lambda: smg.SurfaceFluid(mg, V, F))
    print(label)
    print("  create (geometry, masses, assemble L, clone, precompute): %.1f ms; closed %s" % (1e3 * t_create, obj.closed), flush=True)
    span = float(np.max(V.max(axis=0) - V.min(axis=0)))
    for k in KS:
        s = np.arange(k)[None, :]
        w0 = V[:, [2]] / span + 0.5 * np.sin((3.0 + s) * V[:, [0]] / span) * np.cos((2.0 + 0.5 * s) * V[:, [1]] / span)
        obj.set_vorticity(w0)
        ts, cyc, cfl = [], None, None
        for _ in range(args.reps + 1):
            t, (cfl, tm, cyc) = timed(lambda: obj.step(N_STEPS))
            ts.append(t)
        per = 1e3 * float(np.median(ts[1:])) / N_STEPS
        d = obj.diagnostics()
        none = smg.SolveOpts(tol=0.0, max_iter=0)                              # (the state that these steps leave is not a flow's: timed, then dropped)
        bare = 1e3 * float(np.median([timed(lambda: obj.step(N_STEPS, opts=none))[0] for _ in range(args.reps + 1)][1:])) / N_STEPS
        print("  k = %2d: %.3f ms per step (%.3f per simulation), %.3f without solves: the solves' share %.1f %%" % (k, per, per / k, bare, 100.0 * (per - bare) / per),
              flush=True)
        geometry = 4 * n + 24 * nF + 8 * n
        for name, op, ro, nbytes in (("k_fluid_rhs", 0, 0, 24 * n * k + 12 * n), ("k_fluid_advect<false>", 1, 0, 48 * n * k + geometry),
                                     ("k_fluid_advect<true>", 1, 1, 16 * n * k + geometry), ("k_fluid_diag", 3, 0, 24 * n * k + 8 * n),
                                     ("k_fluid_velocity", 2, 0, 116 * nF + 8 * n * k + 32 * nF * k)):
            ms = C.c_double(0.0)
            rc = L.smg_debug_fluid_time(op, n, nF, k, Fc.ctypes.data_as(C.POINTER(C.c_int)), Vc.ctypes.data_as(C.POINTER(C.c_double)), ro, 20, C.byref(ms))
            assert rc == 0, L.smg_last_error()
            print("          %-22s %.4f ms a launch, %7.1f MB, %5.0f GB/s" % (name, ms.value, nbytes / 1e6, nbytes / ms.value / 1e6), flush=True)
        print("          solve loop entries per step %.1f; cfl %.3f .. %.3f; enstrophy[0] %.6f energy[0] %.6f; "
              "device bytes %.1f MB" % (float(np.mean(cyc)), cfl.min(), cfl.max(), d["enstrophy"][0], d["energy"][0],
                                        obj.device_bytes() / 1e6), flush=True)


if __name__ == "__main__":
    main()
