#!/usr/bin/env python3
"""Membrane time steps (smg_membrane_step; neo-Hookean, StVK or tension-field StVK) on one GPU: ms per step, loop entries of the solves, and the same step on the path a block
caller had before -- H assembled on the host (the numpy restatement of tests/test_membrane_host.py) and handed to smg_precompute.

    python tools/membrane_time.py [--legs bunny,bunny2] [--materials neo_hookean,stvk,tension_field] [--reps 5] [--host-iters 2]

One process measures every requested material on one object per mesh (smg_membrane_set_material between the runs), so the neo-Hookean row of
a session is the yardstick of the other two.  The host-assembly path is timed for the neo-Hookean material only.

bunny: bunny_15K_init (15 804 vertices, the reference's mesh) with mg_precompute_block's defaults; bunny2: its 2 x mid-point subdivision
(252 834 vertices), the same builder.  The reference's configuration: defaults of smg_membrane_params, tol = 2e-1, the stationary loop, ten
Newton iterations.  Every timed step starts from the rest pose at zero velocity (so all repetitions do the same work); median of --reps after
a warm-up step, host clock around a call that ends in a synchronise.  The host path runs --host-iters Newton iterations of the same step
(assembly in numpy, smg_precompute from the host, the device solve, the line search in numpy) and prints each stage per iteration."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="bunny,bunny2")
    ap.add_argument("--materials", default="neo_hookean", help="comma-separated: neo_hookean, stvk, tension_field")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-iters", type=int, default=2, help="Newton iterations of the host-assembly path to time (0: skip it)")
    args = ap.parse_args()
    import surface_multigrid_code_amd as smg
    from oracle import mesh_np as M
    from test_membrane_host import MembraneNp
    for name in args.legs.split(","):
        V, F = M.read_smgm("bunny_15K_init.smgm")
        if name == "bunny2":
            V, F, _ = M.subdivision_hierarchy(V, F, 2)
            V, F = np.ascontiguousarray(V), np.ascontiguousarray(F, dtype=np.int32)
        t0 = time.perf_counter()
        mg = smg.mg_precompute_block(V, F)
        t_h = time.perf_counter() - t0
        t0 = time.perf_counter()
        sim = smg.MembraneSim(mg, V, F)
        t_c = time.perf_counter() - t0
        nV, nF = V.shape[0], F.shape[0]
        print("%s: %d vertices, %d faces, %d levels; hierarchy %.2f s, create %.2f s, device memory of the object %.1f MB"
              % (name, nV, nF, mg.n_levels, t_h, t_c, sim.device_bytes() / 1e6), flush=True)
        for material in args.materials.split(","):
            sim.set_material(material)
            for pcg in (0, 1):
                sim.set_solver(pcg)
                ts, r = [], None
                for rep in range(args.reps + 1):
                    sim.set_state()
                    t1 = time.perf_counter()
                    r = sim.step()
                    if rep:
                        ts.append(1e3 * (time.perf_counter() - t1))
                n_it = len(r["cycles"])
                print("  %-13s %-10s %9.3f ms / step (min %.3f, max %.3f), %.3f ms / Newton iteration  loop entries %s  alpha %s  objective %.10e -> %.10e"
                      % (material, "PCG" if pcg else "stationary", np.median(ts), min(ts), max(ts), np.median(ts) / max(n_it, 1), list(map(int, r["cycles"])),
                         [float(a) for a in r["alpha"]], r["objective"][0], r["objective"][-1]), flush=True)
        sim.set_material("neo_hookean")
        sim.set_solver(0)
        # byte model of the eigen-fix kernel: F, nine corner coordinates, the rest constants in; W, G, H out
        faces = 12 * nF + 72 * nF + 40 * nF + 8 * nF * 55
        print("  algorithmic bytes per launch: k_membrane_faces<2> %.1f MB (of which %.1f MB the 45 Hessian planes)" % (faces / 1e6, 360 * nF / 1e6), flush=True)
        if args.host_iters > 0:
            mb = MembraneNp(V, F)
            mg2 = smg.mg_precompute_block(V, F)
            stage = dict(assemble=0.0, precompute=0.0, solve=0.0)
            opts = smg.SolveOpts(tol=2e-1, max_iter=20)
            orig = mb.system

            def timed_system(*a):
                t = time.perf_counter()
                out = orig(*a)
                stage["assemble"] += time.perf_counter() - t
                return out

            def solve(H, b):
                t = time.perf_counter()
                mg2.precompute(H)
                stage["precompute"] += time.perf_counter() - t
                t = time.perf_counter()
                _, z, _ = mg2.solve(b.reshape(-1, 1), np.zeros((b.size, 1)), None, opts)
                stage["solve"] += time.perf_counter() - t
                return z[:, 0]

            mb.system = timed_system
            mb.step(V.copy(), np.zeros(3 * nV), newton_iters=1, solve=solve)              # warm-up: the pattern-setting precompute
            for k in stage:
                stage[k] = 0.0
            t1 = time.perf_counter()
            mb.step(V.copy(), np.zeros(3 * nV), newton_iters=args.host_iters, solve=solve)
            total = 1e3 * (time.perf_counter() - t1) / args.host_iters
            print("  host assembly path, per Newton iteration: %.1f ms (numpy assembly %.1f, smg_precompute from the host %.1f, solve %.1f, the rest"
                  " is the numpy line search)" % (total, *(1e3 * stage[k] / args.host_iters for k in ("assemble", "precompute", "solve"))), flush=True)
            del mg2
        del sim, mg


if __name__ == "__main__":
    main()
