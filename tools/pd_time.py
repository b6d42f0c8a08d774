#!/usr/bin/env python3
"""Projective-dynamics membrane steps (smg_pd_step) on one GPU: ms per step and per iteration, loop entries of the inner solves, the stationary
loop against PCG, beside the neo-Hookean implicit-Euler step of smg_membrane_step (tools/membrane_time.py's measurement) in the same session.

    python tools/pd_time.py [--legs bunny,bunny2] [--iters 10] [--reps 5] [--no-membrane]

bunny: bunny_15K_init (15 804 vertices) after normalize_unit_area, the scalar hierarchy of mg_precompute(V, F, 0.25, 500, 1); bunny2: its 2 x
mid-point subdivision (252 834 vertices), the same builder.  The step: dt = 1e-2, density = stiffness = 1, band (1, 1), pressure 5, default
inner options (tolerance 1e-8 |b_0|).  Every timed step starts from the rest pose at zero velocity (so all repetitions do the same work);
median of --reps after a warm-up step, host clock around a call that ends in a synchronise.  The membrane rows: the defaults of
smg_membrane_params on the block hierarchy of mg_precompute_block, stationary loop and PCG, as tools/membrane_time.py runs them.  The two
steppers integrate different materials at different step sizes: the rows are costs per call, not a comparison of equal work.
Also prints the algorithmic bytes of the kernels (the byte model of DESIGN.md section 23)."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def median_ms(fn, reset, reps):
    ts, out = [], None
    for rep in range(reps + 1):
        reset()
        t1 = time.perf_counter()
        out = fn()
        if rep:
            ts.append(1e3 * (time.perf_counter() - t1))
    return float(np.median(ts)), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="bunny,bunny2")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-membrane", action="store_true", help="skip the smg_membrane_step rows")
    args = ap.parse_args()
    import surface_multigrid_code_amd as smg
    from oracle import mesh_np as M
    for name in args.legs.split(","):
        V, F = M.read_smgm("bunny_15K_init.smgm")
        if name == "bunny2":
            V, F, _ = M.subdivision_hierarchy(V, F, 2)
            V, F = np.ascontiguousarray(V), np.ascontiguousarray(F, dtype=np.int32)
        Vn = M.normalize_unit_area(V, F)
        n, nF = V.shape[0], F.shape[0]
        t0 = time.perf_counter()
        mg = smg.mg_precompute(Vn, F, 0.25, 500, 1)
        t_h = time.perf_counter() - t0
        t0 = time.perf_counter()
        pd = smg.ProjectiveDynamics(mg, Vn, F, pressure=5.0)
        t_c = time.perf_counter() - t0
        print("%s: %d vertices, %d faces, %d levels; hierarchy %.2f s, create (one precompute) %.2f s, device memory of the object %.1f MB"
              % (name, n, nF, mg.n_levels, t_h, t_c, pd.device_bytes() / 1e6), flush=True)
        zero = np.zeros_like(Vn)
        for pcg in (1, 0):
            pd.set_solver(pcg)
            tag = "PCG" if pcg else "stationary"
            for iters in (args.iters, 0):
                med, (E, cyc) = median_ms(lambda: pd.step(max_iter=iters), lambda: pd.set_state(Vn, zero), args.reps)
                if iters:
                    print("  pd %-10s %2d iterations  %9.3f ms / step  %8.3f ms / iteration   loop entries %s   E %.4e -> %.4e"
                          % (tag, iters, med, med / iters, list(map(int, cyc)), E[0], E[-1]), flush=True)
                else:
                    print("  pd %-10s  0 iterations  %9.3f ms / step  (forces, prediction, one local step, finish)" % (tag, med), flush=True)
        # byte model: every array the kernel needs, once
        faces = 12 * nF + 32 * nF + 24 * n + 8 * nF + 72 * nF                    # F, rest, Q in; the energy term and the 9 shares out
        verts = 4 * (n + 1) + 12 * nF + 72 * nF + 8 * n + 48 * n + 24 * n + 16 * n   # corner lists, shares, m0, S and Q in; B and the two terms out
        predict = 72 * n + 8 * n + 24 * n                                        # x, vel, fext, m0 in; S out
        finish = 24 * n + 24 * n + 48 * n                                        # Q, x in; x, vel out
        print("  algorithmic bytes per launch: k_pd_faces<0> %.1f MB, k_pd_vertices %.1f MB, k_pd_predict %.1f MB, k_pd_finish %.1f MB"
              % (faces / 1e6, verts / 1e6, predict / 1e6, finish / 1e6), flush=True)
        del pd, mg
        if args.no_membrane:
            continue
        mgb = smg.mg_precompute_block(V, F)
        sim = smg.MembraneSim(mgb, V, F)
        for pcg in (0, 1):
            sim.set_solver(pcg)
            med, r = median_ms(lambda: sim.step(), lambda: sim.set_state(), args.reps)
            print("  membrane (neo-Hookean, %s) %9.3f ms / step  (%d Newton iterations, loop entries %s)"
                  % ("PCG" if pcg else "stationary", med, len(r["cycles"]), list(map(int, r["cycles"]))), flush=True)
        del sim, mgb


if __name__ == "__main__":
    main()
