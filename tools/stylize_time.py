#!/usr/bin/env python3
"""Cubic and normal-driven stylization (smg_stylize_run) on one GPU: ms per outer iteration, the local step against smg_arap's, loop entries of
the inner solves and the ADMM statistics of every outer iteration.

    python tools/stylize_time.py [--legs bunny,C3] [--iters 10] [--reps 5] [--lambda 0.2]

bunny: bunny.obj with the reference's hierarchy (mg_precompute(V, F, 0.25, 200, 1)); C3: the bunny_15K_init x3 subdivision hierarchy of
bench.py (1 011 330 vertices).  The mesh is scaled to a unit bounding-box side, vertex 0 is pinned at its rest position, the start is the rest
pose, default parameters and default inner options (tolerance 1e-8 s).  Per leg, between device blocks, median of --reps after a warm-up call,
host clock around a call that ends in a synchronise:
  - the cubic and the normal-driven run with --iters iterations, per call and per iteration, and the call with 0 iterations (set-up, ONE local
    step from the start state -- the most expensive one -- and the energy's sum);
  - smg_arap_solve with the same pin on the same mesh: its iteration has the same right-hand side kernel and the same solve, so the difference
    per iteration is the local step's cost over k_arap_rotations, and the difference of the 0-iteration calls is that of the first local step;
  - the ADMM statistics of the local step of every outer iteration (run t iterations, read smg_stylize_admm_stats: t = 0 .. --iters).
The split of an iteration into k_stylize_local, k_arap_rhs and the solve's kernels is the kernel table of the same command under
`rocprofv3 --kernel-trace --stats -- python tools/stylize_time.py --legs C3`.  Sets no threshold."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def legs(name, smg, mesh, M):
    import bench
    if name == "bunny":
        V, F = M.read_smgm("bunny.smgm")
        mg = smg.mg_precompute(V, F, 0.25, 200, 1)
        return "bunny.obj (%d levels)" % mg.n_levels, mg, V, F
    mg, A, Mb, Vf, Ff, label, _ = bench.build_workload(name, smg, mesh)
    return label, mg, Vf, Ff


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="bunny,C3")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--lambda", dest="lam", type=float, default=0.2)
    args = ap.parse_args()
    import torch
    import surface_multigrid_code_amd as smg
    from surface_multigrid_code_amd import mesh
    from oracle import mesh_np as M
    from stylize_np import cubeness, nearest_axis, unit_box

    def timed(fn):
        ts, out = [], None
        for rep in range(args.reps + 1):
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            if rep:
                ts.append(1e3 * (time.perf_counter() - t1))
        return float(np.median(ts)), out

    for name in args.legs.split(","):
        label, mg, V, F = legs(name, smg, mesh, M)
        V, F = unit_box(np.asarray(V, dtype=np.float64)), np.ascontiguousarray(F, dtype=np.int32)
        n = V.shape[0]
        t0 = time.perf_counter()
        sty = smg.Stylizer(mg, V, F, lambda_=args.lam)
        t_create = time.perf_counter() - t0
        arap = smg.ArapDeformer(mg, V, F, [0])
        print("%s: n = %d, lambda = %g, create %.2f s, device memory of the object %.1f MB" % (label, n, args.lam, t_create, sty.device_bytes() / 1e6), flush=True)
        Ud = torch.empty((3, n), dtype=torch.float64, device="cuda")
        ppd = torch.from_numpy(np.ascontiguousarray(V[:1].T)).cuda()
        rows = {}
        for mode in ("cubic", "normal-driven"):
            sty.set_targets(nearest_axis(sty.normals()[0]) if mode == "normal-driven" else None)
            for iters in (args.iters, 0):
                med, (E, cyc) = timed(lambda: sty.run_device(Ud.data_ptr(), max_iter=iters))
                rows[mode, iters] = med
                if iters:
                    print("  %-13s %2d iterations  %9.3f ms / call  %8.3f ms / iteration   loop entries %s   E %.4e -> %.4e   cubeness %.4f -> %.4f"
                          % (mode, iters, med, med / iters, list(map(int, cyc)), E[0], E[-1], cubeness(V, F), cubeness(Ud.cpu().numpy().T, F)), flush=True)
                else:
                    print("  %-13s  0 iterations  %9.3f ms / call  (set-up, the first local step, U written)" % (mode, med), flush=True)
        sty.set_targets(None)
        for iters in (args.iters, 0):
            med, (E, cyc) = timed(lambda: arap.deform_device(ppd.data_ptr(), Ud.data_ptr(), max_iter=iters))
            rows["arap", iters] = med
            print("  %-13s %2d iterations  %9.3f ms / call  %8.3f ms / iteration   loop entries %s" % ("smg_arap", iters, med, med / max(iters, 1), list(map(int, cyc))),
                  flush=True)
        k = max(args.iters, 1)
        print("  the local step over k_arap_rotations: first (from the start state) %+.3f ms cubic, %+.3f ms normal-driven; per iteration of the run %+.3f ms "
              "cubic, %+.3f ms normal-driven" % (rows["cubic", 0] - rows["arap", 0], rows["normal-driven", 0] - rows["arap", 0],
                                                 (rows["cubic", args.iters] - rows["arap", args.iters]) / k,
                                                 (rows["normal-driven", args.iters] - rows["arap", args.iters]) / k), flush=True)
        for t in range(args.iters + 1):
            sty.run_device(Ud.data_ptr(), max_iter=t)
            st = sty.admm_stats()
            hist = np.bincount(np.minimum(st["iters"], 32), minlength=33)
            waves = st["iters"][:(n // 64) * 64].reshape(-1, 64)
            print("  ADMM, local step %2d: min %d mean %.2f max %d, at the cap %d; per wavefront of 64: mean of the maximum %.2f (lanes busy %.0f %%); "
                  "counts 1 .. 8: %s" % (t, st["min"], st["mean"], st["max"], st["at_cap"], waves.max(axis=1).mean(),
                                         100.0 * waves.mean() / max(waves.max(axis=1).mean(), 1e-300), list(map(int, hist[1:9]))), flush=True)
        del sty, arap, mg


if __name__ == "__main__":
    main()
