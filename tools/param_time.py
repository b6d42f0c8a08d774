#!/usr/bin/env python3
"""Disk parameterization (smg_param_harmonic / smg_param_arap) on one GPU: time per harmonic map and per ARAP iteration, loop entries of the
solves, the stationary loop against PCG, and the host path the library offered before the object.

    python tools/param_time.py [--legs ogre,ogre2] [--iters 10] [--reps 5] [--host-iters 3]

ogre: ogre.obj (19 985 vertices, a disk with a 112-edge boundary loop) with the reference's hierarchy (mg_precompute(V, F, 0.25, 500, 1));
ogre2: its 2x subdivision through mg_precompute_subdiv (about 320 k vertices; the boundary survives subdivision).  Default inner options
(tolerance 1e-8 s).  Per leg and inner solver: ms per harmonic map, ms per --iters-iteration call from the harmonic map held on the device
(median of --reps, host clock around a call between device blocks that ends in a synchronise), the same per iteration, the call with 0
iterations (set-up + one local step), loop entries per solve.  Host path: the local step of tests/test_param_host.py in numpy, the global step
by Hierarchy.solve_pcg on host blocks, per iteration.  Also prints the algorithmic bytes of the kernels (the byte model of DESIGN.md section 22)."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def legs(name, smg, M):
    V, F = M.read_smgm("ogre.smgm")
    V = M.normalize_unit_area(V, F)
    if name == "ogre":
        mg = smg.mg_precompute(V, F, 0.25, 500, 1)
        return "ogre.obj (%d levels)" % mg.n_levels, mg, V, F
    mg, Vf, Ff = smg.mg_precompute_subdiv(V, F, 2, ratio=0.25, nVCoarsest=500)
    return "ogre.obj x2 subdivision (%d levels)" % mg.n_levels, mg, Vf, Ff


def median_ms(fn, reps, sync):
    ts = []
    for rep in range(reps + 1):
        sync()
        t1 = time.perf_counter()
        out = fn()
        sync()
        if rep:
            ts.append(1e3 * (time.perf_counter() - t1))
    return float(np.median(ts)), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="ogre,ogre2")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-iters", type=int, default=3, help="iterations of the host path (0: skip it)")
    args = ap.parse_args()
    import torch
    import surface_multigrid_code_amd as smg
    from surface_multigrid_code_amd import mesh
    from oracle import mesh_np as M
    import test_param_host as T
    sync = torch.cuda.synchronize
    for name in args.legs.split(","):
        label, mg, V, F = legs(name, smg, M)
        t0 = time.perf_counter()
        par = smg.Parameterizer(mg, V, F)
        t_create = time.perf_counter() - t0
        n, nF, loop = V.shape[0], F.shape[0], par.boundary()
        print("%s: nV = %d, nF = %d, boundary loop %d, create %.2f s" % (label, n, nF, loop.size, t_create), flush=True)
        Hd = torch.empty((2, n), dtype=torch.float64, device="cuda")
        Ud = torch.empty((2, n), dtype=torch.float64, device="cuda")
        for pcg in (1, 0):
            par.set_solver(pcg)
            tag = "PCG" if pcg else "stationary"
            med, cyc = median_ms(lambda: par.harmonic_device(Hd.data_ptr()), args.reps, sync)
            print("  %-10s harmonic map   %9.3f ms / call   loop entries %d" % (tag, med, cyc), flush=True)
            for iters in (args.iters, 0):
                med, (E, cyc) = median_ms(lambda: par.flatten_device(Ud.data_ptr(), UV0_ptr=Hd.data_ptr(), max_iter=iters), args.reps, sync)
                if iters:
                    print("  %-10s %2d iterations  %9.3f ms / call  %8.3f ms / iteration   loop entries %s   E %.4e -> %.4e"
                          % (tag, iters, med, med / iters, list(map(int, cyc)), E[0], E[-1]), flush=True)
                else:
                    print("  %-10s  0 iterations  %9.3f ms / call  (set-up, one local step, UV written)" % (tag, med), flush=True)
        par.set_solver(1)
        U = Ud.cpu().numpy().T.copy()
        sigma, stats = par.distortion(U)
        print("  distortion after %d iterations: %s" % (args.iters, stats), flush=True)
        if args.host_iters:
            # the host path: numpy's local step, the global step through the hierarchy on host blocks
            ref = T.ParamNp(V, F)
            mg.precompute(-mesh.cotmatrix(V, F), loop[:1])
            opts = smg.SolveOpts(tol=1e-8 * ref.scale(), max_iter=50)
            Uh = Hd.cpu().numpy().T.copy()
            t_local, t_solve, entries = [], [], []
            for _ in range(args.host_iters):
                t1 = time.perf_counter()
                cs, sn, E = ref.local(Uh)
                b = T.rhs(ref.r, ref.F, n, cs, sn)
                t2 = time.perf_counter()
                conv, Uh, his = mg.solve_pcg(b, Uh, Uh[loop[:1]], opts)
                t3 = time.perf_counter()
                t_local.append(1e3 * (t2 - t1))
                t_solve.append(1e3 * (t3 - t2))
                entries.append(len(his))
            print("  host path  %2d iterations  local step (numpy) %8.1f ms, global step (Hierarchy.solve_pcg, host blocks) %8.3f ms / iteration   "
                  "loop entries %s" % (args.host_iters, np.median(t_local), np.median(t_solve), entries), flush=True)
        # byte model: every array the kernel needs, once
        local = 12 * nF + 48 * nF + 16 * n + 16 * nF + 8 * nF              # F, rest, UV in; R, the energy term out
        rhs = 4 * (n + 1) + 12 * nF + 48 * nF + 16 * nF + 16 * n             # corner lists, rest, R in (a face's are gathered by its three corners); B out
        dist = 12 * nF + 48 * nF + 16 * n + 16 * nF + 56 * nF                # F, rest, UV in; sigma and the 7 planes of terms out
        print("  algorithmic bytes per launch: k_param_local %.1f MB, k_param_rhs %.1f MB, k_param_distortion %.1f MB"
              % (local / 1e6, rhs / 1e6, dist / 1e6), flush=True)
        print("  device memory of the object: %.1f MB" % (par.device_bytes() / 1e6), flush=True)
        del par, mg


if __name__ == "__main__":
    main()
