#!/usr/bin/env python3
"""As-rigid-as-possible deformation (smg_arap_solve) on one GPU: time per call and per iteration, loop entries of the inner solves, the
stationary loop against PCG.

    python tools/arap_time.py [--legs bunny,C3] [--iters 10] [--reps 5] [--stationary 1]

bunny: bunny.obj with the reference's hierarchy (mg_precompute(V, F, 0.25, 200, 1)); C3: the bunny_15K_init x3 subdivision hierarchy of
bench.py (1 011 330 vertices).  Deformation: the twist of tests/test_arap_host.py -- handles = the lowest and highest 5 % of the vertices along
the longest bounding-box axis, the top set rotated by 60 degrees about that axis and shifted by 15 % of the extent -- from the rest pose, default
inner options (tolerance 1e-8 s).  Per leg and inner solver: ms per --iters-iteration call (median of --reps, host clock around a call between
device blocks that ends in a synchronise), the same per iteration, the call with 0 iterations (set-up + one local step), loop entries per solve.
Also prints the algorithmic bytes of the two gather kernels (the byte model of DESIGN.md section 19) for the rates under rocprofv3."""
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
        V = M.normalize_unit_area(V, F)
        mg = smg.mg_precompute(V, F, 0.25, 200, 1)
        return "bunny.obj (%d levels)" % mg.n_levels, mg, V, F
    mg, A, Mb, Vf, Ff, label, _ = bench.build_workload(name, smg, mesh)
    return label, mg, Vf, Ff


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="bunny,C3")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--stationary", type=int, default=1, help="also time the stationary loop as the inner solver (0: PCG, the default, only)")
    args = ap.parse_args()
    import torch
    import surface_multigrid_code_amd as smg
    from surface_multigrid_code_amd import mesh
    from oracle import mesh_np as M
    from test_arap_host import twist
    for name in args.legs.split(","):
        label, mg, V, F = legs(name, smg, mesh, M)
        handles, hp = twist(V)
        t0 = time.perf_counter()
        arap = smg.ArapDeformer(mg, V, F, handles)
        t_create = time.perf_counter() - t0
        n, nh = V.shape[0], handles.size
        nnz = int(mesh.cotmatrix(V, F).nnz)
        print("%s: n = %d, nnz(L) = %d, %d handles, create %.2f s" % (label, n, nnz, nh, t_create), flush=True)
        hpd = torch.from_numpy(np.ascontiguousarray(hp.T)).cuda()
        Ud = torch.empty((3, n), dtype=torch.float64, device="cuda")
        for pcg in ((1, 0) if args.stationary else (1,)):
            arap.set_solver(pcg)
            for iters in (args.iters, 0):
                ts = []
                for rep in range(args.reps + 1):
                    torch.cuda.synchronize()
                    t1 = time.perf_counter()
                    E, cyc = arap.deform_device(hpd.data_ptr(), Ud.data_ptr(), max_iter=iters)
                    torch.cuda.synchronize()
                    if rep:
                        ts.append(1e3 * (time.perf_counter() - t1))
                med = np.median(ts)
                if iters:
                    print("  %-10s %2d iterations  %9.3f ms / call  %8.3f ms / iteration   loop entries %s   E %.4e -> %.4e"
                          % ("PCG" if pcg else "stationary", iters, med, med / iters, list(map(int, cyc)), E[0], E[-1]), flush=True)
                else:
                    print("  %-10s  0 iterations  %9.3f ms / call  (set-up, one local step, U written)" % ("PCG" if pcg else "stationary", med), flush=True)
        arap.set_solver(1)
        # byte model: every array the kernel needs, once.  rotations: rowptr, col, w, P0, P in; R, the energy term out.  rhs: rowptr, col, w, P0, R in; b out.
        rot = 4 * (n + 1) + 12 * nnz + 24 * n + 24 * n + 72 * n + 8 * n
        rhs = 4 * (n + 1) + 12 * nnz + 24 * n + 72 * n + 24 * n
        print("  algorithmic bytes per launch: k_arap_rotations %.1f MB, k_arap_rhs %.1f MB" % (rot / 1e6, rhs / 1e6), flush=True)
        print("  device memory of the object: %.1f MB" % (arap.device_bytes() / 1e6), flush=True)
        del arap, mg


if __name__ == "__main__":
    main()
