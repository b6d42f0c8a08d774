#!/usr/bin/env python3
"""Heat-method geodesic queries (smg_geodesics_solve) on one GPU: time per query, cycles per stage, PCG against the stationary loop.

    python tools/geodesics_time.py [--legs C3,bunny] [--ks 1,8,64] [--reps 5]

C3: the bunny_15K_init x3 subdivision hierarchy of bench.py (1 011 330 vertices); bunny: bunny.obj with the reference's hierarchy
(mg_precompute(V, F, 0.25, 200, 1)).  Per leg, k (single-source sets, sources spread over the mesh) and stage solver (PCG / stationary):
loop entries of the heat and the Poisson solve and ms per query (median of --reps, host clock around a query that writes D to HBM).
Also prints the object's device memory and, for the fused divergence kernel, its algorithmic bytes per query (geometry once: F, W, A_f, the
corner lists; u once and -div once per column) -- divide by the kernel's time from `rocprofv3 --kernel-trace --stats` for the rate."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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
    ap.add_argument("--legs", default="C3,bunny")
    ap.add_argument("--ks", default="1,8,64")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--stationary", type=int, default=1, help="also time the stationary loop (0: PCG only)")
    args = ap.parse_args()
    import torch
    import surface_multigrid_code_amd as smg
    from surface_multigrid_code_amd import mesh
    from oracle import mesh_np as M
    for name in args.legs.split(","):
        label, mg, V, F = legs(name, smg, mesh, M)
        t0 = time.perf_counter()
        geo = smg.HeatGeodesics(mg, V, F)
        t_create = time.perf_counter() - t0
        n, nF = V.shape[0], F.shape[0]
        print("%s: n = %d, nF = %d, t = %.4g, create %.2f s" % (label, n, nF, geo.t, t_create), flush=True)
        for k in [int(x) for x in args.ks.split(",")]:
            sets = [[int(s)] for s in np.linspace(0, n - 1, k).astype(np.int64)]
            D = torch.empty((k, n), dtype=torch.float64, device="cuda")
            for pcg in ((1, 0) if args.stationary else (1,)):
                geo.set_solver(pcg, pcg)
                ts = []
                for rep in range(args.reps + 1):
                    torch.cuda.synchronize()
                    t1 = time.perf_counter()
                    cyc = geo.distance_device(sets, D.data_ptr())
                    torch.cuda.synchronize()
                    if rep:
                        ts.append(1e3 * (time.perf_counter() - t1))
                print("  k = %2d  %-10s heat %3d  poisson %3d entries   %9.2f ms / query  (%.3f ms / source)" %
                      (k, "PCG" if pcg else "stationary", cyc[0], cyc[1], np.median(ts), np.median(ts) / k), flush=True)
            geo.set_solver(1, 1)
            alg = nF * (12 + 72 + 8 + 12) + 4 * (n + 1) + 16 * n * k
            print("  k = %2d  divergence kernel: %.1f MB algorithmic per query" % (k, alg / 1e6), flush=True)
        print("  device memory of the object: %.1f MB (after k = %s)" % (geo.device_bytes() / 1e6, args.ks.split(",")[-1]), flush=True)
        del geo, mg


if __name__ == "__main__":
    main()
