#!/usr/bin/env python3
"""MG (smg_solve) against V-cycle-preconditioned CG (smg_solve_pcg) on one GPU, the same handle, solves alternating.

    python tools/pcg_time.py [--reps 5] [--legs bunny,ogre,C3,C3dec]

Legs: bunny.obj and ogre.obj with the reference's hierarchy (mg_precompute(V, F, 0.25, 200, 1)), Poisson (boundary / pinned vertices) and
mean-curvature-flow systems; C3 (subdivision hierarchy) and C3dec (the reference's hierarchy of the C3 mesh), mean-curvature flow; each at
tol 1e-3 and 1e-10, k = 1 and 3 columns.  Per leg and method: history entries, ms per iteration (solve / (entries - 1)) and ms per solve (median
of --reps, host clock around a synchronised solve on HBM-resident vectors), and max over columns of |z_pcg - z_mg| / |z_mg|."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def problems(name, smg, mesh, M):
    """yields (label, mg, A, RHS builder(k), known)"""
    import bench
    if name in ("bunny", "ogre"):
        V, F = M.read_smgm(name + ".smgm")
        V = M.normalize_unit_area(V, F)
        mg = smg.mg_precompute(V, F, 0.25, 200, 1)
        L = M.cotmatrix(V, F)
        n = V.shape[0]
        Mb = M.massmatrix(V, F, "barycentric")
        A = (Mb - 0.01 * L).tocsr()
        A.sort_indices()
        yield "%s.obj mcf (%d levels)" % (name, mg.n_levels), mg, A, (lambda k: Mb @ np.random.default_rng(1).uniform(-1, 1, (n, k))), None
        Ap = (-L).tocsr()
        Ap.sort_indices()
        known = M.boundary_loop(F)
        if len(known) == 0:
            known = np.sort(np.random.default_rng(0).choice(n, 8, replace=False)).astype(np.int32)
        mv = M.massmatrix(V, F, "voronoi") @ np.ones(n)
        yield "%s.obj poisson (%d levels)" % (name, mg.n_levels), mg, Ap, (lambda k: np.repeat(mv[:, None], k, axis=1) * np.linspace(0.5, 1.5, k)[None]), known
    else:
        mg, A, Mb, Vf, Ff, label, _ = bench.build_workload(name, smg, mesh)
        n = A.shape[0]
        yield "%s mcf (%d levels)" % (name, mg.n_levels), mg, A, (lambda k: Mb @ np.random.default_rng(1).uniform(-1, 1, (n, k))), None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--legs", default="bunny,ogre,C3,C3dec")
    args = ap.parse_args()
    import torch
    import surface_multigrid_code_amd as smg
    from surface_multigrid_code_amd import mesh
    from oracle import mesh_np as M
    dev = torch.device("cuda", 0)
    print("%-34s %5s %2s | %7s %9s %9s | %7s %9s %9s | %9s %s" % ("leg", "tol", "k", "MG ent", "ms/iter", "ms/solve", "PCG ent", "ms/iter", "ms/solve",
                                                               "dz rel", "PCG/MG solve"), flush=True)
    for name in args.legs.split(","):
        for label, mg, A, rhs_of, known in problems(name, smg, mesh, M):
            mg.precompute(A, known)
            n = A.shape[0]
            for k in (1, 3):
                R = np.asfortranarray(rhs_of(k))
                kv = None
                if known is not None:
                    R[known] = 0.0
                    kv = torch.zeros((k, len(known)), dtype=torch.float64, device=dev)
                rhs = torch.from_numpy(np.ascontiguousarray(R.T)).to(dev)      # column-major n x k
                z0 = torch.zeros((k, n), dtype=torch.float64, device=dev)
                for tol in (1e-3, 1e-10):
                    o = smg.SolveOpts(tol=tol, max_iter=400)
                    zs = {m: torch.empty((k, n), dtype=torch.float64, device=dev) for m in ("mg", "pcg")}
                    fn = {"mg": mg.solve_device, "pcg": mg.solve_pcg_device}
                    t = {"mg": [], "pcg": []}
                    his = {}
                    for rep in range(args.reps + 1):
                        for m in ("mg", "pcg"):
                            torch.cuda.synchronize()
                            t0 = time.perf_counter()
                            conv, h = fn[m](rhs.data_ptr(), z0.data_ptr(), zs[m].data_ptr(), n, k, kv.data_ptr() if kv is not None else None,
                                            len(known) if known is not None else 0, opts=o)
                            torch.cuda.synchronize()
                            if rep > 0:
                                t[m].append(1e3 * (time.perf_counter() - t0))
                            his[m] = (conv, h)
                    zm, zp = zs["mg"].cpu().numpy(), zs["pcg"].cpu().numpy()
                    dz = max(np.linalg.norm(zp[c] - zm[c]) / max(np.linalg.norm(zm[c]), 1e-300) for c in range(k))
                    row = []
                    for m in ("mg", "pcg"):
                        ent = len(his[m][1])
                        ms = float(np.median(t[m]))
                        row += [("%d%s" % (ent, "" if his[m][0] else "!")), ms / max(ent - 1, 1), ms]
                    print("%-34s %5.0e %2d | %7s %9.3f %9.3f | %7s %9.3f %9.3f | %9.2e %.2f" % (label, tol, k, row[0], row[1], row[2], row[3], row[4], row[5],
                                                                                          dz, row[5] / row[2]), flush=True)
            del mg


if __name__ == "__main__":
    main()
