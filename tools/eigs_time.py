#!/usr/bin/env python3
"""Timing of smg_eigs (LOBPCG preconditioned by the V-cycle) on one GPU.

    python tools/eigs_time.py [--legs ogre,C3] [--nev 8,16,32] [--reps 3] [--eigsh ogre]

Legs: ogre.obj with the reference's hierarchy (mg_precompute(V, F, 0.25, 200, 1)) and C3 (bench.py's subdivision hierarchy), both with the
mean-curvature-flow system M_bary - 0.01 L and M = M_bary; tol 1e-8 (ogre) and 1e-6 (C3).  Per leg and nev (default block): history rows,
iterations, ms to tolerance (median of --reps, host clock around a synchronised call on HBM-resident mass and X) and ms per iteration.
"host RR" is the median time of the dense generalized eigensolver (smg_debug_dense_geneig_host) at the Rayleigh-Ritz size q = 3 m on this
host, and its share of an iteration.  --eigsh: the legs on which scipy's shift-invert eigsh (a host CPU figure) is timed for context.
For the per-kernel split run it under `rocprofv3 --kernel-trace --stats -- python tools/eigs_time.py ...`."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def problem(name, smg, mesh, M):
    import scipy.sparse as sp
    if name == "ogre":
        V, F = M.read_smgm("ogre.smgm")
        V = M.normalize_unit_area(V, F)
        mg = smg.mg_precompute(V, F, 0.25, 200, 1)
        mass = np.asarray(M.massmatrix(V, F, "barycentric").diagonal())
        A = (sp.diags(mass) - 0.01 * M.cotmatrix(V, F)).tocsr()
        A.sort_indices()
        mg.precompute(A)
        return "ogre.obj mcf (%d levels)" % mg.n_levels, mg, A, mass, 1e-8
    import bench
    mg, A, Mb, Vf, Ff, label, _ = bench.build_workload(name, smg, mesh)
    mg.precompute(A)
    return "%s mcf (%d levels)" % (name, mg.n_levels), mg, A, np.asarray(Mb.diagonal()), 1e-6


def default_block(nev):
    want, b = nev + max(2, nev // 4), 8
    while b < want and b < 64:
        b *= 2
    return b


def host_rr_ms(L, q, reps=5):
    rng = np.random.default_rng(0)
    X = rng.standard_normal((q, q))
    A = np.asfortranarray(X + X.T)
    B = np.asfortranarray(X @ X.T + q * np.eye(q))
    w, V = np.zeros(q), np.zeros((q, q), order="F")
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        L.smg_debug_dense_geneig_host(q, dp(A), dp(B), dp(w), dp(V))
        ts.append(time.perf_counter() - t)
    return 1e3 * float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="ogre,C3")
    ap.add_argument("--nev", default="8,16,32")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--eigsh", default="ogre")
    args = ap.parse_args()
    import torch
    import surface_multigrid_code_amd as smg
    from surface_multigrid_code_amd import _lib, mesh
    from oracle import mesh_np as M
    L = _lib.load()
    print("%-28s %4s %5s | %5s %5s %10s %9s | %9s %7s" % ("leg", "nev", "block", "rows", "iters", "ms/solve", "ms/iter", "host RR", "share"), flush=True)
    for name in args.legs.split(","):
        label, mg, A, mass, tol = problem(name, smg, mesh, M)
        n = A.shape[0]
        dm = torch.tensor(mass, device="cuda")
        for nev in [int(v) for v in args.nev.split(",")]:
            m = default_block(nev)
            dX = torch.zeros((nev, n), dtype=torch.float64, device="cuda")
            opts = smg.SolveOpts(tol=tol, max_iter=300)
            ev, his, nconv = mg.eigs_device(dm.data_ptr(), dX.data_ptr(), n, nev, opts=opts)     # first call: allocations
            ts = []
            for _ in range(args.reps):
                torch.cuda.synchronize()
                t = time.perf_counter()
                ev, his, nconv = mg.eigs_device(dm.data_ptr(), dX.data_ptr(), n, nev, opts=opts)
                torch.cuda.synchronize()
                ts.append(time.perf_counter() - t)
            ms = 1e3 * float(np.median(ts))
            it = his.shape[0] - 1
            rr = host_rr_ms(L, 3 * m)
            per = ms / max(it, 1)
            print("%-28s %4d %5d | %5d %5d %10.2f %9.3f | %9.3f %6.1f%%   converged %d/%d" % (label, nev, m, his.shape[0], it, ms, per, rr,
                                                                                      100.0 * rr / per, nconv, nev), flush=True)
        if name in args.eigsh.split(","):
            import scipy.sparse as sp
            import scipy.sparse.linalg as spla
            for nev in [int(v) for v in args.nev.split(",")]:
                t = time.perf_counter()
                w = spla.eigsh(A.tocsc(), nev, sp.diags(mass).tocsc(), sigma=0, which="LM", tol=tol)[0]
                dt = time.perf_counter() - t
                print("%-28s %4d  host CPU scipy eigsh shift-invert: %.1f ms (smallest %.6f)" % (label, nev, 1e3 * dt, np.min(w)), flush=True)


if __name__ == "__main__":
    main()
