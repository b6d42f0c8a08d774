#!/usr/bin/env python3
"""Gradient-domain morphing (smg_morph_interpolate, smg_morph_reconstruct, smg_morph_transfer) on one GPU: ms per query and the loop entries of
its one solve, for k sets = 3k columns.

    python tools/morph_time.py [--legs C3,bunny] [--ks 1,4,16] [--reps 5]
    python tools/morph_time.py --trace kernel_trace.csv

C3: the bunny_15K_init x3 subdivision hierarchy of bench.py (1 011 330 vertices); bunny: bunny.obj with the reference's hierarchy
(mg_precompute(V, F, 0.25, 200, 1)).  The pose is the rest pose twisted about its longest axis (60 degrees from end to end) and stretched by
diag(1.2, 0.9, 1.1); vertex 0 is pinned; the times of a query are spread over [0, 1]; default options (tolerance 1e-10 |b|_F).  Per leg and k,
between device blocks, median of --reps after a warm-up call, host clock around a call that ends in a synchronise (the method of
tools/geodesics_time.py): interpolate, reconstruct from the gradients of the k blends, transfer of the k blends from the mesh itself.

The split of a query into polar, right-hand side and solve is read from the kernel trace of the same command:

    rocprofv3 --kernel-trace --output-format csv -d DIR -o morph -- python tools/morph_time.py --legs C3 --queries interpolate
    python tools/morph_time.py --trace DIR/.../morph_kernel_trace.csv

--trace walks the dispatches in start order; k_morph_face_polar opens a query, the grid of k_morph_rhs over the smallest one seen gives its k,
and every kernel up to the next query is counted as polar (k_morph_face_polar), right-hand side (k_morph_rhs, the start and pin kernels and the
fixed-order sum up to the solve's first kernel) or solve (the rest).  Per k: the median over the queries of each part's summed kernel time.
Sets no threshold."""
import argparse
import csv
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


def twisted(V, angle_deg=60.0):
    lo, hi = V.min(axis=0), V.max(axis=0)
    ax = int(np.argmax(hi - lo))
    u, v = (ax + 1) % 3, (ax + 2) % 3
    a = np.deg2rad(angle_deg) * (V[:, ax] - lo[ax]) / (hi - lo)[ax]
    ctr = 0.5 * (lo + hi)
    X = V.copy()
    du, dv = V[:, u] - ctr[u], V[:, v] - ctr[v]
    X[:, u] = ctr[u] + np.cos(a) * du - np.sin(a) * dv
    X[:, v] = ctr[v] + np.sin(a) * du + np.cos(a) * dv
    return np.ascontiguousarray((X - ctr) * np.array([1.2, 0.9, 1.1]) + ctr)


def split_trace(path):
    rows = []
    with open(path, newline="") as fh:
        for r in csv.DictReader(fh):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"], int(r.get("Grid_Size_X") or r.get("Grid_Size") or 0)))
    rows.sort()
    queries, cur = [], None
    for start, end, name, grid in rows:
        if "k_morph_face_polar" in name:
            cur = {"polar": 0.0, "rhs": 0.0, "solve": 0.0, "grid": 0, "in_solve": False}
            queries.append(cur)
        if cur is None:
            continue
        us = (end - start) / 1e3
        if "k_morph_face_polar" in name:
            cur["polar"] += us
        elif "k_morph_rhs" in name:
            cur["rhs"] += us
            cur["grid"] = grid
        elif not cur["in_solve"] and ("k_morph" in name or "fixed_sum" in name):
            cur["rhs"] += us
        else:
            cur["in_solve"] = True
            cur["solve"] += us
    if not queries:
        print("no k_morph_face_polar dispatch in", path)
        return
    g1 = min(q["grid"] for q in queries if q["grid"])
    by_k = {}
    for q in queries:
        if q["grid"]:
            by_k.setdefault(int(round(q["grid"] / g1)), []).append(q)
    print("kernel time per query, median over the queries of the trace (us): polar / right-hand side / solve")
    for k in sorted(by_k):
        qs = by_k[k]
        med = lambda key: float(np.median([q[key] for q in qs]))   # noqa: E731
        print("  k = %2d x the smallest (%3d queries)  polar %9.1f  right-hand side %9.1f  solve %10.1f  sum %10.1f" %
              (k, len(qs), med("polar"), med("rhs"), med("solve"), med("polar") + med("rhs") + med("solve")))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="C3,bunny")
    ap.add_argument("--ks", default="1,4,16")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--queries", default="interpolate,reconstruct,transfer")
    ap.add_argument("--trace", default=None, help="a rocprofv3 kernel trace (csv) of this command: print the split and exit")
    args = ap.parse_args()
    if args.trace:
        return split_trace(args.trace)
    import torch
    import surface_multigrid_code_amd as smg
    from surface_multigrid_code_amd import mesh
    from oracle import mesh_np as M

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
        V, F = np.ascontiguousarray(V, dtype=np.float64), np.ascontiguousarray(F, dtype=np.int32)
        n, nF = V.shape[0], F.shape[0]
        t0 = time.perf_counter()
        mo = smg.Morpher(mg, V, F)
        t_create = time.perf_counter() - t0
        print("%s: n = %d, nF = %d, create %.2f s" % (label, n, nF, t_create), flush=True)
        X = twisted(V)
        Vd, Xd = torch.from_numpy(V).cuda(), torch.from_numpy(X).cuda()
        for k in [int(x) for x in args.ks.split(",")]:
            ts = np.linspace(0.0, 1.0, k + 2)[1:-1] if k > 1 else np.array([0.5])
            Ud = torch.empty((3 * k, n), dtype=torch.float64, device="cuda")
            for q in args.queries.split(","):
                if q == "interpolate":
                    med, cyc = timed(lambda: mo.interpolate_device(Xd.data_ptr(), ts, Ud.data_ptr()))
                else:
                    S1 = torch.stack([(1.0 - t) * Vd + t * Xd for t in ts]).contiguous()           # the k blends, k x n x 3
                    if q == "transfer":
                        med, cyc = timed(lambda: mo.transfer_device(Vd.data_ptr(), n, S1.data_ptr(), k, Ud.data_ptr()))
                    else:
                        if n * k > 5_000_000:
                            print("  k = %2d  reconstruct   skipped: %.1f GB of gradients from the host twin" % (k, 72e-9 * nF * k), flush=True)
                            continue
                        J = torch.from_numpy(np.stack([mo_gradients(smg, V, F, (1.0 - t) * V + t * X) for t in ts])).cuda()
                        med, cyc = timed(lambda: mo.reconstruct_device(J.data_ptr(), k, Ud.data_ptr()))
                print("  k = %2d  %-12s %3d loop entries  %9.3f ms / query  (%.3f ms / set)" % (k, q, cyc, med, med / k), flush=True)
        print("  device memory of the object: %.1f MB (after k = %s)" % (mo.device_bytes() / 1e6, args.ks.split(",")[-1]), flush=True)
        del mo, mg


def mo_gradients(smg, V, F, X):
    """nF x 9 face gradients of a pose by the library's host twin"""
    import ctypes as C
    out = np.zeros(9 * F.shape[0])
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    Xc = np.ascontiguousarray(X)
    rc = smg._lib.load().smg_morph_faces_host(0, V.shape[0], F.shape[0], 1, F.ctypes.data_as(ip), V.ctypes.data_as(dp), Xc.ctypes.data_as(dp), None, None, None, 0,
                                              out.ctypes.data_as(dp))
    assert rc == 0
    return out.reshape(-1, 9)


if __name__ == "__main__":
    main()
