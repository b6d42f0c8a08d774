#!/usr/bin/env python3
"""Time of the earth mover's iteration of the device-resident object (smg_emd_*, Python EarthMover) on masses that stay in HBM, for k = 1, 8, 32
pairs of distributions, with the default options (PCG, tol = 1e-8 |b|_F) and a gap_tol that no query reaches, so that a query of N iterations
runs N iterations with a check at every tenth.

    python tools/emd_time.py [workload] [reps] [--no-converge | --for-trace]
    python tools/emd_time.py --trace kernel_trace.csv

Host clock (median over `reps` queries after one that is dropped).  A query carries a fixed cost beside its iterations -- the masses brought to
the host, the refusals' loop, b sent up, the memsets, the residual launch -- which a query with max_iter = 0 shows alone ("per query").  The time
per iteration is therefore a difference, (t(N_LONG) - t(N_SHORT)) / (N_LONG - N_SHORT), both multiples of check_every, in which everything paid
once per query cancels and the checks keep their share of one in ten.  (A query whose inner solve has max_iter = 0 does not isolate the
kernels: phi stays zero, both bounds are zero, and the query ends as converged at its first check.)  Then, unless --no-converge, one query to
the default gap of 1e-2 per k, with its iterations and bounds.

The split into right-hand side, solve, update and checks is read from the kernel trace of the same command, as tools/morph_time.py does:

    rocprofv3 --kernel-trace --output-format csv -d DIR -o emd -- python tools/emd_time.py C3 2 --for-trace
    python tools/emd_time.py --trace DIR/.../emd_kernel_trace.csv

--trace walks the dispatches in start order.  k_emd_rhs<true> opens an iteration, its grid over the smallest one seen is k; every kernel up to
k_emd_update is the solve; the fixed sums, maxima and k_emd_dual that follow are the checks; k_emd_rhs<false> (the residual) ends a query.  Per
k: the median over all iterations of the trace of k_emd_rhs and of k_emd_update with each kernel's algorithmic bytes over its time (every
operand once, from the shapes, which are the two kernels' smallest grids, whole blocks: the state read by both and written by the update, the
two planes, phi, b, r, and the geometry -- corner lists or faces, W2, areas -- once per launch; J, written at a check only, is not counted), and
the mean per iteration of the solve's and the checks' summed kernel times.  --for-trace runs only the full queries of N_SHORT iterations, so
that every iteration of the trace is a whole one.  Sets no threshold."""
import argparse
import csv
import os
import sys
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

N_SHORT, N_LONG = 20, 60
KS = (1, 8, 32)


def kernel_bytes(n, nF, k):
    """algorithmic bytes of one k_emd_rhs<true> launch and of one k_emd_update launch"""
    return k * (32 * nF + 16 * n) + 68 * nF + 4 * n, k * (80 * nF + 8 * n) + 68 * nF


def split_trace(path):
    rows = []
    with open(path, newline="") as fh:
        for r in csv.DictReader(fh):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"], int(r.get("Grid_Size_X") or r.get("Grid_Size") or 0)))
    rows.sort()
    its, cur, phase = [], None, None
    for start, end, name, grid in rows:
        ms = (end - start) / 1e6
        if "k_emd_rhs" in name:
            if "<true>" in name or "ILb1E" in name:
                cur, phase = {"grid": grid, "rhs": ms, "solve": 0.0, "update": 0.0, "checks": 0.0}, "solve"
                its.append(cur)
            else:
                cur, phase = None, None
        elif cur is None:
            continue
        elif "k_emd_update" in name:
            cur["update"] += ms
            cur["ugrid"] = grid
            phase = "checks"
        elif phase == "solve":
            cur["solve"] += ms
        elif "k_emd_dual" in name or "k_fixed_" in name:
            cur["checks"] += ms
    its = [q for q in its if q["update"] > 0.0]
    if not its:
        print("no iteration of k_emd_rhs<true> ... k_emd_update in", path)
        return
    g1, u1 = min(q["grid"] for q in its), min(q["ugrid"] for q in its)      # vertices and faces, rounded up to whole blocks
    by_k = {}
    for q in its:
        by_k.setdefault(int(round(q["grid"] / g1)), []).append(q)
    print("kernel time per iteration from the trace (ms; k_emd_rhs and k_emd_update: median; solve and checks: mean of the summed kernel times)")
    for k in sorted(by_k):
        qs = by_k[k]
        rhs, upd = float(np.median([q["rhs"] for q in qs])), float(np.median([q["update"] for q in qs]))
        sol, chk = float(np.mean([q["solve"] for q in qs])), float(np.mean([q["checks"] for q in qs]))
        rb, ub = kernel_bytes(g1, u1, k)
        print("  k = %2d x the smallest (%4d iterations): k_emd_rhs %.3f (%.1f MB, %.0f GB/s) | solve %.3f | k_emd_update %.3f (%.1f MB, %.0f GB/s) | checks %.3f | sum %.3f"
              % (k, len(qs), rhs, rb / 1e6, rb / rhs / 1e6, sol, upd, ub / 1e6, ub / upd / 1e6, chk, rhs + sol + upd + chk))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("workload", nargs="?", default="C3")
    ap.add_argument("reps", nargs="?", type=int, default=5)
    ap.add_argument("--no-converge", action="store_true", help="leave out the query to the default gap")
    ap.add_argument("--for-trace", action="store_true", help="only the full queries of N_SHORT iterations: the run to trace")
    ap.add_argument("--trace", default=None, help="a rocprofv3 kernel trace (csv) of this command: print the split and exit")
    args = ap.parse_args()
    if args.trace:
        return split_trace(args.trace)
    import bench as B
    import surface_multigrid_code_amd as smg
    from surface_multigrid_code_amd import mesh
    import torch
    mg, A, Mb, V, F, label, _ = B.build_workload(args.workload, smg, mesh)
    n, nF = V.shape[0], F.shape[0]
    dev = torch.device("cuda", 0)
    med = lambda v: 1e3 * float(np.median(v))   # noqa: E731

    def timed(fn):
        t0 = time.perf_counter()
        out = fn()
        return time.perf_counter() - t0, out

    t_create, obj = timed(lambda: smg.EarthMover(mg, V, F))
    print(label)
    print("  create (geometry, assemble L, clone, precompute): %.1f ms" % (1e3 * t_create), flush=True)
    width = 0.1 * float(np.max(V.max(axis=0) - V.min(axis=0)))

    def blob(centre):
        mu = obj.masses(np.exp(-np.sum((V - V[centre]) ** 2, axis=1) / (2.0 * width * width)))
        return mu / mu.sum()

    for k in KS:
        mu0 = np.stack([blob((7919 * s + 1) % n) for s in range(k)])
        mu1 = np.stack([blob((n // 2 + 104729 * s) % n) for s in range(k)])
        m0d, m1d = torch.from_numpy(mu0).to(dev), torch.from_numpy(mu1).to(dev)          # k x n row-major: column-major n x k
        torch.cuda.synchronize()

        def query():
            return obj.distance_device(m0d.data_ptr(), n, m1d.data_ptr(), n, k)

        def queries(iters):
            obj.set_params(max_iter=iters, gap_tol=1e-300)
            return med([timed(query)[0] for _ in range(args.reps + 1)][1:])

        if args.for_trace:
            print("  k = %2d: %d iterations %.1f ms" % (k, N_SHORT, queries(N_SHORT)), flush=True)
            continue
        t0, ts, tl = queries(0), queries(N_SHORT), queries(N_LONG)
        per = (tl - ts) / (N_LONG - N_SHORT)
        print("  k = %2d: per query %.1f ms; %d iterations %.1f ms, %d iterations %.1f ms: %.3f ms per iteration (%.3f per pair)"
              % (k, t0, N_SHORT, ts, N_LONG, tl, per, per / k), flush=True)
        if not args.no_converge:
            obj.set_params(max_iter=2000, gap_tol=1e-2)
            t_conv, r = timed(query)
            print("          to a gap of 1e-2: %d iterations, %.1f ms (%.3f per iteration); upper[0] %.6f lower[0] %.6f; largest gap %.2e, largest residual %.1e"
                  % (r.iterations, 1e3 * t_conv, 1e3 * t_conv / max(r.iterations, 1), r.upper[0], r.lower[0], r.gap.max(), r.residual.max()), flush=True)
        print("          device bytes %.1f MB" % (obj.device_bytes() / 1e6), flush=True)


if __name__ == "__main__":
    main()
