#!/usr/bin/env python3
"""Time of one Helmholtz-Hodge query of the device-resident object (smg_hodge_*, Python HodgeDecomposition) on blocks that stay in HBM: ms per
query for k = 1, 8, 32 fields, median, the first two queries dropped, with the default options (PCG, tol = 1e-10 |rhs|_F).  The object runs a query
as one call, so the split is taken as follows: a query without parts and energies is right-hand side + solve; the parts are the difference to a
query with both; the solve is the library call the object makes, timed on the caller's own hierarchy with -L (vertex 0 known) and this query's
right-hand sides (the same code on the same data; closed meshes only); the right-hand side kernel, its fixed sums and the one host read are the
remainder.  Each stage's algorithmic bytes (every operand once, from the shapes) over its time is printed as GB/s: the stage times include the
fixed-order sums and the synchronise, so these are lower bounds of the kernels' own rates.
usage: tools/hodge_time.py [workload] [reps]"""
import ctypes as C
import os
import sys
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
import bench as B
import surface_multigrid_code_amd as smg
from surface_multigrid_code_amd import mesh

wl = sys.argv[1] if len(sys.argv) > 1 else "C3"
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
mg, A, Mb, V, F, label, _ = B.build_workload(wl, smg, mesh)
n, nF = V.shape[0], F.shape[0]
L = smg._lib.load()
dev = torch.device("cuda", 0)
med = lambda v: 1e3 * float(np.median(v))   # noqa: E731


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


t_create, obj = timed(lambda: smg.HodgeDecomposition(mg, V, F))
closed = obj.is_closed
print(label)
print("  create (geometry, assemble L, clone, precompute): %.1f ms; closed %s" % (1e3 * t_create, closed))
if closed:
    S = (-mesh.cotmatrix(V, F)).tocsr()
    S.sort_indices()
    mg.precompute(S, np.array([0], dtype=np.int32))
c = (V[F[:, 0]] + V[F[:, 1]] + V[F[:, 2]]) / 3.0
for k in (1, 8, 32):
    X = np.stack([np.cross([0.3 + 0.02 * s, -0.5, 0.8], c) + [0.2, 0.01 * s, -0.3] + 0.3 * np.sin((2.0 + 0.1 * s) * c[:, [1, 2, 0]]) for s in range(k)])
    Xd = torch.from_numpy(np.ascontiguousarray(X)).to(dev)
    ud, vd = torch.zeros((k, n), dtype=torch.float64, device=dev), torch.zeros((k, n), dtype=torch.float64, device=dev)
    Pd = torch.zeros((k, nF, 9), dtype=torch.float64, device=dev)
    E, cyc = np.zeros(4 * k), np.zeros(2, dtype=np.int32)
    torch.cuda.synchronize()

    def query(parts):
        rc = L.smg_hodge_decompose(obj.g, Xd.data_ptr(), k, 1, None, ud.data_ptr(), n, vd.data_ptr(), n, Pd.data_ptr() if parts else None,
                                   E.ctypes.data_as(C.POINTER(C.c_double)) if parts else None, cyc.ctypes.data_as(C.POINTER(C.c_int)))
        assert rc == 0, L.smg_last_error()

    t_full = [timed(lambda: query(True))[0] for _ in range(reps + 2)][2:]
    t_half = [timed(lambda: query(False))[0] for _ in range(reps + 2)][2:]
    line = "  k = %2d: query %.2f ms (%.2f per field), cycles %s; without parts %.2f" % (k, med(t_full), med(t_full) / k, cyc.tolist(), med(t_half))
    parts_ms = med(t_full) - med(t_half)
    parts_bytes = k * (24 * nF + 16 * n + 104 * nF) + 116 * nF
    rhs_bytes = k * (24 * nF + 32 * n) + 28 * n + 48 * nF
    if closed:
        # the same solve on the caller's hierarchy: the right-hand sides the object formed are (-L) [u v] on the unknown rows up to the tolerance; form them again
        Z = torch.cat([ud, vd]).cpu().numpy().T                                      # n x 2k
        rhs = np.ascontiguousarray((S @ Z).T)
        rhs_d = torch.from_numpy(rhs).to(dev)
        z0 = torch.zeros_like(rhs_d)
        z = torch.empty_like(rhs_d)
        kv = torch.zeros(2 * k, dtype=torch.float64, device=dev)
        opts = smg.SolveOpts(tol=1e-10 * float(np.linalg.norm(rhs)), max_iter=100)
        torch.cuda.synchronize()
        t_solve = [timed(lambda: (mg.solve_pcg_device(rhs_d.data_ptr(), z0.data_ptr(), z.data_ptr(), n, 2 * k, kv.data_ptr(), 1, opts=opts), mg.synchronize()))[0]
                   for _ in range(reps + 2)][2:]
        rhs_ms = med(t_half) - med(t_solve)
        line += " | rhs + sums %.2f ms (%.0f GB/s) | solve (%d columns, PCG) %.2f ms | parts + energies %.2f ms (%.0f GB/s)" % (
            rhs_ms, rhs_bytes / rhs_ms / 1e6, 2 * k, med(t_solve), parts_ms, parts_bytes / parts_ms / 1e6)
    else:
        line += " | parts + energies %.2f ms (%.0f GB/s)" % (parts_ms, parts_bytes / parts_ms / 1e6)
    print(line)
    share = E.reshape(k, 4)
    print("          shares of field 0: G %.4f R %.4f H %.4f; device bytes %.1f MB" % (share[0, 1] / share[0, 0], share[0, 2] / share[0, 0], share[0, 3] / share[0, 0],
                                                                                     obj.device_bytes() / 1e6))
