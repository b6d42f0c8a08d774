#!/usr/bin/env python3
"""Time of one conformalized mean-curvature-flow step of the device-resident object (smg_flow_*, Python MeanCurvatureFlow) with the reference's
options (delta = 0.01, tol = 5e-7): ms per step, median, the first two steps dropped; and the split by stage.  The object runs a step as one
call, so the split is taken as follows: the sphericity is a call that only measures (step(0)); the value-only re-precompute and the 3-column solve
are the library calls the object makes, timed on the caller's own hierarchy with this step's matrix and right-hand side (the same code on the
same data); the system kernel and the normalisation together are the remainder of a step.  tools/mcf_step_time.py is the torch-glued step this object replaces: run both in one session to compare.
usage: tools/flow_time.py [workload] [steps]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, scipy.sparse as sp, torch
import bench as B
import surface_multigrid_code_amd as smg
from surface_multigrid_code_amd import mesh

wl = sys.argv[1] if len(sys.argv) > 1 else "C3"
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 8
mg, A, Mb, V, F, label, _ = B.build_workload(wl, smg, mesh)
n, delta, tol = V.shape[0], 0.01, 5e-7
med = lambda v: 1e3 * float(np.median(v))   # noqa: E731


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


def run(flow, count):
    """count single-step calls; every call ends synchronised (it returns the sphericity).  -> (seconds per call, cycles per call)"""
    ts, cyc = [], []
    for _ in range(count + 2):
        t, (his, c) = timed(lambda: flow.step(1))
        ts.append(t); cyc.append(int(c[0]))
    return ts[2:], cyc[2:]


t_create, flow = timed(lambda: smg.MeanCurvatureFlow(mg, V, F, delta=delta))
t_call, cyc = run(flow, steps)
t_measure = [timed(lambda: flow.step(0))[0] for _ in range(steps + 2)][2:]
flow.reset()
t_long, (his, cyc_long) = timed(lambda: flow.step(steps + 2))
U = flow.positions()

# the value-only re-precompute and the solve on the caller's hierarchy: this state's M - delta L and M U
Vn = mesh.normalize_unit_area(V, F)
L = mesh.cotmatrix(Vn, F)
mass = mesh.massmatrix(U, F, "barycentric").diagonal()
S = (sp.diags(mass) - delta * L).tocsr(); S.sort_indices()
dev = torch.device("cuda", 0)
mg.precompute(S)
val = torch.from_numpy(np.ascontiguousarray(S.data)).to(dev)
rhs = torch.from_numpy(np.ascontiguousarray((mass[:, None] * U).T)).to(dev)
z0 = torch.from_numpy(np.ascontiguousarray(U.T)).to(dev)
z = torch.empty_like(z0)
torch.cuda.synchronize()
t_pre, t_solve = [], []
for _ in range(steps + 2):
    t_pre.append(timed(lambda: (mg.precompute_values_device(val.data_ptr()), mg.synchronize()))[0])
    t_solve.append(timed(lambda: (mg.solve_pcg_device(rhs.data_ptr(), z0.data_ptr(), z.data_ptr(), n, 3, opts=smg.SolveOpts(tol=tol)), mg.synchronize()))[0])
t_pre, t_solve = t_pre[2:], t_solve[2:]

step_ms = med(t_call) - med(t_measure)          # a call of one step measures twice; an n-step call measures n + 1 times
print(label)
print("  create (normalise, assemble L_0, clone, first precompute): %.1f ms; device bytes %.1f MB" % (1e3 * t_create, flow.device_bytes() / 1e6))
print("  one call of one step (two sphericity measurements): median %.2f ms; cycles per step %s" % (med(t_call), cyc))
print("  one %d-step call: %.2f ms per step (%d measurements for %d steps); sphericity %.4e -> %.4e" % (steps + 2, 1e3 * t_long / (steps + 2), steps + 3, steps + 2, his[0], his[-1]))
print("  stages (ms, median): sphericity %.2f | value-only precompute %.2f | solve (3 columns, PCG) %.2f | system kernel + normalise %.2f (the remainder "
      "of a step)" % (med(t_measure), med(t_pre), med(t_solve), step_ms - med(t_measure) - med(t_pre) - med(t_solve)))
print("object step (sphericity + system + value-only precompute + 3-column solve to %g + normalise): median %.2f ms" % (tol, step_ms))
