#!/usr/bin/env python3
"""Time of the Newton steps of the device-resident conformal metric (smg_conformal_*, Python ConformalMetric) with the default options
(grad_tol = 1e-10, inner tolerance 1e-6 |rhs|_2, PCG): ms per Newton step and the split by stage.  The problem: vertex 0 fixed, Theta = the
angle sums of u* = 0.05 (sin(3 x) + y z) on the normalised mesh, solved from u = 0, so the answer is known and every step is a full step.
The object runs a solve as one call, so the split is taken as follows: an evaluation (the scale, face and row kernels with the matrix values,
the three reductions and their 24-byte copy) is a call that only measures (max_newton = 0, Theta resident in HBM); the value-only re-precompute and the 1-column solve
are the library calls the object makes, timed on the caller's own hierarchy with -L of the rest mesh, vertex 0 known, and the first step's
right-hand side (the same code on the same pattern); the trial evaluation and the row kernel's second pass together are the remainder of a step.
tools/flow_time.py times smg_flow's step at the same size: run both in one session to compare.
usage: tools/conformal_time.py [workload] [repeats]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
import bench as B
import surface_multigrid_code_amd as smg
from surface_multigrid_code_amd import mesh

wl = sys.argv[1] if len(sys.argv) > 1 else "C3"
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
mg, A, Mb, V, F, label, _ = B.build_workload(wl, smg, mesh)
V = mesh.normalize_unit_area(V, F)
n = V.shape[0]
med = lambda v: 1e3 * float(np.median(v))   # noqa: E731


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


fixed = np.array([0], np.int32)
t_create, cm = timed(lambda: smg.ConformalMetric(mg, V, F, fixed))
ustar = 0.05 * (np.sin(3.0 * V[:, 0]) + V[:, 1] * V[:, 2])
ustar -= ustar[0]
cm.set_u(ustar)
Theta = cm.angle_sums()
Td = torch.from_numpy(Theta).to(torch.device("cuda", 0))                      # Theta stays in HBM: a call moves no block
torch.cuda.synchronize()
t_call, runs = [], []
for _ in range(reps + 1):
    cm.reset()
    t, out = timed(lambda: cm.solve_device(Td.data_ptr()))
    t_call.append(t); runs.append(out)
t_call = t_call[1:]
his, st, cyc, conv = runs[-1]
err = float(np.abs(cm.u() - ustar).max())
cm.set_params(max_newton=0)
t_eval = []
for _ in range(reps + 2):
    cm.reset()
    t_eval.append(timed(lambda: cm.solve_device(Td.data_ptr()))[0])
t_eval = t_eval[2:]
g0 = Theta * 0.0
cm.reset()
g0[1:] = (cm.angle_sums() - Theta)[1:]

# the value-only re-precompute and the 1-column solve on the caller's hierarchy: -L of the rest mesh with vertex 0 known, the first step's g
L = (-mesh.cotmatrix(V, F)).tocsr(); L.sort_indices()
dev = torch.device("cuda", 0)
mg.precompute(L, known=fixed)
val = torch.from_numpy(np.ascontiguousarray(L.data)).to(dev)
rhs = torch.from_numpy(np.ascontiguousarray(g0)).to(dev)
z0, kv = torch.zeros(n, dtype=torch.float64, device=dev), torch.zeros(1, dtype=torch.float64, device=dev)
z = torch.empty_like(z0)
tol = 1e-6 * float(np.linalg.norm(g0))
torch.cuda.synchronize()
t_pre, t_solve, entries = [], [], []
for _ in range(reps + 2):
    t_pre.append(timed(lambda: (mg.precompute_values_device(val.data_ptr()), mg.synchronize()))[0])
    t, (out, _) = timed(lambda: (mg.solve_pcg_device(rhs.data_ptr(), z0.data_ptr(), z.data_ptr(), n, 1, known_val_ptr=kv.data_ptr(), ld_kv=1,
                                                     opts=smg.SolveOpts(tol=tol, max_iter=100)), mg.synchronize()))
    t_solve.append(t); entries.append(len(out[1]))
t_pre, t_solve = t_pre[2:], t_solve[2:]

steps = max(st.size, 1)
step_ms = (med(t_call) - med(t_eval)) / steps       # a call of k Newton steps evaluates once before the first step
print(label)
print("  create (rest lengths, assemble -L, clone, first precompute): %.1f ms; device bytes %.1f MB" % (1e3 * t_create, cm.device_bytes() / 1e6))
print("  one solve from u = 0: median %.2f ms for %d Newton steps, t = %s, cycles %s, max |g| = %s, converged %s, max |u - u*| = %.2e"
      % (med(t_call), st.size, st.tolist(), cyc.tolist(), ["%.1e" % h for h in his], conv, err))
print("  stages (ms, median): evaluation with values (scale + faces + rows + 3 reductions + copy) %.2f | value-only precompute %.2f | solve (1 column, PCG, "
      "%d loop entries) %.2f | trial evaluation + rows with values %.2f (the remainder of a step)"
      % (med(t_eval), med(t_pre), entries[-1], med(t_solve), step_ms - med(t_pre) - med(t_solve)))
print("object Newton step (value-only precompute + 1-column solve to 1e-6 |rhs| + trial evaluation + rows): median %.2f ms" % step_ms)
