#!/usr/bin/env python3
"""Time of a step of the device-resident reaction-diffusion object (smg_rd_*, Python ReactionDiffusion) for k = 1, 8, 32 simulations with k
different parameter sets, in the three cases of handle use (Du != Dv: two k-column solves; Du == Dv: one 2k-column solve; Dv == 0: one
k-column solve), with the default options (PCG, tol = 1e-10 |rhs|_F per solve).  The diffusing cases run Gray-Scott at dt = 1; Dv == 0 runs
FitzHugh-Nagumo, whose recovery variable does not diffuse, at dt = 0.1 (explicit Gray-Scott without a diffusing v sharpens into single-vertex
spikes and leaves the explicit reaction's stability range within ten steps at this resolution).

    python tools/rd_time.py [workload] [reps]

Host clock: the median over `reps` calls of N_STEPS steps each after one call that is dropped, divided by N_STEPS.  The diffusivities are scaled
by the squared extent of the mesh so that dt D (-L) is comparable to M.

The split of a step into its solves and its own kernels comes from the same clock: with opts.max_iter = 0 every solve returns its start, so a
step is its kernels, reductions, copies and the host's two round trips alone ("without solves"); the difference to the full step is the solves.

Per kernel: smg_debug_rd_time launches one launcher alone, 20 times back to back between two events, on blocks of zeros of the same shapes; the
line gives the mean time of a launch and the launcher's algorithmic bytes over it (every operand once, from the shapes: per (vertex, column)
k_rd_react reads u and v and writes m u*, m v* and their two squares, 48 bytes; k_rd_close reads u, v, u', v' and writes m u', m v' and the
change, 56 bytes; once per launch the masses, 8 n, and for k_rd_react the table, 160 k).  Sets no threshold."""
import argparse
import ctypes as C
import os
import sys
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

N_STEPS = 10
KS = (1, 8, 32)
CASES = (("Du != Dv (two k-column solves), Gray-Scott", 2.0, 1.0, 1.0), ("Du == Dv (one 2k-column solve), Gray-Scott", 2.0, 2.0, 1.0),
         ("Dv == 0 (one k-column solve), FitzHugh-Nagumo", 2.0, 0.0, 0.1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("workload", nargs="?", default="C3")
    ap.add_argument("reps", nargs="?", type=int, default=5)
    args = ap.parse_args()
    import bench as B
    import surface_multigrid_code_amd as smg
    from surface_multigrid_code_amd import mesh
    mg, A, Mb, V, F, label, _ = B.build_workload(args.workload, smg, mesh)
    n, nF = V.shape[0], F.shape[0]
    L = smg._lib.load()
    Vc, Fc = np.ascontiguousarray(V, dtype=np.float64), np.ascontiguousarray(F, dtype=np.int32)
    Fp, Vp = Fc.ctypes.data_as(C.POINTER(C.c_int)), Vc.ctypes.data_as(C.POINTER(C.c_double))
    span = float(np.max(V.max(axis=0) - V.min(axis=0)))
    print(label)

    def timed(fn):
        t0 = time.perf_counter()
        out = fn()
        return time.perf_counter() - t0, out

    for k in KS:
        print("  k = %2d: the kernels alone" % k)
        for name, op, n_sub, nbytes in (("k_rd_react, 1 sub-step", 0, 1, 48 * n * k + 8 * n + 160 * k), ("k_rd_react, 4 sub-steps", 0, 4, 48 * n * k + 8 * n + 160 * k),
                                        ("k_rd_close", 1, 1, 56 * n * k + 8 * n)):
            ms = C.c_double(0.0)
            rc = L.smg_debug_rd_time(op, n, nF, k, Fp, Vp, n_sub, 20, C.byref(ms))
            assert rc == 0, L.smg_last_error()
            print("          %-24s %.4f ms a launch, %7.1f MB, %5.0f GB/s" % (name, ms.value, nbytes / 1e6, nbytes / ms.value / 1e6), flush=True)
    for case, du, dv, dt in CASES:
        t_create, obj = timed(lambda: smg.ReactionDiffusion(mg, V, F, Du=du * 1e-4 * span * span, Dv=dv * 1e-4 * span * span, dt=dt))
        print("  %s: create (masses, assemble L, clone, precompute) %.1f ms" % (case, 1e3 * t_create), flush=True)
        for k in KS:
            s = np.arange(k)[None, :]
            bump = np.exp(-40.0 * (((V[:, [0]] - V[:, [0]].mean()) / span - 0.1 * np.cos(s)) ** 2 + ((V[:, [1]] - V[:, [1]].mean()) / span - 0.1 * np.sin(s)) ** 2))
            if dv > 0.0:
                coeff = np.stack([smg.reactions.gray_scott(0.030 + 0.0005 * c, 0.055 + 0.0003 * c) for c in range(k)])
                obj.set_state(1.0 - 0.5 * bump, 0.25 * bump, coeff)
            else:
                coeff = np.stack([smg.reactions.fitzhugh_nagumo(0.7, 0.8, 0.08 + 0.001 * c) for c in range(k)])
                obj.set_state(2.0 * bump - 1.2, 0.5 * bump - 0.6, coeff)
            ts, cyc, change = [], None, None
            for _ in range(args.reps + 1):
                t, (mass, change, cyc) = timed(lambda: obj.step(N_STEPS))
                ts.append(t)
            per = 1e3 * float(np.median(ts[1:])) / N_STEPS
            none = smg.SolveOpts(tol=0.0, max_iter=0)                          # (the state that these steps leave is not the method's: timed, then dropped)
            bare = 1e3 * float(np.median([timed(lambda: obj.step(N_STEPS, opts=none))[0] for _ in range(args.reps + 1)][1:])) / N_STEPS
            print("    k = %2d: %.3f ms per step (%.3f per simulation), %.3f without solves: the solves' share %.1f %%; loop entries per step %s; "
                  "last change %.3e; device bytes %.1f MB" % (k, per, per / k, bare, 100.0 * (per - bare) / per, np.mean(cyc, axis=0), change[-1].max(),
                                                             obj.device_bytes() / 1e6), flush=True)
        del obj


if __name__ == "__main__":
    main()
