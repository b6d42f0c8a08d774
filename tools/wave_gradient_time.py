#!/usr/bin/env python3
"""Time of a gradient call of the wave object (smg_wave_gradient, Python WaveEquation.gradient) against a forward call of the same steps
(smg_wave_step), for k = 1 and 8 shots, with the default options (PCG, tol = 1e-10 |b|_F forward and 1e-10 |g|_F backward per solve).

    python tools/wave_gradient_time.py [workload] [reps]

Host clock: the median [smallest, largest] over `reps` calls of N_STEPS steps each after one call that is dropped; the forward and the gradient
calls alternate on ONE object, each from the same state (set_state is outside the clock).  dt is a fifth of the mesh's extent over the wave speed
1, every shot starts from a smooth bump of its own and is driven by a Ricker source; the observed traces are zeros.  The gradient call is timed
with every gradient wanted and with none (the forward half, the kept history aside, and the misfit); the line gives both over the forward call,
the loop entries per solve of both passes, and what the object holds.  One gradient should cost about two forward runs: the backward pass is one
solve of the same matrix per step between pointwise kernels.  Sets no threshold."""
import argparse
import os
import sys
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

N_STEPS = 10
KS = (1, 8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("workload", nargs="?", default="C3")
    ap.add_argument("reps", nargs="?", type=int, default=5)
    args = ap.parse_args()
    import bench as B
    import surface_multigrid_code_amd as smg
    from surface_multigrid_code_amd import mesh
    mg, A, Mb, V, F, label, _ = B.build_workload(args.workload, smg, mesh)
    n = V.shape[0]
    span = float(np.max(V.max(axis=0) - V.min(axis=0)))
    dt = 0.2 * span
    print(label)
    obj = smg.WaveEquation(mg, V, F, dt)
    src = np.array([0, n // 3, (2 * n) // 3], dtype=np.int32)
    rec = np.arange(0, n, max(1, n // 16), dtype=np.int32)[:16]
    obj.set_sources(src)
    obj.set_receivers(rec)
    t = dt * np.arange(N_STEPS + 1)

    def timed(fn):
        t0 = time.perf_counter()
        out = fn()
        return time.perf_counter() - t0, out

    for k in KS:
        s = np.arange(k)[None, :]
        bump = np.exp(-40.0 * (((V[:, [0]] - V[:, [0]].mean()) / span - 0.1 * np.cos(s)) ** 2 + ((V[:, [1]] - V[:, [1]].mean()) / span - 0.1 * np.sin(s)) ** 2))
        sig = np.ascontiguousarray(smg.wavelets.ricker(0.5 / dt, t[:, None, None], 2.0 * dt + 0.0 * s[None]) * np.ones((1, src.size, 1)))
        calls = {"forward": lambda: obj.step(N_STEPS, signal=sig, energy=False),
                 "misfit": lambda: obj.gradient(N_STEPS, signal=sig, speed=False, state=False, grad_signal=False),
                 "gradient": lambda: obj.gradient(N_STEPS, signal=sig)}
        ts, out = {name: [] for name in calls}, {}
        for _ in range(args.reps + 1):
            for name, fn in calls.items():
                obj.set_state(bump, 0.0 * bump)
                tt, out[name] = timed(fn)
                ts[name].append(1e3 * tt)
        ms = {name: np.array(x[1:]) for name, x in ts.items()}
        med = {name: float(np.median(x)) for name, x in ms.items()}
        g = out["gradient"]
        print("  k = %d, %d steps: forward call %.2f ms [%.2f, %.2f]; gradient call without a backward pass %.2f ms [%.2f, %.2f], %.2f of the forward call; "
              "gradient call %.2f ms [%.2f, %.2f], %.2f of the forward call; loop entries per solve forward %.1f, backward %.1f; misfit %s; device bytes %.1f MB, "
              "of them the history %.1f MB"
              % (k, N_STEPS, med["forward"], ms["forward"].min(), ms["forward"].max(), med["misfit"], ms["misfit"].min(), ms["misfit"].max(),
                 med["misfit"] / med["forward"], med["gradient"], ms["gradient"].min(), ms["gradient"].max(), med["gradient"] / med["forward"],
                 float(np.mean(g.cycles[:N_STEPS])), float(np.mean(g.cycles[N_STEPS:])), np.array2string(g.misfit, precision=3), obj.device_bytes() / 1e6,
                 N_STEPS * n * k * 8 / 1e6), flush=True)


if __name__ == "__main__":
    main()
