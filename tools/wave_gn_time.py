#!/usr/bin/env python3
"""Time of a Gauss-Newton product call of the wave object (smg_wave_gauss_newton, Python WaveEquation.gauss_newton) against a forward call and a
gradient call of the same steps, for k = 1 and 8 shots, with the default options (PCG, tol = 1e-10 of each solve's right-hand side).

    python tools/wave_gn_time.py [workload] [reps]

Host clock: the median [smallest, largest] over `reps` calls of N_STEPS steps each after one round that is dropped; the forward call, the
gradient call and the product call alternate on ONE object, the first two each from the same state (set_state is outside the clock), the product
at the point the gradient call before it has left.  The setup is tools/wave_gradient_time.py's.  The product is timed with the backward pass and
without (Born modelling alone); the line gives both in forward calls and the loop entries per solve of both passes.  From the launch list a
product is a tangent run -- a forward step with one more pointwise launch and no sources -- and a backward pass: about two forward calls
(profiles/wave_gn_time.txt: 1.88 at k = 1, 1.89 at k = 8, Born traces alone 1.00).  Sets no threshold."""
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
    d = 0.05 * (1.0 + 0.5 * np.cos(6.0 * (V[:, 0] - V[:, 0].mean()) / span))      # a speed increase of 2.5 to 7.5 percent, one direction for every shot

    def timed(fn):
        t0 = time.perf_counter()
        out = fn()
        return time.perf_counter() - t0, out

    for k in KS:
        s = np.arange(k)[None, :]
        bump = np.exp(-40.0 * (((V[:, [0]] - V[:, [0]].mean()) / span - 0.1 * np.cos(s)) ** 2 + ((V[:, [1]] - V[:, [1]].mean()) / span - 0.1 * np.sin(s)) ** 2))
        sig = np.ascontiguousarray(smg.wavelets.ricker(0.5 / dt, t[:, None, None], 2.0 * dt + 0.0 * s[None]) * np.ones((1, src.size, 1)))
        calls = {"forward": (True, lambda: obj.step(N_STEPS, signal=sig, energy=False)),
                 "gradient": (True, lambda: obj.gradient(N_STEPS, signal=sig)),
                 "born": (False, lambda: obj.gauss_newton(d, product=False)),
                 "product": (False, lambda: obj.gauss_newton(d))}
        ts, out = {name: [] for name in calls}, {}
        for _ in range(args.reps + 1):
            for name, (reset, fn) in calls.items():
                if reset:
                    obj.set_state(bump, 0.0 * bump)
                tt, out[name] = timed(fn)
                ts[name].append(1e3 * tt)
        ms = {name: np.array(x[1:]) for name, x in ts.items()}
        med = {name: float(np.median(x)) for name, x in ms.items()}
        p = out["product"]
        print("  k = %d, %d steps: forward call %.2f ms [%.2f, %.2f]; gradient call %.2f ms [%.2f, %.2f], %.2f of the forward call; Born traces alone %.2f ms "
              "[%.2f, %.2f], %.2f of the forward call; product call %.2f ms [%.2f, %.2f], %.2f of the forward call; loop entries per solve tangent %.1f, "
              "backward %.1f (the gradient call: forward %.1f, backward %.1f); curvature %s; device bytes %.1f MB"
              % (k, N_STEPS, med["forward"], ms["forward"].min(), ms["forward"].max(), med["gradient"], ms["gradient"].min(), ms["gradient"].max(),
                 med["gradient"] / med["forward"], med["born"], ms["born"].min(), ms["born"].max(), med["born"] / med["forward"], med["product"],
                 ms["product"].min(), ms["product"].max(), med["product"] / med["forward"], float(np.mean(p.cycles[:N_STEPS])), float(np.mean(p.cycles[N_STEPS:])),
                 float(np.mean(out["gradient"].cycles[:N_STEPS])), float(np.mean(out["gradient"].cycles[N_STEPS:])), np.array2string(p.curvature, precision=3),
                 obj.device_bytes() / 1e6), flush=True)


if __name__ == "__main__":
    main()
