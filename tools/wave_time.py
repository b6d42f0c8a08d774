#!/usr/bin/env python3
"""Time of a step of the device-resident wave object (smg_wave_*, Python WaveEquation) for k = 1, 8, 32 shots, with the default options (PCG,
tol = 1e-10 |b|_F per solve), with the advance kernel leaving the next step's right-hand side (the default) and without it (SMG_WAVE_FUSED=0, read
at create: every step then runs k_wave_rhs first).

    python tools/wave_time.py [workload] [reps]

Host clock: the median [smallest, largest] over `reps` calls of N_STEPS steps each after one call that is dropped, divided by N_STEPS; the calls of
the two variants alternate, each on an object of its own.  dt is a fifth of the mesh's
extent over the wave speed 1, so that a C is comparable to Mt.  Every shot starts from a smooth bump of its own and is driven by a Ricker source.

The split of a step into its solve and its own kernels comes from the same clock: with opts.max_iter = 0 the solve returns its start, so a step is
its kernels, reductions, copies and the host's round trips alone ("without solves"); the difference to the full step is the solve.  The same
steps without the energy history show what the potential-energy launches and the second host read cost.

Per kernel: smg_debug_wave_time launches one launcher alone, 20 times back to back between two events, on blocks of zeros of the same shapes; the
line gives the mean time of a launch and the launcher's algorithmic bytes over it (every operand once, from the shapes: per (vertex, column)
k_wave_rhs reads u and v and writes b, its square and the warm start, 40 bytes; k_wave_advance reads w, u and v and writes u', v', the kinetic
term and the next b, square and warm start, 72 bytes; once per launch mt and s2, 16 n).  Sets no threshold."""
import argparse
import ctypes as C
import os
import sys
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

N_STEPS = 10
KS = (1, 8, 32)
NAMES = {1: "fused (the advance kernel leaves the next right-hand side)", 0: "two kernels (SMG_WAVE_FUSED=0: k_wave_rhs every step)"}


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
    dt = 0.2 * span
    print(label)

    def timed(fn):
        t0 = time.perf_counter()
        out = fn()
        return time.perf_counter() - t0, out

    for k in KS:
        print("  k = %2d: the kernels alone" % k)
        for name, op, nbytes in (("k_wave_rhs", 0, 40 * n * k + 16 * n), ("k_wave_advance with the next b", 2, 72 * n * k + 16 * n)):
            ms = C.c_double(0.0)
            rc = L.smg_debug_wave_time(op, n, nF, k, Fp, Vp, 20, C.byref(ms))
            assert rc == 0, L.smg_last_error()
            print("          %-32s %.4f ms a launch, %7.1f MB, %5.0f GB/s" % (name, ms.value, nbytes / 1e6, nbytes / ms.value / 1e6), flush=True)
    src = np.array([0, n // 3, (2 * n) // 3], dtype=np.int32)
    rec = np.arange(0, n, max(1, n // 16), dtype=np.int32)[:16]
    t = dt * np.arange(N_STEPS + 1)
    objs = {}
    for fused in (1, 0):
        os.environ["SMG_WAVE_FUSED"] = str(fused)
        t_create, objs[fused] = timed(lambda: smg.WaveEquation(mg, V, F, dt))
        print("  %s: create (masses, assemble L, clone, precompute) %.1f ms" % (NAMES[fused], 1e3 * t_create), flush=True)
        objs[fused].set_sources(src)
        objs[fused].set_receivers(rec)
    none = smg.SolveOpts(tol=0.0, max_iter=0)                                  # (the state that these steps leave is not the method's: timed, then dropped)
    for k in KS:
        s = np.arange(k)[None, :]
        bump = np.exp(-40.0 * (((V[:, [0]] - V[:, [0]].mean()) / span - 0.1 * np.cos(s)) ** 2 + ((V[:, [1]] - V[:, [1]].mean()) / span - 0.1 * np.sin(s)) ** 2))
        sig = np.ascontiguousarray(smg.wavelets.ricker(0.5 / dt, t[:, None, None], 2.0 * dt + 0.0 * s[None]) * np.ones((1, src.size, 1)))
        ts = {(f, kind): [] for f in (1, 0) for kind in ("full", "quiet", "bare")}
        out = {}
        for f in (1, 0):
            objs[f].set_state(bump, 0.0 * bump)
        for kind, kw in (("full", dict()), ("quiet", dict(energy=False)), ("bare", dict(opts=none))):
            for _ in range(args.reps + 1):                                     # the two variants alternate, so that both see the same neighbours
                for f in (1, 0):
                    tt, res = timed(lambda: objs[f].step(N_STEPS, signal=sig, **kw))
                    ts[(f, kind)].append(tt)
                    if kind == "full":
                        out[f] = res
        for f in (1, 0):
            ms = {kind: 1e3 * np.array(ts[(f, kind)][1:]) / N_STEPS for kind in ("full", "quiet", "bare")}
            med = {kind: float(np.median(x)) for kind, x in ms.items()}
            E, tr, cyc = out[f]
            print("    k = %2d, %s: %.3f ms per step [%.3f, %.3f] (%.3f per shot), %.3f [%.3f, %.3f] without the energies, %.3f [%.3f, %.3f] without "
                  "solves: the solve's share %.1f %%; loop entries per step %.1f; last energy %.3e; device bytes %.1f MB"
                  % (k, "fused" if f else "two kernels", med["full"], ms["full"].min(), ms["full"].max(), med["full"] / k, med["quiet"], ms["quiet"].min(),
                     ms["quiet"].max(), med["bare"], ms["bare"].min(), ms["bare"].max(), 100.0 * (med["full"] - med["bare"]) / med["full"], float(np.mean(cyc)),
                     float(E[-1].sum()), objs[f].device_bytes() / 1e6), flush=True)
    objs.clear()
    os.environ.pop("SMG_WAVE_FUSED", None)


if __name__ == "__main__":
    main()
