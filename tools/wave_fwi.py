#!/usr/bin/env python3
"""A small full-waveform inversion with the wave object's adjoint-state gradient (smg_wave_gradient, smg_wave_set_speed): steepest descent on the
speed with Armijo backtracking, on icosphere(3).

    python tools/wave_fwi.py [iterations] [shots]

The data are the traces of `shots` shots (one column and one source each, 24 receivers shared by all) through a speed of 1 with a smooth bump of 20
percent; the inversion starts from the speed 1 everywhere.  An iteration is ONE gradient call for all shots -- the shots' gradients are summed --
and a backtracking line search of forward-only calls (gradient() with no gradient wanted): the first trial changes the speed by at most 5 percent,
a trial is accepted when J(trial) <= J - 1e-4 alpha |g|^2, alpha is halved at most 20 times.  Prints the misfit history and the distance of the
speed to the true one."""
import argparse
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

DT, STEPS = 0.05, 40


def icosphere(mesh, level):
    """the unit sphere: the icosahedron, `level` times split at the edge mid-points (mesh.midpoint_upsample) and projected to the sphere"""
    p = (1.0 + 5 ** 0.5) / 2
    V = np.array([[-1, p, 0], [1, p, 0], [-1, -p, 0], [1, -p, 0], [0, -1, p], [0, 1, p], [0, -1, -p], [0, 1, -p], [p, 0, -1], [p, 0, 1], [-p, 0, -1], [-p, 0, 1]])
    F = np.array([[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2], [10, 7, 6], [7, 1, 8],
                  [3, 9, 4], [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11], [6, 2, 10], [8, 6, 7], [9, 8, 1]], dtype=np.int32)
    for _ in range(level):
        S, F = mesh.midpoint_upsample(V.shape[0], F)
        V = S @ V
        V = V / np.linalg.norm(V, axis=1, keepdims=True)
    return V / np.linalg.norm(V, axis=1, keepdims=True), F


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("iterations", nargs="?", type=int, default=10)
    ap.add_argument("shots", nargs="?", type=int, default=4)
    args = ap.parse_args()
    import surface_multigrid_code_amd as smg
    from surface_multigrid_code_amd import mesh
    V, F = icosphere(mesh, 3)
    n, k = V.shape[0], args.shots
    mg = smg.mg_precompute(V, F, 0.25, 50, 1)
    true = 1.0 + 0.2 * np.exp(-4.0 * np.sum((V - V[0]) ** 2, axis=1))
    src = np.linspace(1, n - 1, k).astype(np.int32)
    rec = np.linspace(0, n - 1, 24).astype(np.int32)
    t = DT * np.arange(STEPS + 1)
    sig = np.zeros((STEPS + 1, k, k))
    for c in range(k):                                                        # shot c drives source c alone
        sig[:, c, c] = smg.wavelets.ricker(2.0, t, 0.5)
    rest = np.zeros((n, k))

    def prepared(speed):
        obj = smg.WaveEquation(mg, V, F, DT, speed=speed)
        obj.set_sources(src)
        obj.set_receivers(rec)
        return obj
    made = prepared(true)
    made.set_state(rest, rest)
    data = made.step(STEPS, signal=sig, energy=False)[1]
    obj, speed = prepared(np.ones(n)), np.ones(n)

    def misfit(s):
        obj.set_speed(s)
        obj.set_state(rest, rest)
        return float(obj.gradient(STEPS, signal=sig, observed=data, speed=False, state=False, grad_signal=False).misfit.sum())
    print("icosphere(3): %d vertices, %d shots, %d receivers, %d steps of dt %g" % (n, k, rec.size, STEPS, DT))
    for it in range(args.iterations):
        obj.set_speed(speed)
        obj.set_state(rest, rest)
        r = obj.gradient(STEPS, signal=sig, observed=data, state=False, grad_signal=False)
        J, g = float(r.misfit.sum()), r.grad_speed.sum(axis=1)
        alpha = 0.05 * speed.min() / np.abs(g).max()
        for halvings in range(21):
            Jt = misfit(speed - alpha * g)
            if Jt <= J - 1e-4 * alpha * float(g @ g):
                break
            alpha *= 0.5
        else:
            print("  iteration %2d: misfit %.6e, no step found in 20 halvings" % (it, J))
            break
        speed = speed - alpha * g
        print("  iteration %2d: misfit %.6e -> %.6e, alpha %.3e after %d halvings, |speed - true| / |1 - true| %.4f, loop entries forward %.1f backward %.1f"
              % (it, J, Jt, alpha, halvings, np.linalg.norm(speed - true) / np.linalg.norm(1.0 - true), float(np.mean(r.cycles[:STEPS])), float(np.mean(r.cycles[STEPS:]))),
              flush=True)


if __name__ == "__main__":
    main()
