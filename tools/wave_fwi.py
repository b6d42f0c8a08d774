#!/usr/bin/env python3
"""A small full-waveform inversion with the wave object's adjoint-state gradient (smg_wave_gradient, smg_wave_set_speed): steepest descent on the
speed with Armijo backtracking, on icosphere(3); with --method gn, truncated Newton on its Gauss-Newton products (smg_wave_gauss_newton).

    python tools/wave_fwi.py [iterations] [shots] [--method sd|gn] [--inner 5] [--damping 1e-3]

The data are the traces of `shots` shots (one column and one source each, 24 receivers shared by all) through a speed of 1 with a smooth bump of 20
percent; the inversion starts from the speed 1 everywhere.  An iteration is ONE gradient call for all shots -- the shots' gradients are summed --
and a backtracking line search of forward-only calls (gradient() with no gradient wanted): the first trial changes the speed by at most 5 percent,
a trial is accepted when J(trial) <= J - 1e-4 alpha |g|^2, alpha is halved at most 20 times.  Prints the misfit history and the distance of the
speed to the true one.

--method gn: an iteration is one gradient call, `--inner` conjugate-gradient iterations on (sum_shots H + lambda I) x = -g from x = 0 -- one
product call each, lambda = `--damping` times the iteration's first <d, H d> / |d|^2 -- and the same backtracking from alpha = 1 on
J(trial) <= J + 1e-4 alpha <g, x>."""
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
    ap.add_argument("--method", choices=("sd", "gn"), default="sd")
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--damping", type=float, default=1e-3)
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

    def linearise(s):
        obj.set_speed(s)
        obj.set_state(rest, rest)
        r = obj.gradient(STEPS, signal=sig, observed=data, state=False, grad_signal=False)
        return r, float(r.misfit.sum()), r.grad_speed.sum(axis=1)

    def backtrack(J, step, slope, alpha):
        """the first alpha, halved at most 20 times, with J(speed + alpha step) <= J + 1e-4 alpha slope -> (alpha, misfit, halvings) or None"""
        for halvings in range(21):
            trial = speed + alpha * step
            Jt = misfit(trial) if trial.min() > 0.0 else np.inf
            if Jt <= J + 1e-4 * alpha * slope:
                return alpha, Jt, halvings
            alpha *= 0.5
        return None

    def descent_step():
        """steepest descent: the first trial changes the speed by at most 5 percent -> (J, the step or None, the line's tail)"""
        r, J, g = linearise(speed)
        found = backtrack(J, -g, -float(g @ g), 0.05 * speed.min() / np.abs(g).max())
        return J, None if found is None else (-g,) + found, "loop entries forward %.1f backward %.1f" % (float(np.mean(r.cycles[:STEPS])), float(np.mean(r.cycles[STEPS:])))

    def newton_step():
        """truncated Newton: conjugate gradients on (sum_shots H + lambda I) x = -g from x = 0, one product call per iteration, then the full step
        first -> (J, the step or None, the line's tail)"""
        r, J, g = linearise(speed)
        x, res = np.zeros(n), -g
        d, rr, lam, entries = res.copy(), float(res @ res), None, []
        for _ in range(args.inner):
            p = obj.gauss_newton(d)
            Hd = p.product.sum(axis=1)
            entries.append(float(np.mean(p.cycles)))
            if lam is None:
                lam = args.damping * float(d @ Hd) / float(d @ d)
            q = Hd + lam * d
            a = rr / float(d @ q)
            x, res = x + a * d, res - a * q
            rr, old = float(res @ res), rr
            d = res + (rr / old) * d
        found = backtrack(J, x, float(g @ x), 1.0)
        return J, None if found is None else (x,) + found, "lambda %.3e, loop entries forward %.1f backward %.1f products %.1f" % (
            lam, float(np.mean(r.cycles[:STEPS])), float(np.mean(r.cycles[STEPS:])), float(np.mean(entries)))

    print("icosphere(3): %d vertices, %d shots, %d receivers, %d steps of dt %g" % (n, k, rec.size, STEPS, DT))
    if args.method == "gn":
        print("truncated Newton: %d conjugate-gradient iterations per step, damping %g" % (args.inner, args.damping))
    for it in range(args.iterations):
        J, found, tail = newton_step() if args.method == "gn" else descent_step()
        if found is None:
            print("  iteration %2d: misfit %.6e, no step found in 20 halvings" % (it, J))
            break
        step, alpha, Jt, halvings = found
        speed = speed + alpha * step
        print("  iteration %2d: misfit %.6e -> %.6e, alpha %.3e after %d halvings, |speed - true| / |1 - true| %.4f, %s"
              % (it, J, Jt, alpha, halvings, np.linalg.norm(speed - true) / np.linalg.norm(1.0 - true), tail), flush=True)


if __name__ == "__main__":
    main()
