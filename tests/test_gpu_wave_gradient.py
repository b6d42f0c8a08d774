"""GPU (-m gpu): adjoint-state gradients of the wave object (include/smg.h: smg_wave_gradient, smg_wave_set_speed).

The host references are tests/wave_adjoint_np.py -- the adjoint pass in the kernels' operation order on wave_np.WaveNp's direct solves -- and the
library's own host twin (smg_wave_adjoint_host).  The kernels are held launcher by launcher (smg_debug_wave_adjoint, guarded buffers, every output
pre-filled with sentinels) bit for bit against both: only +, - and * occur, so there is nothing to bound.  The forward half is held bit for bit to
smg_wave_step on a second object, and the misfit to the restatement's fixed-order sum of the read-back traces.

End to end against the restatement's gradient (the library's own L, direct solves); the setups, dt = 0.05, the non-uniform speed and sigma and the
tolerance -- absolute, 1e-12 of the largest |b|_F of the restatement's forward run, passed to every solve, forward and backward -- are those of
tests/test_gpu_wave.py.

    BOUND      wave_adjoint_np.gradient_bound, whose docstring carries the derivation: the adjoint recursion is lambda_n = S' lambda_(n+1) + (R' rho_n,
               0), so the device's (p, q) is within sum_(j >= n) |S^(j-n)|_2 delta_j of the restatement's, with the norms of wave_np.step_map, the
               per-solve allowance (10 tol + res_np) / mu of CHAIN, and the forward CHAIN (wave_np.Chain, tests/test_gpu_wave.py) entering through
               rho_n = R u_n - observed and through e_n.  It bounds, per column, the 2-norm of (grad_u0, grad_v0) together, of grad_speed, and of
               every time row of grad_signal.  The bound is loose where |S^j|_2 is large (the square: 80 j) and is printed beside each gradient's
               own norm; the ratios of the measured distances to it are logged.
    RELATIVE   what BOUND cannot hold on every setup, a second assertion does: the distances above are at most 1e-8 of the gradients' own norms (for
               grad_signal the largest row's distance over the largest row's norm), and |J - <z0, grad z0> / 2| <= 1e-8 J.  The scale: every solve
               stops at 10 tol, 1e-11 of the run's largest right-hand side, so a solve's answer is off by about kappa 1e-11 relative (kappa =
               cond(A) is 3 to 4 on these setups); 2 N = 16 solves feed a gradient, each carried on by powers of the step map that in the scaled
               state (u, v / q2) stay below 17 (tests/test_wave_adjoint_host.py: ROUNDING): 4 x 1e-11 x 16 x 17 = 1.1e-8.  An index, sign or
               scaling slip in the call's loop moves a gradient by the order of its norm.
    IDENTITY   unforced with observed = 0 the misfit is a quadratic form of z0 = (u0, v0), J = <z0, grad z0> / 2.  The device's J is the
               fixed-order sum of its own traces, off the restatement's by at most sum_n sqrt(M) |rho_n| C_n (rho = R u, |R|_2 <= sqrt(M), C_n the
               forward CHAIN), and <z0, grad z0> / 2 by at most |z0| BOUND_state / 2; the restatement itself keeps the identity to rounding
               (tests/test_wave_adjoint_host.py: ENERGY).  Asserted within twice the sum of the two.
    PAIRS      two device evaluations of the same gradient (k columns against single objects, set_speed against a fresh object) are each within
               BOUND of the restatement: within twice BOUND of each other.
    DESCENT    steepest descent on the speed with Armijo backtracking: with g the sum of the shots' gradients and J the sum of their misfits, the
               trial speed - alpha g is accepted when J(trial) <= J - 1e-4 alpha |g|^2; alpha starts where max |alpha g| is 5 percent of the
               smallest speed and is halved at most 20 times.  A gradient that is a descent direction finds such a step."""
import ctypes as C
import gc
import json

import numpy as np
import pytest

import wave_adjoint_np as A
import wave_np as N
from test_gpu_parity import smg  # noqa: F401  (fixture)
from test_gpu_wave import COARSEST, DT, NONFINITE, run_tol, setups  # noqa: F401  (setups: fixture)
from test_wave_adjoint_host import GOLDEN, host_run
from test_wave_host import INVALID, launcher_cases, ricker_signal

pytestmark = pytest.mark.gpu

EPS = N.EPS
STEPS = 8


def hook_run(smg):
    def run(op, V, F, **kw):
        rc, bad, out = A.hook(smg, op, V, F, **kw)
        assert rc == 0 and bad == 0, (rc, bad)
        return out
    return run


# ---- kernels, launcher by launcher ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", N.LAUNCHER_MESHES + N.PYRAMIDS)
def test_hook_against_restatement_and_host_twin(smg, name):
    """every op alone, k = 1, 3, 8, free and clamped, a receiver list with duplicates, vertex 0 and vertex nV - 1: no guard touched, nothing past
    the extent, nothing of it left at the sentinel (wave_adjoint_np._call)"""
    for k in (1, 3, 8):
        for clamped in sorted({cl for cl, _ in launcher_cases(name)}):
            dev = A.check_launchers(hook_run(smg), name, k, clamped)
            hst = A.check_launchers(host_run(smg), name, k, clamped)
            for op, (a, b) in enumerate(zip(dev, hst)):
                assert np.array_equal(a, b), (name, k, clamped, op)


# ---- the object ----------------------------------------------------------------------------------------------------------------------------------
def lists(s):
    """three sources; four receiver slots, one vertex twice"""
    src = s.lists(3)
    return src, np.concatenate([src[::-1], src[:1]]).astype(np.int32)


def ready(obj, src, rec, u0, v0):
    obj.set_sources(src)
    obj.set_receivers(rec)
    obj.set_state(u0, v0)
    return obj


def reference(s, u0, v0, src, rec, sig, obs, steps=STEPS, speed=None):
    """(the restatement after the run, its gradient, BOUND, the forward CHAIN, the tolerance) of `steps` steps from (u0, v0)"""
    ref = s.ref()
    if speed is not None:
        ref.speed = speed
        ref.system()
    ref.src, ref.rec = src, rec
    tol = run_tol(ref, u0, v0, steps, sig)
    norms = s.norms() if speed is None else N.power_norms(ref.step_map(), 20)
    chain, cb = N.Chain(ref, tol, norms), []
    ref.set_state(u0, v0)
    r = A.gradient(ref, steps, sig, obs, after_step=lambda t: cb.append(chain.after(*((None, None) if sig is None else (sig[t], sig[t + 1])))))
    return ref, r, A.gradient_bound(ref, r, norms, tol, cb), cb, tol


def distances(g, r):
    """the per-column 2-norms BOUND speaks of: (grad_u0, grad_v0) together, grad_speed, the time rows of grad_signal"""
    col = lambda x: np.linalg.norm(x, axis=0)   # noqa: E731
    out = dict(state=np.sqrt(col(g.grad_u0 - r.grad_u0) ** 2 + col(g.grad_v0 - r.grad_v0) ** 2), speed=col(g.grad_speed - r.grad_speed))
    if r.grad_signal is not None:
        out["signal"] = np.linalg.norm(g.grad_signal - r.grad_signal, axis=1)
    return out


def sizes(r):
    col = lambda x: np.linalg.norm(x, axis=0)   # noqa: E731
    return dict(state=np.sqrt(col(r.grad_u0) ** 2 + col(r.grad_v0) ** 2), speed=col(r.grad_speed),
                signal=None if r.grad_signal is None else np.linalg.norm(r.grad_signal, axis=1).max(axis=0))


def within(d, bound, times=1.0):
    return all(np.all(d[key] <= times * bound[key]) for key in d)


def ratios(d, bound):
    return {key: float(np.max(d[key] / bound[key])) for key in d}


@pytest.mark.parametrize("key", ["sphere", "square"])
def test_the_forward_half_is_the_step(smg, setups, key):
    """the state and the traces of smg_wave_gradient equal smg_wave_step's on a second object bit for bit, with and without the backward pass; the
    misfit equals the restatement's fixed-order sum of the read-back traces bit for bit; a following smg_wave_step continues as the second
    object's does (the kept right-hand side is dropped and formed again to the same bits)"""
    s = setups(key)
    k = 3
    u0, v0 = s.state(k)
    src, rec = lists(s)
    sig = ricker_signal(smg, STEPS + 2, DT, 3, k)
    obs = 0.05 * np.random.default_rng(3).standard_normal((STEPS, rec.size, k))
    opts = smg.SolveOpts(tol=1e-9, max_iter=30)
    stepper = ready(s.obj(), src, rec, u0, v0)
    _, tr, cyc = stepper.step(STEPS, signal=sig[:STEPS + 1], energy=False, opts=opts)
    want = stepper.state()
    _, tr2, _ = stepper.step(2, signal=sig[STEPS:], energy=False, opts=opts)
    for backward in (True, False):
        obj = ready(s.obj(), src, rec, u0, v0)
        g = obj.gradient(STEPS, signal=sig[:STEPS + 1], observed=obs, speed=backward, state=backward, grad_signal=backward, opts=opts)
        for x, y in zip(obj.state(), want):
            assert np.array_equal(x, y)
        assert np.array_equal(g.traces, tr) and np.array_equal(g.cycles[:STEPS], cyc) and obj.n_done == STEPS
        assert np.array_equal(g.misfit, 0.5 * A.residual(g.traces, obs)[2]) and np.all(g.misfit > 0.0)
        assert np.all(g.cycles[STEPS:] > 0) if backward else (np.all(g.cycles[STEPS:] == 0) and g.grad_speed is None)
        _, tr3, _ = obj.step(2, signal=sig[STEPS:], energy=False, opts=opts)
        assert np.array_equal(tr3, tr2)
        for x, y in zip(obj.state(), stepper.state()):
            assert np.array_equal(x, y)


@pytest.mark.parametrize("key", ["sphere", "torus", "square", "square free"])
def test_gradients_against_direct_solves(smg, setups, key):
    """BOUND and RELATIVE of the header: 8 forced steps, k = 3, three Ricker sources, four receiver slots (one vertex twice), noisy observed traces: grad_speed,
    grad_u0, grad_v0 and grad_signal; exact zeros on the clamped rows"""
    s = setups(key)
    k = 3
    u0, v0 = s.state(k)
    src, rec = lists(s)
    sig = ricker_signal(smg, STEPS, DT, 3, k)
    obs = 0.05 * np.random.default_rng(5).standard_normal((STEPS, rec.size, k))
    ref, r, bound, cb, tol = reference(s, u0, v0, src, rec, sig, obs)
    obj = ready(s.obj(), src, rec, u0, v0)
    g = obj.gradient(STEPS, signal=sig, observed=obs, opts=smg.SolveOpts(tol=tol, max_iter=100))
    d, size = distances(g, r), sizes(r)
    print("%s: tol %.2e, forward CHAIN %s; |gradient| state %s speed %s signal %s; BOUND state %s speed %s signal %s; largest |dev - np| over BOUND %s; "
          "relative to the gradients' norms state %.2e speed %.2e signal %.2e; cycles %s"
          % (key, tol, cb[-1], size["state"], size["speed"], size["signal"], bound["state"], bound["speed"], bound["signal"].max(axis=0), ratios(d, bound),
             float(np.max(d["state"] / size["state"])), float(np.max(d["speed"] / size["speed"])), float(np.max(d["signal"].max(axis=0) / size["signal"])),
             g.cycles))
    assert within(d, bound)
    assert np.all(d["state"] <= 1e-8 * size["state"]) and np.all(d["speed"] <= 1e-8 * size["speed"]) and np.all(d["signal"].max(axis=0) <= 1e-8 * size["signal"])
    assert np.allclose(g.misfit, r.misfit, rtol=1e-9) and np.all(g.cycles > 0)
    if s.clamped:
        for x in (g.grad_speed, g.grad_u0, g.grad_v0):
            assert np.all(x[ref.known] == 0.0) and np.any(x[~ref.known] != 0.0), "exact zeros on the clamped rows"


@pytest.mark.parametrize("key", ["sphere", "square"])
def test_energy_identity_on_the_device(smg, setups, key):
    """IDENTITY and RELATIVE of the header, k = 2, on the device's own misfit and gradient"""
    s = setups(key)
    u0, v0 = s.state(2)
    src, rec = lists(s)
    ref, r, bound, cb, tol = reference(s, u0, v0, src, rec, None, None)
    obj = ready(s.obj(), src, rec, u0, v0)
    g = obj.gradient(STEPS, opts=smg.SolveOpts(tol=tol, max_iter=100))
    col = lambda x: np.linalg.norm(x, axis=0)   # noqa: E731
    M = float(np.max(np.unique(rec, return_counts=True)[1]))
    allow = 0.5 * np.sqrt(col(u0) ** 2 + col(v0) ** 2) * bound["state"] + sum(np.sqrt(M) * col(r.rho[n].reshape(-1, 2)) * cb[n] for n in range(STEPS))
    half = 0.5 * np.sum(u0 * g.grad_u0 + v0 * g.grad_v0, axis=0)
    print("%s: J %s, <z0, grad z0> / 2 %s, |difference| %s, over twice its allowance %s; the allowance over J %s"
          % (key, g.misfit, half, np.abs(g.misfit - half), np.abs(g.misfit - half) / (2 * allow), allow / g.misfit))
    assert np.all(np.abs(g.misfit - half) <= 2.0 * allow) and g.grad_signal is None and np.all(g.misfit > 0.0)
    assert np.all(np.abs(g.misfit - half) <= 1e-8 * g.misfit)


@pytest.mark.parametrize("key", ["sphere", "square"])
def test_own_traces_give_exact_zeros(smg, setups, key):
    """observed = the traces of a second identical object's call: rho is 0 exactly, every backward solve is skipped (cycles 0), every gradient is
    exactly 0.0"""
    s = setups(key)
    k = 3
    u0, v0 = s.state(k)
    src, rec = lists(s)
    sig = ricker_signal(smg, STEPS, DT, 3, k)
    opts = smg.SolveOpts(tol=1e-9, max_iter=30)
    first = ready(s.obj(), src, rec, u0, v0).gradient(STEPS, signal=sig, opts=opts)
    g = ready(s.obj(), src, rec, u0, v0).gradient(STEPS, signal=sig, observed=first.traces, opts=opts)
    assert np.any(first.grad_speed != 0.0) and np.all(first.cycles[STEPS:] > 0) and np.array_equal(g.traces, first.traces)
    assert np.all(g.misfit == 0.0) and np.all(g.cycles[STEPS:] == 0) and np.array_equal(g.cycles[:STEPS], first.cycles[:STEPS])
    for x in (g.grad_speed, g.grad_u0, g.grad_v0, g.grad_signal):
        assert np.all(x == 0.0)


def test_four_columns_against_single_objects(smg, setups):
    """PAIRS of the header on the torus: k = 4 shots in one call against four single-column objects"""
    s = setups("torus")
    k = 4
    u0, v0 = s.state(k)
    src, rec = lists(s)
    sig = ricker_signal(smg, STEPS, DT, 3, k)
    obs = 0.05 * np.random.default_rng(9).standard_normal((STEPS, rec.size, k))
    ref, r, bound, _, tol = reference(s, u0, v0, src, rec, sig, obs)
    opts = smg.SolveOpts(tol=tol, max_iter=100)
    g = ready(s.obj(), src, rec, u0, v0).gradient(STEPS, signal=sig, observed=obs, opts=opts)
    one = A.Result()
    parts = [ready(s.obj(), src, rec, u0[:, c], v0[:, c]).gradient(STEPS, signal=sig[:, :, c:c + 1], observed=obs[:, :, c:c + 1], opts=opts) for c in range(k)]
    one.grad_speed, one.grad_u0, one.grad_v0 = (np.concatenate([getattr(p, f) for p in parts], axis=1) for f in ("grad_speed", "grad_u0", "grad_v0"))
    one.grad_signal = np.concatenate([p.grad_signal for p in parts], axis=2)
    d = distances(g, one)
    print("k = 4 columns against four objects: largest |block - singles| over twice BOUND %s; block against the restatement over BOUND %s"
          % (ratios(d, {key: 2 * b for key, b in bound.items()}), ratios(distances(g, r), bound)))
    assert within(d, bound, 2.0) and within(distances(g, r), bound)
    assert np.allclose(g.misfit, [p.misfit[0] for p in parts], rtol=1e-9)


def test_same_calls_same_bits(smg, setups):
    """two calls give identical bits, graphs on and off, free and clamped"""
    for key in ("sphere", "square"):
        s = setups(key)
        u0, v0 = s.state(3)
        src, rec = lists(s)
        sig = ricker_signal(smg, STEPS, DT, 3, 3)
        obs = 0.05 * np.random.default_rng(13).standard_normal((STEPS, rec.size, 3))
        runs = []
        for use_graph in (1, 1, 0):
            obj = ready(s.obj(), src, rec, u0, v0)
            g = obj.gradient(STEPS, signal=sig, observed=obs, opts=smg.SolveOpts(tol=1e-9, max_iter=30, use_graph=use_graph))
            runs.append([g.misfit, g.grad_speed, g.grad_u0, g.grad_v0, g.grad_signal, g.traces, g.cycles] + list(obj.state()))
        for other in runs[1:]:
            for x, y in zip(runs[0], other):
                assert np.array_equal(x, y), key


def test_set_speed_against_a_fresh_object(smg, setups):
    """PAIRS of the header on the torus: an object created with the setup's speed, stepped once, then set to another speed (a value-only
    re-precompute), against an object created with that speed: the gradients within twice BOUND; whether bitwise is printed.  set_speed(None) is
    speed 1 everywhere; a refused speed leaves the object as it was"""
    s = setups("torus")
    k = 2
    u0, v0 = s.state(k)
    src, rec = lists(s)
    sig = ricker_signal(smg, STEPS, DT, 3, k)
    obs = 0.05 * np.random.default_rng(17).standard_normal((STEPS, rec.size, k))
    other = s.speed * (1.0 + 0.1 * np.cos(2.0 * s.V[:, 1]))
    ref, r, bound, _, tol = reference(s, u0, v0, src, rec, sig, obs, speed=other)
    opts = smg.SolveOpts(tol=tol, max_iter=100)
    moved = ready(s.obj(), src, rec, u0, v0)
    moved.step(1, opts=opts)                                                  # the old matrix is used once before it is replaced
    moved.set_speed(other)
    moved.set_state(u0, v0)
    a = moved.gradient(STEPS, signal=sig, observed=obs, opts=opts)
    fresh = smg.WaveEquation(s.mg, s.V, s.F, DT, speed=other, sigma=s.sigma, clamped=bool(s.clamped))
    b = ready(fresh, src, rec, u0, v0).gradient(STEPS, signal=sig, observed=obs, opts=opts)
    d = distances(a, b)
    bits = all(np.array_equal(getattr(a, f), getattr(b, f)) for f in ("misfit", "grad_speed", "grad_u0", "grad_v0", "grad_signal", "traces"))
    print("set_speed against a fresh object: largest |difference| over twice BOUND %s; fresh against the restatement over BOUND %s; bitwise %s"
          % (ratios(d, {key: 2 * x for key, x in bound.items()}), ratios(distances(b, r), bound), bits))
    assert within(d, bound, 2.0) and within(distances(b, r), bound) and within(distances(a, r), bound)
    bad = other.copy()
    bad[5] = 0.0
    with pytest.raises(smg.SmgError) as e:
        moved.set_speed(bad)
    assert e.value.code == INVALID and "speed[5]" in str(e.value)
    moved.set_state(u0, v0)
    again = moved.gradient(STEPS, signal=sig, observed=obs, opts=opts)
    assert np.array_equal(again.grad_speed, a.grad_speed) and np.array_equal(again.misfit, a.misfit), "a refused speed changes nothing"
    moved.set_speed(None)
    unit = ready(smg.WaveEquation(s.mg, s.V, s.F, DT, sigma=s.sigma, clamped=bool(s.clamped)), src, rec, u0, v0)
    moved.set_state(u0, v0)
    assert np.allclose(moved.gradient(STEPS, signal=sig, observed=obs, opts=opts).misfit, unit.gradient(STEPS, signal=sig, observed=obs, opts=opts).misfit, rtol=1e-9)


def test_three_descent_iterations_lower_the_misfit(smg, setups):
    """DESCENT of the header on icosphere3, k = 2 shots, 8 steps: the data come from the setup's speed with a bump of 20 percent, the inversion starts
    from the setup's speed; each of three iterations finds a step and lowers the misfit"""
    s = setups("sphere")
    k = 2
    u0, v0 = s.state(k)
    src, rec = lists(s)
    sig = ricker_signal(smg, STEPS, DT, 3, k)
    true = s.speed * (1.0 + 0.2 * np.exp(-4.0 * np.sum((s.V - s.V[rec[0]]) ** 2, axis=1)))
    opts = smg.SolveOpts(tol=1e-10, max_iter=100)
    data = ready(smg.WaveEquation(s.mg, s.V, s.F, DT, speed=true), src, rec, u0, v0).step(STEPS, signal=sig, energy=False, opts=opts)[1]
    obj = ready(s.obj(), src, rec, u0, v0)
    speed, history = s.speed.copy(), []
    for it in range(3):
        obj.set_state(u0, v0)
        r = obj.gradient(STEPS, signal=sig, observed=data, state=False, grad_signal=False, opts=opts)
        J, grad = float(r.misfit.sum()), r.grad_speed.sum(axis=1)
        alpha, found = 0.05 * speed.min() / np.abs(grad).max(), None
        assert np.max(np.abs(alpha * grad) / speed) <= 0.05
        for halvings in range(21):
            trial = speed - alpha * grad
            obj.set_speed(trial)
            obj.set_state(u0, v0)
            Jt = float(obj.gradient(STEPS, signal=sig, observed=data, speed=False, state=False, grad_signal=False, opts=opts).misfit.sum())
            if Jt <= J - 1e-4 * alpha * float(grad @ grad):
                found = halvings
                break
            alpha *= 0.5
        assert found is not None and Jt < J, (it, J, Jt)
        speed = trial
        history.append((J, Jt, found))
    print("icosphere3, three descent iterations: (misfit, misfit after the step, halvings) %s; |speed - true| / |start - true| %.4f"
          % (history, np.linalg.norm(speed - true) / np.linalg.norm(s.speed - true)))
    assert history[2][1] < history[1][1] < history[0][1] < history[0][0]


def test_a_nan_is_refused_and_nothing_is_written(smg, setups):
    """a NaN in observed is SMG_ERR_INVALID before anything runs and the state is kept; a NaN in u ends the call with SMG_ERR_NONFINITE at step 0:
    n_done == 0, neither misfit nor gradient nor traces written"""
    s = setups("sphere")
    Lc = smg._lib.load()
    k = 2
    n = s.V.shape[0]
    u0, v0 = s.state(k)
    src, rec = lists(s)
    sig = ricker_signal(smg, 3, DT, 3, k)
    obj = ready(s.obj(), src, rec, u0, v0)
    obj.step(2, signal=sig[:3])
    kept = obj.state()
    obs = np.zeros((3, rec.size, k))
    obs[1, 2, 1] = np.nan
    with pytest.raises(smg.SmgError) as e:
        obj.gradient(3, signal=sig, observed=obs)
    assert e.value.code == INVALID and "step 1, receiver 2, column 1" in str(e.value) and obj.n_done == 0
    for x, y in zip(obj.state(), kept):
        assert np.array_equal(x, y)
    bad = u0.copy()
    bad[77, 1] = np.nan
    obj.set_state(bad, v0)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    J, gs, gu, gv = np.full(k, N.SENTINEL), np.full((n, k), N.SENTINEL, order="F"), np.full((n, k), N.SENTINEL, order="F"), np.full((n, k), N.SENTINEL, order="F")
    gsig, tr, cyc = np.full((4, 3, k), N.SENTINEL), np.full((3, rec.size, k), N.SENTINEL), np.full(6, -7, dtype=np.int32)
    nd = C.c_int(-1)
    rc = Lc.smg_wave_gradient(obj.o, 3, sig.ctypes.data_as(dp), None, None, J.ctypes.data_as(dp), gs.ctypes.data_as(dp), n, gu.ctypes.data_as(dp),
                              gv.ctypes.data_as(dp), n, gsig.ctypes.data_as(dp), tr.ctypes.data_as(dp), cyc.ctypes.data_as(ip), C.byref(nd))
    assert rc == NONFINITE and nd.value == 0 and b"smg_wave_gradient" in Lc.smg_last_error() and b"step 0" in Lc.smg_last_error()
    for x in (J, gs, gu, gv, gsig, tr):
        assert np.all(x == N.SENTINEL)
    assert np.all(cyc == -7)
    obj.set_state(u0, v0)
    fresh = ready(s.obj(), src, rec, u0, v0)
    a, b = obj.gradient(3, signal=sig), fresh.gradient(3, signal=sig)
    assert np.array_equal(a.grad_speed, b.grad_speed) and np.array_equal(a.misfit, b.misfit)


def test_device_bytes_are_live_buffers(smg):
    """smg_wave_device_bytes equals the library's count of live bytes attributable to the object after a gradient call, is unchanged by a second call
    of the same shape (and by a smaller one), and the count returns to its start after destroy"""
    live = smg._lib.load().smg_device_bytes_live
    for name, clamped in (("icosphere3", False), ("square", True)):
        V, F = N.shape(name)
        mg = smg.mg_precompute(V, F, 0.25, COARSEST[name], 1)                  # the caller's hierarchy stays alive throughout
        u0, v0, _ = N.test_state(V, F, 3, clamped)
        src = N.test_lists(V, F, 3, clamped)
        rec = np.concatenate([src, src[:1]]).astype(np.int32)
        sig = ricker_signal(smg, STEPS, DT, 3, 3)
        obs = np.zeros((STEPS, rec.size, 3))
        gc.collect()
        before = live()
        obj = ready(smg.WaveEquation(mg, V, F, DT, speed=N.nonuniform(V)[0], clamped=clamped), src, rec, u0, v0)
        obj.step(2, signal=sig[:3])
        stepped = obj.device_bytes()
        obj.gradient(STEPS, signal=sig, observed=obs)
        first = obj.device_bytes()
        obj.gradient(STEPS, signal=sig, observed=obs)
        obj.gradient(3, signal=sig[:4])
        counted, held = obj.device_bytes(), live() - before
        print("%s, clamped %d: device_bytes %d after two steps, %d after the first gradient call, %d after the third, live DevBuf bytes held %d; the history %d"
              % (name, clamped, stepped, first, counted, held, STEPS * V.shape[0] * 3 * 8))
        del obj
        gc.collect()
        assert 0 < stepped < first == counted == held and first - stepped >= STEPS * V.shape[0] * 3 * 8 and live() == before


def live_calls(smg):
    """the refusals that need an object -> {name: [code, message]}; nothing may be written by any of them"""
    Lc = smg._lib.load()
    V, F = N.shape("square")
    mg = smg.mg_precompute(V, F, 0.25, COARSEST["square"], 1)
    n, k = V.shape[0], 2
    u0, v0, _ = N.test_state(V, F, k, True)
    inner = N.test_lists(V, F, 3, True)
    make = lambda: smg.WaveEquation(mg, V, F, DT, clamped=True)   # noqa: E731
    empty, deaf, bare, obj = make(), make(), make(), make()
    deaf.set_sources(inner)
    deaf.set_state(u0, v0)                                                     # a state and sources, no receivers
    bare.set_receivers(inner)
    bare.set_state(u0, v0)                                                     # a state and receivers, no sources
    ready(obj, inner, inner, u0, v0)
    dp = C.POINTER(C.c_double)
    out = np.full((n, k), N.SENTINEL, order="F")
    O = out.ctypes.data_as(dp)
    sig, obs = np.zeros((2, 3, k)), np.zeros((1, 3, k))
    sbad, obad = sig.copy(), obs.copy()
    sbad[1, 2, 0], obad[0, 2, 1] = np.inf, np.nan
    sp = lambda x: x.ctypes.data_as(dp)   # noqa: E731
    grad = lambda o, steps=1, signal=None, observed=None, gs=None, ld=n, gu=None, ld0=n, gsig=None: Lc.smg_wave_gradient(   # noqa: E731
        o.o, steps, signal, observed, None, None, gs, ld, gu, None, ld0, gsig, None, None, None)
    spd = np.ones(n)
    speeds = {"zero": (5, 0.0), "nan": (7, np.nan), "negative": (0, -1.0)}

    def set_speed(which):
        x = spd.copy()
        x[speeds[which][0]] = speeds[which][1]
        return Lc.smg_wave_set_speed(obj.o, sp(x))
    calls = {"gradient before set_state": lambda: grad(empty, gs=O),
             "gradient n_steps zero": lambda: grad(obj, steps=0, gs=O),
             "gradient without receivers": lambda: grad(deaf, gs=O),
             "gradient signal without sources": lambda: grad(bare, signal=sp(sig), gs=O),
             "gradient non-finite signal": lambda: grad(obj, signal=sp(sbad), gs=O),
             "gradient non-finite observed": lambda: grad(obj, observed=sp(obad), gs=O),
             "gradient leading dimension of grad_speed": lambda: grad(obj, gs=O, ld=n - 1),
             "gradient leading dimension of grad_u0": lambda: grad(obj, gu=O, ld0=n - 1),
             "gradient grad_signal without a signal": lambda: grad(obj, gsig=O),
             "gradient order: n_steps before receivers": lambda: grad(deaf, steps=0, gs=O),
             "gradient order: receivers before the signal": lambda: grad(deaf, signal=sp(sbad), gs=O),
             "gradient order: signal before observed": lambda: grad(obj, signal=sp(sbad), observed=sp(obad), gs=O),
             "gradient order: observed before the leading dimension": lambda: grad(obj, observed=sp(obad), gs=O, ld=n - 1),
             "gradient order: leading dimension before grad_signal": lambda: grad(obj, gs=O, ld=n - 1, gsig=O),
             "set_speed zero": lambda: set_speed("zero"), "set_speed nan": lambda: set_speed("nan"), "set_speed negative": lambda: set_speed("negative")}
    got = {}
    for name, call in calls.items():
        rc = call()
        got[name] = [rc, Lc.smg_last_error().decode()]
    assert np.all(out == N.SENTINEL)
    u, v = obj.state()
    assert np.array_equal(u, u0) and np.array_equal(v, v0)
    g = obj.gradient(1, signal=np.ones((2, 3, k)))                             # the refused calls have changed nothing
    assert g.grad_speed.shape == (n, k) and np.all(g.misfit > 0.0)
    return got


def test_live_refusals(smg):
    """the refusals that need an object: code and text as recorded in tests/golden/wave_gradient_refusals.json, group "live"; nothing is written"""
    golden = json.load(open(GOLDEN))["live"]
    got = live_calls(smg)
    assert set(got) == set(golden)
    for name, (rc, msg) in got.items():
        assert [rc, msg] == golden[name] and rc == INVALID, name
