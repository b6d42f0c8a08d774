"""GPU (-m gpu): Born traces and Gauss-Newton products of the wave object (include/smg.h: smg_wave_gauss_newton).

The host references are tests/wave_gn_np.py -- the tangent run and the adjoint pass in the kernels' operation order on wave_np.WaveNp's direct
solves -- and the library's own host twin (smg_wave_born_host).  k_wave_born is held through smg_debug_wave_born (guarded buffers, the output
pre-filled with sentinels) bit for bit against both: only + and * occur, so there is nothing to bound.  The setups, DT, the fields and the lists
are those of tests/test_gpu_wave_gradient.py: icosphere(3), the torus, the square free and clamped, 8 steps, k = 3.

    TOLERANCE  one absolute tolerance per test, 1e-12 of the smallest of the restatement's three largest right-hand-side norms -- the forward
               run's |b|_F, the tangent run's, the adjoint pass's |g|_F -- passed to the gradient call and to the product call.
    RELATIVE   as RELATIVE of tests/test_gpu_wave_gradient.py: every solve stops at 10 tol, at most 1e-11 of its half's largest right-hand side, so
               a solve's answer is off by about kappa 1e-11 relative (kappa = cond(A) is 3 to 4 on these setups); 3 N = 24 solves feed a product
               (forward, tangent, adjoint) instead of the gradient's 16, each carried on by powers of the step map that in the scaled state stay
               below 17: 4 x 1e-11 x 24 x 17 = 1.7e-8 of the product's norm per column.  The same bound holds born_traces, the largest row's
               distance over the largest row's norm.  An index, sign or scaling slip moves either by the order of its norm.
    IDENTITIES the device's own <d, product> against its curvature within RELATIVE of the curvature; its product against its own
               gradient(observed = traces - born_traces).grad_speed within twice RELATIVE of the product's norm (two evaluations, each within
               RELATIVE).  d is scaled so that max |J d| >= 1e-2 max |traces|: the subtraction's rounding stays below 1e-13 relative.
    NEWTON     one truncated-Newton step from the start of DESCENT of tests/test_gpu_wave_gradient.py (icosphere3, k = 2, the data from a 20 percent
               bump): five conjugate-gradient iterations on sum_shots H + lambda I, lambda = 1e-3 of the first <d, H d> / |d|^2, then Armijo
               (c = 1e-4, at most 20 halvings): wave_gn_np.newton_step.  The restatement accepts the full step: the misfit falls from 6.95e-2
               to 1.49e-3, where one steepest-descent step from the same start reaches 5.31e-2, a factor 35.6 above -- more than the 1.2 to
               spare that the comparison needs to be asserted.  Asserted on the device: the step is accepted, the misfit falls, and it ends
               below the steepest-descent step's."""
import ctypes as C
import gc
import json

import numpy as np
import pytest

import wave_adjoint_np as A
import wave_gn_np as G
import wave_np as N
from test_gpu_parity import smg  # noqa: F401  (fixture)
from test_gpu_wave import COARSEST, DT, NONFINITE, run_tol, setups  # noqa: F401  (setups: fixture)
from test_gpu_wave_gradient import STEPS, lists, ready
from test_wave_gn_host import GOLDEN, host_run
from test_wave_host import INVALID, launcher_cases, ricker_signal

pytestmark = pytest.mark.gpu

RELATIVE = 1.7e-8
col = lambda x: np.linalg.norm(x, axis=0)   # noqa: E731


def hook_run(smg):
    def run(V, F, **kw):
        rc, bad, out = G.hook(smg, V, F, **kw)
        assert rc == 0 and bad == 0, (rc, bad)
        return out
    return run


# ---- the kernel ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", N.LAUNCHER_MESHES + N.PYRAMIDS)
def test_hook_against_restatement_and_host_twin(smg, name):
    """k = 1, 3, 8, d_cols = 1 and k, free and clamped: no guard touched, nothing past the extent, nothing of it left at the sentinel
    (wave_gn_np._call)"""
    for k in (1, 3, 8):
        for clamped in sorted({cl for cl, _ in launcher_cases(name)}):
            for d_cols in sorted({1, k}):
                dev = G.check_launcher(hook_run(smg), name, k, d_cols, clamped)
                hst = G.check_launcher(host_run(smg), name, k, d_cols, clamped)
                assert np.array_equal(dev, hst), (name, k, d_cols, clamped)


# ---- the object ----------------------------------------------------------------------------------------------------------------------------------
def problem(smg, s, k, seed=5):
    u0, v0 = s.state(k)
    src, rec = lists(s)
    sig = ricker_signal(smg, STEPS, DT, 3, k)
    obs = 0.05 * np.random.default_rng(seed).standard_normal((STEPS, rec.size, k))
    return u0, v0, src, rec, sig, obs


def direction(s, cols):
    """a smooth speed perturbation per column, of both signs"""
    return np.asfortranarray(0.1 * np.cos(2.0 * s.V[:, [0]] - 3.0 * s.V[:, [2]] + 0.9 * np.arange(cols)[None, :]) + 0.03 * np.sin(5.0 * s.V[:, [1]]))


def linearised(smg, s, k, opts, seed=5):
    """(an object after a gradient call with a backward pass, that call's result, the problem)"""
    p = problem(smg, s, k, seed)
    obj = ready(s.obj(), p[2], p[3], p[0], p[1])
    return obj, obj.gradient(STEPS, signal=p[4], observed=p[5], opts=opts), p


def exact(s, problem_, d, scale=None):
    """(the tolerance of TOLERANCE, the three largest right-hand sides, the restatement, its gradient, its product for d, d) with the library's own
    L and direct solves; scale: d is first scaled so that max |J d| is `scale` times max |traces|"""
    u0, v0, src, rec, sig, obs = problem_
    ref = s.ref()
    ref.src, ref.rec = src, rec
    tops = [run_tol(ref, u0, v0, STEPS, sig, rel=1.0)]
    ref.set_state(u0, v0)
    r = A.gradient(ref, STEPS, sig, obs)
    if scale is not None:
        d = d * (scale * np.max(np.abs(r.traces)) / np.max(np.abs(G.born_traces(ref, r.e, d))))
    want = G.gauss_newton(ref, r, d)
    tops += [float(np.sqrt(max(ss for ss, _ in want.tangent))), float(np.sqrt(max(ss for ss, _ in want.adjoint)))]
    return 1e-12 * min(tops), tops, ref, r, want, d


def same(a, b):
    return all((x is None and y is None) or np.array_equal(x, y) for x, y in zip((a.product, a.born_traces, a.curvature, a.cycles),
                                                                                 (b.product, b.born_traces, b.curvature, b.cycles)))


@pytest.mark.parametrize("key", ["sphere", "square"])
def test_curvature_is_the_fixed_order_sum_of_the_returned_traces(smg, setups, key):
    """curvature equals the restatement's fixed-order sum of the squares of the returned born_traces bit for bit; Born modelling alone
    (product=False) returns the same traces, the same curvature and the tangent solves' cycles alone"""
    s = setups(key)
    opts = smg.SolveOpts(tol=1e-9, max_iter=30)
    obj, g, _ = linearised(smg, s, 3, opts)
    d = direction(s, 3)
    gn = obj.gauss_newton(d, traces=True, opts=opts)
    assert np.array_equal(gn.curvature, A.residual(gn.born_traces, None)[2]) and np.all(gn.curvature > 0.0)
    assert gn.cycles.size == 2 * STEPS and np.all(gn.cycles > 0)
    born = obj.gauss_newton(d, product=False, traces=True, opts=opts)
    assert born.product is None and np.array_equal(born.born_traces, gn.born_traces) and np.array_equal(born.curvature, gn.curvature)
    assert np.array_equal(born.cycles, gn.cycles[:STEPS])


@pytest.mark.parametrize("key", ["sphere", "torus", "square", "square free"])
def test_product_and_traces_against_direct_solves(smg, setups, key):
    """TOLERANCE and RELATIVE of the header, k = 3, one direction per shot; exact zeros on the clamped rows"""
    s = setups(key)
    k = 3
    u0, v0, src, rec, sig, obs = problem(smg, s, k)
    tol, tops, ref, r, want, d = exact(s, (u0, v0, src, rec, sig, obs), direction(s, k))
    opts = smg.SolveOpts(tol=tol, max_iter=100)
    obj = ready(s.obj(), src, rec, u0, v0)
    g = obj.gradient(STEPS, signal=sig, observed=obs, opts=opts)
    gn = obj.gauss_newton(d, traces=True, opts=opts)
    dp, dt_ = col(gn.product - want.product) / col(want.product), np.linalg.norm(gn.born_traces - want.born_traces, axis=1).max(axis=0) / np.linalg.norm(want.born_traces, axis=1).max(axis=0)
    dg = col(g.grad_speed - r.grad_speed) / col(r.grad_speed)
    print("%s: largest right-hand sides forward %.3e tangent %.3e adjoint %.3e, tol %.2e; |product - np| / |product| %s; born_traces' largest row distance over the largest row %s; "
          "grad_speed relative %s; curvature relative %s; cycles %s" % (key, tops[0], tops[1], tops[2], tol, dp, dt_, dg, np.abs(gn.curvature - want.curvature) / want.curvature, gn.cycles))
    assert np.all(dp <= RELATIVE) and np.all(dt_ <= RELATIVE) and np.all(gn.cycles > 0)
    assert np.allclose(gn.curvature, want.curvature, rtol=2.0 * RELATIVE)
    if s.clamped:
        assert np.all(gn.product[ref.known] == 0.0) and np.any(gn.product[~ref.known] != 0.0), "exact zeros on the clamped rows"


@pytest.mark.parametrize("key", ["sphere", "square"])
def test_identities_on_the_device(smg, setups, key):
    """IDENTITIES of the header, on the device's own numbers"""
    s = setups(key)
    k = 3
    u0, v0, src, rec, sig, obs = problem(smg, s, k)
    tol, _, _, _, _, d = exact(s, (u0, v0, src, rec, sig, obs), direction(s, 1), scale=5e-2)
    opts = smg.SolveOpts(tol=tol, max_iter=100)
    obj = ready(s.obj(), src, rec, u0, v0)
    g = obj.gradient(STEPS, signal=sig, observed=obs, opts=opts)
    gn = obj.gauss_newton(d, traces=True, opts=opts)
    assert np.max(np.abs(gn.born_traces)) >= 1e-2 * np.max(np.abs(g.traces))
    quad = np.sum(d * gn.product, axis=0)
    obj.set_state(u0, v0)
    other = obj.gradient(STEPS, signal=sig, observed=g.traces - gn.born_traces, opts=opts).grad_speed
    print("%s: |<d, product> - curvature| / curvature %s; |product - grad_speed(observed = traces - born_traces)| / |product| %s"
          % (key, np.abs(quad - gn.curvature) / gn.curvature, col(gn.product - other) / col(gn.product)))
    assert np.all(np.abs(quad - gn.curvature) <= RELATIVE * gn.curvature)
    assert np.all(col(gn.product - other) <= 2.0 * RELATIVE * col(gn.product))


@pytest.mark.parametrize("key", ["sphere", "square"])
def test_the_state_is_untouched(smg, setups, key):
    """state() returns the same bits before and after the product; a following smg_wave_step continues bit for bit as on a second object that never
    ran the product (the kept right-hand side is dropped and formed again to the same bits)"""
    s = setups(key)
    opts = smg.SolveOpts(tol=1e-9, max_iter=30)
    obj, g, p = linearised(smg, s, 3, opts)
    twin, g2, _ = linearised(smg, s, 3, opts)
    more = ricker_signal(smg, STEPS + 2, DT, 3, 3)[STEPS:]
    before = obj.state()
    obj.gauss_newton(direction(s, 3), traces=True, opts=opts)
    for x, y in zip(obj.state(), before):
        assert np.array_equal(x, y)
    a, b = obj.step(2, signal=more, opts=opts), twin.step(2, signal=more, opts=opts)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    for x, y in zip(obj.state(), twin.state()):
        assert np.array_equal(x, y)


def test_one_direction_serves_every_shot(smg, setups):
    """d_cols = 1 against the same column replicated k times: the same bits"""
    s = setups("torus")
    opts = smg.SolveOpts(tol=1e-9, max_iter=30)
    obj, _, _ = linearised(smg, s, 3, opts)
    d = direction(s, 1)
    assert same(obj.gauss_newton(d, traces=True, opts=opts), obj.gauss_newton(np.asfortranarray(np.repeat(d, 3, axis=1)), traces=True, opts=opts))


def test_four_columns_against_single_objects(smg, setups):
    """k = 4 shots in one call against four single-column objects: two device evaluations, each within RELATIVE of exact solves, within twice
    RELATIVE of each other"""
    s = setups("torus")
    k = 4
    u0, v0, src, rec, sig, obs = problem(smg, s, k, seed=9)
    tol, _, _, _, _, d = exact(s, (u0, v0, src, rec, sig, obs), direction(s, k))
    opts = smg.SolveOpts(tol=tol, max_iter=100)
    obj = ready(s.obj(), src, rec, u0, v0)
    obj.gradient(STEPS, signal=sig, observed=obs, opts=opts)
    gn = obj.gauss_newton(d, traces=True, opts=opts)
    parts = []
    for c in range(k):
        one = ready(s.obj(), src, rec, u0[:, c], v0[:, c])
        one.gradient(STEPS, signal=sig[:, :, c:c + 1], observed=obs[:, :, c:c + 1], opts=opts)
        parts.append(one.gauss_newton(d[:, c], traces=True, opts=opts))
    prod, tr = np.concatenate([p.product for p in parts], axis=1), np.concatenate([p.born_traces for p in parts], axis=2)
    dp, dt_ = col(gn.product - prod) / col(prod), np.linalg.norm(gn.born_traces - tr, axis=1).max(axis=0) / np.linalg.norm(tr, axis=1).max(axis=0)
    print("k = 4 columns against four objects: |block - singles| / |singles| product %s, born_traces %s" % (dp, dt_))
    assert np.all(dp <= 2.0 * RELATIVE) and np.all(dt_ <= 2.0 * RELATIVE)
    assert np.allclose(gn.curvature, [p.curvature[0] for p in parts], rtol=4.0 * RELATIVE)


def test_same_calls_same_bits(smg, setups):
    """two calls give identical bits, on one object and on another, graphs on and off, free and clamped"""
    for key in ("sphere", "square"):
        s = setups(key)
        d = direction(s, 3)
        runs = []
        for use_graph in (1, 1, 0):
            opts = smg.SolveOpts(tol=1e-9, max_iter=30, use_graph=use_graph)
            obj, _, _ = linearised(smg, s, 3, opts, seed=13)
            runs.append(obj.gauss_newton(d, traces=True, opts=opts))
            runs.append(obj.gauss_newton(d, traces=True, opts=opts))
        for other in runs[1:]:
            assert same(runs[0], other), key


def refused(smg, call):
    with pytest.raises(smg.SmgError) as e:
        call()
    assert e.value.code == INVALID
    return str(e.value)


def test_the_linearisation_point_lives_as_the_contract_says(smg, setups):
    """refused before any gradient call and after one without a backward pass; kept by step, set_sources, set_state with the same k, a gradient call
    without a backward pass and a refused direction (the product's bits do not move); dropped by set_speed, set_params, set_receivers, set_state
    with another k and a gradient call that fails after its forward half has begun"""
    s = setups("square")
    k = 3
    u0, v0, src, rec, sig, obs = problem(smg, s, k)
    opts = smg.SolveOpts(tol=1e-9, max_iter=30)
    d = direction(s, k)
    obj = ready(s.obj(), src, rec, u0, v0)
    product = lambda: obj.gauss_newton(d, traces=True, opts=opts)   # noqa: E731
    point = lambda: obj.gradient(STEPS, signal=sig, observed=obs, opts=opts)   # noqa: E731
    assert "smg_wave_gradient" in refused(smg, product)
    obj.gradient(STEPS, signal=sig, observed=obs, speed=False, state=False, grad_signal=False, opts=opts)
    assert "no linearisation point" in refused(smg, product)
    obj.set_state(u0, v0)
    point()
    first = product()
    obj.step(2, signal=sig[:3], opts=opts)
    assert same(product(), first), "step keeps the point"
    obj.set_sources(src[:2])
    obj.set_state(v0, u0)
    assert same(product(), first), "set_sources and set_state with the same k keep the point"
    obj.set_sources(src)
    obj.gradient(3, signal=sig[:4], speed=False, state=False, grad_signal=False, opts=opts)
    assert same(product(), first), "a gradient call without a backward pass keeps the point"
    bad = d.copy()
    bad[5, 1] = np.nan
    assert "vertex 5, column 1" in refused(smg, lambda: obj.gauss_newton(bad, opts=opts))
    assert same(product(), first), "a refused direction keeps the point"
    for name, drop in (("set_speed", lambda: obj.set_speed(s.speed * 1.01)), ("set_params", lambda: obj.set_params(dt=DT)),
                       ("set_receivers", lambda: obj.set_receivers(rec)), ("set_state with another k", lambda: obj.set_state(u0[:, :2], v0[:, :2]))):
        obj.set_state(u0, v0)
        point()
        assert product().product.shape == (s.V.shape[0], k)
        drop()
        assert "no linearisation point" in refused(smg, lambda: obj.gauss_newton(d[:, :1], opts=opts)), name
    obj.set_speed(s.speed)
    obj.set_state(u0, v0)
    point()
    nan = u0.copy()
    nan[src[0], 1] = np.nan
    obj.set_state(nan, v0)
    with pytest.raises(smg.SmgError) as e:
        point()
    assert e.value.code == NONFINITE
    obj.set_state(u0, v0)
    assert "no linearisation point" in refused(smg, product), "a gradient call that fails after its forward half has begun drops the point"


def test_a_non_finite_right_hand_side_writes_nothing_and_keeps_the_point(smg, setups):
    """a finite direction whose source overflows: SMG_ERR_NONFINITE at step 0 of the tangent run, no output written, the point kept"""
    s = setups("sphere")
    Lc = smg._lib.load()
    k, n = 2, s.V.shape[0]
    opts = smg.SolveOpts(tol=1e-9, max_iter=30)
    obj, _, p = linearised(smg, s, k, opts)
    d = direction(s, k)
    first = obj.gauss_newton(d, traces=True, opts=opts)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    huge = np.asfortranarray(np.full((n, 1), 1e200))
    prod, tr, cv, cyc = np.full((n, k), N.SENTINEL, order="F"), np.full((STEPS, p[3].size, k), N.SENTINEL), np.full(k, N.SENTINEL), np.full(2 * STEPS, -7, dtype=np.int32)
    rc = Lc.smg_wave_gauss_newton(obj.o, huge.ctypes.data_as(dp), n, 1, None, prod.ctypes.data_as(dp), n, tr.ctypes.data_as(dp), cv.ctypes.data_as(dp), cyc.ctypes.data_as(ip))
    assert rc == NONFINITE and b"smg_wave_gauss_newton" in Lc.smg_last_error() and b"step 0" in Lc.smg_last_error()
    for x in (prod, tr, cv):
        assert np.all(x == N.SENTINEL)
    assert np.all(cyc == -7)
    assert same(obj.gauss_newton(d, traces=True, opts=opts), first)


def test_a_zero_direction_gives_exact_zeros(smg, setups):
    """d = 0: every right-hand side is exactly 0.0, every solve is skipped (cycles 0), product, born_traces and curvature are exact zeros"""
    s = setups("square")
    opts = smg.SolveOpts(tol=1e-9, max_iter=30)
    obj, _, _ = linearised(smg, s, 3, opts)
    z = obj.gauss_newton(np.zeros((s.V.shape[0], 1)), traces=True, opts=opts)
    assert np.all(z.product == 0.0) and np.all(z.born_traces == 0.0) and np.all(z.curvature == 0.0) and np.all(z.cycles == 0) and z.cycles.size == 2 * STEPS


def test_device_bytes_are_live_buffers(smg):
    """smg_wave_device_bytes equals the library's count of live bytes attributable to the object after a product call, grows by the two tangent
    blocks and the plane, is unchanged by a second call of the same shape (and by a smaller one), and the count returns to its start after
    destroy"""
    live = smg._lib.load().smg_device_bytes_live
    for name, clamped in (("icosphere3", False), ("square", True)):
        V, F = N.shape(name)
        n = V.shape[0]
        mg = smg.mg_precompute(V, F, 0.25, COARSEST[name], 1)                  # the caller's hierarchy stays alive throughout
        u0, v0, _ = N.test_state(V, F, 3, clamped)
        src = N.test_lists(V, F, 3, clamped)
        rec = np.concatenate([src, src[:1]]).astype(np.int32)
        sig = ricker_signal(smg, STEPS, DT, 3, 3)
        gc.collect()
        before = live()
        obj = ready(smg.WaveEquation(mg, V, F, DT, speed=N.nonuniform(V)[0], clamped=clamped), src, rec, u0, v0)
        obj.gradient(STEPS, signal=sig)
        grad = obj.device_bytes()
        d = np.cos(V[:, [0]] + np.arange(3)[None, :])
        obj.gauss_newton(d)
        first = obj.device_bytes()
        obj.gauss_newton(d, traces=True)
        obj.gauss_newton(d[:, 0], product=False)
        counted, held = obj.device_bytes(), live() - before
        print("%s, clamped %d: device_bytes %d after the gradient call, %d after the first product call, %d after the third, live DevBuf bytes held %d"
              % (name, clamped, grad, first, counted, held))
        del obj
        gc.collect()
        assert 0 < grad < first == counted == held and first - grad == (2 * 2 * n * 3 + n * 3) * 8 and live() == before


# ---- the refusals that need an object ------------------------------------------------------------------------------------------------------------
def live_calls(smg):
    """-> {name: [code, message]}; nothing may be written by any of them"""
    Lc = smg._lib.load()
    V, F = N.shape("square")
    mg = smg.mg_precompute(V, F, 0.25, COARSEST["square"], 1)
    n, k = V.shape[0], 3
    u0, v0, _ = N.test_state(V, F, k, True)
    inner = N.test_lists(V, F, 3, True)
    make = lambda: ready(smg.WaveEquation(mg, V, F, DT, clamped=True), inner, inner, u0, v0)   # noqa: E731
    sig = np.ones((3, 3, k))
    dp = C.POINTER(C.c_double)
    out = np.full((n, k), N.SENTINEL, order="F")
    O = out.ctypes.data_as(dp)
    d = np.asfortranarray(np.ones((n, k)))
    dbad = d.copy(order="F")
    dbad[5, 1], dbad[9, 2] = np.nan, np.inf
    D, B = d.ctypes.data_as(dp), dbad.ctypes.data_as(dp)
    gn = lambda o, d_=D, ldd=n, cols=k, prod=O, ld=n, tr=None, cv=None: Lc.smg_wave_gauss_newton(o.o, d_, ldd, cols, None, prod, ld, tr, cv, None)   # noqa: E731
    fresh, forward, obj = make(), make(), make()
    forward.gradient(2, signal=sig, speed=False, state=False, grad_signal=False)
    obj.gradient(2, signal=sig)
    dropped = {}
    for name, drop in (("set_speed", lambda o: o.set_speed(np.full(n, 1.1))), ("set_params", lambda o: o.set_params(dt=2 * DT)),
                       ("set_receivers", lambda o: o.set_receivers(inner[:2])), ("set_state with another k", lambda o: o.set_state(u0[:, :2], v0[:, :2]))):
        dropped[name] = make()
        dropped[name].gradient(2, signal=sig)
        drop(dropped[name])
    calls = {"before any gradient call": lambda: gn(fresh),
             "after a gradient call without a backward pass": lambda: gn(forward),
             "after set_speed": lambda: gn(dropped["set_speed"]), "after set_params": lambda: gn(dropped["set_params"]),
             "after set_receivers": lambda: gn(dropped["set_receivers"]),
             "after set_state with another k": lambda: gn(dropped["set_state with another k"], cols=1),
             "d missing": lambda: gn(obj, d_=None),
             "d_cols two of three": lambda: gn(obj, cols=2), "d_cols zero": lambda: gn(obj, cols=0),
             "ldd below nV": lambda: gn(obj, ldd=n - 1),
             "non-finite d": lambda: gn(obj, d_=B),
             "every output missing": lambda: gn(obj, prod=None),
             "leading dimension of product": lambda: gn(obj, ld=n - 1),
             "order: the point before d": lambda: gn(fresh, d_=None),
             "order: d before d_cols": lambda: gn(obj, d_=None, cols=2),
             "order: d_cols before ldd": lambda: gn(obj, cols=2, ldd=n - 1),
             "order: ldd before a non-finite d": lambda: gn(obj, d_=B, ldd=n - 1),
             "order: a non-finite d before the outputs": lambda: gn(obj, d_=B, prod=None),
             "order: the outputs before ld": lambda: gn(obj, prod=None, ld=n - 1)}
    got = {}
    for name, call in calls.items():
        rc = call()
        got[name] = [rc, Lc.smg_last_error().decode()]
    assert np.all(out == N.SENTINEL)
    u, v = fresh.state()
    assert np.array_equal(u, u0) and np.array_equal(v, v0)
    r = obj.gauss_newton(d)                                                    # the refused calls have changed nothing
    assert r.product.shape == (n, k) and np.all(r.curvature > 0.0)
    return got


def test_live_refusals(smg):
    """the refusals that need an object: code and text as recorded in tests/golden/wave_gn_refusals.json, group "live"; nothing is written"""
    golden = json.load(open(GOLDEN))["live"]
    got = live_calls(smg)
    assert set(got) == set(golden)
    for name, (rc, msg) in got.items():
        assert [rc, msg] == golden[name] and rc == INVALID, name


# ---- one truncated-Newton step -------------------------------------------------------------------------------------------------------------------
class DeviceEngine:
    """wave_gn_np.newton_step's engine on one WaveEquation"""

    def __init__(self, smg, obj, u0, v0, sig, data, opts):
        self.obj, self.u0, self.v0, self.sig, self.data, self.opts = obj, u0, v0, sig, data, opts

    def gradient(self, speed):
        self.obj.set_speed(speed)
        self.obj.set_state(self.u0, self.v0)
        r = self.obj.gradient(STEPS, signal=self.sig, observed=self.data, state=False, grad_signal=False, opts=self.opts)
        return float(r.misfit.sum()), r.grad_speed.sum(axis=1)

    def product(self, d):
        return self.obj.gauss_newton(d, opts=self.opts).product.sum(axis=1)

    def misfit(self, speed):
        self.obj.set_speed(speed)
        self.obj.set_state(self.u0, self.v0)
        return float(self.obj.gradient(STEPS, signal=self.sig, observed=self.data, speed=False, state=False, grad_signal=False, opts=self.opts).misfit.sum())


def test_one_truncated_newton_step_lowers_the_misfit(smg, setups):
    """NEWTON of the header"""
    s = setups("sphere")
    k = 2
    u0, v0 = s.state(k)
    src, rec = lists(s)
    sig = ricker_signal(smg, STEPS, DT, 3, k)
    true = s.speed * (1.0 + 0.2 * np.exp(-4.0 * np.sum((s.V - s.V[rec[0]]) ** 2, axis=1)))
    opts = smg.SolveOpts(tol=1e-10, max_iter=100)
    data = ready(smg.WaveEquation(s.mg, s.V, s.F, DT, speed=true), src, rec, u0, v0).step(STEPS, signal=sig, energy=False, opts=opts)[1]
    engine = DeviceEngine(smg, ready(s.obj(), src, rec, u0, v0), u0, v0, sig, data, opts)
    step = G.newton_step(engine, s.speed.copy())
    sd = G.descent_step(engine, s.speed.copy())
    print("icosphere3, one truncated-Newton step: misfit %.6e -> %.6e, alpha %g after %s halvings, lambda %.3e, <d, H d> per iteration %s; one steepest-descent step: "
          "%.6e after %s halvings; |speed - true| / |start - true| %.4f" % (step["J"], step["Jt"], step["alpha"], step["found"], step["lam"], step["curvatures"], sd["Jt"],
                                                                           sd["found"], np.linalg.norm(step["trial"] - true) / np.linalg.norm(s.speed - true)))
    assert step["found"] is not None and step["Jt"] < step["J"] and step["slope"] < 0.0 and all(c > 0.0 for c in step["curvatures"])
    assert sd["found"] is not None and step["Jt"] < sd["Jt"] < sd["J"]
