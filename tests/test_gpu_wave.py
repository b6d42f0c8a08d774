"""GPU (-m gpu): the wave equation on a surface (include/smg.h: smg_wave_*).

The host references are tests/wave_np.py -- the method in the kernels' operation order with direct solves -- and the library's own host twin
(smg_wave_host), which compiles the text the kernels compile.  The kernels are held launcher by launcher (smg_debug_wave, guarded buffers, every
output pre-filled with sentinels) bit for bit against the restatement and against the host twin: only +, - and * occur, so there is nothing to
bound.

End to end against WaveNp's direct solves (the library's own L).  A = diag(0.5 s2 mt) + a C, mu = min_i 0.5 s2_i mt_i, | | the 2-norm of one column
(of u and v together where both are meant), eps = 2^-52, tol = the solves' stopping tolerance as an absolute residual norm (the tests pass it:
1e-12 of the largest |b|_F of the run), res_np = the direct solve's residual.

    ONE STEP   from equal states the right-hand sides are equal bit for bit (asserted through the hook).  C is positive semi-definite, so
               lambda_min(A) >= mu, and a principal submatrix (clamped) obeys the same bound:
                   |u'_dev - u'_np| <= beta = (10 tol + res_np) / mu,     |v'_dev - v'_np| <= q2 beta            (the issue's statement)
    CHAIN      the unforced step is linear, (u', v') = S (u, v); wave_np.step_map forms S densely (at most 1284 x 1284) with exact inverses.  Two
               runs of the same steps from equal states are apart by e_n = S e_(n-1) + delta_n, so |e_n| <= sum_j |S^(n-j)|_2 delta_j, the norms
               from numpy.  delta_j is the step's own injection:
                 - the two solves: beta_j in w, so beta_j in u' and q2 beta_j in v': sqrt(1 + q2^2) beta_j;
                 - b = mt (s2 u + dt v) is two products, a sum and a product, and a source adds a product and two sums: on different inputs the two
                   sides round differently by at most 4 eps mag_b each, mag_b = mt (|s2 u| + dt |v|) + a |f_n + f_n+1|; through the solve this
                   is 8 eps |mag_b| / mu more in beta_j;
                 - u' = w - u is one rounding per side, 2 eps |u'|; v' = q2 (u' - u) - v carries it times q2 and adds a difference, a product and a
                   difference: 2 eps (q2 |u'| + 2 q2 |u' - u| + |v'|).
                   delta_j = sqrt(1 + q2^2) (beta_j + 8 eps |mag_b| / mu) + 2 eps sqrt(|u'|^2 + (q2 |u'| + 2 q2 |u' - u| + |v'|)^2)
               (wave_np.Chain).  Asserted at every one of 20 steps; the test fails if the bound ever exceeds 1e-3 of the amplitude.
    INVARIANTS the identities of tests/test_wave_host.py on the DEVICE's states, read back after every step.  The reported energies equal the
               restatement's energy function of the read-back state bit for bit (the same kernels' terms in the fixed sums' order), so the
               sums' rounding is not a separate term: E below is the exact-arithmetic form 0.5 v' Mt v + 0.5 u' C u evaluated in numpy, whose own
               rounding SLACK (test_wave_host.wave_slack) bounds term by term.  With r = A (u + u') - b measured in numpy from the device's
               states the power balance holds within SLACK; with the solve's promise |r| <= 10 tol alone
                   |E' - E + dt vbar' Sigma Mt vbar - dt vbar' fbar| <= |v + v'| 10 tol / dt + SLACK,
               momentum within q2 (sqrt(nV) (10 tol + 4 eps |mag_b|) + a d |w|) + |mt| eps (q2 |u'| + 2 q2 |u' - u| + |v'|), and an eigenmode's
               amplitude and phase within CHAIN plus the restatement's own distance to the closed form (EIGENMODE of the CPU file, asserted
               here too).
    PAIRS      two device runs of the same steps (reciprocal shots, k columns against single objects, set_params against a fresh object) are
               each within CHAIN of the restatement: within twice CHAIN of each other."""
import ctypes as C
import gc
import json
import math

import numpy as np
import pytest

import wave_np as N
from rd_np import row_sum_defect
from test_gpu_parity import smg  # noqa: F401  (fixture)
from test_wave_host import (GOLDEN, INVALID, eigenmode_bounds, host_run, launcher_cases, mode_recurrence, power_terms, ricker_signal, wave_slack)

pytestmark = pytest.mark.gpu

COARSEST = {"icosphere3": 50, "torus": 50, "square": 20}
NONFINITE = -4
EPS = N.EPS
DT = 0.05


def hook_run(smg):
    def run(op, V, F, **kw):
        rc, bad, out = N.hook(smg, op, V, F, **kw)
        assert rc == 0 and bad == 0, (rc, bad)
        return out
    return run


# ---- kernels, launcher by launcher -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", N.LAUNCHER_MESHES + N.PYRAMIDS)
def test_hook_against_restatement_and_host_twin(smg, name):
    """every op alone, k = 1, 3, 8, free and clamped, lists of 1 and 3 vertices that contain vertex 0 and vertex nV - 1: no guard touched, nothing
    past the extent, nothing of it left at the sentinel (wave_np._call); ADVANCE's next right-hand side equals RHS of (u', v') bit for bit
    (wave_np.check_launchers).  icosphere1 has 42 vertices: a wavefront holds fewer than 64 and the waves of different columns share a block"""
    for k in (1, 3, 8):
        for clamped, count in launcher_cases(name):
            dev = N.check_launchers(hook_run(smg), name, k, clamped, count)
            hst = N.check_launchers(host_run(smg), name, k, clamped, count)
            for op, (a, b) in enumerate(zip(dev, hst)):
                assert np.array_equal(a, b), (name, k, clamped, count, op)


# ---- the objects ----------------------------------------------------------------------------------------------------------------------------------
SETUPS = {"sphere": dict(name="icosphere3", clamped=0, sigma=False), "torus": dict(name="torus", clamped=0, sigma=True),
          "square": dict(name="square", clamped=1, sigma=True), "square free": dict(name="square", clamped=0, sigma=True)}


class Setup:
    """a mesh, its hierarchy, the library's own L, the fields speed and sigma, and per dt the restatement's dense step map's power norms"""

    def __init__(self, smg, key):
        self.smg, self.cfg = smg, SETUPS[key]
        self.V, self.F = N.shape(self.cfg["name"])
        self.mg = smg.mg_precompute(self.V, self.F, 0.25, COARSEST[self.cfg["name"]], 1)
        assert self.mg.n_levels >= 2
        self.L = smg.mesh.cotmatrix(self.V, self.F)                            # the library's own L: the system's bits
        self.speed, sig = N.nonuniform(self.V)
        self.sigma = sig if self.cfg["sigma"] else None
        self.clamped = self.cfg["clamped"]
        self._norms = {}

    def ref(self, dt=DT, damping=0.0):
        return N.WaveNp(self.V, self.F, L=self.L, speed=self.speed, sigma=self.sigma, dt=dt, damping=damping, clamped=self.clamped)

    def obj(self, dt=DT, damping=0.0):
        return self.smg.WaveEquation(self.mg, self.V, self.F, dt, speed=self.speed, sigma=self.sigma, damping=damping, clamped=bool(self.clamped))

    def norms(self, dt=DT, damping=0.0):
        if (dt, damping) not in self._norms:
            self._norms[(dt, damping)] = N.power_norms(self.ref(dt, damping).step_map(), 20)
        return self._norms[(dt, damping)]

    def state(self, k):
        u, v, _ = N.test_state(self.V, self.F, k, bool(self.clamped))
        return u, v

    def lists(self, count):
        return N.test_lists(self.V, self.F, count, bool(self.clamped))


@pytest.fixture(scope="module")
def setups(smg):
    cache = {}

    def get(key):
        if key not in cache:
            cache[key] = Setup(smg, key)
        return cache[key]
    yield get
    cache.clear()
    gc.collect()


def run_tol(ref, u0, v0, steps, signal=None, rel=1e-12):
    """rel times the largest |b|_F of the restatement's run of `steps` steps, which leaves `ref` at its start again: the absolute tolerance the tests
    pass to every solve"""
    ref.set_state(u0, v0)
    top = 0.0
    for t in range(steps):
        ref.step(1, None if signal is None else signal[t:t + 2])
        top = max(top, float(np.sqrt(ref.ss)))
    ref.set_state(u0, v0)
    return rel * top


@pytest.mark.parametrize("key", list(SETUPS))
def test_one_step_against_direct_solves(smg, setups, key):
    """ONE STEP of the header: icosphere3, torus and the square free and clamped, k = 3, non-uniform speed (and sigma except on the sphere), three
    sources; the energies against the restatement's energy function of the read-back state and the traces against the read-back u, bit for bit"""
    s = setups(key)
    k = 3
    u0, v0 = s.state(k)
    src, rec = s.lists(3), s.lists(3)[::-1]
    sig = ricker_signal(smg, 1, DT, 3, k)
    ref = s.ref()
    ref.src, ref.rec = src, rec
    tol = run_tol(ref, u0, v0, 1, sig)
    obj = s.obj()
    obj.set_sources(src)
    obj.set_receivers(rec)
    obj.set_state(u0, v0)
    E, tr, cyc = obj.step(1, signal=sig, opts=smg.SolveOpts(tol=tol, max_iter=100))
    u, v = obj.state()
    En, trn = ref.step(1, sig)
    common = dict(k=k, speed=s.speed, sigma=s.sigma, clamped=s.clamped, dt=DT, u=u0, v=v0)
    b_dev = N.unpack(N.WAVE_SOURCES, hook_run(smg)(N.WAVE_SOURCES, s.V, s.F, idx=src, sig0=sig[0], sig1=sig[1], **common), s.V.shape[0], k, 3)
    assert np.array_equal(b_dev[0], ref.b) and b_dev[3] == ref.ss, "the right-hand sides are equal bit for bit"
    beta = (10.0 * tol + ref.res) / ref.mu
    eu, ev = np.linalg.norm(u - ref.u, axis=0), np.linalg.norm(v - ref.v, axis=0)
    print("%s: tol %.2e, res_np %.2e, mu %.3e; |u'_dev - u'_np| %s, |v'_dev - v'_np| %s; largest ratio to beta %.4f, to q2 beta %.4f; cycles %s"
          % (key, tol, ref.res.max(), ref.mu, eu, ev, float(np.max(eu / beta)), float(np.max(ev / (ref.q2 * beta))), cyc))
    assert np.all(eu <= beta) and np.all(ev <= ref.q2 * beta) and cyc[0] > 0
    assert np.array_equal(E[0], np.concatenate(ref.energy(u, v))) and np.array_equal(tr[0], u[rec])
    assert np.allclose(E, En, rtol=1e-6) and np.allclose(tr, trn, atol=float(np.max(beta)))
    if s.clamped:
        assert np.all(u[ref.known] == 0.0) and np.all(v[ref.known] == 0.0), "exact zeros on the clamped rows"


def run_chained(smg, s, u0, v0, steps, signal=None, src=None, closed=None, label="", dt=DT, damping=0.0):
    """`steps` single steps of an object and of the restatement from equal states; CHAIN asserted at every step, and that it stays below 1e-3 of
    the amplitude.  closed(n) -> (u, v, bound) of a closed form after n steps.  Returns (the object, the restatement, the bounds, the tolerance)"""
    ref = s.ref(dt, damping)
    if src is not None:
        ref.src = src
    tol = run_tol(ref, u0, v0, steps, signal)
    opts = smg.SolveOpts(tol=tol, max_iter=100)
    obj = s.obj(dt, damping)
    if src is not None:
        obj.set_sources(src)
    obj.set_state(u0, v0)
    chain = N.Chain(ref, tol, s.norms(dt, damping))
    amp, worst, bounds = 0.0, 0.0, []
    for n in range(1, steps + 1):
        f = (None, None) if signal is None else (signal[n - 1], signal[n])
        ref.step(1, None if signal is None else signal[n - 1:n + 1])
        bounds.append(chain.after(*f))
        obj.step(1, signal=None if signal is None else signal[n - 1:n + 1], energy=False, opts=opts)
        u, v = obj.state()
        err = N.distance(u, v, ref.u, ref.v)
        amp = np.maximum(amp, np.sqrt(np.sum(ref.u ** 2 + ref.v ** 2, axis=0)))
        line = "%s step %2d: |dev - np|_2 %s, CHAIN %s" % (label, n, err, bounds[-1])
        assert np.all(bounds[-1] <= 1e-3 * amp), "the chained bound is useless at step %d: %s against the amplitude %s" % (n, bounds[-1], amp)
        assert np.all(err <= bounds[-1]), line
        worst = max(worst, float(np.max(err / bounds[-1])))
        if closed is not None:
            cu, cv, cb = closed(n)
            e_np, e_dev = N.distance(ref.u, ref.v, cu, cv), N.distance(u, v, cu, cv)
            line += "; |np - closed|_2 %s (bound %s), |dev - closed|_2 %s" % (e_np, cb, e_dev)
            assert np.all(e_np <= cb) and np.all(e_dev <= bounds[-1] + cb), line
        if n in (1, steps):
            print(line)
    print("%s: largest |dev - np|_2 over CHAIN in %d steps %.4f (|S^19|_2 %.3e)" % (label, steps, worst, s.norms(dt, damping)[-1]))
    return obj, ref, bounds, tol


@pytest.mark.parametrize("key", ["sphere", "torus", "square"])
def test_twenty_steps_stay_within_the_chained_bound(smg, setups, key):
    """CHAIN of the header, k = 3, three Ricker sources, at every one of 20 steps"""
    s = setups(key)
    u0, v0 = s.state(3)
    run_chained(smg, s, u0, v0, 20, signal=ricker_signal(smg, 20, DT, 3, 3), src=s.lists(3), label=key)


def shadow(ref, u0, v0, u1, v1, f0=None, f1=None):
    """`ref` made to hold a device step: the states before and after it, w = u + u' and the right-hand side of the state before (the restatement's
    expression, which the launcher test holds the device to bit for bit)"""
    ref.u, ref.v = u0, v0
    ref.b = ref.right_hand_side(f0, f1)[0]
    ref.u0, ref.v0, ref.u, ref.v, ref.w = u0, v0, u1, v1, u0 + u1


@pytest.mark.parametrize("case", ["undamped, unforced", "damping", "a Ricker source"])
@pytest.mark.parametrize("key", ["torus", "square"])
def test_the_power_balance_holds_on_the_device(smg, setups, key, case):
    """INVARIANTS of the header over 20 steps, k = 2: the energy of an undamped unforced run, and the power balance with damping (the setup's
    non-uniform sigma) and with a source"""
    s = setups(key)
    n = s.V.shape[0]
    damped, forced = case == "damping", case == "a Ricker source"
    ref = N.WaveNp(s.V, s.F, L=s.L, speed=s.speed, sigma=s.sigma if damped else None, dt=DT, clamped=s.clamped)
    obj = smg.WaveEquation(s.mg, s.V, s.F, DT, speed=s.speed, sigma=s.sigma if damped else None, clamped=bool(s.clamped))
    u0, v0 = s.state(2)
    src = s.lists(3)
    sig = ricker_signal(smg, 20, DT, 3, 2) if forced else None
    ref.src = src
    tol = run_tol(ref, u0, v0, 20, sig)
    obj.set_sources(src)
    obj.set_state(u0, v0)
    E, _, cyc = obj.step(20, signal=sig, opts=smg.SolveOpts(tol=tol, max_iter=100))
    obj.set_state(u0, v0)
    up, vp, worst, worst_r, top_r = u0, v0, 0.0, 0.0, 0.0
    for t in range(20):
        f = (None, None) if sig is None else (sig[t], sig[t + 1])
        Et, _, _ = obj.step(1, signal=None if sig is None else sig[t:t + 2], opts=smg.SolveOpts(tol=tol, max_iter=100))
        u, v = obj.state()
        assert np.array_equal(Et[0], E[t]) and np.array_equal(Et[0], np.concatenate(ref.energy(u, v))), "the energies are the read-back state's, bit for bit"
        shadow(ref, up, vp, u, v, *f)
        dE, rate, vs = power_terms(ref, *f)
        slack = wave_slack(ref, *f)[0]
        r = ref.residual(ref.w, ref.b)
        rterm = np.sum(vs * r, axis=0) / DT
        top_r = max(top_r, float(np.linalg.norm(r, axis=0).max() / tol))
        worst_r = max(worst_r, float(np.max(np.abs(dE - rate - rterm) / slack)))
        bound = np.linalg.norm(vs, axis=0) * 10.0 * tol / DT + slack
        worst = max(worst, float(np.max(np.abs(dE - rate) / bound)))
        assert np.all(np.abs(dE - rate - rterm) <= slack), (t, dE, rate, rterm, slack)
        assert np.all(np.abs(dE - rate) <= bound), (t, dE, rate, bound)
        up, vp = u, v
    E0, E1 = ref.E(u0, v0), ref.E(up, vp)
    print("%s, %s: E %s -> %s; largest |E' - E - terms| over |v + v'| 10 tol / dt + slack %.4f, with the measured r over slack %.4f; largest |r| / tol %.3f"
          % (key, case, E0, E1, worst, worst_r, top_r))
    if case == "undamped, unforced":
        assert np.all(np.abs(E1 - E0) <= 20 * bound)
    if damped:
        assert np.all(E1 < E0)
    assert n > 0 and np.all(cyc > 0)


def test_momentum_is_kept_on_the_sphere(smg, setups):
    """INVARIANTS of the header: sum mt v' = sum mt v + dt sum fbar on icosphere3 (free, sigma = 0) at every one of 20 steps with three sources"""
    s = setups("sphere")
    n = s.V.shape[0]
    ref, obj = s.ref(), s.obj()
    u0, v0 = s.state(2)
    src = s.lists(3)
    sig = ricker_signal(smg, 20, DT, 3, 2)
    ref.src = src
    tol = run_tol(ref, u0, v0, 20, sig)
    obj.set_sources(src)
    obj.set_state(u0, v0)
    d = row_sum_defect(ref.C)
    fs = lambda x: np.array([math.fsum(ref.mt * c) for c in x.T])   # noqa: E731
    up, vp, worst = u0, v0, 0.0
    for t in range(20):
        obj.step(1, signal=sig[t:t + 2], energy=False, opts=smg.SolveOpts(tol=tol, max_iter=100))
        u, v = obj.state()
        shadow(ref, up, vp, u, v, sig[t], sig[t + 1])
        dv = wave_slack(ref, sig[t], sig[t + 1])[1]
        mag = ref.mt[:, None] * (np.abs(ref.s2[:, None] * up) + DT * np.abs(vp))
        mag[src] += ref.a * np.abs(sig[t] + sig[t + 1])
        bound = ref.q2 * (np.sqrt(n) * (10.0 * tol + 4 * EPS * np.linalg.norm(mag, axis=0)) + ref.a * d * np.linalg.norm(ref.w, axis=0)) + np.linalg.norm(ref.mt) * dv
        defect = np.abs(fs(v) - fs(vp) - DT * np.sum(0.5 * (sig[t] + sig[t + 1]), axis=0))
        worst = max(worst, float(np.max(defect / bound)))
        assert np.all(defect <= bound), (t, defect, bound)
        up, vp = u, v
    print("icosphere3: sum mt v %s -> %s; largest defect over its bound %.4f (last bound %s)" % (fs(v0), fs(vp), worst, bound))
    assert np.all(np.abs(fs(vp) - fs(v0)) > 1e3 * bound)


def test_an_eigenmode_keeps_its_amplitude_and_phase(smg, setups):
    """INVARIANTS of the header on icosphere3, undamped, three columns (a low mode, a middle one and the highest): within CHAIN of the
    restatement and within CHAIN plus EIGENMODE (tests/test_wave_host.py) of (alpha_n phi, beta_n phi), whose amplitude is constant and whose
    phase is n theta, theta = 2 atan(dt sqrt(lambda) / 2)"""
    import scipy.linalg
    s = setups("sphere")
    ref = s.ref()
    Cd = np.asarray(ref.C.todense())
    lam, phi = scipy.linalg.eigh(0.5 * (Cd + Cd.T), np.diag(ref.mt))
    cols = np.array([1, 7, lam.size - 1])
    lc = lam[cols]
    res = np.linalg.norm(Cd @ phi[:, cols] - (ref.mt[:, None] * phi[:, cols]) * lc[None, :], axis=0)
    amps = mode_recurrence(ref, lc, [1.0, -0.5, 0.25], [0.3, 1.0, -2.0], 20)
    u0, v0 = phi[:, cols] * amps[0][0], phi[:, cols] * amps[0][1]
    ref.set_state(u0, v0)
    cb = eigenmode_bounds(ref, lc, res, s.norms(), amps, 20)

    def closed(n):
        return phi[:, cols] * amps[n][0], phi[:, cols] * amps[n][1], cb[n - 1]
    obj, ref, bounds, _ = run_chained(smg, s, u0, v0, 20, closed=closed, label="icosphere3, eigenmodes")
    u, v = obj.state()
    al, be = np.sum(phi[:, cols] * (ref.mt[:, None] * u), axis=0), np.sum(phi[:, cols] * (ref.mt[:, None] * v), axis=0)   # M-inner products with unit vectors
    theta = 2.0 * np.arctan(0.5 * DT * np.sqrt(lc))
    rad0, rad = np.sqrt(amps[0][0] ** 2 + amps[0][1] ** 2 / lc), np.sqrt(al ** 2 + be ** 2 / lc)
    turned = np.arctan2(amps[0][1] / np.sqrt(lc), amps[0][0]) - np.arctan2(be / np.sqrt(lc), al)
    off = np.abs(np.angle(np.exp(1j * (turned - 20 * theta))))
    slack = np.sqrt(ref.mt.max()) * (bounds[-1] + cb[-1]) * np.maximum(1.0, 1.0 / np.sqrt(lc))
    print("icosphere3: lambda %s, theta %s; amplitude %s -> %s, phase turned %s against 20 theta %s (bound on both %s)" % (lc, theta, rad0, rad, turned, 20 * theta, slack))
    assert np.all(np.abs(rad - rad0) <= slack + 64 * 20 * EPS * rad0) and np.all(off * rad0 <= 2 * slack + 64 * 20 * EPS * rad0)


def test_reciprocity_of_two_shots(smg, setups):
    """PAIRS of the header on icosphere3 from rest: ONE k = 2 call, column 0 driven at p, column 1 driven at q != p, receivers {p, q}:
    traces[:, q, 0] against traces[:, p, 1] at every one of 20 steps within twice CHAIN"""
    s = setups("sphere")
    n = s.V.shape[0]
    p, q = int(s.F[0, 0]), int(s.F[0, 1])                                      # neighbours: the wave from one reaches the other within the run
    wavelet = smg.wavelets.ricker(2.0, DT * np.arange(21), 0.3)
    sig = np.zeros((21, 2, 2))
    sig[:, 0, 0], sig[:, 1, 1] = wavelet, wavelet
    zero = np.zeros((n, 2))
    ref = s.ref()
    ref.src, ref.rec = np.array([p, q]), np.array([p, q])
    tol = run_tol(ref, zero, zero, 20, sig)
    chain = N.Chain(ref, tol, s.norms())
    bounds = []
    for t in range(20):
        ref.step(1, sig[t:t + 2])
        bounds.append(chain.after(sig[t], sig[t + 1]))
    obj = s.obj()
    obj.set_sources([p, q])
    obj.set_receivers([p, q])
    obj.set_state(zero, zero)
    _, tr, cyc = obj.step(20, signal=sig, energy=False, opts=smg.SolveOpts(tol=tol, max_iter=100))
    a, b = tr[:, 1, 0], tr[:, 0, 1]
    twice = 2.0 * np.array([bd.max() for bd in bounds])
    print("icosphere3, shots at %d and %d: largest trace %.3e, largest |trace(q; p) - trace(p; q)| %.3e, largest ratio to twice CHAIN %.4f (last twice CHAIN %.3e)"
          % (p, q, np.abs(a).max(), np.abs(a - b).max(), float(np.max(np.abs(a - b) / twice)), twice[-1]))
    assert np.all(np.abs(a - b) <= twice) and twice[-1] <= 1e-3 * np.abs(a).max() and not np.array_equal(tr[:, 0, 0], tr[:, 1, 1])


def chain_bound(s, u0, v0, steps, signal=None, src=None, dt=DT):
    ref = s.ref(dt)
    if src is not None:
        ref.src = src
    tol = run_tol(ref, u0, v0, steps, signal)
    chain, bound = N.Chain(ref, tol, s.norms(dt)), None
    for t in range(steps):
        ref.step(1, None if signal is None else signal[t:t + 2])
        bound = chain.after(*((None, None) if signal is None else (signal[t], signal[t + 1])))
    return tol, bound, ref


def test_eight_columns_against_single_objects(smg, setups):
    """PAIRS of the header on the torus: k = 8 columns with their own signals against eight single-column objects, 5 steps"""
    s = setups("torus")
    u0, v0 = s.state(8)
    src = s.lists(3)
    sig = ricker_signal(smg, 5, DT, 3, 8)
    tol, bound, ref = chain_bound(s, u0, v0, 5, sig, src)
    opts = smg.SolveOpts(tol=tol, max_iter=100)
    obj = s.obj()
    obj.set_sources(src)
    obj.set_state(u0, v0)
    obj.step(5, signal=sig, energy=False, opts=opts)
    u, v = obj.state()
    su, sv = [], []
    for c in range(8):
        o = s.obj()
        o.set_sources(src)
        o.set_state(u0[:, c], v0[:, c])
        o.step(5, signal=sig[:, :, c:c + 1], energy=False, opts=opts)
        a, b = o.state()
        su.append(a[:, 0]), sv.append(b[:, 0])
    su, sv = np.stack(su, axis=1), np.stack(sv, axis=1)
    d = N.distance(u, v, su, sv)
    print("k = 8 columns, 5 steps: |block - singles|_2 %s, twice CHAIN %s; block against the restatement %s" % (d, 2 * bound, N.distance(u, v, ref.u, ref.v)))
    assert np.all(d <= 2 * bound) and np.all(N.distance(u, v, ref.u, ref.v) <= bound)


def test_two_calls_of_ten_equal_one_call_of_twenty(smg, setups):
    """the right-hand side kept across calls is the one a call recomputes: states, energies, traces and cycles are equal bit for bit; and a
    set_state of the same state in between (which drops the kept right-hand side) changes nothing either"""
    s = setups("square")
    u0, v0 = s.state(3)
    src, rec = s.lists(3), s.lists(3)
    sig = ricker_signal(smg, 20, DT, 3, 3)
    opts = smg.SolveOpts(tol=1e-9, max_iter=30)
    outs = []
    for split in (False, True, "reset"):
        obj = s.obj()
        obj.set_sources(src)
        obj.set_receivers(rec)
        obj.set_state(u0, v0)
        if not split:
            E, tr, cyc = obj.step(20, signal=sig, opts=opts)
        else:
            E1, tr1, cyc1 = obj.step(10, signal=sig[:11], opts=opts)
            if split == "reset":
                obj.set_state(*obj.state())
            E2, tr2, cyc2 = obj.step(10, signal=sig[10:], opts=opts)
            E, tr, cyc = np.concatenate([E1, E2]), np.concatenate([tr1, tr2]), np.concatenate([cyc1, cyc2])
        outs.append([E, tr, cyc] + list(obj.state()))
    for other in outs[1:]:
        for x, y in zip(outs[0], other):
            assert np.array_equal(x, y)
    assert outs[0][1].shape == (20, 3, 3) and np.any(outs[0][1] != 0.0)


def test_the_two_kernel_step_gives_the_same_bits(smg, setups, monkeypatch):
    """SMG_WAVE_FUSED=0 at create (the A/B knob of tools/wave_time.py: k_wave_rhs before every solve, k_wave_advance without the next right-hand
    side) against the default, 6 forced steps in two calls, free and clamped: states, energies, traces and cycles are equal bit for bit"""
    for key in ("sphere", "square"):
        s = setups(key)
        u0, v0 = s.state(3)
        src = s.lists(3)
        sig = ricker_signal(smg, 6, DT, 3, 3)
        runs = []
        for fused in ("1", "0"):
            monkeypatch.setenv("SMG_WAVE_FUSED", fused)
            obj = s.obj()
            monkeypatch.delenv("SMG_WAVE_FUSED")
            obj.set_sources(src)
            obj.set_receivers(src)
            obj.set_state(u0, v0)
            a = obj.step(4, signal=sig[:5], opts=smg.SolveOpts(tol=1e-9, max_iter=30))
            b = obj.step(2, signal=sig[4:], opts=smg.SolveOpts(tol=1e-9, max_iter=30))
            runs.append(list(a) + list(b) + list(obj.state()))
        for x, y in zip(*runs):
            assert np.array_equal(x, y), key


def test_set_params_to_a_new_dt_against_a_fresh_object(smg, setups):
    """PAIRS of the header on the torus: an object created with dt = 0.025 and set to dt = 0.05 (a value-only re-precompute), then 3 steps,
    against a fresh object created with dt = 0.05: within twice CHAIN; whether bitwise is printed.  A change of clamped is refused"""
    s = setups("torus")
    u0, v0 = s.state(2)
    tol, bound, ref = chain_bound(s, u0, v0, 3)
    opts = smg.SolveOpts(tol=tol, max_iter=100)
    outs = []
    for first_dt in (0.025, DT):
        o = s.obj(first_dt)
        o.set_state(u0, v0)
        if first_dt != DT:
            o.step(1, opts=opts)                                              # the old matrix is used once before it is replaced
            o.set_params(dt=DT)
            o.set_state(u0, v0)
        o.step(3, opts=opts)
        outs.append(o.state())
    d = N.distance(outs[0][0], outs[0][1], outs[1][0], outs[1][1])
    print("set_params(dt) against a fresh object, 3 steps: |difference|_2 %s, twice CHAIN %s, bitwise %s"
          % (d, 2 * bound, np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])))
    assert np.all(d <= 2 * bound) and np.all(N.distance(outs[1][0], outs[1][1], ref.u, ref.v) <= bound)
    with pytest.raises(smg.SmgError) as e:
        o.set_params(clamped=1)
    assert e.value.code == INVALID and "smg_wave_set_params" in str(e.value)


def test_a_nan_is_refused_and_the_state_is_kept(smg, setups):
    """a NaN in the signal is SMG_ERR_INVALID before anything runs; a NaN in u ends the call with SMG_ERR_NONFINITE at step 0, n_done == 0, nothing
    written past the histories' start; after a valid set_state the next call equals a fresh object's to the bit"""
    s = setups("sphere")
    Lc = smg._lib.load()
    k = 2
    u0, v0 = s.state(k)
    src = s.lists(3)
    sig = ricker_signal(smg, 3, DT, 3, k)
    obj = s.obj()
    obj.set_sources(src)
    obj.set_receivers(src)
    obj.set_state(u0, v0)
    obj.step(2, signal=sig[:3])
    kept = obj.state()
    bad_sig = sig.copy()
    bad_sig[2, 1, 1] = np.nan
    with pytest.raises(smg.SmgError) as e:
        obj.step(3, signal=bad_sig)
    assert e.value.code == INVALID and "time 2, source 1, column 1" in str(e.value) and obj.n_done == 0
    for x, y in zip(obj.state(), kept):
        assert np.array_equal(x, y)
    bad = u0.copy()
    bad[77, 1] = np.nan
    obj.set_state(bad, v0)
    E, tr, cyc = np.full((3, 2 * k), N.SENTINEL), np.full((3, 3, k), N.SENTINEL), np.full(3, -7, dtype=np.int32)
    nd = C.c_int(-1)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    rc = Lc.smg_wave_step(obj.o, 3, sig.ctypes.data_as(dp), None, E.ctypes.data_as(dp), tr.ctypes.data_as(dp), cyc.ctypes.data_as(ip), C.byref(nd))
    assert rc == NONFINITE and nd.value == 0 and b"smg_wave_step" in Lc.smg_last_error() and b"step 0" in Lc.smg_last_error()
    assert np.all(E == N.SENTINEL) and np.all(tr == N.SENTINEL) and np.all(cyc == -7)
    with pytest.raises(smg.SmgError) as e:
        obj.step(3)
    assert e.value.code == NONFINITE and obj.n_done == 0
    ku, kv = obj.state()
    assert np.isnan(ku[77, 1]) and np.array_equal(np.delete(ku, 77, axis=0), np.delete(bad, 77, axis=0)) and np.array_equal(kv, v0)
    obj.set_state(u0, v0)
    fresh = s.obj()
    fresh.set_sources(src)
    fresh.set_receivers(src)
    fresh.set_state(u0, v0)
    for x, y in zip(obj.step(2, signal=sig[:3]), fresh.step(2, signal=sig[:3])):
        assert np.array_equal(x, y)
    for x, y in zip(obj.state(), fresh.state()):
        assert np.array_equal(x, y)


def test_same_calls_same_bits(smg, setups):
    """two runs of 10 forced steps give identical bits, graphs on and off, free and clamped"""
    for key in ("sphere", "square"):
        s = setups(key)
        u0, v0 = s.state(3)
        src = s.lists(3)
        sig = ricker_signal(smg, 10, DT, 3, 3)
        runs = []
        for use_graph in (1, 1, 0):
            obj = s.obj()
            obj.set_sources(src)
            obj.set_receivers(src)
            obj.set_state(u0, v0)
            out = obj.step(10, signal=sig, opts=smg.SolveOpts(tol=1e-9, max_iter=30, use_graph=use_graph))
            runs.append(list(out) + list(obj.state()))
        for other in runs[1:]:
            for x, y in zip(runs[0], other):
                assert np.array_equal(x, y), key


def test_device_bytes_are_live_buffers(smg):
    """smg_wave_device_bytes equals the library's count of live bytes attributable to the object, free and clamped, does not grow with further
    steps of the same shape, and the count returns to its start after destroy"""
    live = smg._lib.load().smg_device_bytes_live
    for name, clamped in (("icosphere3", False), ("square", True), ("torus", False)):
        V, F = N.shape(name)
        mg = smg.mg_precompute(V, F, 0.25, COARSEST[name], 1)                  # the caller's hierarchy stays alive throughout
        u0, v0, _ = N.test_state(V, F, 3, clamped)
        src = N.test_lists(V, F, 3, clamped)
        sig = ricker_signal(smg, 8, DT, 3, 3)
        gc.collect()
        before = live()
        obj = smg.WaveEquation(mg, V, F, DT, speed=N.nonuniform(V)[0], clamped=clamped)
        obj.set_sources(src)
        obj.set_receivers(src)
        obj.set_state(u0, v0)
        obj.step(8, signal=sig)
        second = obj.device_bytes()
        obj.step(8, signal=sig)
        obj.step(2)
        counted, held = obj.device_bytes(), live() - before
        print("%s, clamped %d: device_bytes %d after the first call, %d after the third, live DevBuf bytes held %d" % (name, clamped, second, counted, held))
        del obj
        gc.collect()
        assert 0 < counted == held and counted == second and live() == before


def live_calls(smg, record=False):
    """the refusals that need an object -> {name: [code, message]}; nothing may be written by any of them"""
    Lc = smg._lib.load()
    V, F = N.shape("square")
    mg = smg.mg_precompute(V, F, 0.25, COARSEST["square"], 1)
    n = V.shape[0]
    u0, v0, _ = N.test_state(V, F, 2, True)
    u0, v0 = np.asfortranarray(u0), np.asfortranarray(v0)
    bnd = N.boundary_vertices(np.asarray(F))
    inner = N.test_lists(V, F, 3, True)
    ub = u0.copy(order="F")
    ub[bnd[0], 1] = 1e-300
    out = np.full((n, 2), N.SENTINEL, order="F")
    empty = smg.WaveEquation(mg, V, F, DT, clamped=True)
    obj = smg.WaveEquation(mg, V, F, DT, clamped=True)
    bare = smg.WaveEquation(mg, V, F, DT, clamped=True)                        # a state, no sources
    obj.set_sources(inner)
    obj.set_state(u0, v0)
    bare.set_state(u0, v0)
    p = obj.params
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    ints = lambda *x: np.array(x, dtype=np.int32)   # noqa: E731
    sig = np.zeros((2, 3, 2))
    sbad = sig.copy()
    sbad[1, 2, 0] = np.inf

    def setp(**kw):
        q = type(p)(*[getattr(p, f) for f, _ in p._fields_])
        for key, val in kw.items():
            setattr(q, key, val)
        return Lc.smg_wave_set_params(obj.o, C.byref(q))
    U, W, O = u0.ctypes.data, v0.ctypes.data, out.ctypes.data
    lists = {"twice": ints(inner[0], inner[1], inner[0]), "range": ints(inner[0], n), "negative": ints(-1), "boundary": ints(inner[0], bnd[-1])}
    calls = {"set_state null block": lambda: Lc.smg_wave_set_state(empty.o, U, None, n, 2, 0),
             "set_state k zero": lambda: Lc.smg_wave_set_state(empty.o, U, W, n, 0, 0),
             "set_state index range": lambda: Lc.smg_wave_set_state(empty.o, U, W, n, 2 ** 31 // n, 0),
             "set_state memspace": lambda: Lc.smg_wave_set_state(empty.o, U, W, n, 2, 2),
             "set_state leading dimension": lambda: Lc.smg_wave_set_state(empty.o, U, W, n - 1, 2, 0),
             "set_state non-zero on the clamped boundary": lambda: Lc.smg_wave_set_state(empty.o, ub.ctypes.data, W, n, 2, 0),
             "step before set_state": lambda: Lc.smg_wave_step(empty.o, 1, None, None, None, None, None, None),
             "step n_steps zero": lambda: Lc.smg_wave_step(obj.o, 0, None, None, None, None, None, None),
             "step signal without sources": lambda: Lc.smg_wave_step(bare.o, 1, sig.ctypes.data_as(dp), None, None, None, None, None),
             "step non-finite signal": lambda: Lc.smg_wave_step(obj.o, 1, sbad.ctypes.data_as(dp), None, None, None, None, None),
             "state before set_state": lambda: Lc.smg_wave_state(empty.o, O, O, n, 0),
             "state null block": lambda: Lc.smg_wave_state(obj.o, O, None, n, 0),
             "state memspace": lambda: Lc.smg_wave_state(obj.o, O, O, n, 3),
             "state leading dimension": lambda: Lc.smg_wave_state(obj.o, O, O, n - 1, 0),
             "set_sources negative count": lambda: Lc.smg_wave_set_sources(obj.o, lists["twice"].ctypes.data_as(ip), -1),
             "set_sources null list": lambda: Lc.smg_wave_set_sources(obj.o, None, 2),
             "set_sources vertex twice": lambda: Lc.smg_wave_set_sources(obj.o, lists["twice"].ctypes.data_as(ip), 3),
             "set_sources index range": lambda: Lc.smg_wave_set_sources(obj.o, lists["range"].ctypes.data_as(ip), 2),
             "set_sources on the clamped boundary": lambda: Lc.smg_wave_set_sources(obj.o, lists["boundary"].ctypes.data_as(ip), 2),
             "set_receivers negative index": lambda: Lc.smg_wave_set_receivers(obj.o, lists["negative"].ctypes.data_as(ip), 1),
             "set_receivers index range": lambda: Lc.smg_wave_set_receivers(obj.o, lists["range"].ctypes.data_as(ip), 2),
             "set_params clamped": lambda: setp(clamped=0),
             "set_params dt": lambda: setp(dt=0.0),
             "set_params damping": lambda: setp(damping=-1.0)}
    got = {}
    for name, call in calls.items():
        rc = call()
        got[name] = [rc, Lc.smg_last_error().decode()]
    assert np.all(out == N.SENTINEL)
    u, v = obj.state()
    assert np.array_equal(u, u0) and np.array_equal(v, v0) and obj.params.dt == DT and obj.n_src == 3
    E, _, _ = obj.step(1, signal=np.ones((2, 3, 2)))                           # the refused lists have not replaced the kept one
    assert E.shape == (1, 4)
    assert Lc.smg_wave_set_receivers(obj.o, lists["twice"].ctypes.data_as(ip), 3) == 0, "receivers may repeat"
    assert Lc.smg_wave_set_sources(obj.o, None, 0) == 0 and Lc.smg_wave_set_receivers(obj.o, None, 0) == 0, "empty lists are allowed"
    return got


def test_live_refusals(smg):
    """the refusals that need an object: code and text as recorded in tests/golden/wave_refusals.json, group "live"; nothing is written"""
    golden = json.load(open(GOLDEN))["live"]
    got = live_calls(smg)
    assert set(got) == set(golden)
    for name, (rc, msg) in got.items():
        assert [rc, msg] == golden[name] and rc == INVALID, name


def test_the_timing_hook_times_both_launchers(smg):
    """smg_debug_wave_time: a positive time for both launchers on a mesh of more than one block, k = 3"""
    Lc = smg._lib.load()
    V, F = N.shape("icosphere3")
    Fp, Vp = F.ctypes.data_as(C.POINTER(C.c_int)), V.ctypes.data_as(C.POINTER(C.c_double))
    ms = C.c_double(-1.0)
    for op in (N.WAVE_RHS, N.WAVE_ADVANCE):
        assert Lc.smg_debug_wave_time(op, V.shape[0], F.shape[0], 3, Fp, Vp, 3, C.byref(ms)) == 0 and 0.0 < ms.value < 1e3, (op, ms.value)
