"""CPU: adjoint-state gradients of the wave object (include/smg.h: smg_wave_gradient, smg_wave_set_speed) -- the ABI and its refusals without a GPU,
the library's host twin (smg_wave_adjoint_host) against the numpy restatement (tests/wave_adjoint_np.py) bit for bit, and the restatement's gradient
against derivatives that do not use it.

    DERIVATIVE  J is evaluated once more in complex arithmetic (wave_adjoint_np.misfit_complex: the scheme's operations, complex direct solves,
                rho rho without a conjugate) at x + i h d, h = 1e-30, x one of speed, u0, v0, the signal: Im J / h is the derivative along d with
                no subtraction, so only rounding separates it from <gradient, d>.
    ROUNDING    the bound on that separation, first order in eps = 2^-52.  In the scaled state z~ = (u, v / q2) a step is z~' = S~ z~ (+ forces),
                S~ = D S D^-1 with S = wave_np.step_map and D = diag(I, I / q2); P_j = |S~^j|_2 from numpy (in this scaling the powers stay of
                order 1 to 10, where |S^j|_2 grows like 2 q2 j).  A step in floating point: b = mt (s2 u + dt v) is three roundings; the sparse
                LU is backward stable, its componentwise backward error a few eps (four are allowed); both reach w through A^-1, at most
                7 kappa eps relative, kappa = cond_2 of A's unknown block; u' and v' add four roundings that no solve amplifies.  So a step
                returns S~ z~ up to (7 kappa + 4) eps (|z~_m| + |z~_m+1|), and after n steps a run is off by
                    E_n(z) = (7 kappa + 4) eps sum_(m < n) P_(n-1-m) (|z~_m| + |z~_m+1|).
                The complex run's imaginary part over h is the tangent run dz, dz~_m+1 = S~ dz~_m + tau_m with tau_m the injection of the
                perturbed parameter (0 for u0 and v0); its operations round relative to their own operands, of which tau_m is one more:
                    E_n(dz) = (7 kappa + 4) eps sum_(m < n) P_(n-1-m) (|dz~_m| + |dz~_m+1| + |tau_m|),    tau_m = dz~_m+1 - S~ dz~_m from numpy.
                D = sum_n rho_n' R du_n, with |R' R|_2 <= M, the largest number of slots of one vertex, so the complex-step value is off by at
                most  sum_n (|R' rho_n| E_n(dz) + M |du_n| E_n(z)),  and the adjoint evaluates the same products in the transposed association:
                the same again.  ROUNDING = twice that sum.  It is a bound in norms: every step's worst case is added, so it sits orders above
                what rounding does.  It is asserted; the largest ratio to it is printed, and its own size relative to sum_n |R' rho_n| |du_n|,
                the size of D's terms (about 1e-11).  What keeps small errors from hiding under it is RELATIVE.
    RELATIVE    beside ROUNDING, the scale the issue sets: its own check of these formulas (12 nodes, 7 steps, direct solves) agreed with
                complex-step derivatives to 5e-15 relative and it calls a bound far above 1e-12 relative one that hides errors.  Asserted:
                |complex step - <gradient, d>| <= 1e-12 |complex step| for every direction, and for ENERGY |J - <z0, grad z0> / 2| <= 1e-12 J.
    ENERGY      unforced with observed = 0, J is a quadratic form of z0 = (u0, v0): <grad z0, z0> = 2 J, within ROUNDING of the direction z0
                (dz = z, tau = 0) plus 4 N n_rec eps J for J's own sum, and within RELATIVE.
    ZERO        observed equal to the run's own traces: rho = 0 exactly, |g|_F^2 == 0.0 at every step, every solve is skipped: every gradient is
                exactly 0.0.
    TAYLOR      J(s + h d) - J(s) - h <grad_speed, d> = h^2 d' H d / 2 + O(h^3): halving h divides it by 4 (1 + O(h)).  d is a speed
                increase everywhere, between 1/3 and 1 on speeds in [0.75, 1.25] (a direction of one sign, as an inversion's update is: along an
                oscillating d the quadratic term can cancel and leave the cubic one).  With h = 1e-3 and 5e-4 the speed moves by at most 0.13
                percent; the remainder is of the order h^2 J, asserted to be more than 1e4 times J's rounding noise (N n_rec eps J), and the
                cubic term moves the ratio by a few h: asserted within 4 +- 0.1."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import wave_adjoint_np as A
import wave_np as N
from test_wave_host import INVALID, NO_DEVICE, ROOT, check_cases, launcher_cases, ricker_signal

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wave_gradient_refusals.json")
EPS = N.EPS
MESHES = N.LAUNCHER_MESHES
SYMBOLS = ("smg_wave_gradient", "smg_wave_set_speed", "smg_wave_adjoint_host", "smg_debug_wave_adjoint")


# ---- the ABI and its refusals --------------------------------------------------------------------------------------------------------------------
def test_abi_present(smg_mod):
    L = smg_mod._lib.load()
    for name in SYMBOLS:
        assert hasattr(L, name)
    assert L.smg_version() >= 550
    assert hasattr(smg_mod.WaveEquation, "gradient") and hasattr(smg_mod.WaveEquation, "set_speed") and hasattr(smg_mod, "WaveGradient")


def null_object_cases(smg):
    L = smg._lib.load()
    X = np.ones(8)
    dp = X.ctypes.data_as(C.POINTER(C.c_double))
    calls = {"gradient": lambda: L.smg_wave_gradient(None, 1, None, None, None, dp, dp, 8, dp, dp, 8, None, None, None, None),
             "set_speed": lambda: L.smg_wave_set_speed(None, dp)}
    return [("null object: " + k, (lambda f=f: (f(), L.smg_last_error().decode())), False) for k, f in calls.items()]


def host_twin_cases(smg, call=None, prefix="host twin"):
    """the operand checks smg_wave_adjoint_host and smg_debug_wave_adjoint share"""
    call = call or (lambda *a, **k: A.host(smg, *a, **k)[0])
    L = smg._lib.load()
    V, F = N.shape("icosphere1")
    n = V.shape[0]
    u, v, w = N.test_state(V, F, 2)
    Fo = np.array(F)
    Fo[1, 2] = n
    rec, src = np.array([0, n - 1, 0], dtype=np.int32), np.array([0, n - 1], dtype=np.int32)
    tr, row, gs = np.ones((2, 3, 2)), np.ones((3, 2)), np.ones((2, 2))
    bad_speed, bad_sigma = np.ones(n), np.zeros(n)
    bad_speed[3], bad_sigma[4] = 0.0, np.nan
    ke, rh, ad = dict(k=2, x=(u, v, w)), dict(k=2, x=(u, v)), dict(k=2, x=(w, u, v, u, v))
    inj, sg, rs = dict(k=2, x=(u, row), idx=rec), dict(k=2, x=(w, gs, gs), idx=src), dict(k=2, x=(tr, tr), idx=rec, n_rows=2)
    thunks = {
        "unknown op": lambda: call(7, V, F, **rh), "negative op": lambda: call(-1, V, F, **rh),
        "out missing": lambda: call(A.RHS, V, F, over=dict(out=None), **rh),
        "V missing": lambda: call(A.RHS, V, F, over=dict(V=None), **rh),
        "F missing": lambda: call(A.ADVANCE, V, F, over=dict(F=None), **ad),
        "no vertex": lambda: call(A.RHS, V, F, over=dict(nV=0), **rh),
        "keep: u missing": lambda: call(A.KEEP, V, F, k=2, x=(None, v, w)),
        "keep: u' missing": lambda: call(A.KEEP, V, F, k=2, x=(u, v)),
        "advance: G missing": lambda: call(A.ADVANCE, V, F, k=2, x=(w, u, v, u)),
        "residual: traces missing": lambda: call(A.RESIDUAL, V, F, k=2, x=(None, tr), idx=rec, n_rows=2),
        "inject: list missing": lambda: call(A.INJECT, V, F, k=2, x=(u, row)),
        "signal: list missing": lambda: call(A.SIGNAL, V, F, k=2, x=(w, gs, gs)),
        "k zero": lambda: call(A.RHS, V, F, **dict(rh, k=0)),
        "k negative": lambda: call(A.ADVANCE, V, F, **dict(ad, k=-2)),
        "dt zero": lambda: call(A.RHS, V, F, dt=0.0, **rh),
        "dt nan": lambda: call(A.ADVANCE, V, F, dt=float("nan"), **ad),
        "clamped two": lambda: call(A.RHS, V, F, clamped=2, **rh),
        "speed zero": lambda: call(A.SCALE, V, F, speed=bad_speed, k=2, x=(u,)),
        "sigma nan": lambda: call(A.KEEP, V, F, sigma=bad_sigma, **ke),
        "face index": lambda: call(A.ADVANCE, V, Fo, **ad),
        "residual: no rows": lambda: call(A.RESIDUAL, V, F, **dict(rs, n_rows=0)),
        "residual: no slots": lambda: call(A.RESIDUAL, V, F, k=2, x=(tr, tr), n_rows=2),
        "empty list": lambda: call(A.INJECT, V, F, over=dict(n_idx=0), **inj),
        "list index": lambda: call(A.INJECT, V, F, **dict(inj, idx=np.array([0, n, 1], dtype=np.int32))),
        "negative list index": lambda: call(A.SIGNAL, V, F, **dict(sg, idx=np.array([-1, 2], dtype=np.int32))),
        "source twice": lambda: call(A.SIGNAL, V, F, **dict(sg, idx=np.array([5, 5], dtype=np.int32))),
        "order: operands before k": lambda: call(A.ADVANCE, V, F, k=0, x=(w, u, v, u)),
        "order: k before dt": lambda: call(A.RHS, V, F, dt=0.0, **dict(rh, k=0)),
        "order: dt before clamped": lambda: call(A.RHS, V, F, dt=0.0, clamped=2, **rh),
        "order: clamped before speed": lambda: call(A.RHS, V, F, clamped=2, speed=bad_speed, **rh),
        "order: speed before sigma": lambda: call(A.RHS, V, F, speed=bad_speed, sigma=bad_sigma, **rh),
        "order: sigma before faces": lambda: call(A.RHS, V, Fo, sigma=bad_sigma, **rh),
        "order: faces before the list": lambda: call(A.INJECT, V, Fo, **dict(inj, idx=np.array([0, n, 1], dtype=np.int32))),
    }
    return [("%s: %s" % (prefix, k), (lambda f=f: (f(), L.smg_last_error().decode())), False) for k, f in thunks.items()]


def test_refusals_keep_code_and_message(smg_mod):
    """every refusal of the calls on a missing object and of the host twin's operand checks, with the code and the smg_last_error() text recorded
    in tests/golden/wave_gradient_refusals.json.  The refusals that need a live object (group "live") are checked by
    tests/test_gpu_wave_gradient.py.  Every message carries its entry point's name; a receiver list may repeat a vertex."""
    golden = json.load(open(GOLDEN))
    assert check_cases(smg_mod, null_object_cases(smg_mod), golden["null"]) == set(golden["null"])
    assert check_cases(smg_mod, host_twin_cases(smg_mod), golden["host"]) == set(golden["host"])
    h = golden["host"]
    assert h["host twin: order: operands before k"] == h["host twin: advance: G missing"]
    assert h["host twin: order: k before dt"] == h["host twin: k zero"]
    assert h["host twin: order: dt before clamped"] == h["host twin: dt zero"]
    assert h["host twin: order: clamped before speed"] == h["host twin: clamped two"]
    assert h["host twin: order: speed before sigma"] == h["host twin: speed zero"]
    assert h["host twin: order: sigma before faces"] == h["host twin: sigma nan"]
    assert h["host twin: order: faces before the list"] == h["host twin: face index"]
    assert all(v[1].startswith("smg_wave_adjoint_host: ") for v in h.values())
    for name, (code, msg) in golden["null"].items():
        assert msg == "smg_wave_" + name.split(": ")[1] + ": null object"
    for name, (code, msg) in golden["live"].items():
        assert code == INVALID and msg.startswith("smg_wave_" + name.split()[0] + ": "), name
    assert {n.split()[0] for n in golden["live"]} == {"gradient", "set_speed"}


def test_hook_refuses_what_the_host_twin_refuses(smg_mod):
    golden = json.load(open(GOLDEN))["host"]
    hook = lambda *a, **k: A.hook(smg_mod, *a, **k)[0]   # noqa: E731
    for name, thunk, _ in host_twin_cases(smg_mod, hook, "hook"):
        rc, msg = thunk()
        want = golden[name.replace("hook: ", "host twin: ")]
        assert [rc, msg] == [want[0], want[1].replace("smg_wave_adjoint_host", "smg_debug_wave_adjoint")], name
    if smg_mod._lib.load().smg_device_count() == 0:
        V, F = N.shape("icosphere1")
        u, v, _ = N.test_state(V, F, 1)
        assert A.hook(smg_mod, A.RHS, V, F, x=(u, v))[0] == NO_DEVICE


# ---- the host twin against the restatement -------------------------------------------------------------------------------------------------------
def host_run(smg):
    def run(op, V, F, **kw):
        rc, out = A.host(smg, op, V, F, **kw)
        assert rc == 0
        return out
    return run


@pytest.mark.parametrize("k", [1, 3, 8])
@pytest.mark.parametrize("name", MESHES)
def test_host_twin_against_restatement(smg_mod, name, k):
    """all seven ops, free and clamped, a receiver list with duplicates, vertex 0 and vertex nV - 1, bit for bit"""
    for clamped in sorted({cl for cl, _ in launcher_cases(name)}):
        A.check_launchers(host_run(smg_mod), name, k, clamped)


# ---- the restatement's gradient ------------------------------------------------------------------------------------------------------------------
STEPS, DT = 8, 0.05
CASES = [("icosphere2", 0, 0.0), ("icosphere2", 0, 0.8), ("square", 1, 0.0), ("square", 1, 0.8)]


def run_case(smg, name, clamped, damping, forced=True, observed="noise"):
    """(the restatement, its gradient, u0, v0, the signal, observed, (S~, (P_j)), kappa) of 8 steps, k = 2, non-uniform speed, two Ricker sources,
    six receiver slots with duplicates; everything is made anew for each caller"""
    V, F = N.shape(name)
    ref = N.WaveNp(V, F, speed=N.nonuniform(V)[0], dt=DT, damping=damping, clamped=clamped)
    k = 2
    u0, v0, _ = N.test_state(V, F, k, bool(clamped))
    ref.src, ref.rec = N.test_lists(V, F, 2, bool(clamped)), A.receiver_list(V, F, bool(clamped))
    sig = ricker_signal(smg, STEPS, DT, 2, k) if forced else None
    obs = 0.05 * np.random.default_rng(7).standard_normal((STEPS, ref.rec.size, k)) if observed == "noise" else None
    n = V.shape[0]
    D = np.concatenate([np.ones(n), np.full(n, 1.0 / ref.q2)])
    St = D[:, None] * ref.step_map() / D[None, :]
    P = (St, N.power_norms(St, STEPS + 1))
    kappa = float(np.linalg.cond(ref.Auu.toarray()))
    ref.set_state(u0, v0)
    return ref, A.gradient(ref, STEPS, sig, obs), u0, v0, sig, obs, P, kappa


def rounding(ref, r, z, dz, P, kappa):
    """ROUNDING of the header, per column; z, dz: [(u_n, v_n)], n = 0 .. N, the run and its tangent; P: (S~, its powers' norms)"""
    St, P = P
    col = lambda x: np.linalg.norm(x, axis=0)   # noqa: E731
    stack = lambda s: np.concatenate([s[0], s[1] / ref.q2])   # noqa: E731
    size = lambda s: col(stack(s))   # noqa: E731
    c = (7.0 * kappa + 4.0) * EPS
    tau = [col(stack(dz[m + 1]) - St @ stack(dz[m])) for m in range(len(dz) - 1)]
    E = lambda s, n, inj: c * sum(P[n - 1 - m] * (size(s[m]) + size(s[m + 1]) + (inj[m] if inj else 0.0)) for m in range(n))   # noqa: E731
    groups = A.group(ref.rec, ref.known)
    M = float(np.max(np.unique(ref.rec, return_counts=True)[1]))
    total, terms = 0.0, 0.0
    for n in range(1, len(z)):
        Rt = col(A.inject(np.zeros(z[0][0].shape), r.rho[n - 1], groups))
        total = total + Rt * E(dz, n, tau) + M * col(dz[n][0]) * E(z, n, None)
        terms = terms + Rt * col(dz[n][0])
    return 2.0 * total, terms


@pytest.mark.parametrize("name,clamped,damping", CASES)
def test_gradient_against_complex_step_derivatives(smg_mod, name, clamped, damping):
    """DERIVATIVE and ROUNDING of the header on icosphere(2) and the clamped square, damped and undamped, 8 forced steps: the speed, u0, v0 and the
    signal, three random directions each"""
    ref, r, u0, v0, sig, obs, P, kappa = run_case(smg_mod, name, clamped, damping)
    n, k, h = u0.shape[0], u0.shape[1], 1e-30
    J0 = A.misfit_complex(ref, u0, v0, STEPS, sig, obs)
    assert np.allclose(J0.real, r.misfit, rtol=1e-12) and np.all(J0.imag == 0.0)
    rng = np.random.default_rng(11)
    worst, rel, loose = 0.0, 0.0, 0.0
    for what, shape, grad in (("speed", (n,), r.grad_speed), ("u0", (n, k), r.grad_u0), ("v0", (n, k), r.grad_v0), ("signal", sig.shape, r.grad_signal)):
        for _ in range(3):
            d = rng.standard_normal(shape)
            if what in ("u0", "v0"):
                d[ref.known] = 0.0                                             # the clamped rows of a state stay 0
            i = 1j * h * d
            z = []
            Jc = A.misfit_complex(ref, u0 + (i if what == "u0" else 0.0), v0 + (i if what == "v0" else 0.0), STEPS, sig + (i if what == "signal" else 0.0), obs,
                                  speed=ref.speed + i if what == "speed" else None, states=z)
            cs = Jc.imag / h
            ad = np.sum((grad * (d[:, None] if what == "speed" else d)).reshape(-1, k), axis=0)
            bound, terms = rounding(ref, r, [(a.real, b.real) for a, b in z], [(a.imag / h, b.imag / h) for a, b in z], P, kappa)
            worst, rel, loose = max(worst, float(np.max(np.abs(cs - ad) / bound))), max(rel, float(np.max(np.abs(cs - ad) / np.abs(cs)))), max(loose, float(np.max(bound / terms)))
            assert np.all(np.abs(cs - ad) <= bound), (what, cs, ad, bound)
            assert np.all(np.abs(cs - ad) <= 1e-12 * np.abs(cs)), (what, cs, ad)
    print("%s, clamped %d, damping %g: kappa %.1f, P %s; largest |complex step - <gradient, d>| over ROUNDING %.2e, relative to the derivative %.2e (asserted: 1e-12); ROUNDING is at most %.2e of the terms' size"
          % (name, clamped, damping, kappa, np.round(P[1], 2), worst, rel, loose))


@pytest.mark.parametrize("name,clamped,damping", CASES)
def test_energy_identity_of_an_unforced_run(smg_mod, name, clamped, damping):
    """ENERGY of the header"""
    ref, r, u0, v0, _, _, P, kappa = run_case(smg_mod, name, clamped, damping, forced=False, observed=None)
    z = [(f[0], f[1]) for f in r.fwd] + [(r.fwd[-1][2], r.fwd[-1][3])]
    bound = rounding(ref, r, z, z, P, kappa)[0] + 4.0 * STEPS * ref.rec.size * EPS * r.misfit
    twice = np.sum(u0 * r.grad_u0 + v0 * r.grad_v0, axis=0)
    print("%s, clamped %d, damping %g: J %s, |J - <z0, grad z0> / 2| %s, over its bound %s" % (name, clamped, damping, r.misfit, np.abs(r.misfit - 0.5 * twice),
                                                                                             np.abs(2.0 * r.misfit - twice) / bound))
    assert np.all(np.abs(2.0 * r.misfit - twice) <= bound) and np.all(r.misfit > 0.0) and r.grad_signal is None
    assert np.all(np.abs(r.misfit - 0.5 * twice) <= 1e-12 * r.misfit)


@pytest.mark.parametrize("name,clamped,damping", CASES[1:3])
def test_own_traces_give_exact_zeros(smg_mod, name, clamped, damping):
    """ZERO of the header; every backward solve is skipped"""
    ref, r, u0, v0, sig, _, _, _ = run_case(smg_mod, name, clamped, damping)
    ref.set_state(u0, v0)
    z = A.gradient(ref, STEPS, sig, r.traces)
    assert np.all(z.misfit == 0.0) and np.all(z.rho == 0.0)
    for g in (z.grad_speed, z.grad_u0, z.grad_v0, z.grad_signal):
        assert np.all(g == 0.0)
    assert all(np.all(y == 0.0) and np.all(res == 0.0) for _, _, y, res, _, _ in z.bwd)


def test_clamped_rows_are_exact_zeros(smg_mod):
    """on the clamped rows y, p, q and G are exact zeros at every step, although vertex 0 and vertex nV - 1 -- boundary corners -- are receivers"""
    ref, r, *_ = run_case(smg_mod, "square", 1, 0.8)
    kn = ref.known
    assert kn[0] and kn[-1] and 0 in ref.rec and kn.size - 1 in ref.rec
    for g in (r.grad_speed, r.grad_u0, r.grad_v0):
        assert np.all(g[kn] == 0.0) and np.any(g[~kn] != 0.0)
    for _, g, y, _, p, q in r.bwd:
        assert np.all(g[kn] == 0.0) and np.all(y[kn] == 0.0) and np.all(p[kn] == 0.0) and np.all(q[kn] == 0.0)


@pytest.mark.parametrize("name,clamped,damping", CASES[:1] + CASES[3:])
def test_taylor_remainder_falls_by_four(smg_mod, name, clamped, damping):
    """TAYLOR of the header: h = 1e-3 and 5e-4"""
    ref, r, u0, v0, sig, obs, _, _ = run_case(smg_mod, name, clamped, damping)
    d = (1.0 + 0.5 * np.cos(3.0 * ref.V[:, 0] + ref.V[:, 1])) / 1.5
    slope = np.sum(r.grad_speed * d[:, None], axis=0)

    def J(h):
        other = N.WaveNp(ref.V, ref.F, speed=ref.speed + h * d, dt=DT, damping=damping, clamped=clamped)
        other.src, other.rec = ref.src, ref.rec
        other.set_state(u0, v0)
        return A.gradient(other, STEPS, sig, obs, backward=False).misfit
    rem = [np.abs(J(h) - r.misfit - h * slope) for h in (1e-3, 5e-4)]
    noise = STEPS * ref.rec.size * EPS * r.misfit
    print("%s, clamped %d, damping %g: remainders %s and %s, ratio %s; J's rounding noise about %s" % (name, clamped, damping, rem[0], rem[1], rem[0] / rem[1], noise))
    assert np.all(rem[1] > 1e4 * noise) and np.all(np.abs(rem[0] / rem[1] - 4.0) <= 0.1)


# ---- the kernels' registers, the host maths under sanitizers -------------------------------------------------------------------------------------
def test_kernels_keep_everything_in_registers():
    """the ISA notes of the kernels of smg_wave_adjoint_device.hip (the build's flags, device side only): no scratch, no spills, no contraction, no
    fp64 division"""
    import re
    from surface_multigrid_code_amd import build as B
    src = os.path.join(B.CSRC, "smg_wave_adjoint_device.hip")
    asm = subprocess.check_output([B._hipcc()] + B.FLAGS + ["--cuda-device-only", "-S", src, "-o", "-"], text=True, stderr=subprocess.DEVNULL)
    notes = dict(re.findall(r"\.name:\s+(\S*k_wave_adj\S*)(.*?)\.wavefront_size", asm, flags=re.S))
    assert len(notes) == 7                                                    # keep, residual, inject, rhs, advance, signal, scale
    for kernel, body in notes.items():
        field = lambda k: int(re.search(r"\.%s:\s+(\d+)" % k, body).group(1))   # noqa: E731
        print("%s: vgpr_count %d, sgpr_count %d, private_segment_fixed_size %d" % (kernel, field("vgpr_count"), field("sgpr_count"), field("private_segment_fixed_size")))
        assert field("private_segment_fixed_size") == 0 and field("vgpr_spill_count") == 0 and field("sgpr_spill_count") == 0 and field("vgpr_count") <= 32
    for word in ("v_fma_f64", "v_fmac_f64", "v_div_scale_f64", "v_div_fmas_f64", "v_div_fixup_f64", "v_rcp_f64"):
        assert word not in asm, "no contraction and no fp64 division (the lane's column and vertex are an integer division)"


def test_host_maths_under_sanitizers(tmp_path):
    """tests/wave_gradient_asan_driver.cpp, a stand-alone program: the host twin's loops (smg::wave_adj_host_* and wave_group_receivers of
    csrc/smg_wave_adjoint_inl.hpp, what smg_wave_adjoint_host runs after its checks) on exactly-sized heap arrays, under AddressSanitizer and
    UndefinedBehaviorSanitizer (static runtimes: run directly, nothing preloaded, nothing loaded into python)"""
    exe = str(tmp_path / "wave_gradient_asan_driver")
    csrc = os.path.join(ROOT, "surface_multigrid_code_amd", "csrc")
    srcs = [os.path.join(ROOT, "tests", "wave_gradient_asan_driver.cpp"), os.path.join(csrc, "smg_mesh.cpp"), os.path.join(csrc, "smg_sparse.cpp")]
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-ffp-contract=off", "-pthread", "-I" + csrc] + srcs + ["-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    run = subprocess.run([exe], env=env, capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0 and run.stdout.count("ok 1") == 6 and "ERROR" not in run.stderr
