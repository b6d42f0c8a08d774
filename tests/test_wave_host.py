"""CPU: the wave equation on a surface (include/smg.h: smg_wave_*) -- the ABI and its refusals without a GPU, the library's host twin
(smg_wave_host) against the numpy restatement (tests/wave_np.py), and the restatement itself against the scheme's exact discrete identities.

The right-hand side, the sources, the advance and every sum are correctly rounded +, - and * in one order on both sides: held bit for bit.

The identities, every quantity computed on the CPU from the restatement WaveNp (direct solves); A = diag(0.5 s2 mt) + a C; r = A w - b the direct
solve's own residual; E = 0.5 v' Mt v + 0.5 u' C u; vbar = (v + v') / 2, fbar = (f_n + f_n+1) / 2; | | the 2-norm of one column; eps = 2^-52:

    POWER      E' - E = -dt vbar' Sigma Mt vbar + dt vbar' fbar + (v + v')' r / dt.  In floating point the restatement leaves this within
               SLACK = |v + v'| / dt (4 eps |mag_b| + 16 eps ||A| |w| + |b||)        b's rounding and the evaluation of r act as a residual
                     + |Mt v'| eps (q2 |u'| + 2 q2 |u' - u| + |v'|) + |C u'| eps |u'|   the roundings of u' and v' move E' by grad E . delta
                     + 16 eps (Eabs + Eabs' + dt |vbar|' (Sigma Mt |vbar| + |fbar|))   the evaluation of the identity's own terms
               with mag_b = mt (|s2 u| + dt |v|) + a |f_n + f_n+1| and Eabs the sum E with every term's absolute value (wave_slack below).
    MOMENTUM   free boundary, sigma = 0: 1' A w = sum mt w + a (C 1)' w, so sum mt v' = sum mt v + dt sum fbar + q2 (sum r - a (C 1)' w): off by
               at most q2 (sqrt(nV) (|r| + 4 eps |mag_b|) + a d |w|) + |mt| eps (q2 |u'| + 2 q2 |u' - u| + |v'|), d = |C 1|_2 of the stored
               matrix (rd_np.row_sum_defect, correctly rounded); the sums by math.fsum.
    EIGENMODE  C phi = lambda Mt phi and uniform damping: (alpha phi, beta phi) follows (0.5 s2 + a lambda) omega = s2 alpha + dt beta,
               alpha' = omega - alpha, beta' = q2 (alpha' - alpha) - beta.  The computed pair leaves r_phi = |C phi - lambda Mt phi|_2: a step's w
               is off by at most (res + a |omega| r_phi) / min(0.5 s2 mt), chained by wave_np.Chain (tol = 0).  Undamped this is the rotation by
               theta = 2 atan(dt sqrt(lambda) / 2) in (alpha, beta / sqrt(lambda)): the amplitude is kept and the phase after n steps is n theta.
    CLAMPED    u, v and w are exact zeros on the boundary rows at every step.
    POTENTIAL  the reported potential energy is the sum of the face terms 0.5 A_f |grad u|^2, grad u = sum_i u_i W_fi: against 0.5 u' C u within
               16 eps sum_f A_f (sum_i |u_i| |W_fi|)^2 (three products and two sums per component, the square, the area, the half, the sum)."""
import ctypes as C
import functools
import json
import math
import os
import subprocess

import numpy as np
import pytest
import scipy.linalg

import wave_np as N
from morph_np import rest_faces
from rd_np import row_sum_defect
from test_arap_host import _fake_hierarchy
from test_geodesics_host import flat_square

INVALID, NO_DEVICE = -1, -2
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wave_refusals.json")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = N.EPS
MESHES = N.LAUNCHER_MESHES

WAVE_SYMBOLS = ("smg_wave_params_default", "smg_wave_create", "smg_wave_destroy", "smg_wave_set_params", "smg_wave_set_solver", "smg_wave_device_bytes",
                "smg_wave_set_state", "smg_wave_state", "smg_wave_set_sources", "smg_wave_set_receivers", "smg_wave_step", "smg_wave_host", "smg_debug_wave",
                "smg_debug_wave_time")


# ---- the ABI and its refusals --------------------------------------------------------------------------------------------------------------------
def test_abi_present(smg_mod):
    L = smg_mod._lib.load()
    for name in WAVE_SYMBOLS:
        assert hasattr(L, name)
    assert hasattr(smg_mod, "WaveEquation") and hasattr(smg_mod, "wave_params") and hasattr(smg_mod, "wavelets")
    assert L.smg_version() >= 540
    assert L.smg_wave_device_bytes(None) == 0
    p = L.smg_wave_params_default()
    assert {f: getattr(p, f) for f, _ in p._fields_} == N.DEFAULTS
    t = np.linspace(0.0, 2.0, 9)
    a = (np.pi * 1.5 * (t - 1.0)) ** 2
    assert np.allclose(smg_mod.wavelets.ricker(1.5, t, 1.0), (1 - 2 * a) * np.exp(-a)) and smg_mod.wavelets.ricker(1.5, 1.0, 1.0) == 1.0


def _create(smg, h, V, F, nV=None, null=None, speed=None, sigma=None, **params):
    """smg_wave_create -> (code, message); a successful create is destroyed at once"""
    L = smg._lib.load()
    ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
    V, F = np.ascontiguousarray(V, dtype=np.float64), np.ascontiguousarray(F, dtype=np.int32)
    speed = None if speed is None else np.ascontiguousarray(speed, dtype=np.float64)
    sigma = None if sigma is None else np.ascontiguousarray(sigma, dtype=np.float64)
    p = L.smg_wave_params_default()
    for key, val in params.items():
        setattr(p, key, val)
    out = C.c_void_p(0xdead)
    rc = L.smg_wave_create(None if null == "h" else h, None if null == "V" else V.ctypes.data_as(dp), V.shape[0] if nV is None else nV,
                           None if null == "F" else F.ctypes.data_as(ip), F.shape[0], None if speed is None else speed.ctypes.data_as(dp),
                           None if sigma is None else sigma.ctypes.data_as(dp), None if null == "p" else C.byref(p), None if null == "out" else C.byref(out))
    if rc == 0:
        L.smg_wave_destroy(out)
        return rc, ""
    assert null == "out" or out.value is None, "a refused create must leave *out == NULL"
    return rc, L.smg_last_error().decode()


BAD_PARAMS = (("dt zero", dict(dt=0.0)), ("dt negative", dict(dt=-0.1)), ("dt nan", dict(dt=float("nan"))), ("dt infinite", dict(dt=float("inf"))),
              ("damping negative", dict(damping=-0.5)), ("damping nan", dict(damping=float("nan"))), ("damping infinite", dict(damping=float("inf"))),
              ("clamped two", dict(clamped=2)), ("clamped negative", dict(clamped=-1)))


def create_cases(smg):
    """[(name, thunk -> (code, message), holds only without a device)]: the base's checks in its order, the levels, the mesh, the parameters, speed,
    sigma, then the clamped boundary"""
    V, F = flat_square(8)
    n = V.shape[0]
    keep = {"mg": smg.mg_precompute(V, F, 0.25, 20, 1), "blk": smg.mg_precompute_block(V, F, 0.25, 20, 1)}
    keep["un"] = smg.Hierarchy.union([keep["mg"], keep["mg"]])
    mg, fake = keep["mg"], _fake_hierarchy(smg, n)
    V2, F2 = np.concatenate([V, V + 3.0]), np.concatenate([F, F + n])
    cases = [("null %s" % a, (lambda a=a: _create(smg, mg.h, V, F, null=a)), False) for a in ("h", "V", "F", "p", "out")]
    cases.append(("block hierarchy", lambda: _create(smg, keep["blk"].h, V, F), False))
    cases.append(("union", lambda: _create(smg, keep["un"].h, V2, F2), False))
    cases.append(("rows", lambda: _create(smg, mg.h, V[:-1], F, nV=n - 1), False))
    keep["one"] = smg.mg_precompute(V, F, 0.25, 200, 1)                       # 81 vertices, coarsest level 200: the mesh itself
    assert keep["one"].n_levels == 1
    cases.append(("one level", lambda: _create(smg, keep["one"].h, V, F), False))
    Fo = F.copy()
    Fo[3, 1] = n
    cases.append(("face index", lambda: _create(smg, fake.h, V, Fo), False))
    Vz = V.copy()
    Vz[F[0, 1]] = Vz[F[0, 0]]
    cases.append(("zero area", lambda: _create(smg, fake.h, Vz, F), False))
    keep["two"] = _fake_hierarchy(smg, 2 * n)
    cases.append(("two components", lambda: _create(smg, keep["two"].h, V2, F2), False))
    for name, bad in BAD_PARAMS:
        cases.append(("parameter: " + name, (lambda bad=bad: _create(smg, fake.h, V, F, **bad)), False))
    ones = np.ones(n)
    for name, val in (("zero", 0.0), ("negative", -1.0), ("nan", np.nan), ("infinite", np.inf)):
        x = ones.copy()
        x[5] = val
        cases.append(("speed " + name, (lambda x=x: _create(smg, fake.h, V, F, speed=x)), False))
    for name, val in (("negative", -1e-3), ("nan", np.nan), ("infinite", np.inf)):
        x = 0.1 * ones
        x[7] = val
        cases.append(("sigma " + name, (lambda x=x: _create(smg, fake.h, V, F, sigma=x)), False))
    Vc, Fc = N.shape("icosphere1")
    keep["closed"] = _fake_hierarchy(smg, Vc.shape[0])
    cases.append(("clamped without boundary", lambda: _create(smg, keep["closed"].h, Vc, Fc, clamped=1), False))
    Vt, Ft = flat_square(1)                                                   # 4 vertices, 2 faces: every vertex is on the boundary
    keep["tiny"] = _fake_hierarchy(smg, Vt.shape[0])
    cases.append(("clamped without interior vertex", lambda: _create(smg, keep["tiny"].h, Vt, Ft, clamped=1), False))
    bad_speed, bad_sigma = ones.copy(), ones.copy()
    bad_speed[0], bad_sigma[0] = 0.0, -1.0
    cases.append(("order: hierarchy before levels", lambda: _create(smg, keep["blk"].h, Vz, F), False))
    cases.append(("order: levels before mesh", lambda: _create(smg, keep["one"].h, Vz, F), False))
    cases.append(("order: mesh before parameters", lambda: _create(smg, fake.h, Vz, F, dt=-1.0), False))
    cases.append(("order: dt before damping", lambda: _create(smg, fake.h, V, F, dt=0.0, damping=-0.5), False))
    cases.append(("order: damping before clamped", lambda: _create(smg, fake.h, V, F, damping=-0.5, clamped=2), False))
    cases.append(("order: parameters before speed", lambda: _create(smg, fake.h, V, F, clamped=2, speed=bad_speed), False))
    cases.append(("order: speed before sigma", lambda: _create(smg, fake.h, V, F, speed=bad_speed, sigma=bad_sigma), False))
    cases.append(("order: sigma before the boundary", lambda: _create(smg, keep["closed"].h, Vc, Fc, clamped=1, sigma=np.full(Vc.shape[0], -1.0)), False))
    for case, kw in (("free", dict()), ("clamped", dict(clamped=1)), ("speed and sigma", dict(speed=2.0 * ones, sigma=0.1 * ones))):
        cases.append(("valid, real hierarchy, " + case, (lambda kw=kw: _create(smg, mg.h, V, F, dt=0.1, **kw)), True))
    cases.append(("valid, closed, fake hierarchy", lambda: _create(smg, keep["closed"].h, Vc, Fc), True))
    return cases, keep


def null_object_cases(smg):
    """every entry point that takes the object, called without one"""
    L = smg._lib.load()
    X, I = np.zeros(40), np.zeros(4, dtype=np.int32)
    dp, ip = X.ctypes.data_as(C.POINTER(C.c_double)), I.ctypes.data_as(C.POINTER(C.c_int))
    p = L.smg_wave_params_default()
    calls = {"set_solver": lambda: L.smg_wave_set_solver(None, 1), "set_params": lambda: L.smg_wave_set_params(None, C.byref(p)),
             "set_state": lambda: L.smg_wave_set_state(None, X.ctypes.data, X.ctypes.data, 4, 1, 0),
             "state": lambda: L.smg_wave_state(None, X.ctypes.data, X.ctypes.data, 4, 0), "set_sources": lambda: L.smg_wave_set_sources(None, ip, 1),
             "set_receivers": lambda: L.smg_wave_set_receivers(None, ip, 1), "step": lambda: L.smg_wave_step(None, 1, None, None, dp, dp, None, None)}
    return [("null object: " + k, (lambda f=f: (f(), L.smg_last_error().decode())), False) for k, f in calls.items()]


def host_twin_cases(smg, call=None, prefix="host twin"):
    """the operand checks smg_wave_host and smg_debug_wave share"""
    call = call or (lambda *a, **k: N.host(smg, *a, **k)[0])
    L = smg._lib.load()
    V, F = N.shape("icosphere1")
    n = V.shape[0]
    u, v, w = N.test_state(V, F, 2)
    Fo = np.array(F)
    Fo[1, 2] = n
    idx = np.array([0, n - 1], dtype=np.int32)
    sg = np.ones((2, 2))
    bad_speed, bad_sigma = np.ones(n), np.zeros(n)
    bad_speed[3], bad_sigma[4] = 0.0, np.nan
    rh, ad = dict(k=2, u=u, v=v), dict(k=2, u=u, v=v, w=w)
    so, rc_ = dict(k=2, u=u, v=v, idx=idx, sig0=sg, sig1=sg), dict(k=2, u=u, idx=idx)
    thunks = {
        "unknown op": lambda: call(4, V, F, **rh), "negative op": lambda: call(-1, V, F, **rh),
        "out missing": lambda: call(N.WAVE_RHS, V, F, over=dict(out=None), **rh),
        "V missing": lambda: call(N.WAVE_RHS, V, F, over=dict(V=None), **rh),
        "F missing": lambda: call(N.WAVE_ADVANCE, V, F, over=dict(F=None), **ad),
        "no vertex": lambda: call(N.WAVE_RHS, V, F, over=dict(nV=0), **rh),
        "u missing": lambda: call(N.WAVE_RHS, V, F, k=2, v=v),
        "v missing": lambda: call(N.WAVE_ADVANCE, V, F, k=2, u=u, w=w),
        "w missing": lambda: call(N.WAVE_ADVANCE, V, F, **rh),
        "list missing": lambda: call(N.WAVE_RECORD, V, F, k=2, u=u),
        "signal missing": lambda: call(N.WAVE_SOURCES, V, F, k=2, u=u, v=v, idx=idx, sig0=sg),
        "k zero": lambda: call(N.WAVE_RHS, V, F, **dict(rh, k=0)),
        "k negative": lambda: call(N.WAVE_ADVANCE, V, F, **dict(ad, k=-2)),
        "dt zero": lambda: call(N.WAVE_RHS, V, F, dt=0.0, **rh),
        "dt nan": lambda: call(N.WAVE_ADVANCE, V, F, dt=float("nan"), **ad),
        "clamped two": lambda: call(N.WAVE_RHS, V, F, clamped=2, **rh),
        "speed zero": lambda: call(N.WAVE_RHS, V, F, speed=bad_speed, **rh),
        "sigma nan": lambda: call(N.WAVE_RHS, V, F, sigma=bad_sigma, **rh),
        "face index": lambda: call(N.WAVE_ADVANCE, V, Fo, **ad),
        "empty list": lambda: call(N.WAVE_RECORD, V, F, over=dict(n_idx=0), **rc_),
        "list index": lambda: call(N.WAVE_RECORD, V, F, **dict(rc_, idx=np.array([0, n], dtype=np.int32))),
        "negative list index": lambda: call(N.WAVE_SOURCES, V, F, **dict(so, idx=np.array([-1, 2], dtype=np.int32))),
        "source twice": lambda: call(N.WAVE_SOURCES, V, F, **dict(so, idx=np.array([5, 5], dtype=np.int32))),
        "order: operands before k": lambda: call(N.WAVE_ADVANCE, V, F, k=0, u=u, v=v),
        "order: k before dt": lambda: call(N.WAVE_RHS, V, F, dt=0.0, **dict(rh, k=0)),
        "order: dt before clamped": lambda: call(N.WAVE_RHS, V, F, dt=0.0, clamped=2, **rh),
        "order: clamped before speed": lambda: call(N.WAVE_RHS, V, F, clamped=2, speed=bad_speed, **rh),
        "order: speed before sigma": lambda: call(N.WAVE_RHS, V, F, speed=bad_speed, sigma=bad_sigma, **rh),
        "order: sigma before faces": lambda: call(N.WAVE_RHS, V, Fo, sigma=bad_sigma, **rh),
        "order: faces before the list": lambda: call(N.WAVE_RECORD, V, Fo, **dict(rc_, idx=np.array([0, n], dtype=np.int32))),
    }
    return [("%s: %s" % (prefix, k), (lambda f=f: (f(), L.smg_last_error().decode())), False) for k, f in thunks.items()]


def check_cases(smg, cases, golden):
    no_device = smg._lib.load().smg_device_count() == 0
    seen = set()
    for name, thunk, device_only in cases:
        if device_only and not no_device:
            continue
        rc, msg = thunk()
        seen.add(name)
        assert [rc, msg] == golden[name], name
        assert rc == (NO_DEVICE if device_only else INVALID), name
    return seen


def test_refusals_keep_code_and_message(smg_mod):
    """every refusal of smg_wave_create, of the calls on a missing object and of the host twin's operand checks, with the code and the
    smg_last_error() text recorded in tests/golden/wave_refusals.json; all of create's come before SMG_ERR_NO_DEVICE, which a valid call meets on
    a box without a GPU.  The refusals that need a live object (group "live") are checked by tests/test_gpu_wave.py.  Every message carries its
    entry point's name."""
    golden = json.load(open(GOLDEN))
    cases, keep = create_cases(smg_mod)
    assert check_cases(smg_mod, cases, golden["create"]) == set(golden["create"]) - (
        set() if smg_mod._lib.load().smg_device_count() == 0 else {c[0] for c in cases if c[2]})
    assert check_cases(smg_mod, null_object_cases(smg_mod), golden["null"]) == set(golden["null"])
    assert check_cases(smg_mod, host_twin_cases(smg_mod), golden["host"]) == set(golden["host"])
    g = golden["create"]
    assert g["order: hierarchy before levels"] == g["block hierarchy"]
    assert g["order: levels before mesh"] == g["one level"]
    assert g["order: mesh before parameters"] == g["zero area"]
    assert g["order: dt before damping"] == g["parameter: dt zero"]
    assert g["order: damping before clamped"] == g["parameter: damping negative"]
    assert g["order: parameters before speed"] == g["parameter: clamped two"]
    assert "speed[0]" in g["order: speed before sigma"][1] and "sigma[0]" in g["order: sigma before the boundary"][1]
    assert "two levels" in g["one level"][1] and "no boundary" in g["clamped without boundary"][1] and "interior" in g["clamped without interior vertex"][1]
    assert all(v[1].startswith("smg_wave_create: ") for v in g.values())
    for name, _ in BAD_PARAMS:
        assert name.split()[0] in g["parameter: " + name][1]
    h = golden["host"]
    assert h["host twin: order: operands before k"] == h["host twin: w missing"]
    assert h["host twin: order: k before dt"] == h["host twin: k zero"]
    assert h["host twin: order: dt before clamped"] == h["host twin: dt zero"]
    assert h["host twin: order: clamped before speed"] == h["host twin: clamped two"]
    assert h["host twin: order: speed before sigma"] == h["host twin: speed zero"]
    assert h["host twin: order: sigma before faces"] == h["host twin: sigma nan"]
    assert h["host twin: order: faces before the list"] == h["host twin: face index"]
    assert all(v[1].startswith("smg_wave_host: ") for v in h.values())
    for name, (code, msg) in golden["null"].items():
        assert msg.startswith("smg_wave_" + name.split(": ")[1] + ": ")
    for name, (code, msg) in golden["live"].items():
        assert code == INVALID and msg.startswith("smg_wave_" + name.split()[0] + ": "), name


def test_hook_refuses_what_the_host_twin_refuses(smg_mod):
    golden = json.load(open(GOLDEN))["host"]
    hook = lambda *a, **k: N.hook(smg_mod, *a, **k)[0]   # noqa: E731
    for name, thunk, _ in host_twin_cases(smg_mod, hook, "hook"):
        rc, msg = thunk()
        want = golden[name.replace("hook: ", "host twin: ")]
        assert [rc, msg] == [want[0], want[1].replace("smg_wave_host", "smg_debug_wave")], name
    if smg_mod._lib.load().smg_device_count() == 0:
        V, F = N.shape("icosphere1")
        u, v, _ = N.test_state(V, F, 1)
        assert N.hook(smg_mod, N.WAVE_RHS, V, F, u=u, v=v)[0] == NO_DEVICE


def test_timing_hook_refuses_before_the_device(smg_mod):
    """smg_debug_wave_time: another op, k < 1, reps < 1, a missing array and a face index out of range are SMG_ERR_INVALID; a valid call without a
    GPU is SMG_ERR_NO_DEVICE"""
    L = smg_mod._lib.load()
    V, F = N.shape("icosphere1")
    Fp, Vp = F.ctypes.data_as(C.POINTER(C.c_int)), V.ctypes.data_as(C.POINTER(C.c_double))
    n, nF, ms = V.shape[0], F.shape[0], C.c_double(0.0)
    for bad in ((N.WAVE_SOURCES, n, nF, 1, Fp, Vp, 1, C.byref(ms)), (N.WAVE_RECORD, n, nF, 1, Fp, Vp, 1, C.byref(ms)), (0, n, nF, 0, Fp, Vp, 1, C.byref(ms)),
                (0, n, nF, 1, Fp, Vp, 0, C.byref(ms)), (0, n, nF, 1, None, Vp, 1, C.byref(ms)), (2, n, nF, 1, Fp, Vp, 1, None),
                (2, n - 1, nF, 1, Fp, Vp, 1, C.byref(ms))):
        assert L.smg_debug_wave_time(*bad) == INVALID and L.smg_last_error().startswith(b"smg_debug_wave_time: ")
    if L.smg_device_count() == 0:
        assert L.smg_debug_wave_time(N.WAVE_ADVANCE, n, nF, 1, Fp, Vp, 1, C.byref(ms)) == NO_DEVICE


def test_no_gpu_comes_after_every_argument_check(smg_mod):
    """without a GPU WaveEquation(...) raises the no-device error, and only once every argument check has passed"""
    if smg_mod._lib.load().smg_device_count() > 0:
        pytest.skip("a GPU is present")
    V, F = flat_square(8)
    fake = _fake_hierarchy(smg_mod, V.shape[0])
    with pytest.raises(smg_mod.SmgError) as e:
        smg_mod.WaveEquation(fake, V, F, 0.1, speed=2.0, sigma=0.1, clamped=True)
    assert e.value.code == NO_DEVICE and "smg_wave_create" in str(e.value) and "no CPU fallback" in str(e.value)
    with pytest.raises(smg_mod.SmgError) as e:
        smg_mod.WaveEquation(fake, V, F, -0.1)
    assert e.value.code == INVALID
    with pytest.raises(smg_mod.SmgError) as e:
        smg_mod.WaveEquation(fake, V, F, 0.1, speed=0.0)
    assert e.value.code == INVALID and "speed[0]" in str(e.value)
    with pytest.raises(TypeError):
        smg_mod.WaveEquation(fake, V, F, 0.1, beta=1.0)


# ---- the host twin against the restatement ---------------------------------------------------------------------------------------------------------
def host_run(smg):
    def run(op, V, F, **kw):
        rc, out = N.host(smg, op, V, F, **kw)
        assert rc == 0
        return out
    return run


def launcher_cases(name):
    """(clamped, list length) pairs of a launcher mesh: free everywhere, clamped where there is a boundary; lists of 1 and of 3"""
    has_boundary = N.boundary_vertices(np.asarray(N.shape(name)[1])).size > 0
    return [(cl, cnt) for cl in ((False, True) if has_boundary else (False,)) for cnt in (1, 3)]


@pytest.mark.parametrize("k", [1, 3, 8])
@pytest.mark.parametrize("name", MESHES)
def test_host_twin_against_restatement(smg_mod, name, k):
    """all four ops, free and clamped, lists of 1 and 3 vertices that contain vertex 0 and vertex nV - 1, bit for bit"""
    for clamped, count in launcher_cases(name):
        N.check_launchers(host_run(smg_mod), name, k, clamped, count)


# ---- the restatement itself: the identities of the header -------------------------------------------------------------------------------------------
def wave_slack(ref, f0=None, f1=None):
    """SLACK of POWER for the step `ref` has just made, per column; and the 2-norm eps (q2 |u'| + 2 q2 |u' - u| + |v'|) of v's rounding"""
    col = lambda x: np.linalg.norm(x, axis=0)   # noqa: E731
    dt, q2 = ref.p["dt"], ref.q2
    mag = ref.mt[:, None] * (np.abs(ref.s2[:, None] * ref.u0) + dt * np.abs(ref.v0))
    fbar = np.zeros(ref.u.shape)
    if f0 is not None:
        mag[ref.src] += ref.a * np.abs(f0 + f1)
        fbar[ref.src] = 0.5 * (f0 + f1)
    Aw = abs(ref.A) @ np.abs(ref.w) + np.abs(ref.b)
    Aw[ref.known] = 0.0
    dv = EPS * (q2 * col(ref.u) + 2.0 * q2 * col(ref.u - ref.u0) + col(ref.v))
    vbar = 0.5 * np.abs(ref.v0 + ref.v)
    sig = (ref.s2 - 2.0) / dt
    slack = (col(ref.v0 + ref.v) / dt * (4.0 * EPS * col(mag) + 16.0 * EPS * col(Aw)) + col(ref.mt[:, None] * ref.v) * dv + col(ref.C @ ref.u) * EPS * col(ref.u)
             + 16.0 * EPS * (ref.E_abs(ref.u0, ref.v0) + ref.E_abs(ref.u, ref.v) + dt * np.sum(vbar * ((sig * ref.mt)[:, None] * vbar + np.abs(fbar)), axis=0)))
    return slack, dv


def power_terms(ref, f0=None, f1=None):
    """(E' - E, the damping and force terms of POWER, v + v') for the step `ref` has just made, per column"""
    dt = ref.p["dt"]
    vbar = 0.5 * (ref.v0 + ref.v)
    sig = (ref.s2 - 2.0) / dt
    rate = -dt * np.sum(vbar * ((sig * ref.mt)[:, None] * vbar), axis=0)
    if f0 is not None:
        fbar = np.zeros(ref.u.shape)
        fbar[ref.src] = 0.5 * (f0 + f1)
        rate = rate + dt * np.sum(vbar * fbar, axis=0)
    return ref.E(ref.u, ref.v) - ref.E(ref.u0, ref.v0), rate, ref.v0 + ref.v


def ricker_signal(smg, n_steps, dt, n_src, k, f0=2.0, t0=0.3):
    """(n_steps + 1) x n_src x k: a Ricker wavelet per (source, column) with its own delay and sign"""
    t = dt * np.arange(n_steps + 1)
    j, c = np.arange(n_src)[None, :, None], np.arange(k)[None, None, :]
    return np.ascontiguousarray((1.0 - 0.5 * (j % 2)) * smg.wavelets.ricker(f0, t[:, None, None], t0 + 0.05 * c + 0.02 * j))


POWER_CASES = {"undamped, unforced": dict(damping=0.0, force=False), "uniform damping": dict(damping=0.8, force=False),
               "a Ricker source": dict(damping=0.0, force=True)}


@pytest.mark.parametrize("case", list(POWER_CASES))
@pytest.mark.parametrize("name,clamped", [("icosphere2", 0), ("square", 0), ("square", 1)])
def test_power_balance_at_every_step(smg_mod, name, clamped, case):
    """POWER of the header at every one of 20 steps, k = 2 with a non-uniform speed; r is the direct solve's own residual"""
    V, F = N.shape(name)
    cfg = POWER_CASES[case]
    ref = N.WaveNp(V, F, speed=N.nonuniform(V)[0], dt=0.05, damping=cfg["damping"], clamped=clamped)
    u0, v0, _ = N.test_state(V, F, 2, clamped)
    ref.set_state(u0, v0)
    ref.src = N.test_lists(V, F, 3, clamped)
    sig = ricker_signal(smg_mod, 20, 0.05, 3, 2) if cfg["force"] else None
    worst, E0 = 0.0, ref.E(ref.u, ref.v)
    for t in range(20):
        f = (None, None) if sig is None else (sig[t], sig[t + 1])
        ref.step(1, None if sig is None else sig[t:t + 2])
        dE, rate, vs = power_terms(ref, *f)
        rterm = np.sum(vs * ref.residual(ref.w, ref.b), axis=0) / ref.p["dt"]
        slack = wave_slack(ref, *f)[0]
        worst = max(worst, float(np.max(np.abs(dE - rate - rterm) / slack)))
        assert np.all(np.abs(dE - rate - rterm) <= slack), (t, dE, rate, rterm, slack)
        if case == "undamped, unforced":
            assert np.all(np.abs(dE) <= np.linalg.norm(vs, axis=0) * ref.res / ref.p["dt"] + slack)
        if case == "uniform damping":
            assert np.all(dE < 0.0)
    E1 = ref.E(ref.u, ref.v)
    print("%s, clamped %d, %s: E %s -> %s; largest |E' - E - terms| over its slack %.3f (last slack %s)" % (name, clamped, case, E0, E1, worst, slack))
    if case == "undamped, unforced":
        assert np.all(np.abs(E1 - E0) <= 1e-10 * E0)
    if case == "uniform damping":
        assert np.all(E1 < 0.9 * E0)
    if case == "a Ricker source":
        assert np.all(np.abs(E1 - E0) > 1e-6 * E0)


@pytest.mark.parametrize("name", ["icosphere2", "square"])
def test_momentum_on_a_free_boundary(smg_mod, name):
    """MOMENTUM of the header at every one of 20 steps with a Ricker source, k = 2, non-uniform speed"""
    V, F = N.shape(name)
    n, dt = V.shape[0], 0.05
    ref = N.WaveNp(V, F, speed=N.nonuniform(V)[0], dt=dt)
    u0, v0, _ = N.test_state(V, F, 2)
    ref.set_state(u0, v0)
    ref.src = N.test_lists(V, F, 3)
    sig = ricker_signal(smg_mod, 20, dt, 3, 2)
    d = row_sum_defect(ref.C)
    fs = lambda x: np.array([math.fsum(ref.mt * c) for c in x.T])   # noqa: E731
    P0, worst = fs(ref.v), 0.0
    for t in range(20):
        ref.step(1, sig[t:t + 2])
        want = fs(ref.v0) + dt * np.sum(0.5 * (sig[t] + sig[t + 1]), axis=0)
        slack, dv = wave_slack(ref, sig[t], sig[t + 1])
        mag = ref.mt[:, None] * (np.abs(ref.s2[:, None] * ref.u0) + dt * np.abs(ref.v0))
        bound = ref.q2 * (np.sqrt(n) * (ref.res + 4 * EPS * np.linalg.norm(mag, axis=0)) + ref.a * d * np.linalg.norm(ref.w, axis=0)) + np.linalg.norm(ref.mt) * dv
        worst = max(worst, float(np.max(np.abs(fs(ref.v) - want) / bound)))
        assert np.all(np.abs(fs(ref.v) - want) <= bound), (t, fs(ref.v), want, bound)
    print("%s: sum mt v %s -> %s; largest defect over its bound %.3f (last bound %s)" % (name, P0, fs(ref.v), worst, bound))
    assert np.all(np.abs(fs(ref.v) - P0) > 1e3 * bound), "the source has changed the momentum"


@functools.lru_cache(maxsize=None)
def eigen_setup(name, clamped, damping, dt=0.05, L_key=None):
    """(the restatement, lambda, phi extended by zeros, the pairs' residuals, the norms of the step map's powers) of EIGENMODE on a test mesh with a
    non-uniform speed; L_key: None or a hashable holder of the library's own L"""
    V, F = N.shape(name)
    ref = N.WaveNp(V, F, L=None if L_key is None else L_key.L, speed=N.nonuniform(V)[0], dt=dt, damping=damping, clamped=clamped)
    Cd = np.asarray(ref.C.todense())
    free = ref.free
    lam, ph = scipy.linalg.eigh(0.5 * (Cd + Cd.T)[np.ix_(free, free)], np.diag(ref.mt[free]))
    phi = np.zeros((V.shape[0], lam.size))
    phi[free] = ph
    r = Cd @ phi - (ref.mt[:, None] * phi) * lam[None, :]
    r[ref.known] = 0.0
    return ref, lam, phi, np.linalg.norm(r, axis=0), N.power_norms(ref.step_map(), 20)


def mode_recurrence(ref, lam, alpha, beta, steps):
    """[(alpha_n, beta_n, omega_n)] of EIGENMODE; alpha, beta, lam: k values"""
    s2, a, dt, q2 = 2.0 + ref.p["damping"] * ref.p["dt"], ref.a, ref.p["dt"], ref.q2
    out = [(np.array(alpha, dtype=np.float64), np.array(beta, dtype=np.float64), None)]
    for _ in range(steps):
        al, be, _ = out[-1]
        om = (s2 * al + dt * be) / (0.5 * s2 + a * lam)
        al1 = om - al
        out.append((al1, q2 * (al1 - al) - be, om))
    return out


def eigenmode_bounds(ref, lam_c, res_c, norms, amps, steps):
    """EIGENMODE's bound after every step along `ref`, which this advances"""
    chain, bounds = N.Chain(ref, 0.0, norms), []
    for n in range(1, steps + 1):
        ref.step(1)
        bounds.append(chain.after(extra=ref.a * np.abs(amps[n][2]) * res_c / ref.mu))
    return bounds


MODE_COLUMNS = (1, 7, -1)


@pytest.mark.parametrize("name,clamped", [("icosphere3", 0), ("square", 1)])
@pytest.mark.parametrize("damping", [0.0, 0.8])
def test_eigenmodes_follow_the_2x2_recurrence(smg_mod, name, clamped, damping):
    """EIGENMODE of the header over 20 steps, three columns: a low mode, a middle one and the highest; on the clamped square with the interior
    block; undamped also the closed-form rotation"""
    ref, lam, phi, res, norms = eigen_setup(name, clamped, damping)
    cols = np.array(MODE_COLUMNS)
    lc = lam[cols]
    assert np.all(lc > 0.0)
    amps = mode_recurrence(ref, lc, [1.0, -0.5, 0.25], [0.3, 1.0, -2.0], 20)
    ref.set_state(phi[:, cols] * amps[0][0], phi[:, cols] * amps[0][1])
    bounds = eigenmode_bounds(ref, lc, res[cols], norms, amps, 20)
    ref.set_state(phi[:, cols] * amps[0][0], phi[:, cols] * amps[0][1])
    worst = 0.0
    for n in range(1, 21):
        ref.step(1)
        err = N.distance(ref.u, ref.v, phi[:, cols] * amps[n][0], phi[:, cols] * amps[n][1])
        worst = max(worst, float(np.max(err / bounds[n - 1])))
        assert np.all(err <= bounds[n - 1]), (n, err, bounds[n - 1])
    size = np.sqrt(amps[0][0] ** 2 + amps[0][1] ** 2) * np.linalg.norm(phi[:, cols], axis=0)
    print("%s, clamped %d, damping %g: lambda %s; largest |np - recurrence|_2 over its bound %.3f (last bound %s, |S^19|_2 %.3e)"
          % (name, clamped, damping, lc, worst, bounds[-1], norms[-1]))
    assert np.all(bounds[-1] <= 1e-6 * size), "the bound is far below the run's amplitude"
    rad = lambda a: np.sqrt(a[0] ** 2 + a[1] ** 2 / lc)   # noqa: E731
    if damping == 0.0:
        theta = 2.0 * np.arctan(0.5 * ref.p["dt"] * np.sqrt(lc))
        g0 = amps[0][1] / np.sqrt(lc)
        for n in range(1, 21):
            ca, sa = np.cos(n * theta), np.sin(n * theta)
            want_a, want_g = amps[0][0] * ca + g0 * sa, -amps[0][0] * sa + g0 * ca
            tol = 64 * n * EPS * rad(amps[0])
            assert np.all(np.abs(amps[n][0] - want_a) <= tol) and np.all(np.abs(amps[n][1] / np.sqrt(lc) - want_g) <= tol), n
            assert np.all(np.abs(rad(amps[n]) - rad(amps[0])) <= tol), "the amplitude is kept"
    else:
        assert np.all(rad(amps[20]) < rad(amps[0]))


def test_clamped_rows_stay_exact_zeros(smg_mod):
    """CLAMPED of the header: 20 steps on the square with a source and damping"""
    V, F = N.shape("square")
    ref = N.WaveNp(V, F, dt=0.05, damping=0.3, clamped=1)
    u0, v0, _ = N.test_state(V, F, 2, True)
    ref.set_state(u0, v0)
    ref.src = N.test_lists(V, F, 3, True)
    sig = ricker_signal(smg_mod, 20, 0.05, 3, 2)
    assert ref.known.sum() > 0 and not np.any(ref.known[ref.src])
    for t in range(20):
        ref.step(1, sig[t:t + 2])
        for x in (ref.u, ref.v, ref.w, ref.b):
            assert np.all(x[ref.known] == 0.0) and np.any(x[~ref.known] != 0.0)


@pytest.mark.parametrize("name", ["icosphere2", "torus", "square", "bunny.smgm"])
def test_potential_energy_is_the_quadratic_form(name):
    """POTENTIAL of the header"""
    V, F = N.shape(name)
    ref = N.WaveNp(V, F)
    u = N.test_state(V, F, 3)[0]
    W, _, A = rest_faces(V, F)
    absg = sum(np.abs(u[F[:, i]])[:, :, None] * np.abs(W[:, i, :])[:, None, :] for i in range(3))        # nF x k x 3
    scale = np.sum(A[:, None] * np.sum(absg, axis=2) ** 2, axis=0)
    pe, quad = N.potential(V, F, u), 0.5 * np.sum(u * (ref.C @ u), axis=0)
    print("%s: potential %s, |face sum - 0.5 u'Cu| / (16 eps scale) %s" % (name, pe, np.abs(pe - quad) / (16 * EPS * scale)))
    assert np.all(np.abs(pe - quad) <= 16 * EPS * scale) and np.all(pe > 0.0)


# ---- the kernels' registers, the host maths under sanitizers -------------------------------------------------------------------------------------
def test_kernels_keep_everything_in_registers():
    """the ISA notes of the kernels of smg_wave_device.hip (the build's flags, device side only): no scratch, no spills, no contraction"""
    import re
    from surface_multigrid_code_amd import build as B
    src = os.path.join(B.CSRC, "smg_wave_device.hip")
    asm = subprocess.check_output([B._hipcc()] + B.FLAGS + ["--cuda-device-only", "-S", src, "-o", "-"], text=True, stderr=subprocess.DEVNULL)
    notes = dict(re.findall(r"\.name:\s+(\S*k_wave\S*)(.*?)\.wavefront_size", asm, flags=re.S))
    assert len(notes) == 6                                                    # rhs, sources, advance with and without the next b, record, rows_nonzero
    for kernel, body in notes.items():
        field = lambda k: int(re.search(r"\.%s:\s+(\d+)" % k, body).group(1))   # noqa: E731
        print("%s: vgpr_count %d, sgpr_count %d, private_segment_fixed_size %d" % (kernel, field("vgpr_count"), field("sgpr_count"), field("private_segment_fixed_size")))
        assert field("private_segment_fixed_size") == 0 and field("vgpr_spill_count") == 0 and field("sgpr_spill_count") == 0 and field("vgpr_count") <= 32
    for word in ("v_fma_f64", "v_fmac_f64", "v_div_scale_f64", "v_div_fmas_f64", "v_div_fixup_f64", "v_rcp_f64"):
        assert word not in asm, "no contraction and no fp64 division (the lane's column and vertex are an integer division)"


def test_host_maths_under_sanitizers(tmp_path):
    """tests/wave_asan_driver.cpp, a stand-alone program: the host twin's loops (smg::wave_host_* of csrc/smg_wave_inl.hpp, what smg_wave_host runs
    after its checks) on exactly-sized heap arrays, under AddressSanitizer and UndefinedBehaviorSanitizer (static runtimes: run directly, nothing
    preloaded, nothing loaded into python)"""
    exe = str(tmp_path / "wave_asan_driver")
    csrc = os.path.join(ROOT, "surface_multigrid_code_amd", "csrc")
    srcs = [os.path.join(ROOT, "tests", "wave_asan_driver.cpp"), os.path.join(csrc, "smg_mesh.cpp"), os.path.join(csrc, "smg_sparse.cpp")]
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-ffp-contract=off", "-pthread", "-I" + csrc] + srcs + ["-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    run = subprocess.run([exe], env=env, capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0 and run.stdout.count("ok 1") == 6 and "ERROR" not in run.stderr
