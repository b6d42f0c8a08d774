"""CPU: incompressible flow on a surface in vorticity form (include/smg.h: smg_fluid_*) -- the ABI and its refusals without a GPU, the library's host
twin (smg_fluid_host) against the numpy restatement (tests/fluid_np.py), and the restatement itself against the scheme's exact invariants.

Masses, right-hand sides, both forms of the transport with each (a, b) pair, the velocity, the diagnostics' terms, every sum and the step's closing
arithmetic are correctly rounded +, -, *, /, max and fabs in one order on both sides: held bit for bit.

The identities, every quantity computed on the CPU from the restatement; eps = 2^-52, deg = the largest number of corners of a vertex, t_s = the
transport term (0.5 (Phi - theta |Phi|)) (w_nbr - w_i) of a segment, G = 2 deg + 32 (2 deg sequential additions of a corner list, the tree of
a fixed-order sum, the few operations of a term):

    FLUX         the geometric flux of u_f = n_f x grad psi_f through a dual segment a -> b of face f, u_f . ((b - a) x n_f), equals psi(a) - psi(b),
                 the Phi of the kernels: |difference| <= 16 eps kappa_f (|psi_0| + |psi_1| + |psi_2|) (|W_f0| + |W_f1| + |W_f2|) |b - a|,
                 kappa_f = max(1, P_f / h_f) with P_f the largest |position| of the face and h_f its smallest altitude (the gradient is a sum of
                 three products whose terms cancel; the cross and dot products add a few eps of the same size; every edge, and with it the
                 normal, W and b - a, is a difference of positions with the absolute error eps P_f, a relative error eps P_f / h_f at worst)
    DIVERGENCE   the segment fluxes of every vertex sum to zero (with psi = 0 on the boundary, at boundary vertices too):
                 |sum| <= G eps sum_segments (|psi_i| + |psi_j| + |psi_k|)
    CIRCULATION  sum m out = a sum m wn + b sum m w for any stage: |difference| <= G eps (a sum m |wn| + b sum m |w| + b dt sum_i sum_s |t_s|)
    ENSTROPHY    theta = 0: sum_i m_i w_i adv_i = 0: |sum| <= G eps sum_i |w_i| sum_s |t_s|
    MAXIMUM      theta = 1 and dt rate_i <= 1: min and max of w over i and its ring bound out_i, up to G eps max |w| (a convex combination whose
                 weights sum to one up to rounding); the three-stage step is a convex combination of such stages
    VISCOUS      sum m w_new = sum m w*: |difference| <= |r|_1 + G eps (sum m |w_new| + viscosity dt sum_ij |L_ij| |w_new_j|), r the direct solve's
                 residual: the columns of L sum to zero

The physics, on FluidNp (direct solves) on icosphere(3) with w = z, where the exact stream function is -z / 2 and the exact velocity
(1/2) z^ x n (measured on the restatement: 7.27e-4, 6.48e-3 and a drift of 1.64e-3; the first two bounds carry a factor 2, the third is the issue's):

    STREAM       max |(psi - mean) - (-z / 2)| <= 1.5e-3
    VELOCITY     max_f |u_f - (1/2) z^ x centroid_f| <= 1.3e-2
    STEADY       max |w - z| after 50 default steps <= 0.01 max |w|"""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import fluid_np as N
from hodge_np import cross3, dot3
from morph_np import rest_faces
from test_arap_host import _fake_hierarchy
from test_geodesics_host import flat_square

INVALID, NO_DEVICE = -1, -2
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fluid_refusals.json")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = N.EPS
MESHES = N.LAUNCHER_MESHES

FLUID_SYMBOLS = ("smg_fluid_params_default", "smg_fluid_create", "smg_fluid_destroy", "smg_fluid_set_params", "smg_fluid_set_solver", "smg_fluid_is_closed",
                 "smg_fluid_device_bytes", "smg_fluid_set_vorticity", "smg_fluid_vorticity", "smg_fluid_step", "smg_fluid_stream", "smg_fluid_velocity",
                 "smg_fluid_diagnostics", "smg_fluid_host", "smg_debug_fluid", "smg_debug_fluid_time")


# ---- the ABI and its refusals --------------------------------------------------------------------------------------------------------------------
def test_abi_present(smg_mod):
    L = smg_mod._lib.load()
    for name in FLUID_SYMBOLS:
        assert hasattr(L, name)
    assert hasattr(smg_mod, "SurfaceFluid") and hasattr(smg_mod, "fluid_params")
    assert L.smg_version() >= 520
    assert L.smg_fluid_device_bytes(None) == 0 and L.smg_fluid_is_closed(None) == 0
    p = L.smg_fluid_params_default()
    assert (p.theta, p.stages, p.viscosity, p.dt, p.cfl) == (0.0, 3, 0.0, 0.0, 0.5)
    assert {f: getattr(p, f) for f, _ in p._fields_} == N.DEFAULTS


def _create(smg, h, V, F, nV=None, null=None, **params):
    """smg_fluid_create -> (code, message); a successful create is destroyed at once"""
    L = smg._lib.load()
    ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
    V, F = np.ascontiguousarray(V, dtype=np.float64), np.ascontiguousarray(F, dtype=np.int32)
    p = L.smg_fluid_params_default()
    for key, val in params.items():
        setattr(p, key, val)
    out = C.c_void_p(0xdead)
    rc = L.smg_fluid_create(None if null == "h" else h, None if null == "V" else V.ctypes.data_as(dp), V.shape[0] if nV is None else nV,
                            None if null == "F" else F.ctypes.data_as(ip), F.shape[0], None if null == "p" else C.byref(p),
                            None if null == "out" else C.byref(out))
    if rc == 0:
        L.smg_fluid_destroy(out)
        return rc, ""
    assert null == "out" or out.value is None, "a refused create must leave *out == NULL"
    return rc, L.smg_last_error().decode()


BAD_PARAMS = (("theta negative", dict(theta=-0.1)), ("theta above one", dict(theta=1.5)), ("theta nan", dict(theta=float("nan"))),
              ("stages zero", dict(stages=0)), ("stages four", dict(stages=4)), ("viscosity negative", dict(viscosity=-1.0, dt=0.1)),
              ("viscosity nan", dict(viscosity=float("nan"), dt=0.1)), ("viscosity without dt", dict(viscosity=0.1)), ("dt negative", dict(dt=-0.1)),
              ("dt infinite", dict(dt=float("inf"))), ("cfl zero", dict(cfl=0.0)), ("cfl nan", dict(cfl=float("nan"))))


def create_cases(smg):
    """[(name, thunk -> (code, message), holds only without a device)]: the base's checks in its order, no interior vertex, then the parameters"""
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
    Fo = F.copy()
    Fo[3, 1] = n
    cases.append(("face index", lambda: _create(smg, fake.h, V, Fo), False))
    Vz = V.copy()
    Vz[F[0, 1]] = Vz[F[0, 0]]
    cases.append(("zero area", lambda: _create(smg, fake.h, Vz, F), False))
    keep["plus"] = _fake_hierarchy(smg, n + 1)                                # one more vertex, in no face: the areas pass, the coordinate does not
    Vi = np.concatenate([V, [[np.inf, 0.0, 0.0]]])
    cases.append(("non-finite coordinate", lambda: _create(smg, keep["plus"].h, Vi, F), False))
    keep["two"] = _fake_hierarchy(smg, 2 * n)
    cases.append(("two components", lambda: _create(smg, keep["two"].h, V2, F2), False))
    Vt, Ft = flat_square(1)                                                   # four vertices, all of them on the boundary
    keep["tiny"] = _fake_hierarchy(smg, Vt.shape[0])
    cases.append(("no interior vertex", lambda: _create(smg, keep["tiny"].h, Vt, Ft), False))
    for name, bad in BAD_PARAMS:
        cases.append(("parameter: " + name, (lambda bad=bad: _create(smg, fake.h, V, F, **bad)), False))
    keep["one"] = smg.mg_precompute(V, F, 0.25, 200, 1)                       # 81 vertices, coarsest level 200: the mesh itself
    assert keep["one"].n_levels == 1
    cases.append(("one level with viscosity", lambda: _create(smg, keep["one"].h, V, F, viscosity=0.1, dt=0.1), False))
    cases.append(("order: hierarchy before mesh", lambda: _create(smg, keep["blk"].h, Vz, F), False))
    cases.append(("order: mesh before parameters", lambda: _create(smg, fake.h, Vz, F, theta=2.0), False))
    cases.append(("order: interior before parameters", lambda: _create(smg, keep["tiny"].h, Vt, Ft, stages=0), False))
    cases.append(("valid, real hierarchy", lambda: _create(smg, mg.h, V, F), True))
    cases.append(("valid, one level", lambda: _create(smg, keep["one"].h, V, F), True))
    Vc, Fc = N.shape("icosphere1")
    keep["closed"] = _fake_hierarchy(smg, Vc.shape[0])
    cases.append(("valid, closed, fake hierarchy", lambda: _create(smg, keep["closed"].h, Vc, Fc), True))
    return cases, keep


def null_object_cases(smg):
    """every entry point that takes the object, called without one"""
    L = smg._lib.load()
    X = np.zeros(12)
    dp = X.ctypes.data_as(C.POINTER(C.c_double))
    p = L.smg_fluid_params_default()
    calls = {"set_solver": lambda: L.smg_fluid_set_solver(None, 1), "set_params": lambda: L.smg_fluid_set_params(None, C.byref(p)),
             "set_vorticity": lambda: L.smg_fluid_set_vorticity(None, X.ctypes.data, 4, 1, 0), "vorticity": lambda: L.smg_fluid_vorticity(None, X.ctypes.data, 4, 0),
             "step": lambda: L.smg_fluid_step(None, 1, None, dp, dp, None, None), "stream": lambda: L.smg_fluid_stream(None, None, X.ctypes.data, 4, 0),
             "velocity": lambda: L.smg_fluid_velocity(None, None, X.ctypes.data, 0), "diagnostics": lambda: L.smg_fluid_diagnostics(None, None, dp)}
    return [("null object: " + k, (lambda f=f: (f(), L.smg_last_error().decode())), False) for k, f in calls.items()]


def host_twin_cases(smg, call=None, prefix="host twin"):
    """the operand checks smg_fluid_host and smg_debug_fluid share"""
    call = call or (lambda *a, **k: N.host(smg, *a, **k)[0])
    L = smg._lib.load()
    V, F = N.shape("icosphere1")
    psi, w, wn, dt = N.test_state(V, F, 1)
    Fo = np.array(F)
    Fo[1, 2] = V.shape[0]
    full = dict(psi=psi, w=w, wn=wn, dt=dt)
    thunks = {
        "unknown op": lambda: call(5, V, F, **full), "negative op": lambda: call(-1, V, F, **full),
        "out missing": lambda: call(N.FLUID_RHS, V, F, w=w, over=dict(out=None)),
        "V missing": lambda: call(N.FLUID_RHS, V, F, w=w, over=dict(V=None)),
        "F missing": lambda: call(N.FLUID_RHS, V, F, w=w, over=dict(F=None)),
        "no vertex": lambda: call(N.FLUID_RHS, V, F, w=w, over=dict(nV=0)),
        "w missing": lambda: call(N.FLUID_RHS, V, F),
        "psi missing": lambda: call(N.FLUID_ADVECT, V, F, rates_only=True),
        "wn missing": lambda: call(N.FLUID_ADVECT, V, F, psi=psi, w=w, dt=dt),
        "dt missing": lambda: call(N.FLUID_ADVECT, V, F, psi=psi, w=w, wn=wn),
        "psi missing for the velocity": lambda: call(N.FLUID_VELOCITY, V, F),
        "w missing for the diagnostics": lambda: call(N.FLUID_DIAG, V, F),
        "times missing": lambda: call(N.FLUID_DT, V, F, w=np.ones((3, 1))),
        "k zero": lambda: call(N.FLUID_RHS, V, F, w=w, k=0),
        "k negative": lambda: call(N.FLUID_VELOCITY, V, F, psi=psi, k=-2),
        "theta above one": lambda: call(N.FLUID_ADVECT, V, F, theta=1.25, **full),
        "theta nan": lambda: call(N.FLUID_ADVECT, V, F, theta=float("nan"), **full),
        "face index": lambda: call(N.FLUID_RHS, V, Fo, w=w),
        "order: operands before k": lambda: call(N.FLUID_VELOCITY, V, F, k=0),
        "order: k before theta": lambda: call(N.FLUID_ADVECT, V, F, k=0, theta=2.0, **full),
        "order: theta before faces": lambda: call(N.FLUID_ADVECT, V, Fo, theta=1.25, **full),
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
    """every refusal of smg_fluid_create, of the calls on a missing object and of the host twin's operand checks, with the code and the
    smg_last_error() text recorded in tests/golden/fluid_refusals.json; all of create's come before SMG_ERR_NO_DEVICE, which a valid call meets on
    a box without a GPU.  The refusals that need a live object (group "live") are checked by tests/test_gpu_fluid.py.  Every message carries its
    entry point's name."""
    golden = json.load(open(GOLDEN))
    cases, keep = create_cases(smg_mod)
    assert check_cases(smg_mod, cases, golden["create"]) == set(golden["create"]) - (
        set() if smg_mod._lib.load().smg_device_count() == 0 else {c[0] for c in cases if c[2]})
    assert check_cases(smg_mod, null_object_cases(smg_mod), golden["null"]) == set(golden["null"])
    assert check_cases(smg_mod, host_twin_cases(smg_mod), golden["host"]) == set(golden["host"])
    g = golden["create"]
    assert g["order: hierarchy before mesh"] == g["block hierarchy"]
    assert g["order: mesh before parameters"] == g["zero area"]
    assert g["order: interior before parameters"] == g["no interior vertex"]
    assert "no interior vertex" in g["no interior vertex"][1]
    assert all(v[1].startswith("smg_fluid_create: ") for v in g.values())
    for name, _ in BAD_PARAMS:
        assert name.split()[0] in g["parameter: " + name][1]
    h = golden["host"]
    assert h["host twin: order: operands before k"] == h["host twin: psi missing for the velocity"]
    assert h["host twin: order: k before theta"][1] == h["host twin: k zero"][1]
    assert h["host twin: order: theta before faces"] == h["host twin: theta above one"]
    assert all(v[1].startswith("smg_fluid_host: ") for v in h.values())
    for name, (code, msg) in golden["null"].items():
        assert msg.startswith("smg_fluid_" + name.split(": ")[1] + ": ")
    for name, (code, msg) in golden["live"].items():
        assert code == INVALID and msg.startswith("smg_fluid_" + name.split()[0] + ": "), name
    del keep


def test_hook_refuses_what_the_host_twin_refuses(smg_mod):
    golden = json.load(open(GOLDEN))["host"]
    hook = lambda *a, **k: N.hook(smg_mod, *a, **k)[0]   # noqa: E731
    for name, thunk, _ in host_twin_cases(smg_mod, hook, "hook"):
        rc, msg = thunk()
        want = golden[name.replace("hook: ", "host twin: ")]
        assert [rc, msg] == [want[0], want[1].replace("smg_fluid_host", "smg_debug_fluid")], name
    if smg_mod._lib.load().smg_device_count() == 0:
        V, F = N.shape("icosphere1")
        assert N.hook(smg_mod, N.FLUID_RHS, V, F, w=np.ones((V.shape[0], 1)))[0] == NO_DEVICE


def test_timing_hook_refuses_before_the_device(smg_mod):
    """smg_debug_fluid_time: the DT op, k < 1, reps < 1, a missing array and a face index out of range are SMG_ERR_INVALID; a valid call without
    a GPU is SMG_ERR_NO_DEVICE"""
    L = smg_mod._lib.load()
    V, F = N.shape("icosphere1")
    Fp, Vp = F.ctypes.data_as(C.POINTER(C.c_int)), V.ctypes.data_as(C.POINTER(C.c_double))
    n, nF, ms = V.shape[0], F.shape[0], C.c_double(0.0)
    for bad in ((N.FLUID_DT, n, nF, 1, Fp, Vp, 0, 1, C.byref(ms)), (0, n, nF, 0, Fp, Vp, 0, 1, C.byref(ms)), (0, n, nF, 1, Fp, Vp, 0, 0, C.byref(ms)),
                (0, n, nF, 1, None, Vp, 0, 1, C.byref(ms)), (0, n, nF, 1, Fp, Vp, 0, 1, None), (0, n - 1, nF, 1, Fp, Vp, 0, 1, C.byref(ms))):
        assert L.smg_debug_fluid_time(*bad) == INVALID and L.smg_last_error().startswith(b"smg_debug_fluid_time: ")
    if L.smg_device_count() == 0:
        assert L.smg_debug_fluid_time(N.FLUID_ADVECT, n, nF, 1, Fp, Vp, 0, 1, C.byref(ms)) == NO_DEVICE


def test_no_gpu_comes_after_every_argument_check(smg_mod):
    """without a GPU SurfaceFluid(...) raises the no-device error, and only once every argument check has passed"""
    if smg_mod._lib.load().smg_device_count() > 0:
        pytest.skip("a GPU is present")
    V, F = flat_square(8)
    fake = _fake_hierarchy(smg_mod, V.shape[0])
    with pytest.raises(smg_mod.SmgError) as e:
        smg_mod.SurfaceFluid(fake, V, F)
    assert e.value.code == NO_DEVICE and "smg_fluid_create" in str(e.value) and "no CPU fallback" in str(e.value)
    with pytest.raises(smg_mod.SmgError) as e:
        smg_mod.SurfaceFluid(fake, V, F, theta=2.5)
    assert e.value.code == INVALID
    with pytest.raises(TypeError):
        smg_mod.SurfaceFluid(fake, V, F, beta=1.0)


# ---- the host twin against the restatement ---------------------------------------------------------------------------------------------------------
def host_run(smg):
    def run(op, V, F, **kw):
        rc, out = N.host(smg, op, V, F, **kw)
        assert rc == 0
        return out
    return run


@pytest.mark.parametrize("theta", [0.0, 0.3, 1.0])
@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("name", MESHES)
def test_host_twin_against_restatement(smg_mod, name, k, theta):
    """all five ops, both forms of the transport and the three (a, b) pairs, bit for bit"""
    N.check_launchers(host_run(smg_mod), name, k, theta)


# ---- the restatement itself: the identities of the header ------------------------------------------------------------------------------------------
def degree(F, nV):
    return int(np.bincount(np.asarray(F).reshape(-1), minlength=nV).max())


def segment_terms(F, psi, w, theta):
    """(t_ij, t_ik, Phi_ij, Phi_ik), 3 nF x k each, and the three vertices of every corner"""
    F = np.asarray(F)
    vi, vj, vk = F.reshape(-1), F[:, [1, 2, 0]].reshape(-1), F[:, [2, 0, 1]].reshape(-1)
    fij, fik = N.fluxes(F, psi)
    tij = (0.5 * (fij - theta * np.abs(fij))) * (w[vj] - w[vi])
    tik = (0.5 * (fik - theta * np.abs(fik))) * (w[vk] - w[vi])
    return tij, tik, fij, fik, (vi, vj, vk)


@pytest.mark.parametrize("name", MESHES)
def test_geometric_flux_is_the_psi_difference(name):
    """FLUX of the header, on both segments of every corner"""
    V, F = N.shape(name)
    psi = N.test_state(V, F, 1)[0]
    W, nrm, _ = rest_faces(V, F)
    U = N.velocity(V, F, psi)[0][0]                                           # nF x 3
    fij, fik = N.fluxes(F, psi)
    P = V[F]                                                                  # nF x 3 x 3
    cen = (P[:, 0] + P[:, 1] + P[:, 2]) / 3.0
    pabs = np.abs(psi[F[:, 0], 0]) + np.abs(psi[F[:, 1], 0]) + np.abs(psi[F[:, 2], 0])
    wabs = sum(np.sqrt(dot3(W[:, i], W[:, i])) for i in range(3))
    A = rest_faces(V, F)[2]
    emax = np.max(np.stack([np.linalg.norm(P[:, (i + 1) % 3] - P[:, i], axis=1) for i in range(3)]), axis=0)
    kappa = np.maximum(1.0, np.max(np.linalg.norm(P, axis=2), axis=1) / (2.0 * A / emax))
    worst = 0.0
    for i in range(3):
        mij, mik = 0.5 * (P[:, i] + P[:, (i + 1) % 3]), 0.5 * (P[:, i] + P[:, (i + 2) % 3])
        for a, b, phi in ((mij, cen, fij[i::3, 0]), (cen, mik, fik[i::3, 0])):
            geo = dot3(U, cross3(b - a, nrm))
            bound = 16 * EPS * kappa * pabs * wabs * np.sqrt(dot3(b - a, b - a))
            assert np.all(np.abs(geo - phi) <= bound)
            worst = max(worst, float(np.max(np.abs(geo - phi)[bound > 0.0] / bound[bound > 0.0])))
    print("%s: largest |geometric flux - Phi| over its bound %.3f" % (name, worst))
    assert 0.0 < worst <= 1.0


@pytest.mark.parametrize("name", MESHES)
def test_fluxes_sum_to_zero_at_every_vertex(name):
    """DIVERGENCE of the header"""
    V, F = N.shape(name)
    n = V.shape[0]
    psi = N.test_state(V, F, 2)[0]
    fij, fik = N.fluxes(F, psi)
    vi, vj, vk = F.reshape(-1), F[:, [1, 2, 0]].reshape(-1), F[:, [2, 0, 1]].reshape(-1)
    div, scale = np.zeros(psi.shape), np.zeros(psi.shape)
    np.add.at(div, vi, fij + fik)
    np.add.at(scale, vi, 2.0 * (np.abs(psi[vi]) + np.abs(psi[vj]) + np.abs(psi[vk])))
    G = 2 * degree(F, n) + 32
    ratio = np.abs(div) / (G * EPS * scale + 1e-300)
    print("%s: largest |sum of a vertex's fluxes| over its bound %.3f" % (name, ratio.max()))
    assert np.all(np.abs(div) <= G * EPS * scale)


@pytest.mark.parametrize("theta", [0.0, 0.3, 1.0])
@pytest.mark.parametrize("name", MESHES)
def test_a_stage_keeps_the_circulation(name, theta):
    """CIRCULATION of the header, for each of the three (a, b) pairs"""
    V, F = N.shape(name)
    n, k = V.shape[0], 2
    psi, w, wn, dt = N.test_state(V, F, k)
    m, _ = N.mass(V, F)
    tij, tik, _, _, (vi, _, _) = segment_terms(F, psi, w, theta)
    tabs = np.zeros(w.shape)
    np.add.at(tabs, vi, np.abs(tij) + np.abs(tik))
    G = 2 * degree(F, n) + 32
    sm = lambda x: np.array([N.fixed_sum(t) for t in (m[:, None] * x).T])   # noqa: E731
    for a, b in N.PAIRS[3]:
        out = N.advect(V, F, psi, w, wn, a, b, dt, theta)[0]
        diff = sm(out) - (a * sm(wn) + b * sm(w))
        bound = G * EPS * (a * sm(np.abs(wn)) + b * sm(np.abs(w)) + b * dt * tabs.sum(axis=0))
        print("%s theta %.1f (a, b) = (%.3f, %.3f): |circulation change| over its bound %s" % (name, theta, a, b, np.abs(diff) / bound))
        assert np.all(np.abs(diff) <= bound)


@pytest.mark.parametrize("name", MESHES)
def test_the_central_flux_keeps_the_enstrophy_rate_at_zero(name):
    """ENSTROPHY of the header"""
    V, F = N.shape(name)
    n, k = V.shape[0], 2
    psi, w, wn, dt = N.test_state(V, F, k)
    m, _ = N.mass(V, F)
    out = N.advect(V, F, psi, w, w, 0.0, 1.0, np.ones(k), 0.0)[0]             # dt = 1: out - w = adv
    adv = out - w
    tij, tik, _, _, (vi, _, _) = segment_terms(F, psi, w, 0.0)
    tabs = np.zeros(w.shape)
    np.add.at(tabs, vi, np.abs(tij) + np.abs(tik))
    rate = np.sum(m[:, None] * w * adv, axis=0)
    G = 2 * degree(F, n) + 32
    bound = G * EPS * np.sum(np.abs(w) * (tabs + m[:, None] * np.abs(w)), axis=0)   # out - w itself is rounded at the size of w
    print("%s: |sum m w adv| %s over its bound %s" % (name, np.abs(rate), np.abs(rate) / bound))
    assert np.all(np.abs(rate) <= bound)


def ring_min_max(F, w):
    n = w.shape[0]
    lo, hi = w.copy(), w.copy()
    for a, b in ((0, 1), (1, 2), (2, 0), (1, 0), (2, 1), (0, 2)):
        np.minimum.at(lo, F[:, a], w[F[:, b]])
        np.maximum.at(hi, F[:, a], w[F[:, b]])
    assert lo.shape[0] == n
    return lo, hi


@pytest.mark.parametrize("name", ["icosphere3", "torus", "square"])
def test_upwind_obeys_the_maximum_principle(name):
    """MAXIMUM of the header: one stage at dt max rate = 1 exactly, and three-stage steps of the whole method at cfl = 0.5 -- there against the
    extremes of the step's start, which bound every stage's ring extremes"""
    V, F = N.shape(name)
    n, k = V.shape[0], 2
    psi, w, _, _ = N.test_state(V, F, k)
    rate, rmax = N.rates(V, F, psi)
    G = 2 * degree(F, n) + 32
    out = N.advect(V, F, psi, w, w, 0.0, 1.0, 1.0 / rmax, 1.0)[0]
    lo, hi = ring_min_max(np.asarray(F), w)
    tol = G * EPS * np.abs(w).max()
    print("%s: one stage at dt rate = 1: out - ring max %.3e, ring min - out %.3e, tolerance %.3e" % (name, (out - hi).max(), (lo - out).max(), tol))
    assert np.all(out <= hi + tol) and np.all(out >= lo - tol)
    assert np.any(out > w) and np.any(out < w)
    sim = N.FluidNp(V, F, theta=1.0, cfl=0.5)
    sim.set_vorticity(w)
    for _ in range(3):
        w0 = sim.w
        cfl, _ = sim.step(1)
        assert np.all(cfl <= 1.0)
        assert np.all(sim.w <= w0.max(axis=0) + 3 * tol) and np.all(sim.w >= w0.min(axis=0) - 3 * tol)


def test_the_viscous_solve_keeps_the_circulation():
    """VISCOUS of the header, on the torus"""
    V, F = N.shape("torus")
    n = V.shape[0]
    w = N.test_state(V, F, 2)[1]
    nu, dt = 0.05, 0.02
    sim = N.FluidNp(V, F, viscosity=nu, dt=dt)
    sim.set_vorticity(w)
    sim.step(1)
    ws = sim.w                                                                # one more viscous solve on the new state alone
    S = (sp.diags(sim.m) + (nu * dt) * sim.A).tocsr()
    wnew = sim.lu_v.solve(sim.m[:, None] * ws)
    r = sim.m[:, None] * ws - S @ wnew
    diff = np.sum(sim.m[:, None] * wnew, axis=0) - np.sum(sim.m[:, None] * ws, axis=0)
    G = 2 * degree(F, n) + 32
    bound = np.abs(r).sum(axis=0) + G * EPS * (np.sum(sim.m[:, None] * np.abs(wnew), axis=0) + nu * dt * np.sum(abs(sim.A) @ np.abs(wnew), axis=0))
    print("torus: |circulation change of the viscous solve| %s over its bound %s" % (np.abs(diff), np.abs(diff) / bound))
    assert np.all(np.abs(diff) <= bound)
    assert np.all(np.sum(sim.m[:, None] * wnew * wnew, axis=0) < np.sum(sim.m[:, None] * ws * ws, axis=0))


# ---- the physics of the header ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sphere():
    V, F = N.shape("icosphere3")
    assert np.allclose(np.linalg.norm(V, axis=1), 1.0)
    sim = N.FluidNp(V, F)
    sim.set_vorticity(V[:, 2])
    return sim


def test_stream_function_and_velocity_of_rigid_rotation(sphere):
    """STREAM and VELOCITY of the header"""
    V, F = sphere.V, sphere.F
    psi = sphere.stream()
    mean = np.sum(sphere.m * psi[:, 0]) / sphere.msum
    e_psi = float(np.max(np.abs((psi[:, 0] - mean) + 0.5 * V[:, 2])))
    cen = (V[F[:, 0]] + V[F[:, 1]] + V[F[:, 2]]) / 3.0
    exact = 0.5 * np.cross(np.array([0.0, 0.0, 1.0]), cen)
    e_u = float(np.max(np.linalg.norm(N.velocity(V, F, psi)[0][0] - exact, axis=1)))
    print("icosphere3, w = z: max |psi - mean + z / 2| = %.3e, max |u - (1/2) z^ x c| = %.3e" % (e_psi, e_u))
    assert e_psi <= 1.5e-3 and e_u <= 1.3e-2


def test_rigid_rotation_is_steady(sphere):
    """STEADY of the header"""
    V = sphere.V
    sphere.set_vorticity(V[:, 2])
    d0 = sphere.diagnostics()
    cfl, time = sphere.step(50)
    drift = float(np.max(np.abs(sphere.w[:, 0] - V[:, 2])))
    d1 = sphere.diagnostics()
    print("icosphere3, w = z: drift after 50 default steps %.3e (time %.3f, cfl %.3f .. %.3f); energy %.6f -> %.6f, enstrophy %.6f -> %.6f, circulation %.3e -> %.3e"
          % (drift, time[-1, 0], cfl.min(), cfl.max(), d0["energy"][0], d1["energy"][0], d0["enstrophy"][0], d1["enstrophy"][0], d0["circulation"][0],
             d1["circulation"][0]))
    assert drift <= 0.01 * np.abs(V[:, 2]).max()
    assert np.all(cfl >= 0.5 * (1.0 - 4 * EPS))                               # the first stage's own rate gives 0.5 up to rounding


# ---- the kernels' registers, the host maths under sanitizers -------------------------------------------------------------------------------------
def test_kernels_keep_everything_in_registers():
    """the ISA notes of every kernel of smg_fluid_device.hip (the build's flags, device side only): no scratch, no spills"""
    import re
    from surface_multigrid_code_amd import build as B
    src = os.path.join(B.CSRC, "smg_fluid_device.hip")
    asm = subprocess.check_output([B._hipcc()] + B.FLAGS + ["--cuda-device-only", "-S", src, "-o", "-"], text=True, stderr=subprocess.DEVNULL)
    notes = re.findall(r"\.name:\s+(\S*k_fluid\S*)(.*?)\.wavefront_size", asm, flags=re.S)
    assert len(notes) == 7
    for kernel, body in notes:
        field = lambda k: int(re.search(r"\.%s:\s+(\d+)" % k, body).group(1))   # noqa: E731
        print("%s: vgpr_count %d, sgpr_count %d, private_segment_fixed_size %d" % (kernel, field("vgpr_count"), field("sgpr_count"), field("private_segment_fixed_size")))
        assert field("private_segment_fixed_size") == 0 and field("vgpr_spill_count") == 0 and field("sgpr_spill_count") == 0
        assert field("vgpr_count") <= 128


def test_host_maths_under_sanitizers(tmp_path):
    """tests/fluid_asan_driver.cpp, a stand-alone program: the host twin's loops (smg::fluid_host_* of csrc/smg_fluid_inl.hpp, what smg_fluid_host
    runs after its checks) on exactly-sized heap arrays, under AddressSanitizer and UndefinedBehaviorSanitizer (static runtimes: run directly,
    nothing preloaded, nothing loaded into python)"""
    exe = str(tmp_path / "fluid_asan_driver")
    csrc = os.path.join(ROOT, "surface_multigrid_code_amd", "csrc")
    srcs = [os.path.join(ROOT, "tests", "fluid_asan_driver.cpp"), os.path.join(csrc, "smg_mesh.cpp"), os.path.join(csrc, "smg_sparse.cpp")]
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-ffp-contract=off", "-pthread", "-I" + csrc] + srcs + ["-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    run = subprocess.run([exe], env=env, capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0 and run.stdout.count("ok 1") == 5 and "ERROR" not in run.stderr
