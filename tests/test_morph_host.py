"""CPU: gradient-domain morphing (include/smg.h: smg_morph_*) -- the ABI and its refusals without a GPU, the library's host twin
(smg_morph_faces_host) against the numpy restatement (tests/morph_np.py: LAPACK SVDs, direct solves), and the restatement itself against the exact
answers of the method.

The bounds.  Face gradients, stretches from given rotations, right-hand sides from given gradients, pins and starts are correctly rounded +, -, *, /
and sqrt in one order on both sides: held bit for bit.  A rotation is a one-sided Jacobi fit on one side and a LAPACK SVD on the other: held to the
polar factor's perturbation bound ROT_BOUND eps / gap as tests/test_gpu_arap.py does, gap = (sigma_2 + sigma_3) / sigma_1; on the cases of
morph_np.CASES the restatement alone shows gap >= 0.889 and theta <= 2.561 on every face (asserted: >= 1e-3, <= pi - 0.1), so no face is left out;
measured max err * gap / eps = 69.8 (bunny.smgm, twist).

OMEGA_BOUND.  The rotation vector against scipy's Rotation.from_matrix(R_np).as_rotvec().  Measured on the CPU: the numpy restatement of the
kernel's formula (Shepperd's branch, 2 atan2(|v|, w)) applied to R_np is within 6.66e-16 of scipy on these cases (every case but icosphere(3),
3.33e-16); the bound is 16 x that, 1.066e-14.  The host twin, whose rotations are the Jacobi fit's, measured 5.77e-15 against scipy (bunny.smgm).

INTERP_C.  k_morph_rhs<true> against the restatement evaluated in numpy.longdouble from the same omega and S: each entry within
INTERP_C eps sum_corners A_f |S_f(t)|_F |W_fj|.  The ROCm documentation installed with the compiler states no error bound for the device's sin
and cos (no mention of one under share/doc or in the HIP headers), so by the issue's rule the constant is 8 x the measured distance of the float64
restatement from the longdouble one on these cases and the times of morph_np.TIMES: measured 0.822 (torus, stretch), INTERP_C = 6.58.  For scale, a
count of the roundings of one corner's term: 3 for t omega, 6 for |t omega| and 3 for the axis; sin and cos; 1 for 1 - cos; at most 5 per entry
of R; 3 per entry of S(t); 5 per entry of R S(t); 5 for J w; 1 for the area and 1 for the accumulation: about 35 per corner, most of them on
quantities well below the scale, which is why the measured constant is below 1."""
import ctypes as C
import json
import math
import os
import re
import subprocess

import numpy as np
import pytest
from scipy.spatial.transform import Rotation

import morph_np as N
from test_arap_host import _fake_hierarchy, bbox_diag, rotation_matrix
from test_geodesics_host import flat_square

INVALID, NO_DEVICE = -1, -2
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "morph_refusals.json")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = N.EPS
ROT_BOUND = 256                     # |R - R_np|_F <= ROT_BOUND eps / gap (tests/test_gpu_arap.py)
GAP_MIN, THETA_MAX = 1e-3, math.pi - 0.1
OMEGA_BOUND = 16 * 6.66e-16         # see the header
INTERP_C = 8 * 0.822                # see the header
EXACT_BOUND = 1e-11                 # the restatement's direct solves against the exact answers, in bounding-box diagonals (measured <= 3e-13)

MORPH_SYMBOLS = ("smg_morph_create", "smg_morph_destroy", "smg_morph_set_solver", "smg_morph_device_bytes", "smg_morph_reconstruct",
                 "smg_morph_interpolate", "smg_morph_transfer", "smg_morph_faces_host", "smg_debug_morph")


# ---- the ABI and its refusals --------------------------------------------------------------------------------------------------------------------
def test_abi_present(smg_mod):
    L = smg_mod._lib.load()
    for name in MORPH_SYMBOLS:
        assert hasattr(L, name)
    assert hasattr(smg_mod, "Morpher")
    assert L.smg_version() >= 514
    assert L.smg_morph_device_bytes(None) == 0


def _create(smg, h, V, F, pins=(0,), nV=None, n_pins=None, null=None):
    """smg_morph_create -> (code, message); a successful create is destroyed at once"""
    L = smg._lib.load()
    ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
    V, F = np.ascontiguousarray(V, dtype=np.float64), np.ascontiguousarray(F, dtype=np.int32)
    pins = np.ascontiguousarray(pins, dtype=np.int32)
    out = C.c_void_p(0xdead)
    rc = L.smg_morph_create(None if null == "h" else h, None if null == "V" else V.ctypes.data_as(dp), V.shape[0] if nV is None else nV,
                            None if null == "F" else F.ctypes.data_as(ip), F.shape[0], None if null == "pins" else pins.ctypes.data_as(ip),
                            pins.shape[0] if n_pins is None else n_pins, None if null == "out" else C.byref(out))
    if rc == 0:
        L.smg_morph_destroy(out)
        return rc, ""
    assert null == "out" or out.value is None, "a refused create must leave *out == NULL"
    return rc, L.smg_last_error().decode()


def create_cases(smg):
    """[(name, thunk -> (code, message), holds only without a device)]: the base's checks in its order, then the pins"""
    V, F = flat_square(8)
    n = V.shape[0]
    keep = {"mg": smg.mg_precompute(V, F, 0.25, 20, 1), "blk": smg.mg_precompute_block(V, F, 0.25, 20, 1)}
    keep["un"] = smg.Hierarchy.union([keep["mg"], keep["mg"]])
    mg, fake = keep["mg"], _fake_hierarchy(smg, n)
    V2, F2 = np.concatenate([V, V + 3.0]), np.concatenate([F, F + n])
    cases = [("null %s" % a, (lambda a=a: _create(smg, mg.h, V, F, null=a)), False) for a in ("h", "V", "F", "pins", "out")]
    cases.append(("block hierarchy", lambda: _create(smg, keep["blk"].h, V, F), False))
    cases.append(("union", lambda: _create(smg, keep["un"].h, V2, F2), False))
    cases.append(("rows", lambda: _create(smg, mg.h, V[:-1], F, nV=n - 1), False))
    Fo = F.copy()
    Fo[3, 2] = n
    cases.append(("face index", lambda: _create(smg, fake.h, V, Fo), False))
    Vz = V.copy()
    Vz[F[0, 1]] = Vz[F[0, 0]]
    cases.append(("zero area", lambda: _create(smg, fake.h, Vz, F), False))
    for tag, bad in (("nan", np.nan), ("inf", np.inf)):
        Vn = V.copy()
        Vn[F[F.shape[0] - 1, 0], 1] = bad
        cases.append(("%s coordinate" % tag, lambda Vn=Vn: _create(smg, fake.h, Vn, F), False))
    keep["two"] = _fake_hierarchy(smg, 2 * n)
    cases.append(("two components", lambda: _create(smg, keep["two"].h, V2, F2), False))
    cases.append(("no pin", lambda: _create(smg, fake.h, V, F, n_pins=0), False))
    cases.append(("pin past the end", lambda: _create(smg, fake.h, V, F, pins=[0, n]), False))
    cases.append(("pin negative", lambda: _create(smg, fake.h, V, F, pins=[-1, 3]), False))
    cases.append(("pin repeated", lambda: _create(smg, fake.h, V, F, pins=[4, 7, 4]), False))
    cases.append(("all pinned", lambda: _create(smg, fake.h, V, F, pins=np.arange(n)), False))
    cases.append(("order: mesh before pins", lambda: _create(smg, fake.h, Vz, F, pins=[n]), False))
    cases.append(("order: hierarchy before mesh", lambda: _create(smg, keep["blk"].h, Vz, F), False))
    cases.append(("valid, real hierarchy", lambda: _create(smg, mg.h, V, F), True))
    cases.append(("valid, fake hierarchy, two pins", lambda: _create(smg, fake.h, V, F, pins=[n - 1, 2]), True))
    return cases, keep


def null_object_cases(smg):
    """every entry point that takes the object, called without one"""
    L = smg._lib.load()
    X, t = np.zeros(12), np.zeros(1)
    dp = C.POINTER(C.c_double)
    calls = {"set_solver": lambda: L.smg_morph_set_solver(None, 1),
             "reconstruct": lambda: L.smg_morph_reconstruct(None, X.ctypes.data, 1, None, 0, None, 0, 0, None, X.ctypes.data, 4, None),
             "interpolate": lambda: L.smg_morph_interpolate(None, X.ctypes.data, t.ctypes.data_as(dp), 1, None, 0, None, 0, 0, None, X.ctypes.data, 4, None),
             "transfer": lambda: L.smg_morph_transfer(None, X.ctypes.data, 4, None, X.ctypes.data, 1, None, 0, None, 0, 0, None, X.ctypes.data, 4, None)}
    return [("null object: " + k, (lambda f=f: (f(), L.smg_last_error().decode())), False) for k, f in calls.items()]


def host_twin_cases(smg, call=None, prefix="host twin"):
    """the operand checks smg_morph_faces_host and smg_debug_morph share"""
    call = call or (lambda *a, **k: N.faces_host(smg, *a, **k)[0])
    L = smg._lib.load()
    V, F = N.shape("icosphere1")
    nF = F.shape[0]
    X = np.ascontiguousarray(V * 1.5)
    Fo = np.array(F)
    Fo[1, 2] = V.shape[0]
    J, fac, pins = np.zeros(9 * nF), np.zeros(9 * nF), [0, 3]
    thunks = {
        "unknown op": lambda: call(5, V, F, X=X), "negative op": lambda: call(-1, V, F, X=X),
        "out missing": lambda: call(N.MORPH_FACE_GRADIENT, V, F, X=X, over=dict(out=None)),
        "V0 missing": lambda: call(N.MORPH_FACE_GRADIENT, V, F, X=X, over=dict(V0=None)),
        "X missing": lambda: call(N.MORPH_FACE_POLAR, V, F),
        "gradients missing": lambda: call(N.MORPH_RHS_GRADIENT, V, F),
        "t missing": lambda: call(N.MORPH_RHS_INTERP, V, F, inp=fac),
        "t missing with a pose": lambda: call(N.MORPH_PINS, V, F, X=X, pins=pins),
        "pins missing": lambda: call(N.MORPH_PINS, V, F),
        "k zero": lambda: call(N.MORPH_RHS_GRADIENT, V, F, k=0, inp=J),
        "t nan": lambda: call(N.MORPH_RHS_INTERP, V, F, k=2, t=[0.5, np.nan], inp=fac),
        "t inf": lambda: call(N.MORPH_PINS, V, F, k=1, X=X, t=[np.inf], pins=pins),
        "face index": lambda: call(N.MORPH_FACE_GRADIENT, V, Fo, X=X),
        "pin out of range": lambda: call(N.MORPH_PINS, V, F, pins=[0, V.shape[0]]),
        "pin negative": lambda: call(N.MORPH_PINS, V, F, pins=[-1]),
        "order: operands before k": lambda: call(N.MORPH_RHS_GRADIENT, V, F, k=0),
        "order: t before faces": lambda: call(N.MORPH_RHS_INTERP, V, Fo, k=1, t=[np.nan], inp=fac),
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
    """every refusal of smg_morph_create, of the calls on a missing object and of the host twin's operand checks, with the code and the
    smg_last_error() text recorded in tests/golden/morph_refusals.json; all of create's come before SMG_ERR_NO_DEVICE, which a valid call meets on
    a box without a GPU.  The refusals that need a live object (group "live") are checked by tests/test_gpu_morph.py.  Every message carries its
    entry point's name."""
    golden = json.load(open(GOLDEN))
    cases, keep = create_cases(smg_mod)
    assert check_cases(smg_mod, cases, golden["create"]) == set(golden["create"]) - (
        set() if smg_mod._lib.load().smg_device_count() == 0 else {c[0] for c in cases if c[2]})
    assert check_cases(smg_mod, null_object_cases(smg_mod), golden["null"]) == set(golden["null"])
    assert check_cases(smg_mod, host_twin_cases(smg_mod), golden["host"]) == set(golden["host"])
    g = golden["create"]
    own = ["no pin", "pin past the end", "pin repeated", "all pinned"]
    assert len({g[k][1] for k in own}) == len(own)                                          # each has its own message
    assert g["order: mesh before pins"] == g["zero area"] and g["order: hierarchy before mesh"] == g["block hierarchy"]
    assert all(v[1].startswith("smg_morph_create: ") for v in g.values())
    h = golden["host"]
    assert h["host twin: order: operands before k"] == h["host twin: gradients missing"]
    assert h["host twin: order: t before faces"][1] == h["host twin: t nan"][1].replace("t[1]", "t[0]")
    assert all(v[1].startswith("smg_morph_faces_host: ") for v in h.values())
    for name, (code, msg) in golden["null"].items():
        assert msg.startswith("smg_morph_" + name.split(": ")[1])
    for name, (code, msg) in golden["live"].items():
        assert code == INVALID and msg.startswith("smg_morph_" + name.split()[0] + ": "), name
    del keep


def test_hook_refuses_what_the_host_twin_refuses(smg_mod):
    golden = json.load(open(GOLDEN))["host"]
    hook = lambda *a, **k: N.hook(smg_mod, *a, **k)[0]   # noqa: E731
    for name, thunk, _ in host_twin_cases(smg_mod, hook, "hook"):
        rc, msg = thunk()
        want = golden[name.replace("hook: ", "host twin: ")]
        assert [rc, msg] == [want[0], want[1].replace("smg_morph_faces_host", "smg_debug_morph")], name
    if smg_mod._lib.load().smg_device_count() == 0:
        V, F = N.shape("icosphere1")
        assert N.hook(smg_mod, N.MORPH_FACE_POLAR, V, F, X=np.ascontiguousarray(V * 1.5))[0] == NO_DEVICE


# ---- the kernels' arithmetic, one launcher at a time: shared with tests/test_gpu_morph.py --------------------------------------------------------
def check_launchers(run, name, kind, k, device):
    """run(op, V0, F, **operands) -> out.  Returns the figures it printed: (rotation err * gap / eps, omega against scipy, interp constant)"""
    V, F = N.shape(name)
    X = N.pose(name, kind)
    n, nF = V.shape[0], F.shape[0]
    ts = np.array(N.TIMES[:k])
    # poses of the k sets: the pose itself and blends of it with the rest pose
    Xs = np.stack([N.blend(V, X, 1.0 - 0.2 * c) for c in range(k)])
    Jn = np.stack([N.gradient(V, F, Xc) for Xc in Xs])
    J = N.unpack(N.MORPH_FACE_GRADIENT, run(N.MORPH_FACE_GRADIENT, V, F, k=k, X=Xs), n, nF, k)
    assert np.array_equal(J, Jn)
    B, bsq = N.unpack(N.MORPH_RHS_GRADIENT, run(N.MORPH_RHS_GRADIENT, V, F, k=k, inp=J), n, nF, k)
    Bn, bsqn = N.rhs(V, F, Jn)
    assert np.array_equal(B, Bn) and np.array_equal(bsq, bsqn)
    pins = np.array([n - 1, 0, n // 2], dtype=np.int32)
    for pose_, t_ in ((X, ts), (None, None)):
        hp, U = N.unpack(N.MORPH_PINS, run(N.MORPH_PINS, V, F, k=k, X=pose_, t=t_, pins=pins), n, nF, k, pins.size)
        hpn, Un = N.pins_and_start(V, pose_, t_, pins, k)
        assert np.array_equal(hp, hpn) and np.array_equal(U, Un)
    # the polar factors: on these poses the restatement alone keeps every face
    Rn, Sn, gap, _ = N.polar(Jn[0])
    rotvec = Rotation.from_matrix(Rn).as_rotvec()
    assert gap.min() >= GAP_MIN and np.linalg.norm(rotvec, axis=1).max() <= THETA_MAX
    R, om, S6 = N.unpack(N.MORPH_FACE_POLAR, run(N.MORPH_FACE_POLAR, V, F, X=Xs[0]), n, nF, 1)
    err = np.linalg.norm((R - Rn).reshape(nF, 9), axis=1)
    worst = (err * gap / EPS).max()
    d_om = np.abs(om - rotvec).max()
    print("%s, %s, k = %d: max |R - R_np| gap / eps = %.1f (bound %d), min gap %.3f, max theta %.3f; max |omega - scipy| = %.2e (bound %.2e)"
          % (name, kind, k, worst, ROT_BOUND, gap.min(), np.linalg.norm(rotvec, axis=1).max(), d_om, OMEGA_BOUND))
    assert np.all(err <= ROT_BOUND * EPS / gap)
    assert np.abs(np.einsum("nji,njk->nik", R, R) - np.eye(3)).max() <= 32 * EPS and np.all(np.linalg.det(R) > 0)
    assert np.array_equal(S6, N.stretch_of(R, Jn[0]))                  # S = sym(R^T J) of the library's own R, stored as six entries: symmetric to the bit
    assert np.abs(S6 - N.sym6(Sn)).max() <= 3 * ROT_BOUND * EPS * np.abs(Jn[0]).max() / gap.min()
    assert d_om <= OMEGA_BOUND
    # the interpolated right-hand side from the library's own omega and S, against the restatement in extended precision
    fac = np.concatenate([om.ravel(), S6.ravel()])
    B, bsq = N.unpack(N.MORPH_RHS_INTERP, run(N.MORPH_RHS_INTERP, V, F, k=k, t=ts, inp=fac), n, nF, k)
    ld = [N.interp(om, S6, t, np.longdouble) for t in ts]
    Bld, _ = N.rhs(V, F, np.stack([j for j, _ in ld]))
    scale = np.repeat(N.rhs_scale(V, F, [s for _, s in ld]), 3, axis=1)
    const = float((np.abs(B.astype(np.longdouble) - Bld) / (EPS * scale)).max())
    print("  interpolated right-hand side against longdouble: max error / (eps scale) = %.3f (bound %.2f)" % (const, INTERP_C))
    assert const <= INTERP_C
    assert np.array_equal(bsq, (B[:, 0::3] * B[:, 0::3] + B[:, 1::3] * B[:, 1::3] + B[:, 2::3] * B[:, 2::3]).T)
    if not device:                                                      # the host's libm is numpy's: the float64 restatement to the bit
        assert np.array_equal(B, N.rhs(V, F, np.stack([N.interp(om, S6, t)[0] for t in ts]))[0])
    return worst, d_om, const


def host_run(smg):
    def run(op, V0, F, **kw):
        rc, out = N.faces_host(smg, op, V0, F, **kw)
        assert rc == 0
        return out
    return run


@pytest.mark.parametrize("case,k", list(zip(N.CASES, (1, 2, 5, 1, 2))) + [(N.CASES[1], 5)])
def test_host_twin_against_restatement(smg_mod, case, k):
    check_launchers(host_run(smg_mod), case[0], case[1], k, device=False)


def test_log_formula_against_scipy():
    """the figure OMEGA_BOUND is built on: the restatement of the kernel's formula on LAPACK's rotations against scipy, every case"""
    worst = 0.0
    for name, kind in N.CASES:
        V, F = N.shape(name)
        Rn = N.polar(N.gradient(V, F, N.pose(name, kind)))[0]
        worst = max(worst, np.abs(N.log_rotation(Rn) - Rotation.from_matrix(Rn).as_rotvec()).max())
    print("max |log_np(R_np) - scipy| = %.3e; OMEGA_BOUND = %.3e" % (worst, OMEGA_BOUND))
    assert worst <= OMEGA_BOUND / 16 * 1.001


def test_log_covers_every_branch():
    """rotations about each axis by angles on both sides of the branch points, and the identity: Shepperd's four branches against scipy"""
    Rs = [np.eye(3)] + [rotation_matrix(ax, a) for ax in ([1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 1], [1, -2, 0.5])
                        for a in (1e-9, 0.3, 1.5, 2.2, 3.0, math.pi - 1e-6)]
    R = np.stack(Rs)
    om = N.log_rotation(R)
    ref = Rotation.from_matrix(R).as_rotvec()
    tr = np.trace(R, axis1=1, axis2=2)
    assert np.any(tr >= R[:, 0, 0]) and np.any(tr < np.max(R[:, [0, 1, 2], [0, 1, 2]], axis=1))     # both kinds of branch are taken
    assert np.array_equal(om[0], np.zeros(3)) and np.abs(om - ref).max() <= 1e-9                  # near pi the logarithm is ill conditioned


# ---- the restatement itself against exact answers ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sphere():
    V, F = N.shape("icosphere3")
    return V, F, N.MorphNp(V, F, pins=[0])


def diag_err(U, want, V):
    return np.abs(U - want).max() / bbox_diag(V)


def test_reconstruct_returns_the_pose(sphere):
    V, F, m = sphere
    X = N.pose("icosphere3", "twist")
    U, _ = m.reconstruct(N.gradient(V, F, X)[None], pin_pos=X[[0]][None])
    print("reconstruct: %.2e diagonals" % diag_err(U[0], X, V))
    assert diag_err(U[0], X, V) <= EXACT_BOUND


def test_interpolate_ends(sphere):
    V, F, m = sphere
    X = N.pose("icosphere3", "twist")
    U, _ = m.interpolate(X, [0.0, 1.0])
    print("interpolate: t = 0 %.2e, t = 1 %.2e diagonals" % (diag_err(U[0], V, V), diag_err(U[1], X, V)))
    assert diag_err(U[0], V, V) <= EXACT_BOUND and diag_err(U[1], X, V) <= EXACT_BOUND


def rigid_pose(V, angle, axis=(1.0, 2.0, -0.5), pin=0):
    return (V - V[pin]) @ rotation_matrix(axis, angle).T + V[pin]


def test_interpolate_rigid_and_scale(sphere):
    V, F, m = sphere
    ts = [0.25, 0.5, 1.5]
    U, _ = m.interpolate(rigid_pose(V, 2.4), ts)
    for c, t in enumerate(ts):
        assert diag_err(U[c], rigid_pose(V, 2.4 * t), V) <= EXACT_BOUND
    s = 1.7
    U, _ = m.interpolate(V[0] + s * (V - V[0]), ts)
    for c, t in enumerate(ts):
        assert diag_err(U[c], V[0] + (1.0 + t * (s - 1.0)) * (V - V[0]), V) <= EXACT_BOUND


def affine_source(V, general):
    """(S0, S1, B): the source = the target under x -> A x + a, its pose = the source under x -> B x + b"""
    A = np.array([[1.3, 0.2, -0.1], [0.0, 0.8, 0.3], [0.1, -0.2, 1.1]]) if general else 1.6 * np.eye(3)
    B = rotation_matrix([0.3, -1.0, 0.4], 0.9) @ np.diag([1.4, 0.8, 1.1])
    S0 = V @ A.T + np.array([0.5, -0.25, 2.0])
    return S0, S0 @ B.T + np.array([-1.0, 0.5, 0.25]), B


def test_transfer(sphere):
    V, F, m = sphere
    X = N.pose("icosphere3", "twist")
    same = m.transfer(V, X[None])[0][0]
    one = m.interpolate(X, [1.0], pin_pos=V[[0]][None])[0][0]
    print("transfer of the target itself against interpolate at t = 1: %.2e diagonals" % diag_err(same, one, V))
    assert diag_err(same, one, V) <= EXACT_BOUND
    S0, S1, B = affine_source(V, general=False)
    U = m.transfer(S0, S1[None])[0][0]
    print("transfer from a scaled source: %.2e diagonals from V B^T" % diag_err(U, N.exact_transfer(V, m.pins, B), V))
    assert diag_err(U, N.exact_transfer(V, m.pins, B), V) <= EXACT_BOUND
    S0, S1, B = affine_source(V, general=True)
    U = m.transfer(S0, S1[None])[0][0]
    far = diag_err(U, N.exact_transfer(V, m.pins, B), V)
    print("transfer from a sheared source: %.2e diagonals from V B^T (no closed form: the planes of source and target faces differ)" % far)
    assert np.all(np.isfinite(U)) and 1e-6 < far < 0.5


def test_sets_are_independent(sphere):
    """a k = 3 right-hand side is the three k = 1 right-hand sides, column block by column block"""
    V, F, m = sphere
    X = N.pose("icosphere3", "twist")
    ts = [0.25, 0.5, 1.5]
    _, B = m.interpolate(X, ts)
    for c, t in enumerate(ts):
        assert np.array_equal(B[:, 3 * c:3 * c + 3], m.interpolate(X, [t])[1])


# ---- the kernels' registers, the host maths under sanitizers -------------------------------------------------------------------------------------
def test_kernels_keep_everything_in_registers():
    """the ISA notes of every kernel of smg_morph_device.hip (the build's flags, device side only): no scratch, no spills; the face and the
    interpolating kernels fit 128 VGPRs (92 and 88)"""
    from surface_multigrid_code_amd import build as B
    src = os.path.join(B.CSRC, "smg_morph_device.hip")
    asm = subprocess.check_output([B._hipcc()] + B.FLAGS + ["--cuda-device-only", "-S", src, "-o", "-"], text=True, stderr=subprocess.DEVNULL)
    notes = re.findall(r"\.name:\s+(\S*k_morph\S*)(.*?)\.wavefront_size", asm, flags=re.S)
    assert len(notes) == 8
    for kernel, body in notes:
        field = lambda k: int(re.search(r"\.%s:\s+(\d+)" % k, body).group(1))   # noqa: E731
        print("%s: vgpr_count %d, sgpr_count %d, private_segment_fixed_size %d" % (kernel, field("vgpr_count"), field("sgpr_count"), field("private_segment_fixed_size")))
        assert field("private_segment_fixed_size") == 0 and field("vgpr_spill_count") == 0 and field("sgpr_spill_count") == 0
        assert field("vgpr_count") <= 128


def test_host_maths_under_sanitizers(tmp_path):
    """tests/morph_asan_driver.cpp, a stand-alone program: the host twin's loops (smg::morph_host_*, what smg_morph_faces_host runs after its
    checks) on exactly-sized heap arrays for the 255, 256 and 257 vertex strips and the tetrahedron, k = 1, 2 and 5, under AddressSanitizer and
    UndefinedBehaviorSanitizer (static runtimes: run directly, nothing preloaded, nothing loaded into python)"""
    exe = str(tmp_path / "morph_asan_driver")
    csrc = os.path.join(ROOT, "surface_multigrid_code_amd", "csrc")
    srcs = [os.path.join(ROOT, "tests", "morph_asan_driver.cpp"), os.path.join(csrc, "smg_mesh.cpp"), os.path.join(csrc, "smg_sparse.cpp")]
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-ffp-contract=off", "-pthread", "-I" + csrc] + srcs + ["-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    run = subprocess.run([exe], env=env, capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0 and run.stdout.count("ok 1") == 12 and "ERROR" not in run.stderr
