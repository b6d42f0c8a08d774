"""CPU: cubic and normal-driven stylization (include/smg.h: smg_stylize_*) -- the ABI and its refusals without a GPU, the library's host twin of the
local step (smg_stylize_local_host) against the numpy restatement written from the formulas (tests/stylize_np.py: LAPACK SVDs, direct solves),
and the restatement itself against the figures of the method's prototype.

The bounds.  Normals, areas, and -- for given rotations -- shrinkage, residuals, the rho rule and the energy terms are correctly rounded +, -, *,
/ and sqrt in one order on both sides: the host twin measured 0 against numpy on every shape, and they are held bit for bit.  A rotation is a
one-sided Jacobi fit on one side and a LAPACK SVD on the other: held to the polar factor's perturbation bound ROT_BOUND eps / gap as
tests/test_gpu_arap.py does (measured max err * gap / eps = 60.7, bunny.smgm; the restatement's smallest gap on these inputs is 3.4e-3, so no
vertex is left out), and z, u to the same bound, shrinkage being 1-Lipschitz (measured 42.3).  The rho decision agreed at every vertex of every
shape.  The whole local step, lambda in {0.2, 0.4}, pose V + 0.02 N(0, 1): no iteration count differed on any shape; rotations of the host twin
against the restatement differ by at most 1.55e-14 on icosphere(4) and 8.97e-13 over all shapes (bunny.smgm, lambda = 0.4), so by the
project's rule (100 x the measured maximum, rounded up to a power of ten) LOCAL_BOUND = 1e-10; tests/test_gpu_stylize.py holds the device to
the same numbers."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import stylize_np as N
from test_arap_host import _fake_hierarchy, rotation_matrix, rotations_np
from test_geodesics_host import flat_square

INVALID, NO_DEVICE = -1, -2
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stylize_refusals.json")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = N.EPS
ROT_BOUND = 256          # |R - R_np|_F <= ROT_BOUND eps / gap (tests/test_gpu_arap.py)
GAP_MIN = 1e-3           # vertices with a smaller gap may be left out, at most 1 % of a mesh
TIE = 1e-9               # the rho decision may be left out where r and mu s, or s and mu r, agree to this relative distance; at most 1 %
LOCAL_BOUND = 1e-10      # rotations after the whole local step, vertices with equal iteration counts (at most 1 % may differ)

STY_SYMBOLS = ("smg_stylize_params_default", "smg_stylize_create", "smg_stylize_destroy", "smg_stylize_device_bytes", "smg_stylize_set_solver",
               "smg_stylize_set_params", "smg_stylize_set_lambda", "smg_stylize_set_frame", "smg_stylize_set_targets", "smg_stylize_normals",
               "smg_stylize_run", "smg_stylize_admm_stats", "smg_stylize_local_host", "smg_debug_stylize")


# ---- the ABI and its refusals --------------------------------------------------------------------------------------------------------------------
def test_abi_present(smg_mod):
    L = smg_mod._lib.load()
    for name in STY_SYMBOLS:
        assert hasattr(L, name)
    assert hasattr(smg_mod, "Stylizer") and hasattr(smg_mod, "stylize_params")
    assert L.smg_version() >= 513
    p = smg_mod.stylize_params()
    assert (p.lambda_, p.rho0, p.abs_tol, p.rel_tol, p.mu, p.tau, p.admm_iters) == (0.2, 1e-4, 1e-5, 1e-3, 10.0, 2.0, 100)
    assert L.smg_stylize_device_bytes(None) == 0


def _create(smg, h, V, F, pins=(0,), nV=None, n_pins=None, null=None, **par):
    """smg_stylize_create -> (code, message); a successful create is destroyed at once"""
    L = smg._lib.load()
    ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
    V, F = np.ascontiguousarray(V, dtype=np.float64), np.ascontiguousarray(F, dtype=np.int32)
    pins = np.ascontiguousarray(pins, dtype=np.int32)
    p = N.params_c(smg, **par)
    out = C.c_void_p(0xdead)
    rc = L.smg_stylize_create(None if null == "h" else h, None if null == "V" else V.ctypes.data_as(dp), V.shape[0] if nV is None else nV,
                              None if null == "F" else F.ctypes.data_as(ip), F.shape[0], None if null == "pins" else pins.ctypes.data_as(ip),
                              pins.shape[0] if n_pins is None else n_pins, None if null == "p" else C.byref(p), None if null == "out" else C.byref(out))
    if rc == 0:
        L.smg_stylize_destroy(out)
        return rc, ""
    assert null == "out" or out.value is None, "a refused create must leave *out == NULL"
    return rc, L.smg_last_error().decode()


PARAM_CASES = [("lambda_", ("negative", -0.1), ("nan", np.nan), ("inf", np.inf)),
               ("rho0", ("zero", 0.0), ("negative", -1.0), ("nan", np.nan), ("inf", np.inf)),
               ("abs_tol", ("zero", 0.0), ("negative", -1.0), ("nan", np.nan), ("inf", np.inf)),
               ("rel_tol", ("zero", 0.0), ("negative", -1.0), ("nan", np.nan), ("inf", np.inf)),
               ("mu", ("one", 1.0), ("nan", np.nan), ("inf", np.inf)),
               ("tau", ("one", 1.0), ("nan", np.nan), ("inf", np.inf)),
               ("admm_iters", ("zero", 0))]


def create_cases(smg):
    """[(name, thunk -> (code, message), holds only without a device)]: the base's checks in its order, then the pins, then the parameters"""
    V, F = flat_square(8)
    n = V.shape[0]
    keep = {"mg": smg.mg_precompute(V, F, 0.25, 20, 1), "blk": smg.mg_precompute_block(V, F, 0.25, 20, 1)}
    keep["un"] = smg.Hierarchy.union([keep["mg"], keep["mg"]])
    mg, fake = keep["mg"], _fake_hierarchy(smg, n)
    V2, F2 = np.concatenate([V, V + 3.0]), np.concatenate([F, F + n])
    cases = [("null %s" % a, (lambda a=a: _create(smg, mg.h, V, F, null=a)), False) for a in ("h", "V", "F", "pins", "p", "out")]
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
    for field, *bads in PARAM_CASES:
        for tag, bad in bads:
            cases.append(("%s %s" % (field, tag), lambda field=field, bad=bad: _create(smg, fake.h, V, F, **{field: bad}), False))
    cases.append(("order: mesh before pins", lambda: _create(smg, fake.h, Vz, F, pins=[n]), False))
    cases.append(("order: pins before params", lambda: _create(smg, fake.h, V, F, pins=[n], lambda_=-0.1), False))
    fields = [c[0] for c in PARAM_CASES]
    for a, b in zip(fields[:-1], fields[1:]):
        bad = {c[0]: c[1][1] for c in PARAM_CASES}
        cases.append(("order: %s before %s" % (a, b), lambda a=a, b=b: _create(smg, fake.h, V, F, **{a: bad[a], b: bad[b]}), False))
    cases.append(("valid, real hierarchy", lambda: _create(smg, mg.h, V, F), True))
    cases.append(("valid, fake hierarchy, two pins, lambda zero", lambda: _create(smg, fake.h, V, F, pins=[n - 1, 2], lambda_=0.0), True))
    return cases, keep


def null_object_cases(smg):
    """every entry point that takes the object, called without one"""
    L = smg._lib.load()
    X = np.zeros(12)
    p = N.params_c(smg)
    calls = {"set_solver": lambda: L.smg_stylize_set_solver(None, 1), "set_params": lambda: L.smg_stylize_set_params(None, C.byref(p)),
             "set_lambda": lambda: L.smg_stylize_set_lambda(None, None), "set_frame": lambda: L.smg_stylize_set_frame(None, None),
             "set_targets": lambda: L.smg_stylize_set_targets(None, None), "normals": lambda: L.smg_stylize_normals(None, None, None),
             "run": lambda: L.smg_stylize_run(None, None, 1, None, 0, 0, 1, 0.0, None, X.ctypes.data, 4, None, None, None),
             "admm_stats": lambda: L.smg_stylize_admm_stats(None, None, None, None, None, None)}
    return [("null object: " + k, (lambda f=f: (f(), L.smg_last_error().decode())), False) for k, f in calls.items()]


def host_twin_cases(smg, call=None, prefix="host twin"):
    """the operand checks smg_stylize_local_host and smg_debug_stylize share (the setters run the same value checks)"""
    call = call or (lambda *a, **k: N.local_host(smg, *a, **k)[0])
    L = smg._lib.load()
    V, F = N.shape("tetrahedron")
    A = N.rest("tetrahedron")
    n = A.n
    P, R = np.ascontiguousarray(V * 1.5), np.tile(np.eye(3).ravel(), n)
    t = np.tile([0.0, 0.0, 1.0], (n, 1))
    mirror = np.diag([1.0, 1.0, -1.0])
    skew = np.eye(3) + 1e-6 * np.arange(9).reshape(3, 3)
    bad_t, nan_t = t.copy(), t.copy()
    bad_t[2] = [0.0, 0.6, 0.9]
    nan_t[1, 0] = np.nan
    Fo = np.array(F)
    Fo[1, 2] = n
    cb, pb = A.col.copy(), A.rowptr.copy()
    cb[3] = n
    pb[0] = 1
    ip = C.POINTER(C.c_int)
    thunks = {
        "unknown op": lambda: call(5, A, F, P), "negative op": lambda: call(-1, A, F, P),
        "out missing": lambda: call(N.STY_NORMALS, A, F, over=dict(out=None)),
        "P missing": lambda: call(N.STY_LOCAL, A, F, None),
        "iters missing": lambda: call(N.STY_LOCAL, A, F, P, over=dict(iters=None)),
        "targets missing": lambda: call(N.STY_LOCAL_TARGETS, A, F, P),
        "R_in missing": lambda: call(N.STY_ENERGY, A, F, P),
        "bad params": lambda: call(N.STY_LOCAL, A, F, P, tau=1.0),
        "face index": lambda: call(N.STY_NORMALS, A, Fo),
        "rowptr[0]": lambda: call(N.STY_LOCAL, A, F, P, over=dict(rowptr=pb.ctypes.data_as(ip))),
        "column out of range": lambda: call(N.STY_LOCAL, A, F, P, over=dict(col=cb.ctypes.data_as(ip))),
        "lambda negative": lambda: call(N.STY_LOCAL, A, F, P, lam=np.array([0.1, 0.1, -0.1, 0.1])),
        "lambda nan": lambda: call(N.STY_LOCAL, A, F, P, lam=np.array([0.1, np.nan, 0.1, 0.1])),
        "frame not orthonormal": lambda: call(N.STY_LOCAL, A, F, P, Q=skew),
        "frame nan": lambda: call(N.STY_LOCAL, A, F, P, Q=np.full((3, 3), np.nan)),
        "frame reflection": lambda: call(N.STY_LOCAL, A, F, P, Q=mirror),
        "target not unit": lambda: call(N.STY_LOCAL_TARGETS, A, F, P, targets=bad_t),
        "target nan": lambda: call(N.STY_LOCAL_TARGETS, A, F, P, targets=nan_t),
        "order: params before faces": lambda: call(N.STY_LOCAL, A, Fo, P, tau=1.0),
        "order: CSR before lambda": lambda: call(N.STY_LOCAL, A, F, P, lam=np.full(n, -1.0), over=dict(col=cb.ctypes.data_as(ip))),
    }
    del R
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
    """every refusal of smg_stylize_create, of the calls on a missing object and of the host twin's operand checks, with the code and the
    smg_last_error() text recorded in tests/golden/stylize_refusals.json; all of create's come before SMG_ERR_NO_DEVICE, which a valid call
    meets on a box without a GPU.  The refusals that need a live object (group "live") are checked by tests/test_gpu_stylize.py."""
    golden = json.load(open(GOLDEN))
    cases, keep = create_cases(smg_mod)
    assert check_cases(smg_mod, cases, golden["create"]) == set(golden["create"]) - (
        set() if smg_mod._lib.load().smg_device_count() == 0 else {c[0] for c in cases if c[2]})
    assert check_cases(smg_mod, null_object_cases(smg_mod), golden["null"]) == set(golden["null"])
    assert check_cases(smg_mod, host_twin_cases(smg_mod), golden["host"]) == set(golden["host"])
    g = golden["create"]
    own = ["%s %s" % (c[0], c[1][0]) for c in PARAM_CASES] + ["no pin", "pin past the end", "pin repeated", "all pinned"]
    assert len({g[k][1] for k in own}) == len(own)                                          # each has its own message
    assert g["order: mesh before pins"] == g["zero area"] and g["order: pins before params"] == g["pin past the end"]
    fields = [c[0] for c in PARAM_CASES]
    for a, b in zip(fields[:-1], fields[1:]):
        first = {c[0]: c[1][0] for c in PARAM_CASES}[a]
        assert g["order: %s before %s" % (a, b)] == g["%s %s" % (a, first)]
    h = golden["host"]
    assert h["host twin: order: params before faces"] == h["host twin: bad params"]
    assert h["host twin: order: CSR before lambda"] == h["host twin: column out of range"]
    # the setters word their refusals as the host twin does, under their own names
    live = golden["live"]
    for setter, twin in (("set_lambda negative", "lambda negative"), ("set_frame reflection", "frame reflection"), ("set_targets not unit", "target not unit")):
        name = "smg_stylize_" + setter.split()[0]
        assert live[setter] == [INVALID, h["host twin: " + twin][1].replace("smg_stylize_local_host", name)]
    del keep


def test_hook_refuses_what_the_host_twin_refuses(smg_mod):
    golden = json.load(open(GOLDEN))["host"]
    hook = lambda *a, **k: N.hook(smg_mod, *a, **k)[0]   # noqa: E731
    for name, thunk, _ in host_twin_cases(smg_mod, hook, "hook"):
        rc, msg = thunk()
        want = golden[name.replace("hook: ", "host twin: ")]
        assert [rc, msg] == [want[0], want[1].replace("smg_stylize_local_host", "smg_debug_stylize")], name
    if smg_mod._lib.load().smg_device_count() == 0:
        A, (V, F) = N.rest("tetrahedron"), N.shape("tetrahedron")
        assert N.hook(smg_mod, N.STY_NORMALS, A, F)[0] == NO_DEVICE
        assert N.hook(smg_mod, N.STY_LOCAL, A, F, np.ascontiguousarray(V * 1.5))[0] == NO_DEVICE


# ---- the host twin against the restatement -----------------------------------------------------------------------------------------------------
def check_fit(label, R, Rn, gap, z=None, zn=None, u=None, un=None):
    """rotations (and with them z, u: shrinkage is 1-Lipschitz) to the polar factor's perturbation bound; returns the measured err * gap / eps"""
    n = R.shape[0]
    keep = gap >= GAP_MIN
    assert np.all(np.isfinite(R)) and n - keep.sum() <= 0.01 * n
    err = np.linalg.norm((R - Rn).reshape(n, 9), axis=1)
    worst = (err * gap / EPS)[keep].max()
    assert np.all(err[keep] <= ROT_BOUND * EPS / gap[keep])
    assert np.abs(np.einsum("nji,njk->nik", R, R) - np.eye(3)).max() <= 32 * EPS and np.all(np.linalg.det(R) > 0)
    for a, b in ((z, zn), (u, un)):
        if a is not None:
            e = np.linalg.norm(a - b, axis=1)
            worst = max(worst, (e * gap / EPS)[keep].max())
            assert np.all(e[keep] <= ROT_BOUND * EPS / gap[keep])
    print("%s: max err * gap / eps = %.1f, min gap %.2e, left out %d of %d" % (label, worst, gap.min(), n - keep.sum(), n))
    return worst


def check_admm_steps(run, name, steps=3, Q=None, lam=None):
    """`steps` single iterations, each from the state the library returned, against the restatement from the same state"""
    V, F = N.shape(name)
    A = N.rest(name)
    n = A.n
    nn, aa = N.vertex_normals_areas(V, F)
    P = N.noisy_pose(V)
    p = N.params()
    Qm = np.eye(3) if Q is None else Q
    la = (p["lambda_"] if lam is None else lam) * aa
    S = N.covariance(A, P)
    state = N.start_state(n, p)
    for step in range(steps):
        out, it = run(N.STY_ADMM_ONE, A, F, P, lam=lam, Q=Q, state_in=None if step == 0 else N.pack_state(state))
        R, terms, (z, u, rho) = N.unpack(N.STY_ADMM_ONE, out, n)
        Rn, zn, un, rhon, _, aux = N.admm_one(S, nn, Qm, la, p, *state)
        if Q is None and lam is None:
            assert aux["gap"].min() >= GAP_MIN                                         # on the issue's inputs the restatement itself leaves out none
        check_fit("%s, iteration %d" % (name, step + 1), R, Rn, aux["gap"], z, zn, u, np.where((rho == rhon)[:, None], un, u))
        # from the library's own rotation everything after the fit is correctly rounded arithmetic in one order: bit for bit
        z2, u2, rho2, _, _ = N.admm_after_fit(R, nn, Qm, la, p, *state)
        assert np.array_equal(z, z2) and np.array_equal(u, u2) and np.array_equal(rho, rho2) and np.all(it == 1)
        assert np.array_equal(terms, N.energy_terms(A, P, R, nn, la, Qm))
        r, s = aux["r"], aux["s"]
        tie = (np.abs(r - p["mu"] * s) <= TIE * np.maximum(r, p["mu"] * s)) | (np.abs(s - p["mu"] * r) <= TIE * np.maximum(s, p["mu"] * r))
        print("  rho decisions equal at %d of %d vertices, %d near a tie" % (np.sum(rho == rhon), n, tie.sum()))
        assert tie.sum() <= 0.01 * n and np.array_equal(rho[~tie], rhon[~tie])
        state = (z, u, rho)


def check_local(run, name, lambda_, bound=LOCAL_BOUND):
    V, F = N.shape(name)
    A = N.rest(name)
    nn, aa = N.vertex_normals_areas(V, F)
    P = N.noisy_pose(V)
    out, it = run(N.STY_LOCAL, A, F, P, lambda_=lambda_)
    R, terms, (z, u, rho) = N.unpack(N.STY_LOCAL, out, A.n)
    Rn, (zn, un, rhon), itn, tn = N.local(A, P, nn, aa, N.params(lambda_=lambda_))
    same = it == itn
    diff = np.abs(R - Rn)[same].max()
    print("%s, lambda %.1f: iterations mean %.2f, max %d, at the cap %d; counts differ at %d of %d; max |R - R_np| = %.2e (bound %.0e)"
          % (name, lambda_, it.mean(), it.max(), np.sum(it == 100), np.sum(~same), A.n, diff, bound))
    assert np.sum(~same) <= 0.01 * A.n and diff <= bound
    assert np.abs(terms - tn)[same].max() <= bound * np.abs(tn).max()
    assert np.array_equal(terms, N.energy_terms(A, P, R, nn, lambda_ * aa))
    return it


def host_run(smg):
    def run(op, A, F, P=None, **kw):
        rc, out, it = N.local_host(smg, op, A, F, P, **kw)
        assert rc == 0
        return out, it
    return run


@pytest.mark.parametrize("name", N.KERNEL_SHAPES)
def test_host_twin_against_restatement(smg_mod, name):
    run = host_run(smg_mod)
    V, F = N.shape(name)
    A = N.rest(name)
    n = A.n
    nn, aa = N.vertex_normals_areas(V, F)
    ln, la_ = N.unpack(N.STY_NORMALS, run(N.STY_NORMALS, A, F)[0], n)
    assert np.array_equal(ln, nn) and np.array_equal(la_, aa)
    assert np.all(np.abs(N.norm3(nn) - 1.0) <= 4 * EPS) and np.all(aa > 0)
    if name.startswith("strip"):
        assert np.all(nn[:, :2] == 0.0) and np.all(N.covariance(A, N.noisy_pose(V))[:, 2, :] == 0.0)      # flat: rank-2 covariances
    check_admm_steps(run, name)
    check_admm_steps(run, name, steps=2, Q=rotation_matrix([1.0, -2.0, 0.5], 0.7), lam=np.linspace(0.0, 0.5, n))
    for lambda_ in (0.2, 0.4):
        check_local(run, name, lambda_)
    P = N.noisy_pose(V)
    t = N.nearest_axis(nn)
    R, terms = N.unpack(N.STY_LOCAL_TARGETS, run(N.STY_LOCAL_TARGETS, A, F, P, targets=t)[0], n)
    Rn, _, gap = N.local_targets(A, P, nn, aa, N.params(), t)
    check_fit(name + ", normal-driven", R, Rn, gap)
    assert np.array_equal(terms, N.energy_terms(A, P, R, nn, 0.2 * aa, None, t))
    for tgt in (None, t):
        assert np.array_equal(N.unpack(N.STY_ENERGY, run(N.STY_ENERGY, A, F, P, targets=tgt, R_in=Rn)[0], n), N.energy_terms(A, P, Rn, nn, 0.2 * aa, None, tgt))


def test_local_step_reaches_the_cap_on_icosphere4(smg_mod):
    """the issue's full-step case: some vertices of icosphere(4) use all 100 iterations at the prototype's pose"""
    for lambda_ in (0.2, 0.4):
        it = check_local(host_run(smg_mod), "icosphere4", lambda_)
        assert it.max() == 100 and it.min() >= 1


# ---- the restatement itself --------------------------------------------------------------------------------------------------------------------
def test_cubic_run_reproduces_the_prototype():
    S, U, E, counts = N.reference_run("icosphere3")
    V, F = N.shape("icosphere3")
    c0, c1 = N.cubeness(V, F), N.cubeness(U, F)
    first, later = counts[0].mean(), max(c.mean() for c in counts[1:])
    print("cubeness %.4f -> %.4f; E" % (c0, c1), np.array2string(E, precision=5), "ADMM mean %.2f then <= %.2f, max %d" % (first, later, max(c.max() for c in counts)))
    assert np.all(E[1:] < E[:-1])
    assert abs(c0 - 1.4995) <= 0.005 and abs(c1 - 1.2139) <= 0.005
    assert 8 <= first <= 12 and 2 <= later <= 5.5 and max(c.max() for c in counts) == 20


def test_lambda_zero_is_arap():
    V, F = N.shape("icosphere3")
    A = N.rest("icosphere3")
    nn, aa = N.vertex_normals_areas(V, F)
    P = N.noisy_pose(V)
    R, _, it, _ = N.local(A, P, nn, aa, N.params(lambda_=0.0))
    Rn, _, _ = rotations_np(N.covariance(A, P))
    print("lambda = 0: iterations", np.unique(it), "max |R - R_arap| = %.2e" % np.abs(R - Rn).max())
    assert np.all(it == 2) and np.abs(R - Rn).max() <= 1e-12


def test_normal_driven_run_reproduces_the_prototype():
    S, U, E, _ = N.reference_run("icosphere3", "targets")
    c1 = N.cubeness(U, N.shape("icosphere3")[1])
    print("normal-driven: cubeness -> %.4f; E" % c1, np.array2string(E, precision=5))
    assert np.all(E[1:] <= E[:-1]) and abs(c1 - 1.3046) <= 0.005


def test_frame_rotates_the_result():
    """with Q a rotation of the axes and the mesh rotated by Q^T, the result is the rotated result of the identity-frame run"""
    V, F = N.shape("icosphere3")
    _, U, E, _ = N.reference_run("icosphere3")
    Q = rotation_matrix([1.0, 2.0, -0.5], 1.1)
    S = N.StylizeNp(V @ Q, F)                # rows v Q = (Q^T v)^T
    S.Q = Q
    UQ, EQ, _ = S.run(n_iter=10)
    print("frame: max |U_Q - Q^T U| = %.2e, energies %.2e" % (np.abs(UQ - U @ Q).max(), np.abs(EQ - E).max()))
    assert np.abs(UQ - U @ Q).max() <= 1e-10 and np.abs(EQ - E).max() <= 1e-10


# ---- the kernel's registers, the host maths under sanitizers -------------------------------------------------------------------------------------
def test_local_kernel_keeps_everything_in_registers():
    """the ISA notes of every k_stylize_local instantiation and of k_stylize_normals (the build's flags, device side only): no scratch, no
    spills; the cubic loop fits 128 VGPRs, 4 waves per SIMD (127 with __launch_bounds__(256, 4), 130 without)"""
    from surface_multigrid_code_amd import build as B
    src = os.path.join(B.CSRC, "smg_stylize_device.hip")
    asm = subprocess.check_output([B._hipcc()] + B.FLAGS + ["--cuda-device-only", "-S", src, "-o", "-"], text=True)
    bound = {"k_stylize_localILi0E": 128, "k_stylize_localILi1E": 128, "k_stylize_localILi2E": 72, "k_stylize_normals": 64}
    for kernel, vgprs in bound.items():
        notes = re.findall(r"\.name:\s+(\S*%s\S*)(.*?)\.wavefront_size" % kernel, asm, flags=re.S)
        assert len(notes) == 1
        body = notes[0][1]
        field = lambda k: int(re.search(r"\.%s:\s+(\d+)" % k, body).group(1))   # noqa: E731
        print("%s: vgpr_count %d, sgpr_count %d, private_segment_fixed_size %d, vgpr_spill_count %d, sgpr_spill_count %d"
              % (kernel, field("vgpr_count"), field("sgpr_count"), field("private_segment_fixed_size"), field("vgpr_spill_count"), field("sgpr_spill_count")))
        assert field("private_segment_fixed_size") == 0 and field("vgpr_spill_count") == 0 and field("sgpr_spill_count") == 0
        assert field("vgpr_count") <= vgprs


def test_host_maths_under_sanitizers(tmp_path):
    """tests/stylize_asan_driver.cpp, a stand-alone program: the host twin's body (smg::sty_local_host, what smg_stylize_local_host runs after its
    checks) on exactly-sized heap arrays for the 255, 256 and 257 vertex strips and the tetrahedron, under AddressSanitizer and
    UndefinedBehaviorSanitizer (static runtimes: run directly, nothing preloaded, nothing loaded into python)"""
    exe = str(tmp_path / "stylize_asan_driver")
    csrc = os.path.join(ROOT, "surface_multigrid_code_amd", "csrc")
    srcs = [os.path.join(ROOT, "tests", "stylize_asan_driver.cpp"), os.path.join(csrc, "smg_mesh.cpp"), os.path.join(csrc, "smg_sparse.cpp")]
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-ffp-contract=off", "-pthread", "-I" + csrc] + srcs + ["-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    run = subprocess.run([exe], env=env, capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0 and run.stdout.count("ok 1") == 4 and "ERROR" not in run.stderr
