"""CPU: projective-dynamics membrane steps (include/smg.h: smg_pd_*) -- the ABI and its refusals without a GPU, the library's host twin of the
face maths (smg_pd_project_host) against an SVD projection, and the numpy / scipy restatement of the method (tests/pd_np.py, direct solves)
that tests/test_gpu_pd.py checks the device against.

The projection bound: per face |T - T_svd|_F <= B eps (sigma1 / sigma2)^2 with B = PROJECTION_B = 1e3, 100 x the maximum measured on the host
twin over the compared poses (6.98), rounded up to a power of ten.  The factor (sigma1 / sigma2)^2 is the conditioning of lambda2 = m - r."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import pd_np as N
from oracle import mesh_np as M
from test_arap_host import _fake_hierarchy
from test_geodesics_host import flat_square

INVALID, NO_DEVICE = -1, -2
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pd_refusals.json")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = N.EPS
PROJECTION_B = 1e3
BANDS = [(1.0, 1.0), (0.9, 1.2)]
MESHES = ["ogre_sim.smgm", "bunny_15K_init.smgm"]

# the issue's table: band (1, 1), pressure 5, h = 1e-2, rho = k = 1, unit-area meshes, 10 iterations, direct solves: (E_0, E_1, E_2, E_10) per step
TABLE = {"ogre_sim.smgm": [(3.193227e-05, 2.426916e-05, 2.411633e-05, 2.408179e-05), (2.047768e-04, 1.627862e-04, 1.620281e-04, 1.618670e-04),
                           (5.832829e-04, 4.822585e-04, 4.806514e-04, 4.803290e-04)],
         "bunny_15K_init.smgm": [(2.936951e-04, 1.300974e-04, 1.248978e-04, 1.212681e-04), (1.042264e-03, 5.670580e-04, 5.502275e-04, 5.381248e-04),
                                 (1.907405e-03, 1.227633e-03, 1.202462e-03, 1.184763e-03)]}


def projection_errors(T, Fg, band):
    """per face (|T - T_svd|_F, the bound B eps (sigma1 / sigma2)^2) against the SVD projection of the same Fg"""
    s, Tsvd = N.project_svd(Fg, *band)
    return np.sqrt(np.sum((T - Tsvd) ** 2, axis=1)), PROJECTION_B * EPS * (s[:, 0] / s[:, 1]) ** 2, s


def compared_poses(name, band):
    V, F = N.load_mesh(name)
    _, _, states = N.reference_run(name, band)
    return V, F, [("rest", V), ("amp 0.02", N.perturbed(V, F, 0.02)), ("amp 0.3", N.perturbed(V, F, 0.3)), ("after one step", np.array(states[1][0]))]


# ---- the ABI and its refusals --------------------------------------------------------------------------------------------------------------------
PD_SYMBOLS = ("smg_pd_params_default", "smg_pd_create", "smg_pd_destroy", "smg_pd_device_bytes", "smg_pd_set_solver", "smg_pd_set_state",
              "smg_pd_get_state", "smg_pd_set_forces", "smg_pd_set_strain_limits", "smg_pd_step", "smg_pd_strain", "smg_pd_project_host", "smg_debug_pd")


def test_abi_present(smg_mod):
    L = smg_mod._lib.load()
    for name in PD_SYMBOLS:
        assert hasattr(L, name)
    assert hasattr(smg_mod, "ProjectiveDynamics")
    assert L.smg_version() >= 511
    p = smg_mod.pd_params()
    assert (p.dt, p.density, p.stiffness, p.sigma_min, p.sigma_max, p.pressure, tuple(p.gravity)) == (1e-2, 1.0, 1.0, 1.0, 1.0, 0.0, (0.0, 0.0, 0.0))
    assert L.smg_pd_device_bytes(None) == 0
    st = np.zeros(4)
    dp = C.POINTER(C.c_double)
    for rc in (L.smg_pd_set_solver(None, 1), L.smg_pd_set_state(None, None, None, 0), L.smg_pd_get_state(None, None, None, 0),
               L.smg_pd_set_forces(None, 0.0, None), L.smg_pd_set_strain_limits(None, 1.0, 1.0),
               L.smg_pd_step(None, None, 0, 1, 0.0, None, None, None, None), L.smg_pd_strain(None, 0, None, st.ctypes.data_as(dp))):
        assert rc == INVALID


def _create(smg, h, V, F, pins=(), nV=None, null=None, **params):
    """smg_pd_create -> (code, message); a successful create is destroyed at once"""
    L = smg._lib.load()
    ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
    V, F = np.ascontiguousarray(V, dtype=np.float64), np.ascontiguousarray(F, dtype=np.int32)
    pins = np.ascontiguousarray(pins, dtype=np.int32)
    par = N.pd_params_c(smg, **params)
    out = C.c_void_p(0xdead)
    rc = L.smg_pd_create(None if null == "h" else h, None if null == "V" else V.ctypes.data_as(dp), V.shape[0] if nV is None else nV,
                         None if null == "F" else F.ctypes.data_as(ip), F.shape[0], pins.ctypes.data_as(ip) if pins.size and null != "pins" else None,
                         pins.size, None if null == "p" else C.byref(par), None if null == "out" else C.byref(out))
    if rc == 0:
        L.smg_pd_destroy(out)
        return rc, ""
    assert null == "out" or out.value is None, "a refused create must leave *out == NULL"
    return rc, L.smg_last_error().decode()


def refusal_cases(smg):
    """[(name, thunk -> (code, message), holds only without a device)]: the base's checks in its order, then the object's own"""
    V, F = flat_square(8)
    n = V.shape[0]
    keep = {"mg": smg.mg_precompute(V, F, 0.25, 20, 1), "blk": smg.mg_precompute_block(V, F, 0.25, 20, 1)}
    keep["un"] = smg.Hierarchy.union([keep["mg"], keep["mg"]])
    mg, fake = keep["mg"], _fake_hierarchy(smg, n)
    V2, F2 = np.concatenate([V, V + 3.0]), np.concatenate([F, F + n])
    cases = [("null %s" % a, (lambda a=a: _create(smg, mg.h, V, F, pins=[0], null=a)), False) for a in ("h", "V", "F", "p", "out", "pins")]
    cases.append(("negative n_pins", lambda: (smg._lib.load().smg_pd_create(mg.h, V.ctypes.data_as(C.POINTER(C.c_double)), n,
                                                                             F.ctypes.data_as(C.POINTER(C.c_int)), F.shape[0], None, -1,
                                                                             C.byref(N.pd_params_c(smg)), C.byref(C.c_void_p())),
                                              smg._lib.load().smg_last_error().decode()), False))
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
    for field in ("dt", "density", "stiffness"):
        for tag, bad in (("zero", 0.0), ("negative", -1.0), ("nan", np.nan), ("inf", np.inf)):
            cases.append(("%s %s" % (field, tag), lambda field=field, bad=bad: _create(smg, fake.h, V, F, **{field: bad}), False))
    for tag, band in (("negative sigma_min", (-0.1, 1.0)), ("sigma_min above sigma_max", (1.1, 1.0)), ("nan sigma_min", (np.nan, 1.0)),
                      ("inf sigma_max", (1.0, np.inf))):
        cases.append((tag, lambda band=band: _create(smg, fake.h, V, F, sigma_min=band[0], sigma_max=band[1]), False))
    cases.append(("nan pressure", lambda: _create(smg, fake.h, V, F, pressure=np.nan), False))
    cases.append(("inf gravity", lambda: _create(smg, fake.h, V, F, gravity=(0.0, np.inf, 0.0)), False))
    cases.append(("pin out of range", lambda: _create(smg, fake.h, V, F, pins=[0, n]), False))
    cases.append(("pin negative", lambda: _create(smg, fake.h, V, F, pins=[-1]), False))
    cases.append(("pin repeated", lambda: _create(smg, fake.h, V, F, pins=[3, 5, 3]), False))
    cases.append(("every vertex pinned", lambda: _create(smg, fake.h, V, F, pins=np.arange(n)), False))
    # the object's own checks come in this order: a bad dt wins over a bad band, a bad band over a bad pin
    cases.append(("order: dt before band", lambda: _create(smg, fake.h, V, F, dt=0.0, sigma_min=2.0, pins=[n]), False))
    cases.append(("order: band before pins", lambda: _create(smg, fake.h, V, F, sigma_min=2.0, pins=[n]), False))
    cases.append(("order: mesh before params", lambda: _create(smg, fake.h, Vz, F, dt=0.0), False))
    cases.append(("valid, real hierarchy", lambda: _create(smg, mg.h, V, F, pins=[0, 8]), True))
    cases.append(("valid, no pins, fake hierarchy", lambda: _create(smg, fake.h, V, F), True))
    return cases, keep


def test_create_refusals_keep_code_and_message(smg_mod):
    """every refusal of smg_pd_create, with the code and the smg_last_error() text recorded in tests/golden/pd_refusals.json; all of them come
    before SMG_ERR_NO_DEVICE, which a valid call meets on a box without a GPU"""
    L = smg_mod._lib.load()
    golden = json.load(open(GOLDEN))
    cases, keep = refusal_cases(smg_mod)
    no_device = L.smg_device_count() == 0
    seen = set()
    for name, thunk, device_only in cases:
        if device_only and not no_device:
            continue
        rc, msg = thunk()
        seen.add(name)
        assert [rc, msg] == golden[name], name
        assert rc == (NO_DEVICE if device_only else INVALID), name
    assert seen == set(golden) - (set() if no_device else {c[0] for c in cases if c[2]})
    own = ("dt zero", "density zero", "stiffness zero", "negative sigma_min", "nan pressure", "pin out of range", "pin repeated", "every vertex pinned")
    assert len({golden[k][1] for k in own}) == len(own)                                          # each has its own message
    assert golden["order: dt before band"] == golden["dt zero"] and golden["order: band before pins"][1] == golden["sigma_min above sigma_max"][1]
    assert golden["order: mesh before params"] == golden["zero area"]
    del keep


def test_setter_and_host_twin_refusals(smg_mod):
    V, F = flat_square(4)
    for band in ((-1.0, 1.0), (2.0, 1.0), (np.nan, 1.0), (0.5, np.inf)):
        assert N.project_host(smg_mod, V, V, F, *band)[0] == INVALID
    Fo = F.copy()
    Fo[1, 1] = V.shape[0]
    assert N.project_host(smg_mod, V, V, Fo, 1.0, 1.0)[0] == INVALID
    L = smg_mod._lib.load()
    assert L.smg_pd_project_host(None, None, 4, None, 2, 1.0, 1.0, None, None, None, None) == INVALID


def test_hook_refusals(smg_mod):
    V, F = flat_square(4)
    n, nF = V.shape[0], F.shape[0]
    vel = np.zeros(3 * n)
    assert N.pd_hook(smg_mod, 9, n, F, V, V, vel, 4 * nF)[0] == INVALID                       # unknown op
    assert N.pd_hook(smg_mod, -1, n, F, V, V, vel, 4 * nF)[0] == INVALID
    assert N.pd_hook(smg_mod, N.PD_REST, n, F, None, V, vel, 4 * nF)[0] == INVALID            # V0 missing
    assert N.pd_hook(smg_mod, N.PD_FACES, n, F, V, None, vel, 24 * nF)[0] == INVALID          # the pose missing
    assert N.pd_hook(smg_mod, N.PD_STRAIN, n, F, V, None, vel, 5 * nF)[0] == INVALID
    assert N.pd_hook(smg_mod, N.PD_PREDICT, n, F, V, V, None, 6 * n)[0] == INVALID            # in missing
    assert N.pd_hook(smg_mod, N.PD_VERTICES, n, F, V, V, None, 5 * n)[0] == INVALID
    assert N.pd_hook(smg_mod, N.PD_ENERGY, n, F, V, V, None, 1)[0] == INVALID
    assert N.pd_hook(smg_mod, N.PD_FINISH, n, F, V, V, None, 6 * n)[0] == INVALID
    assert N.pd_hook(smg_mod, N.PD_REST, n, F, V, V, vel, 0)[0] == INVALID                    # out missing
    for bad in (n, -1):                                                                        # a face index out of range
        Fo = F.copy()
        Fo[2, 1] = bad
        assert N.pd_hook(smg_mod, N.PD_REST, n, Fo, V, V, vel, 4 * nF)[0] == INVALID
    if smg_mod._lib.load().smg_device_count() == 0:
        assert N.pd_hook(smg_mod, N.PD_REST, n, F, V, V, vel, 4 * nF)[0] == NO_DEVICE
        assert N.pd_hook(smg_mod, N.PD_ENERGY, n, F, V, V, np.zeros(nF + n), 1)[0] == NO_DEVICE


# ---- the host twin of the face maths --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("band", BANDS, ids=["polar", "band"])
@pytest.mark.parametrize("name", MESHES)
def test_host_projection_against_svd(smg_mod, name, band):
    V, F, poses = compared_poses(name, band)
    r = N.rest_constants(V, F)
    worst = 0.0
    for label, Q in poses:
        rc, Fg, sigma, T, hits = N.project_host(smg_mod, V, Q, F, *band)
        assert rc == 0 and hits == 0                                                   # no guard fires on a compared pose
        Fn = N.gradient(r, F, Q)
        sn, Tn, guard = N.project(Fn, *band)
        assert np.array_equal(Fg, Fn) and np.array_equal(sigma, sn) and np.array_equal(T, Tn) and not guard.any()   # the restatement is the twin's text
        err, bound, s = projection_errors(T, Fg, band)
        worst = max(worst, float((err / (bound / PROJECTION_B)).max()))
        counts = N.clamp_outcomes(sigma, *band)
        print("%s %s %-14s |T - T_svd| <= %.2f eps (s1/s2)^2, min s2/s1 %.2e, inside / above / below %s"
              % (name, band, label, (err / (bound / PROJECTION_B)).max(), (s[:, 1] / s[:, 0]).min(), counts))
        assert np.all(np.isfinite(T)) and np.all(err <= bound)                         # every face compared: none is left out
        assert np.all(np.abs(sigma - s) <= 16 * EPS * (s[:, 0] / s[:, 1])[:, None] ** 2 * s[:, :1])
        if label == "amp 0.3":
            # sigma1 > sigma_max and sigma2 < sigma_min both occur; a face inside the band needs a band with an interior
            assert counts[1] > 0 and counts[2] > 0 and (band[0] == band[1] or counts[0] > 0)
    print("  worst ratio %.2f (PROJECTION_B = %g)" % (worst, PROJECTION_B))


def test_hand_made_faces_and_the_two_guards(smg_mod):
    band = (0.9, 1.2)
    F1 = np.array([[0, 1, 2]], dtype=np.int32)
    outcomes = {}
    for label, pose, guard in N.hand_faces(band):
        rc, Fg, sigma, T, hits = N.project_host(smg_mod, N.REST_FACE, pose, F1, *band)
        assert rc == 0 and hits == (1 if guard else 0), label
        sn, Tn, gn = N.project(N.gradient(N.rest_constants(N.REST_FACE, F1), F1, pose), *band)
        assert np.array_equal(T, Tn) and np.array_equal(sigma, sn) and bool(gn[0]) == guard
        outcomes[label] = (sigma[0], T[0])
        if not guard:
            err, bound, _ = projection_errors(T, Fg, band)
            assert err[0] <= bound[0], label
    assert N.clamp_outcomes(outcomes["inside"][0][None], *band) == (1, 0, 0)
    assert N.clamp_outcomes(outcomes["above"][0][None], *band) == (0, 1, 0)
    assert N.clamp_outcomes(outcomes["below"][0][None], *band) == (0, 0, 1)
    # the segment: f1 = (2, 0, 0), f2 = 0: u1 = e_x, the axis with the smallest |u1_j| is y (the lowest j of the tie y, z), sigma2 = 0 clamps to 0.9
    assert np.array_equal(outcomes["segment"][0], [2.0, 0.0]) and np.array_equal(outcomes["segment"][1], [1.2, 0, 0, 0, 0.9, 0])
    # the point: lambda1 == 0, T = (t, 0, 0), (0, t, 0) with t = clamp(0) = 0.9
    assert np.array_equal(outcomes["point"][0], [0.0, 0.0]) and np.array_equal(outcomes["point"][1], [0.9, 0, 0, 0, 0.9, 0])
    # all five in one call: the count is the number of faces on which a guard fired
    V5 = np.tile(N.REST_FACE, (5, 1))
    P5 = np.concatenate([pose for _, pose, _ in N.hand_faces(band)])
    F5 = np.arange(15, dtype=np.int32).reshape(5, 3)
    assert N.project_host(smg_mod, V5, P5, F5, *band)[4] == 2


# ---- the restatement itself --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MESHES)
def test_rest_gradients_assemble_the_cotangent_matrix(name):
    """sum_f A_f G_f^T G_f = -L: the constraint term of the global matrix is the cotangent matrix smg_assemble gives (bound 1e-13 of max |L|)"""
    import scipy.sparse as sp
    V, F = N.load_mesh(name)
    r = N.rest_constants(V, F)
    g1 = np.stack([1.0 / r[:, 0], 0.0 - r[:, 1] / (r[:, 0] * r[:, 2])], axis=1)
    g2 = np.stack([np.zeros(F.shape[0]), 1.0 / r[:, 2]], axis=1)
    g = [(0.0 - g1) - g2, g1, g2]
    I, J, W = [], [], []
    for i in range(3):
        for j in range(3):
            I.append(F[:, i]); J.append(F[:, j]); W.append(r[:, 3] * np.sum(g[i] * g[j], axis=1))
    K = sp.coo_matrix((np.concatenate(W), (np.concatenate(I), np.concatenate(J))), shape=(V.shape[0],) * 2).tocsr()
    L = M.cotmatrix(V, F).tocsr()
    err = abs(K + L).max() / abs(L).max()
    print(name, "|sum A G^T G + L| / max |L| = %.2e" % err)
    assert err <= 1e-13


@pytest.mark.parametrize("band", BANDS, ids=["polar", "band"])
def test_energy_descends_with_direct_solves(band):
    P, Es, _ = N.reference_run("ogre_sim.smgm", band)
    floor = 1e-20 * P.p["stiffness"] * P.area()
    for step, E in enumerate(Es):
        print(band, "step", step, np.array2string(E, precision=6))
        assert np.all(np.isfinite(E)) and np.all(E[1:] <= E[:-1] * (1 + 1e-12) + floor)


@pytest.mark.parametrize("name", MESHES)
def test_restatement_reproduces_the_table(name):
    _, Es, _ = N.reference_run(name, (1.0, 1.0))
    for E, want in zip(Es, TABLE[name]):
        for t, w in zip((0, 1, 2, 10), want):
            assert abs(E[t] / w - 1.0) <= 1e-3


def test_momentum_without_forces_or_pins():
    V, F = N.load_mesh("ogre_sim.smgm")
    P = N.PdNp(V, F)
    c, w = np.array([0.3, -0.2, 0.1]), np.array([0.5, 0.25, -1.0])
    P.x, P.v = V @ N.ROT.T + c, np.tile(w, (V.shape[0], 1))
    x0 = P.x.copy()
    E, _ = P.step(n_iter=10)
    diag = np.linalg.norm(x0.max(axis=0) - x0.min(axis=0))
    print("max |x' - (x + h w)| / diagonal = %.2e, max E_t = %.2e" % (np.abs(P.x - (x0 + P.p["dt"] * w)).max() / diag, E.max()))
    assert np.abs(P.x - (x0 + P.p["dt"] * w)).max() <= 1e-12 * diag
    assert np.all(E <= 1e-20 * P.p["stiffness"] * P.area())


def test_fixed_sum_restatement_is_a_sum():
    import math
    rng = np.random.default_rng(3)
    for n in (1, 255, 257, 2049, 7684, 50000):
        t = rng.standard_normal(n) ** 2
        assert abs(N.fixed_sum(t) - math.fsum(t)) <= 2 * n * EPS * t.sum()


# ---- the kernels' registers, the host maths under sanitizers -------------------------------------------------------------------------------------
def test_face_kernels_keep_everything_in_registers():
    """the ISA notes of k_pd_faces in both modes (the build's flags, device side only): no scratch, no spills"""
    from surface_multigrid_code_amd import build as B
    src = os.path.join(B.CSRC, "smg_pd_device.hip")
    asm = subprocess.check_output([B._hipcc()] + B.FLAGS + ["--cuda-device-only", "-S", src, "-o", "-"], text=True)
    for pattern in (r"k_pd_facesILi0E", r"k_pd_facesILi1E"):
        notes = re.findall(r"\.name:\s+(\S*%s\S*)(.*?)\.wavefront_size" % pattern, asm, flags=re.S)
        assert len(notes) == 1
        body = notes[0][1]
        field = lambda k: int(re.search(r"\.%s:\s+(\d+)" % k, body).group(1))   # noqa: E731
        print("%s: vgpr_count %d, private_segment_fixed_size %d, vgpr_spill_count %d"
              % (pattern, field("vgpr_count"), field("private_segment_fixed_size"), field("vgpr_spill_count")))
        assert field("private_segment_fixed_size") == 0 and field("vgpr_spill_count") == 0
        assert field("vgpr_count") <= 64          # 512 / 64 = 8 waves per SIMD (56 in both modes)


def test_host_projection_under_sanitizers(tmp_path):
    """tests/pd_project_driver.cpp, a stand-alone program: smg_pd_inl.hpp on exactly-sized heap arrays, guard faces included, under
    AddressSanitizer and UndefinedBehaviorSanitizer (static runtimes: run directly, nothing preloaded, nothing loaded into python)"""
    exe = str(tmp_path / "pd_project_driver")
    src = os.path.join(ROOT, "tests", "pd_project_driver.cpp")
    inc = os.path.join(ROOT, "surface_multigrid_code_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-ffp-contract=off", "-I" + inc, src, "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    run = subprocess.run([exe], env=env, capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0 and "guard faces 2" in run.stdout and "ERROR" not in run.stderr
