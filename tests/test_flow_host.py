"""CPU: the conformalized mean-curvature flow (include/smg.h: smg_flow_*) -- the ABI and its refusals without a GPU, the library's host twin
(smg_flow_host) against the numpy restatement (tests/flow_np.py), and the restatement itself against the method's known behaviour.

The bounds.  Masses, right-hand sides, matrix values, normalised positions, the sphericity's sums, the sphere map and its singular values are
correctly rounded +, -, *, / and sqrt in one order on both sides: held bit for bit.  The mass is also held bit for bit to smg_mesh_massmatrix.

SIGMA_BOUND.  The closed form of flow_sigma against numpy.linalg.svd of the same Jacobian, relative to sigma1.  Measured on the CPU on the five
meshes of flow_np.LAUNCHER_MESHES (a wobbled state mapped to the sphere): the largest |sigma - sigma_svd| / sigma1 is 9.23e-16 (bunny.smgm);
the bound is 16 x that, 1.5e-14.

NORMALIZE_C.  smg_mesh_normalize_unit_area sums the double areas and the columns sequentially, the kernels by launch_fixed_sum: bits may differ.
Each of the three sums of n terms carries at most (n - 1) eps relative error in either order (Higham, Accuracy and Stability, section 4.2), the
scale enters under a square root (half of it) and the shift adds the column's; so every coordinate agrees within
NORMALIZE_C n eps max |U| with NORMALIZE_C = 4 (two orders x (1/2 + 1), rounded up), n = max(nV, nF).

FlowNp on bunny_15K_init, 20 steps of delta = 0.01: the restatement gave sphericity 6.832093e-3 (from 0.2963635), no flipped face, and an
area-weighted mean sigma1 / sigma2 of 1.070294.  They are pinned within PIN_REL = 1e-5 relative: seven digits are written down (1e-7), the direct
solves are accurate to about 1e-12 and the flow contracts towards the sphere, so another BLAS or SuperLU build moves these figures by far less,
while a change of the method (the order of the normalisation, another mass) moves them by 1e-3 and more."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import flow_np as N
from test_arap_host import _fake_hierarchy
from test_geodesics_host import flat_square

INVALID, NO_DEVICE = -1, -2
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "flow_refusals.json")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = N.EPS
SIGMA_BOUND = 1.5e-14                # see the header
NORMALIZE_C = 4                     # see the header
PIN_REL = 1e-5                      # see the header
BUNNY_20 = dict(sphericity=6.832093e-3, mean_ratio=1.070294)  # the restatement's own run, see the header

FLOW_SYMBOLS = ("smg_flow_params_default", "smg_flow_create", "smg_flow_destroy", "smg_flow_set_params", "smg_flow_set_solver", "smg_flow_device_bytes",
                "smg_flow_step", "smg_flow_positions", "smg_flow_set_positions", "smg_flow_reset", "smg_flow_sphere", "smg_flow_host", "smg_debug_flow")


# ---- the ABI and its refusals --------------------------------------------------------------------------------------------------------------------
def test_abi_present(smg_mod):
    L = smg_mod._lib.load()
    for name in FLOW_SYMBOLS:
        assert hasattr(L, name)
    assert hasattr(smg_mod, "MeanCurvatureFlow")
    assert L.smg_version() >= 515
    assert L.smg_flow_device_bytes(None) == 0
    p = L.smg_flow_params_default()
    assert (p.delta, p.normalize, p.stop_sphericity) == (0.01, 1, 0.0)


def _create(smg, h, V, F, nV=None, null=None, **params):
    """smg_flow_create -> (code, message); a successful create is destroyed at once"""
    L = smg._lib.load()
    ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
    V, F = np.ascontiguousarray(V, dtype=np.float64), np.ascontiguousarray(F, dtype=np.int32)
    p = L.smg_flow_params_default()
    for k, v in params.items():
        setattr(p, k, v)
    out = C.c_void_p(0xdead)
    rc = L.smg_flow_create(None if null == "h" else h, None if null == "V" else V.ctypes.data_as(dp), V.shape[0] if nV is None else nV,
                           None if null == "F" else F.ctypes.data_as(ip), F.shape[0], None if null == "p" else C.byref(p),
                           None if null == "out" else C.byref(out))
    if rc == 0:
        L.smg_flow_destroy(out)
        return rc, ""
    assert null == "out" or out.value is None, "a refused create must leave *out == NULL"
    return rc, L.smg_last_error().decode()


def create_cases(smg):
    """[(name, thunk -> (code, message), holds only without a device)]: the base's checks in its order, then the parameters in theirs"""
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
    cases.append(("single level", lambda: _create(smg, keep["one"].h, V, F), False))
    Vz = V.copy()
    Vz[F[0, 1]] = Vz[F[0, 0]]
    cases.append(("order: levels before mesh", lambda: _create(smg, keep["one"].h, Vz, F), False))
    cases.append(("zero area", lambda: _create(smg, fake.h, Vz, F), False))
    keep["two"] = _fake_hierarchy(smg, 2 * n)
    cases.append(("two components", lambda: _create(smg, keep["two"].h, V2, F2), False))
    for tag, d in (("zero", 0.0), ("negative", -0.01), ("nan", np.nan), ("inf", np.inf)):
        cases.append(("delta %s" % tag, lambda d=d: _create(smg, fake.h, V, F, delta=d), False))
    cases.append(("normalize 2", lambda: _create(smg, fake.h, V, F, normalize=2), False))
    cases.append(("normalize negative", lambda: _create(smg, fake.h, V, F, normalize=-1), False))
    cases.append(("stop negative", lambda: _create(smg, fake.h, V, F, stop_sphericity=-1e-3), False))
    cases.append(("stop nan", lambda: _create(smg, fake.h, V, F, stop_sphericity=np.nan), False))
    cases.append(("order: hierarchy before mesh", lambda: _create(smg, keep["blk"].h, Vz, F), False))
    cases.append(("order: mesh before delta", lambda: _create(smg, fake.h, Vz, F, delta=0.0), False))
    cases.append(("order: delta before normalize", lambda: _create(smg, fake.h, V, F, delta=0.0, normalize=2), False))
    cases.append(("order: normalize before stop", lambda: _create(smg, fake.h, V, F, normalize=2, stop_sphericity=-1.0), False))
    cases.append(("valid, real hierarchy", lambda: _create(smg, mg.h, V, F), True))
    cases.append(("valid, fake hierarchy, no normalisation", lambda: _create(smg, fake.h, V, F, normalize=0, delta=1e-3, stop_sphericity=0.5), True))
    return cases, keep


def null_object_cases(smg):
    """every entry point that takes the object, called without one"""
    L = smg._lib.load()
    X, st = np.zeros(12), np.zeros(4)
    dp = C.POINTER(C.c_double)
    p = L.smg_flow_params_default()
    calls = {"set_params": lambda: L.smg_flow_set_params(None, C.byref(p)),
             "set_solver": lambda: L.smg_flow_set_solver(None, 1),
             "step": lambda: L.smg_flow_step(None, 1, None, None, None, None),
             "positions": lambda: L.smg_flow_positions(None, 0, X.ctypes.data, 4),
             "set_positions": lambda: L.smg_flow_set_positions(None, X.ctypes.data, 4, 0),
             "reset": lambda: L.smg_flow_reset(None),
             "sphere": lambda: L.smg_flow_sphere(None, 0, None, 0, None, st.ctypes.data_as(dp))}
    return [("null object: " + k, (lambda f=f: (f(), L.smg_last_error().decode())), False) for k, f in calls.items()]


def host_twin_cases(smg, call=None, prefix="host twin"):
    """the operand checks smg_flow_host and smg_debug_flow share"""
    call = call or (lambda *a, **k: N.host(smg, *a, **k)[0])
    L = smg._lib.load()
    V, F = N.shape("icosphere1")
    rowptr, col, L0 = N.cotan_csr("icosphere1")
    Fo = np.array(F)
    Fo[1, 2] = V.shape[0]
    no_diag = col.copy()
    no_diag[N.diagonal(rowptr, col)[3]] = (3 + 20) % V.shape[0]
    bad_ptr = rowptr.copy()
    bad_ptr[5] = bad_ptr[4] - 1
    off = rowptr + 1
    col_out = col.copy()
    col_out[7] = V.shape[0]
    csr = (rowptr, col, L0)
    thunks = {
        "unknown op": lambda: call(4, V, F), "negative op": lambda: call(-1, V, F),
        "out missing": lambda: call(N.FLOW_NORMALIZE, V, F, over=dict(out=None)),
        "U missing": lambda: call(N.FLOW_SPHERICITY, V, F, over=dict(U=None)),
        "F missing": lambda: call(N.FLOW_NORMALIZE, V, F, over=dict(F=None)),
        "no vertex": lambda: call(N.FLOW_NORMALIZE, V, F, over=dict(nV=0)),
        "L0 missing": lambda: call(N.FLOW_SYSTEM, V, F, csr=(rowptr, col, None)),
        "rowptr missing": lambda: call(N.FLOW_SYSTEM, V, F, csr=(None, col, L0)),
        "V0 missing": lambda: call(N.FLOW_SPHERE, V, F),
        "face index": lambda: call(N.FLOW_NORMALIZE, V, Fo),
        "delta zero": lambda: call(N.FLOW_SYSTEM, V, F, csr=csr, delta=0.0),
        "delta nan": lambda: call(N.FLOW_SYSTEM, V, F, csr=csr, delta=np.nan),
        "rowptr start": lambda: call(N.FLOW_SYSTEM, V, F, csr=(off, col, L0)),
        "rowptr order": lambda: call(N.FLOW_SYSTEM, V, F, csr=(bad_ptr, col, L0)),
        "column out of range": lambda: call(N.FLOW_SYSTEM, V, F, csr=(rowptr, col_out, L0)),
        "no diagonal": lambda: call(N.FLOW_SYSTEM, V, F, csr=(rowptr, no_diag, L0)),
        "order: operands before faces": lambda: call(N.FLOW_SPHERE, V, Fo),
        "order: faces before delta": lambda: call(N.FLOW_SYSTEM, V, Fo, csr=csr, delta=0.0),
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
    """every refusal of smg_flow_create, of the calls on a missing object and of the host twin's operand checks, with the code and the
    smg_last_error() text recorded in tests/golden/flow_refusals.json; all of create's come before SMG_ERR_NO_DEVICE, which a valid call meets on
    a box without a GPU.  The refusals that need a live object (group "live": n_steps < 0, a bad memspace, a leading dimension below nV, a changed
    normalize, the sphere map of a mesh with a boundary and of a torus) are checked by tests/test_gpu_flow.py.  Every message carries its entry
    point's name."""
    golden = json.load(open(GOLDEN))
    cases, keep = create_cases(smg_mod)
    assert check_cases(smg_mod, cases, golden["create"]) == set(golden["create"]) - (
        set() if smg_mod._lib.load().smg_device_count() == 0 else {c[0] for c in cases if c[2]})
    assert check_cases(smg_mod, null_object_cases(smg_mod), golden["null"]) == set(golden["null"])
    assert check_cases(smg_mod, host_twin_cases(smg_mod), golden["host"]) == set(golden["host"])
    g = golden["create"]
    own = ["delta zero", "normalize 2", "stop negative"]
    assert len({g[k][1] for k in own}) == len(own)                                          # each has its own message
    assert g["order: hierarchy before mesh"] == g["block hierarchy"] and g["order: mesh before delta"] == g["zero area"]
    assert g["order: levels before mesh"] == g["single level"]
    assert g["order: delta before normalize"] == g["delta zero"] and g["order: normalize before stop"] == g["normalize 2"]
    assert all(v[1].startswith("smg_flow_create: ") for v in g.values())
    h = golden["host"]
    assert h["host twin: order: operands before faces"] == h["host twin: V0 missing"]
    assert h["host twin: order: faces before delta"] == h["host twin: face index"]
    assert all(v[1].startswith("smg_flow_host: ") for v in h.values())
    for name, (code, msg) in golden["null"].items():
        assert msg.startswith("smg_flow_" + name.split(": ")[1] + ": ")
    for name, (code, msg) in golden["live"].items():
        assert code == INVALID and msg.startswith("smg_flow_" + name.split()[0] + ": "), name
    del keep


def test_hook_refuses_what_the_host_twin_refuses(smg_mod):
    golden = json.load(open(GOLDEN))["host"]
    hook = lambda *a, **k: N.hook(smg_mod, *a, **k)[0]   # noqa: E731
    for name, thunk, _ in host_twin_cases(smg_mod, hook, "hook"):
        rc, msg = thunk()
        want = golden[name.replace("hook: ", "host twin: ")]
        assert [rc, msg] == [want[0], want[1].replace("smg_flow_host", "smg_debug_flow")], name
    if smg_mod._lib.load().smg_device_count() == 0:
        V, F = N.shape("icosphere1")
        assert N.hook(smg_mod, N.FLOW_NORMALIZE, V, F)[0] == NO_DEVICE


def test_no_gpu_comes_after_every_argument_check(smg_mod):
    """without a GPU MeanCurvatureFlow(...) raises the no-device error, and only once every argument check has passed"""
    if smg_mod._lib.load().smg_device_count() > 0:
        pytest.skip("a GPU is present")
    V, F = flat_square(8)
    fake = _fake_hierarchy(smg_mod, V.shape[0])
    with pytest.raises(smg_mod.SmgError) as e:
        smg_mod.MeanCurvatureFlow(fake, V, F)
    assert e.value.code == NO_DEVICE and "smg_flow_create" in str(e.value) and "no CPU fallback" in str(e.value)
    with pytest.raises(smg_mod.SmgError) as e:
        smg_mod.MeanCurvatureFlow(fake, V, F, delta=-1.0)
    assert e.value.code == INVALID
    with pytest.raises(smg_mod.SmgError) as e:
        smg_mod.MeanCurvatureFlow(fake, V, F, stop_sphericity=-1.0)
    assert e.value.code == INVALID


# ---- the host twin against the restatement ---------------------------------------------------------------------------------------------------------
def host_run(smg):
    def run(op, U, F, **kw):
        rc, out = N.host(smg, op, U, F, **kw)
        assert rc == 0
        return out
    return run


@pytest.mark.parametrize("name", N.LAUNCHER_MESHES)
def test_host_twin_against_restatement(smg_mod, name):
    """every op bit for bit; the mass bit for bit against smg_mesh_massmatrix; sigma against LAPACK; the normalisation against
    smg_mesh_normalize_unit_area within the bound of the header"""
    from surface_multigrid_code_amd import mesh
    V, F = N.shape(name)
    U = N.wobbled(name)
    m, Un, sig, S = N.check_launchers(host_run(smg_mod), name)
    assert np.array_equal(m, mesh.massmatrix(U, F, "barycentric").diagonal())
    ref = N.sigma_svd(V, S, F)
    dev = float((np.abs(sig - ref) / ref[:, [0]]).max())
    print("%s: max |sigma - sigma_svd| / sigma1 = %.2e (bound %.0e)" % (name, dev, SIGMA_BOUND))
    assert dev <= SIGMA_BOUND
    bound = NORMALIZE_C * max(U.shape[0], F.shape[0]) * EPS * np.abs(U).max()
    far = float(np.abs(Un - mesh.normalize_unit_area(U, F)).max())
    print("%s: max |normalised - smg_mesh_normalize_unit_area| = %.2e (bound %.2e)" % (name, far, bound))
    assert far <= bound


# ---- the restatement itself ------------------------------------------------------------------------------------------------------------------------
def test_a_normalising_step_leaves_a_normalised_mesh():
    V, F = N.shape("squashed")
    flow = N.FlowNp(V, F)
    flow.step(1)
    U = flow.U
    n = U.shape[0]
    area = 0.5 * N.darea(U, F).sum()
    print("area - 1 = %.2e, mean x %.2e, mean y %.2e, min z %.2e" % (area - 1.0, U[:, 0].mean(), U[:, 1].mean(), U[:, 2].min()))
    assert abs(area - 1.0) <= 4 * F.shape[0] * EPS                                # a sum of nF terms
    assert abs(U[:, 0].mean()) <= 4 * n * EPS * np.abs(U).max() and abs(U[:, 1].mean()) <= 4 * n * EPS * np.abs(U).max()
    assert U[:, 2].min() == 0.0


def test_squashed_sphere_rounds_out():
    """sphericity 0.255 -> about 1.25e-2 in 30 steps, no flipped face; it is not monotone afterwards and is not asserted to be"""
    V, F = N.shape("squashed")
    flow = N.FlowNp(V, F)
    his = flow.step(30)
    _, _, _, stats = flow.sphere()
    print("squashed icosphere(3): sphericity %.4e -> %.4e, flipped %d, mean ratio %.4f" % (his[0], his[-1], stats[2], stats[0]))
    assert 0.2 < his[0] < 0.3 and his[-1] < 2e-2 and stats[2] == 0.0 and np.all(np.isfinite(flow.U))


@pytest.fixture(scope="module")
def bunny_20():
    V, F = N.shape("bunny_15K_init.smgm")
    flow = N.FlowNp(V, F)
    his = flow.step(20)
    return flow, his


def test_bunny_reaches_the_sphere(bunny_20):
    flow, his = bunny_20
    _, sig, _, stats = flow.sphere()
    print("bunny_15K_init: sphericity %.6e -> %.6e after 20 steps; flipped %d; mean sigma1 / sigma2 %.6f, max %.3f"
          % (his[0], his[-1], stats[2], stats[0], stats[1]))
    assert stats[2] == 0.0 and np.all(np.isfinite(flow.U))
    assert abs(his[-1] - BUNNY_20["sphericity"]) <= PIN_REL * BUNNY_20["sphericity"]
    assert abs(stats[0] - BUNNY_20["mean_ratio"]) <= PIN_REL * BUNNY_20["mean_ratio"]
    assert stats[3] == his[-1]


# ---- the kernels' registers, the host maths under sanitizers -------------------------------------------------------------------------------------
def test_kernels_keep_everything_in_registers():
    """the ISA notes of every kernel of smg_flow_device.hip (the build's flags, device side only): no scratch, no spills"""
    import re
    from surface_multigrid_code_amd import build as B
    src = os.path.join(B.CSRC, "smg_flow_device.hip")
    asm = subprocess.check_output([B._hipcc()] + B.FLAGS + ["--cuda-device-only", "-S", src, "-o", "-"], text=True, stderr=subprocess.DEVNULL)
    notes = re.findall(r"\.name:\s+(\S*k_flow\S*)(.*?)\.wavefront_size", asm, flags=re.S)
    assert len(notes) == 11                                                      # k_flow_system in its two forms
    for kernel, body in notes:
        field = lambda k: int(re.search(r"\.%s:\s+(\d+)" % k, body).group(1))   # noqa: E731
        print("%s: vgpr_count %d, sgpr_count %d, private_segment_fixed_size %d" % (kernel, field("vgpr_count"), field("sgpr_count"), field("private_segment_fixed_size")))
        assert field("private_segment_fixed_size") == 0 and field("vgpr_spill_count") == 0 and field("sgpr_spill_count") == 0
        assert field("vgpr_count") <= 128


def test_host_maths_under_sanitizers(tmp_path):
    """tests/flow_asan_driver.cpp, a stand-alone program: the host twin's loops (smg::flow_host_* of csrc/smg_flow_inl.hpp, what smg_flow_host runs
    after its checks) for every op on exactly-sized heap arrays, under AddressSanitizer and UndefinedBehaviorSanitizer (static runtimes: run
    directly, nothing preloaded, nothing loaded into python)"""
    exe = str(tmp_path / "flow_asan_driver")
    csrc = os.path.join(ROOT, "surface_multigrid_code_amd", "csrc")
    srcs = [os.path.join(ROOT, "tests", "flow_asan_driver.cpp"), os.path.join(csrc, "smg_mesh.cpp"), os.path.join(csrc, "smg_sparse.cpp")]
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-ffp-contract=off", "-pthread", "-I" + csrc] + srcs + ["-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    run = subprocess.run([exe], env=env, capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0 and run.stdout.count("ok 1") == 4 and "ERROR" not in run.stderr
