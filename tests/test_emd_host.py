"""CPU: the earth mover's distance on a mesh (include/smg.h: smg_emd_*) -- the ABI and its refusals without a GPU, the library's host twin
(smg_emd_host) against the numpy restatement (tests/emd_np.py), and the restatement itself against the method's exact properties.

Geometry, right-hand sides, the update, the bounds' terms and sums, the potential and the flow are correctly rounded +, -, *, /, sqrt and max in one
order on both sides: held bit for bit.

The properties, every quantity computed on the CPU from the restatement (EmdNp: direct solves); res = |weak divergence of J - b|_2 over the unknown
rows, psi = the returned potential (dual feasible by construction), eps = 2^-52:

    CERTIFICATE  lower <= upper + res |psi|_2 at every iteration of every case of the table: b . psi = sum_f A_f J_f . grad psi_f - (div J - b) . psi
                 and |grad psi_f| <= 1
    TABLE        the iterations to a gap of 1e-2 and of 1e-3 with the default parameters, checked at every iteration
    SWAP         swapping mu0 and mu1 gives the same upper and lower bit for bit: every operation is odd in b
    HALVING      multiplying b by 0.5 halves both bit for bit with the same iteration count: a power of two, and rho scales with it
    FLAT         on the flat square, deltas give upper + res |psi|_2 >= the Euclidean distance: a linear function of unit slope is dual feasible
    TRIANGLE     lower(a, c) <= upper(a, b) + upper(b, c) + the residual terms across three blob distributions
    POTENTIAL    max_f |grad potential_f| <= 1 + 4 eps, and b . potential (the fixed-order sum) == lower bit for bit
    WARM         warm=True after a converged call ends at the first check"""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import emd_np as N
from test_arap_host import _fake_hierarchy
from test_geodesics_host import flat_square

INVALID, NO_DEVICE = -1, -2
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "emd_refusals.json")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = N.EPS
MESHES = N.LAUNCHER_MESHES

EMD_SYMBOLS = ("smg_emd_params_default", "smg_emd_create", "smg_emd_destroy", "smg_emd_set_params", "smg_emd_set_solver", "smg_emd_device_bytes",
               "smg_emd_solve", "smg_emd_host", "smg_debug_emd")

# iterations to a gap of 1e-2 and of 1e-3, and upper at 1e-3, with the default parameters and a check at every iteration
TABLE = {
    ("icosphere1", "deltas"): (34, 64, 2.051223), ("icosphere1", "blobs"): (117, 463, 2.016492),
    ("icosphere3", "deltas"): (38, 623, 1.447333), ("icosphere3", "blobs"): (121, 908, 1.408243),
    ("torus", "deltas"): (61, 352, 3.354780), ("torus", "blobs"): (72, 370, 2.869564),
    ("square", "deltas"): (23, 564, 0.642824), ("square", "blobs"): (67, 441, 0.566423),
    ("bunny.smgm", "deltas"): (149, 864, 0.252524), ("bunny.smgm", "blobs"): (167, 1130, 0.236291),
}


# ---- the ABI and its refusals --------------------------------------------------------------------------------------------------------------------
def test_abi_present(smg_mod):
    L = smg_mod._lib.load()
    for name in EMD_SYMBOLS:
        assert hasattr(L, name)
    assert hasattr(smg_mod, "EarthMover")
    assert L.smg_version() >= 518
    assert L.smg_emd_device_bytes(None) == 0
    p = L.smg_emd_params_default()
    assert (p.gap_tol, p.max_iter, p.check_every, p.alpha, p.rho_scale, p.inner_rel_tol) == (1e-2, 2000, 10, 1.7, 0.1, 1e-8)
    assert {f: getattr(p, f) for f, _ in p._fields_} == N.DEFAULTS


def _create(smg, h, V, F, nV=None, null=None, **params):
    """smg_emd_create -> (code, message); a successful create is destroyed at once"""
    L = smg._lib.load()
    ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
    V, F = np.ascontiguousarray(V, dtype=np.float64), np.ascontiguousarray(F, dtype=np.int32)
    p = L.smg_emd_params_default()
    for key, val in params.items():
        setattr(p, key, val)
    out = C.c_void_p(0xdead)
    rc = L.smg_emd_create(None if null == "h" else h, None if null == "V" else V.ctypes.data_as(dp), V.shape[0] if nV is None else nV,
                          None if null == "F" else F.ctypes.data_as(ip), F.shape[0], None if null == "p" else C.byref(p),
                          None if null == "out" else C.byref(out))
    if rc == 0:
        L.smg_emd_destroy(out)
        return rc, ""
    assert null == "out" or out.value is None, "a refused create must leave *out == NULL"
    return rc, L.smg_last_error().decode()


BAD_PARAMS = (("gap_tol zero", dict(gap_tol=0.0)), ("gap_tol nan", dict(gap_tol=float("nan"))), ("gap_tol infinite", dict(gap_tol=float("inf"))),
              ("max_iter negative", dict(max_iter=-1)), ("check_every zero", dict(check_every=0)), ("alpha zero", dict(alpha=0.0)),
              ("alpha two", dict(alpha=2.0)), ("alpha nan", dict(alpha=float("nan"))), ("rho_scale negative", dict(rho_scale=-0.1)),
              ("rho_scale infinite", dict(rho_scale=float("inf"))), ("inner_rel_tol zero", dict(inner_rel_tol=0.0)),
              ("inner_rel_tol nan", dict(inner_rel_tol=float("nan"))))


def create_cases(smg):
    """[(name, thunk -> (code, message), holds only without a device)]: the base's checks in its order, then the parameters"""
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
    for name, bad in BAD_PARAMS:
        cases.append(("parameter: " + name, (lambda bad=bad: _create(smg, fake.h, V, F, **bad)), False))
    cases.append(("order: hierarchy before mesh", lambda: _create(smg, keep["blk"].h, Vz, F), False))
    cases.append(("order: mesh before parameters", lambda: _create(smg, fake.h, Vz, F, alpha=2.0), False))
    cases.append(("valid, real hierarchy", lambda: _create(smg, mg.h, V, F), True))
    keep["one"] = smg.mg_precompute(V, F, 0.25, 200, 1)                       # 81 vertices, coarsest level 200: the mesh itself
    assert keep["one"].n_levels == 1
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
    p = L.smg_emd_params_default()
    calls = {"set_solver": lambda: L.smg_emd_set_solver(None, 1), "set_params": lambda: L.smg_emd_set_params(None, C.byref(p)),
             "solve": lambda: L.smg_emd_solve(None, X.ctypes.data, 4, X.ctypes.data, 4, 1, 0, None, 0, dp, dp, None, None, None, 4, None)}
    return [("null object: " + k, (lambda f=f: (f(), L.smg_last_error().decode())), False) for k, f in calls.items()]


def host_twin_cases(smg, call=None, prefix="host twin"):
    """the operand checks smg_emd_host and smg_debug_emd share"""
    call = call or (lambda *a, **k: N.host(smg, *a, **k)[0])
    L = smg._lib.load()
    V, F = N.shape("icosphere1")
    mu0, mu1 = N.pairs(V, F, 1)
    b = mu1 - mu0
    phi, ZU, rho, alpha = N.test_state(V, F, 1)
    J = ZU[:, :, :2]
    Fo = np.array(F)
    Fo[1, 2] = V.shape[0]
    thunks = {
        "unknown op": lambda: call(6, V, F, b=b, phi=phi, state=ZU, rho=rho), "negative op": lambda: call(-1, V, F, b=b, phi=phi, state=ZU, rho=rho),
        "out missing": lambda: call(N.EMD_RHS, V, F, b=b, state=ZU, over=dict(out=None)),
        "V missing": lambda: call(N.EMD_RHS, V, F, b=b, state=ZU, over=dict(V=None)),
        "F missing": lambda: call(N.EMD_RHS, V, F, b=b, state=ZU, over=dict(F=None)),
        "no vertex": lambda: call(N.EMD_RHS, V, F, b=b, state=ZU, over=dict(nV=0)),
        "b missing": lambda: call(N.EMD_RHS, V, F, state=ZU),
        "state missing": lambda: call(N.EMD_RHS, V, F, b=b),
        "phi missing": lambda: call(N.EMD_UPDATE, V, F, state=ZU, rho=rho),
        "rho missing": lambda: call(N.EMD_UPDATE, V, F, phi=phi, state=ZU),
        "gmax missing": lambda: call(N.EMD_DUAL, V, F, b=b, phi=phi, rho=rho),
        "J missing": lambda: call(N.EMD_FLOW, V, F),
        "b missing for the residual": lambda: call(N.EMD_RESIDUAL, V, F, state=J),
        "k zero": lambda: call(N.EMD_RHS, V, F, b=b, state=ZU, k=0),
        "k negative": lambda: call(N.EMD_FLOW, V, F, state=J, k=-2),
        "face index": lambda: call(N.EMD_RHS, V, Fo, b=b, state=ZU),
        "order: operands before k": lambda: call(N.EMD_FLOW, V, F, k=0),
        "order: k before faces": lambda: call(N.EMD_RHS, V, Fo, b=b, state=ZU, k=0),
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
    """every refusal of smg_emd_create, of the calls on a missing object and of the host twin's operand checks, with the code and the
    smg_last_error() text recorded in tests/golden/emd_refusals.json; all of create's come before SMG_ERR_NO_DEVICE, which a valid call meets on a
    box without a GPU.  The refusals that need a live object (group "live") are checked by tests/test_gpu_emd.py.  Every message carries its
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
    assert all(v[1].startswith("smg_emd_create: ") for v in g.values())
    for name, _ in BAD_PARAMS:
        assert name.split()[0] in g["parameter: " + name][1]
    h = golden["host"]
    assert h["host twin: order: operands before k"] == h["host twin: J missing"]
    assert h["host twin: order: k before faces"] == h["host twin: k zero"]
    assert all(v[1].startswith("smg_emd_host: ") for v in h.values())
    for name, (code, msg) in golden["null"].items():
        assert msg.startswith("smg_emd_" + name.split(": ")[1] + ": ")
    for name, (code, msg) in golden["live"].items():
        assert code == INVALID and msg.startswith("smg_emd_" + name.split()[0] + ": "), name
    del keep


def test_hook_refuses_what_the_host_twin_refuses(smg_mod):
    golden = json.load(open(GOLDEN))["host"]
    hook = lambda *a, **k: N.hook(smg_mod, *a, **k)[0]   # noqa: E731
    for name, thunk, _ in host_twin_cases(smg_mod, hook, "hook"):
        rc, msg = thunk()
        want = golden[name.replace("hook: ", "host twin: ")]
        assert [rc, msg] == [want[0], want[1].replace("smg_emd_host", "smg_debug_emd")], name
    if smg_mod._lib.load().smg_device_count() == 0:
        V, F = N.shape("icosphere1")
        assert N.hook(smg_mod, N.EMD_GEOMETRY, V, F)[0] == NO_DEVICE


def test_no_gpu_comes_after_every_argument_check(smg_mod):
    """without a GPU EarthMover(...) raises the no-device error, and only once every argument check has passed"""
    if smg_mod._lib.load().smg_device_count() > 0:
        pytest.skip("a GPU is present")
    V, F = flat_square(8)
    fake = _fake_hierarchy(smg_mod, V.shape[0])
    with pytest.raises(smg_mod.SmgError) as e:
        smg_mod.EarthMover(fake, V, F)
    assert e.value.code == NO_DEVICE and "smg_emd_create" in str(e.value) and "no CPU fallback" in str(e.value)
    with pytest.raises(smg_mod.SmgError) as e:
        smg_mod.EarthMover(fake, V, F, alpha=2.5)
    assert e.value.code == INVALID
    with pytest.raises(TypeError):
        smg_mod.EarthMover(fake, V, F, beta=1.0)


# ---- the host twin against the restatement ---------------------------------------------------------------------------------------------------------
def host_run(smg):
    def run(op, V, F, **kw):
        rc, out = N.host(smg, op, V, F, **kw)
        assert rc == 0
        return out
    return run


@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("name", MESHES + N.PYRAMIDS)
def test_host_twin_against_restatement(smg_mod, name, k):
    """all six ops bit for bit"""
    N.check_launchers(host_run(smg_mod), name, k)


# ---- the restatement itself ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def refs():
    """EmdNp per mesh; built once"""
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = N.EmdNp(*N.shape(name))
        return cache[name]
    return get


def psi_norm(d):
    return np.linalg.norm(d["potential"], axis=0)


@pytest.mark.parametrize("kind", ["deltas", "blobs"])
@pytest.mark.parametrize("name", MESHES)
def test_certificate_and_iteration_counts(refs, name, kind):
    """CERTIFICATE and TABLE of the header: one run to a gap of 1e-3 with a check at every iteration"""
    ref = refs(name)
    mu0, mu1 = getattr(N, kind)(ref.V, ref.F)
    d = ref.solve(mu0, mu1, gap_tol=1e-3, check_every=1, history=True)
    his = d["his"]
    worst = max(float((h[1] - (h[0] + h[2] * h[3])).max()) for h in his)
    gaps = np.array([(h[0][0] - h[1][0]) / h[0][0] for h in his])
    first = int(np.argmax(gaps <= 1e-2)) + 1
    print("%s %s: %d iterations to 1e-2, %d to 1e-3, upper %.6f, lower %.6f; max over the iterations of lower - (upper + res |psi|) = %.3e"
          % (name, kind, first, d["iterations"], d["upper"][0], d["lower"][0], worst))
    assert worst <= 0.0
    assert gaps[first - 1] <= 1e-2 and d["upper"][0] - d["lower"][0] <= 1e-3 * d["upper"][0]
    want = TABLE[(name, kind)]
    assert (first, d["iterations"]) == want[:2] and abs(d["upper"][0] - want[2]) <= 5e-7


@pytest.mark.parametrize("name", ["icosphere1", "torus", "square"])
def test_swap_and_halving(refs, name):
    """SWAP and HALVING of the header, three columns at once"""
    ref = refs(name)
    mu0, mu1 = N.pairs(ref.V, ref.F, 3)
    a = ref.solve(mu0, mu1)
    s = ref.solve(mu1, mu0)
    h = ref.solve(0.5 * mu0, 0.5 * mu1)
    assert a["iterations"] == s["iterations"] == h["iterations"] and a["iterations"] % 10 == 0
    assert np.array_equal(a["upper"], s["upper"]) and np.array_equal(a["lower"], s["lower"]) and np.array_equal(a["potential"], -s["potential"])
    assert np.array_equal(0.5 * a["upper"], h["upper"]) and np.array_equal(0.5 * a["lower"], h["lower"]) and np.array_equal(a["potential"], h["potential"])
    assert np.all(a["upper"] - a["lower"] <= 1e-2 * a["upper"])


def test_flat_square_is_at_least_euclidean(refs):
    """FLAT of the header, on deltas between three pairs of vertices"""
    ref = refs("square")
    V, F, n = ref.V, ref.F, ref.V.shape[0]
    ij = [(1, n // 2), (0, n - 1), (5, 100)]
    mu = [N.deltas(V, F, i, j) for i, j in ij]
    d = ref.solve(np.stack([m[0] for m in mu], axis=1), np.stack([m[1] for m in mu], axis=1), gap_tol=1e-3)
    euclid = np.array([np.linalg.norm(V[i] - V[j]) for i, j in ij])
    slack = d["res_abs"] * psi_norm(d)
    print("square: upper %s, Euclidean %s, res |psi| %s" % (d["upper"], euclid, slack))
    assert np.all(d["upper"] + slack >= euclid) and np.all(d["lower"] <= d["upper"] + slack)


def test_triangle_inequality(refs):
    """TRIANGLE of the header"""
    ref = refs("torus")
    V, F, n = ref.V, ref.F, ref.V.shape[0]
    a, b, c = N.blob(V, F, 1), N.blob(V, F, n // 2), N.blob(V, F, n // 3)
    d = ref.solve(np.stack([a, a, b], axis=1), np.stack([c, b, c], axis=1))
    slack = d["res_abs"] * psi_norm(d)
    print("torus: lower(a, c) %.6f, upper(a, b) %.6f, upper(b, c) %.6f" % (d["lower"][0], d["upper"][1], d["upper"][2]))
    assert d["lower"][0] <= (d["upper"][1] + slack[1]) + (d["upper"][2] + slack[2])


@pytest.mark.parametrize("name", ["icosphere1", "square"])
def test_potential_is_feasible_and_gives_lower(refs, name):
    """POTENTIAL of the header"""
    ref = refs(name)
    mu0, mu1 = N.pairs(ref.V, ref.F, 3)
    d = ref.solve(mu0, mu1)
    g = N.grad2(ref.W2, ref.F, d["potential"])
    gmax = np.sqrt(g[:, :, 0] * g[:, :, 0] + g[:, :, 1] * g[:, :, 1]).max(axis=1)
    print("%s: max |grad potential| - 1 = %s" % (name, gmax - 1.0))
    assert np.all(gmax <= 1.0 + 4 * EPS)
    bp = np.array([N.fixed_sum(t) for t in ((mu1 - mu0) * d["potential"]).T])
    assert np.array_equal(bp, d["lower"])
    assert np.all(d["potential"][0] == 0.0)


def test_warm_start_ends_at_the_first_check(refs):
    """WARM of the header; a cold call after it repeats the first"""
    ref = refs("icosphere1")
    mu0, mu1 = N.pairs(ref.V, ref.F, 2)
    a = ref.solve(mu0, mu1)
    w = ref.solve(mu0, mu1, warm=True)
    c = ref.solve(mu0, mu1)
    assert a["iterations"] > 10 and w["iterations"] == 10
    assert np.all(w["upper"] - w["lower"] <= 1e-2 * w["upper"])
    assert c["iterations"] == a["iterations"] and np.array_equal(c["upper"], a["upper"]) and np.array_equal(c["lower"], a["lower"])


def test_zero_column_and_max_iter(refs):
    """a column with b = 0 returns upper = lower = 0 beside a live one, which it leaves unchanged; reaching max_iter is no error"""
    ref = refs("icosphere1")
    mu0, mu1 = N.pairs(ref.V, ref.F, 1)
    one = ref.solve(mu0, mu1, max_iter=20)
    two = ref.solve(np.concatenate([mu0, mu0], axis=1), np.concatenate([mu1, mu0], axis=1), max_iter=20)
    assert one["iterations"] == two["iterations"] == 20
    assert two["upper"][1] == 0.0 and two["lower"][1] == 0.0 and two["residual"][1] == 0.0
    assert two["upper"][0] == one["upper"][0] and two["lower"][0] == one["lower"][0]


# ---- the kernels' registers, the host maths under sanitizers -------------------------------------------------------------------------------------
def test_kernels_keep_everything_in_registers():
    """the ISA notes of every kernel of smg_emd_device.hip (the build's flags, device side only): no scratch, no spills"""
    import re
    from surface_multigrid_code_amd import build as B
    src = os.path.join(B.CSRC, "smg_emd_device.hip")
    asm = subprocess.check_output([B._hipcc()] + B.FLAGS + ["--cuda-device-only", "-S", src, "-o", "-"], text=True, stderr=subprocess.DEVNULL)
    notes = re.findall(r"\.name:\s+(\S*k_emd\S*)(.*?)\.wavefront_size", asm, flags=re.S)
    assert len(notes) == 6
    for kernel, body in notes:
        field = lambda k: int(re.search(r"\.%s:\s+(\d+)" % k, body).group(1))   # noqa: E731
        print("%s: vgpr_count %d, sgpr_count %d, private_segment_fixed_size %d" % (kernel, field("vgpr_count"), field("sgpr_count"), field("private_segment_fixed_size")))
        assert field("private_segment_fixed_size") == 0 and field("vgpr_spill_count") == 0 and field("sgpr_spill_count") == 0
        assert field("vgpr_count") <= 128


def test_host_maths_under_sanitizers(tmp_path):
    """tests/emd_asan_driver.cpp, a stand-alone program: the host twin's loops (smg::emd_host_* of csrc/smg_emd_inl.hpp, what smg_emd_host runs after
    its checks) on exactly-sized heap arrays, under AddressSanitizer and UndefinedBehaviorSanitizer (static runtimes: run directly, nothing
    preloaded, nothing loaded into python)"""
    exe = str(tmp_path / "emd_asan_driver")
    csrc = os.path.join(ROOT, "surface_multigrid_code_amd", "csrc")
    srcs = [os.path.join(ROOT, "tests", "emd_asan_driver.cpp"), os.path.join(csrc, "smg_mesh.cpp"), os.path.join(csrc, "smg_sparse.cpp")]
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-ffp-contract=off", "-pthread", "-I" + csrc] + srcs + ["-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    run = subprocess.run([exe], env=env, capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0 and run.stdout.count("ok 1") == 9 and "ERROR" not in run.stderr
