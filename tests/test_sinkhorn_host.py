"""CPU: heat-kernel optimal transport on a mesh (include/smg.h: smg_sinkhorn_host) -- the entry point and its refusals, the library's host twin
against the numpy restatement (tests/sinkhorn_np.py), and the restatement itself against the method's properties.

SCALE and SUBSTEP are correctly rounded +, -, *, /, max and abs in one order on both sides: held bit for bit, their sums too.  VALUE and GEOMEAN go
through log and exp: a term is held to 16 eps |term| (VALUE's sums to 16 eps sum |terms|), a barycentre mass to a relative
16 eps (1 + sum_c |alpha_c ln d_c|): the absolute error of an exponent is the relative error of the exponential, and 16 eps is the allowance
tests/test_conformal_host.py gives the library's exp against numpy's.  A new scaling r_v,c = (m mu) / z_eff adds one rounding of the division to
the mass's error: 1.5 times the mass's bound covers it (16 eps / 2 >= eps / 2).

The properties, every quantity computed on the CPU from the restatement (SinkhornNp: direct solves), are in the tests' docstrings; the table is the
one of DESIGN.md section 35: t = (0.05)^2 area, substeps 1, tol 1e-6, a check at every iteration, emd_np.blob at the vertices 1 and nV / 2, the
three columns (mu0, mu1), (mu0, mu0), (mu1, mu1) of the debiased call."""
import json
import os
import subprocess

import numpy as np
import pytest

import sinkhorn_np as N
from test_geodesics_host import flat_square

INVALID = -1
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sinkhorn_refusals.json")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = N.EPS

# mesh: (iterations to 1e-6, value, debiased value (None: not recorded), iterations of the five blends to a change of 1e-6)
TABLE = {"icosphere3": (10, 0.97827471, 0.89573623, 8), "regular12": (24, 0.12301820, 0.09902626, 11), "bunny.smgm": (82, None, None, None)}


# ---- the ABI and its refusals --------------------------------------------------------------------------------------------------------------------
def test_abi_present(smg_mod):
    L = smg_mod._lib.load()
    assert hasattr(L, "smg_sinkhorn_host")
    assert L.smg_version() >= 551
    assert (N.SK_SCALE, N.SK_SUBSTEP, N.SK_VALUE, N.SK_GEOMEAN) == (0, 1, 2, 3)


def host_twin_cases(smg, call=None, prefix="host twin"):
    """the operand checks of smg_sinkhorn_host"""
    call = call or (lambda *a, **k: N.host(smg, *a, **k)[0])
    L = smg._lib.load()
    V, F = N.shape("icosphere1")
    mu0, mu1 = N.pairs(V, F, 2)
    y, r = N.test_state(V, F, 2)
    sr, al = N.sums(r.T), np.array([[0.25, 0.75]])
    Fo = np.array(F)
    Fo[1, 2] = V.shape[0]
    S, G = N.SK_SCALE, N.SK_GEOMEAN
    thunks = {
        "unknown op": lambda: call(4, V, F, k=2, kin=2, y=y, r=r, mu=mu0, sr=sr), "negative op": lambda: call(-1, V, F, k=2, kin=2, y=y, r=r, mu=mu0, sr=sr),
        "out missing": lambda: call(S, V, F, k=2, kin=2, y=y, r=r, mu=mu0, sr=sr, over=dict(out=None)),
        "V missing": lambda: call(S, V, F, k=2, kin=2, y=y, r=r, mu=mu0, sr=sr, over=dict(V=None)),
        "F missing": lambda: call(S, V, F, k=2, kin=2, y=y, r=r, mu=mu0, sr=sr, over=dict(F=None)),
        "no vertex": lambda: call(S, V, F, k=2, kin=2, y=y, r=r, mu=mu0, sr=sr, over=dict(nV=0)),
        "y missing": lambda: call(N.SK_SUBSTEP, V, F, k=2),
        "r missing": lambda: call(S, V, F, k=2, kin=2, y=y, mu=mu0, sr=sr),
        "mu missing": lambda: call(S, V, F, k=2, kin=2, y=y, r=r, sr=sr),
        "sr missing": lambda: call(S, V, F, k=2, kin=2, y=y, r=r, mu=mu0),
        "mu1 missing": lambda: call(N.SK_VALUE, V, F, k=2, y=y, r=r, mu=mu0),
        "alphas missing": lambda: call(G, V, F, k=1, kin=2, y=y, r=r, mu=mu0[:, :1], sr=sr),
        "k zero": lambda: call(N.SK_SUBSTEP, V, F, k=0, y=y),
        "k_in zero": lambda: call(G, V, F, k=1, kin=0, y=y, r=r, mu=mu0[:, :1], sr=sr, alphas=al),
        "floor negative": lambda: call(S, V, F, k=2, kin=2, y=y, r=r, mu=mu0, sr=sr, floor=-1.0),
        "floor nan": lambda: call(G, V, F, k=1, kin=2, y=y, r=r, mu=mu0[:, :1], sr=sr, alphas=al, floor=float("nan")),
        "face index": lambda: call(N.SK_SUBSTEP, V, Fo, k=2, y=y),
        "order: operands before k": lambda: call(N.SK_SUBSTEP, V, F, k=0),
        "order: k before faces": lambda: call(N.SK_SUBSTEP, V, Fo, k=0, y=y),
    }
    return [("%s: %s" % (prefix, k), (lambda f=f: (f(), L.smg_last_error().decode())), False) for k, f in thunks.items()]


def check_cases(smg, cases, golden):
    seen = set()
    for name, thunk, device_only in cases:
        rc, msg = thunk()
        seen.add(name)
        assert [rc, msg] == golden[name], name
        assert rc == INVALID, name
    return seen


def test_refusals_keep_code_and_message(smg_mod):
    """every refusal of the host twin's operand checks, with the code and the smg_last_error() text recorded in
    tests/golden/sinkhorn_refusals.json; the checks run in the contract's order and every message carries the entry point's name"""
    golden = json.load(open(GOLDEN))
    assert check_cases(smg_mod, host_twin_cases(smg_mod), golden["host"]) == set(golden["host"])
    h = golden["host"]
    assert h["host twin: order: operands before k"] == h["host twin: y missing"]
    assert h["host twin: order: k before faces"] == h["host twin: k zero"]
    assert all(v[1].startswith("smg_sinkhorn_host: ") for v in h.values())


# ---- the host twin against the restatement ---------------------------------------------------------------------------------------------------------
def host_run(smg):
    def run(op, V, F, **kw):
        rc, out = N.host(smg, op, V, F, **kw)
        assert rc == 0
        return out
    return run


@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("name", N.LAUNCHER_MESHES + N.PYRAMIDS)
def test_host_twin_against_restatement(smg_mod, name, k):
    """all four ops with the bounds of the header; k_in = 1, 2, 3 and G = 1, 5; zero masses (column 1) and a zero alpha among the inputs"""
    for kin, G in ((1, 1), (2, 5), (3, 1), (3, 5)):
        N.check_launchers(host_run(smg_mod), name, k, kin, G)


def test_host_twin_without_floor_gives_non_finite_scalings(smg_mod):
    """kernel_floor = 0 on a block with non-positive entries gives infinite scalings and non-finite sums; the floor keeps all of them finite"""
    V, F = N.shape("icosphere1")
    n = V.shape[0]
    y, r = N.test_state(V, F, 1)
    mu = N.pairs(V, F, 1)[0]
    assert np.any(y <= 0.0)
    out = host_run(smg_mod)(N.SK_SCALE, V, F, k=1, kin=1, y=y, r=r, mu=mu, sr=N.sums(r.T), floor=0.0)
    rn, _, _, srn, _, tot = N.unpack(N.SK_SCALE, out, n, 1, 1)
    assert np.all(np.isinf(rn[(y <= 0.0) & (mu > 0.0)])) and not np.isfinite(srn[0]) and not np.isfinite(tot)
    out = host_run(smg_mod)(N.SK_SCALE, V, F, k=1, kin=1, y=y, r=r, mu=mu, sr=N.sums(r.T), floor=1e-10)
    assert np.all(np.isfinite(out))


# ---- the restatement itself ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def refs():
    """SinkhornNp per (mesh, floor); built once"""
    cache = {}

    def get(name, floor=0.0, **kw):
        key = (name, floor, tuple(sorted(kw.items())))
        if key not in cache:
            cache[key] = N.SinkhornNp(*N.shape(name), kernel_floor=floor, **kw)
        return cache[key]
    return get


def blob_pair(ref):
    n = ref.V.shape[0]
    return N.blob(ref.V, ref.F, 1)[:, None], N.blob(ref.V, ref.F, n // 2)[:, None]


@pytest.mark.parametrize("floor", [0.0, 1e-10])
@pytest.mark.parametrize("name", list(TABLE))
def test_table(refs, name, floor):
    """the table of the header: the counts with and without the floor; the 8-digit values are those of kernel_floor = 0 and asserted there alone
    (the floor moves them by up to 2e-8)"""
    ref = refs(name, floor)
    mu0, mu1 = blob_pair(ref)
    deb, d = ref.debiased(mu0, mu1, check_every=1)
    count, value, debiased, _ = TABLE[name]
    print("%s floor %g: %d iterations, value %.8f, debiased %.8f, e0 %s" % (name, floor, d["iterations"], d["value"][0], deb[0], d["marginal_err"]))
    assert d["iterations"] == count
    assert np.all(d["marginal_err"] <= 1e-6 * 1.0000001)
    if value is not None:
        bound = 5e-9 if floor == 0.0 else 5e-9 + 2e-8
        assert abs(d["value"][0] - value) <= bound and abs(deb[0] - debiased) <= bound


@pytest.mark.parametrize("name", ["icosphere3", "regular12"])
def test_blend_counts_and_mass(refs, name):
    """five blends at 0, 1/4, 1/2, 3/4, 1 reach a change of 1e-6 in the table's count; every barycentre has mass 1 to 1e-12"""
    ref = refs(name, 1e-10)
    mu0, mu1 = blob_pair(ref)
    b = ref.interpolate(mu0[:, 0], mu1[:, 0], [0.0, 0.25, 0.5, 0.75, 1.0], check_every=1)
    print("%s: %d iterations, mass - 1 %s" % (name, b["iterations"], b["mass"] - 1.0))
    assert b["iterations"] == TABLE[name][3]
    assert np.all(np.abs(b["mass"] - 1.0) <= 1e-12) and np.all(np.abs(b["bary"].sum(axis=0) - 1.0) <= 1e-12)


@pytest.mark.parametrize("name,want", [("icosphere3", 8), ("regular12", 12)])
def test_blend_counts_in_the_largest_density_change(refs, name, want):
    """the counts 8 and 12 recorded with the method's prototype are those of another measure: the first iteration at which the largest change of the
    density, max_i |mu - previous|, is <= 1e-6.  The contract's measure, sum_i |m mu - previous| against tol times the mass, gives 8 and 11
    (test_blend_counts_and_mass); on the grid the two differ at iteration 11 (3.8e-7 in the sum, above 1e-6 in the largest density change)"""
    ref = refs(name, 1e-10)
    mu0, mu1 = blob_pair(ref)
    his = ref.interpolate(mu0[:, 0], mu1[:, 0], [0.0, 0.25, 0.5, 0.75, 1.0], n_iter=14)["his"]
    dens = np.array([h[1].max() for h in his])
    print("%s: largest density change per iteration %s" % (name, dens))
    assert 1 + int(np.argmax(dens <= 1e-6)) == want


@pytest.mark.parametrize("name", ["icosphere1", "icosphere3", "regular12", "bunny.smgm"])
def test_clamped_matrix(refs, name):
    """the clamped S has no positive off-diagonal and S 1 = m to rounding"""
    ref = refs(name)
    S = ref.S.tocoo()
    off = S.row != S.col
    assert np.all(S.data[off] <= 0.0)
    one = np.asarray(ref.S @ np.ones(ref.m.size)).ravel()
    scale = np.abs(ref.S).sum(axis=1).A1 if hasattr(np.abs(ref.S).sum(axis=1), "A1") else np.asarray(np.abs(ref.S).sum(axis=1)).ravel()
    assert np.all(np.abs(one - ref.m) <= 8 * EPS * scale)


@pytest.mark.parametrize("name", ["icosphere1", "regular4"])
def test_dense_kernel_is_symmetric_and_positive(refs, name):
    ref = refs(name)
    H = np.linalg.inv(ref.S.toarray())
    print("%s: min of S^-1 %.3e, asymmetry %.3e" % (name, H.min(), np.abs(H - H.T).max()))
    assert H.min() > 0.0 and np.abs(H - H.T).max() <= 64 * EPS * np.abs(H).max()


def test_negative_edge_counts():
    """the negative edges of the issue's meshes: none on the icosphere, the torus and the regular grid (whose lowest weight is rounding of
    cot 90 degrees), 6 on the bunny, 70 on the jittered square"""
    import scipy.sparse as sp
    from oracle import mesh_np as M
    for name, want in (("icosphere3", 0), ("torus", 0), ("regular12", 0), ("bunny.smgm", 6)):
        V, F = N.shape(name)
        assert N.clamped(sp.csr_matrix(-M.cotmatrix(V, F)))[1] == want, name
    V, F = flat_square(12)
    _, count, wmin = N.clamped(sp.csr_matrix(-M.cotmatrix(V, F)))
    assert count == 70 and wmin < 0.0
    Vr, Fr = N.shape("regular12")
    assert -1e-15 < N.clamped(sp.csr_matrix(-M.cotmatrix(Vr, Fr)))[2] <= 0.0


def test_jittered_square_needs_clamping(refs):
    """on the jittered flat_square(12) clamp_weights = 0 is refused; with clamping 70 edges are clamped and the table-style run converges"""
    V, F = flat_square(12)
    with pytest.raises(ValueError):
        N.SinkhornNp(V, F, clamp_weights=0)
    ref = N.SinkhornNp(V, F, kernel_floor=0.0)
    assert ref.n_clamped == 70
    mu0, mu1 = blob_pair(ref)
    deb, d = ref.debiased(mu0, mu1, check_every=1)
    print("jittered square: %d iterations, value %.8f, debiased %.8f" % (d["iterations"], d["value"][0], deb[0]))
    assert d["iterations"] < 500 and np.all(d["marginal_err"] <= 1e-6) and np.all(np.isfinite(d["value"]))


@pytest.mark.parametrize("s", [1, 2])
@pytest.mark.parametrize("name", ["icosphere3", "regular12"])
def test_half_steps_hold_their_marginal(refs, name, s):
    """after each half step the updated marginal holds to rounding: r_v K(r_w)_eff = mu0 and r_w K(r_v)_eff = mu1, with direct solves"""
    ref = refs(name, 1e-10, substeps=s)
    mu0, mu1 = (np.ascontiguousarray(x) for x in N.pairs(ref.V, ref.F, 3))
    d3, d = ref.distance(mu0, mu1, n_iter=3), ref.distance(mu0, mu1, n_iter=4)
    rv, rw = d["r_v"], d["r_w"]
    # a run of n iterations ends with r_v's update: r_v against the kernel of r_w; r_w is a half step older: against the kernel of the r_v before
    assert np.all(np.abs(rv * ref.apply(rw) - mu0) <= 4 * EPS * mu0)
    assert np.all(np.abs(rw * ref.apply(d3["r_v"]) - mu1) <= 4 * EPS * mu1)
    assert np.all(rv[mu0 == 0.0] == 0.0) and np.all(rw[mu1 == 0.0] == 0.0) and np.any(mu0 == 0.0)


def test_value_is_symmetric_and_debias_of_equal_inputs_is_zero(refs):
    """value(mu0, mu1) and value(mu1, mu0) agree to 10 tol of the larger magnitude; the debiased value of (a, a) is exactly 0"""
    ref = refs("icosphere3", 1e-10)
    mu0, mu1 = blob_pair(ref)
    a, b = ref.distance(mu0, mu1), ref.distance(mu1, mu0)
    big = max(abs(a["value"][0]), abs(b["value"][0]))
    print("value %.10f against swapped %.10f" % (a["value"][0], b["value"][0]))
    assert abs(a["value"][0] - b["value"][0]) <= 10 * 1e-6 * big
    deb, _ = ref.debiased(mu0, mu0)
    assert deb[0] == 0.0


def test_blend_centroids_move_along_the_great_circle(refs):
    """blend centroids on icosphere(3) at 0, 1/4, 1/2, 3/4, 1: the fractions of the way increase, the half-way one is in [0.49, 0.51] (the
    prototype: 0.4999), and every centroid lies on the great circle through the endpoints' centroids to 1e-3 rad"""
    ref = refs("icosphere3", 1e-10)
    mu0, mu1 = blob_pair(ref)
    b = ref.interpolate(mu0[:, 0], mu1[:, 0], [0.0, 0.25, 0.5, 0.75, 1.0])
    cen = b["bary"].T @ ref.V
    cen = cen / np.linalg.norm(cen, axis=1)[:, None]
    a, c = cen[0], cen[-1]
    normal = np.cross(a, c)
    normal /= np.linalg.norm(normal)
    total = np.arccos(np.clip(a @ c, -1.0, 1.0))
    frac = np.array([np.arctan2(np.cross(a, p) @ normal, a @ p) for p in cen]) / total
    off = np.abs(np.arcsin(np.clip(cen @ normal, -1.0, 1.0)))
    print("fractions %s, off the great circle %s rad" % (frac, off))
    assert np.all(np.diff(frac) > 0.0) and 0.49 <= frac[2] <= 0.51 and np.all(off <= 1e-3)


# ---- the kernels' registers, the host maths under sanitizers -------------------------------------------------------------------------------------
def test_host_maths_under_sanitizers(tmp_path):
    """tests/sinkhorn_asan_driver.cpp, a stand-alone program: the host twin's loops (smg::sinkhorn_host_* of csrc/smg_sinkhorn_inl.hpp, what
    smg_sinkhorn_host runs after its checks) on exactly-sized heap arrays, under AddressSanitizer and UndefinedBehaviorSanitizer (static runtimes:
    run directly, nothing preloaded, nothing loaded into python)"""
    exe = str(tmp_path / "sinkhorn_asan_driver")
    csrc = os.path.join(ROOT, "surface_multigrid_code_amd", "csrc")
    srcs = [os.path.join(ROOT, "tests", "sinkhorn_asan_driver.cpp"), os.path.join(csrc, "smg_mesh.cpp"), os.path.join(csrc, "smg_sparse.cpp")]
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-ffp-contract=off", "-pthread", "-I" + csrc] + srcs + ["-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    run = subprocess.run([exe], env=env, capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0 and run.stdout.count("ok 1") == 8 and "ERROR" not in run.stderr
