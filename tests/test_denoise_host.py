"""CPU: feature-preserving denoising (include/smg.h: smg_denoise_*) -- the ABI and its refusals without a GPU, smg_mesh_face_neighbours against
a set-based build, the library's host twin of the per-face maths (smg_denoise_faces_host) against the numpy restatement written from the
formulas (tests/denoise_np.py, direct solves), and the restatement itself: descent of the energy and the normal error on the noisy cube.

The bounds.  The rest constants, the spacing terms and the projection are correctly rounded +, -, *, / and sqrt in one order on both sides: the
host twin measured 0 against numpy on every shape, and they are held bit for bit.  The filter calls exp (numpy's and libm's differ in the last
bit): measured on the host twin over the kernel shapes 1.00 eps after 1 iteration and 5.50 eps after 5 (ogre_sim), so by the project's rule
(100 x the measured maximum, rounded up to a power of ten) FILTER_BOUND = 1e2 eps and 1e3 eps; tests/test_gpu_denoise.py holds the device to
the same two numbers."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import denoise_np as N
from test_arap_host import _fake_hierarchy
from test_geodesics_host import flat_square

INVALID, NO_DEVICE = -1, -2
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "denoise_refusals.json")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = N.EPS
FILTER_BOUND = {1: 1e2, 5: 1e3}          # eps, on the components of unit normals, after that many iterations
KERNEL_SHAPES = ["strip63", "strip64", "strip65", "fan65", "tetrahedron", "square", "ogre_sim"]


def kernel_shapes():
    """label -> (V, F): strips at the wave and block edges, the fan (rows of 64), the tetrahedron (rows of 3), two triangles, ogre_sim with noise"""
    out = {"strip63": N.strip(63), "strip64": N.strip(64), "strip65": N.strip(65), "fan65": N.fan(65), "tetrahedron": N.tetrahedron(),
           "square": N.square2()}
    V, F = N.load_mesh("ogre_sim.smgm")
    out["ogre_sim"] = (N.noisy(V, F), F)
    return out


@pytest.fixture(scope="module")
def shapes():
    return kernel_shapes()


# ---- the ABI and its refusals --------------------------------------------------------------------------------------------------------------------
DN_SYMBOLS = ("smg_denoise_params_default", "smg_denoise_create", "smg_denoise_destroy", "smg_denoise_device_bytes", "smg_denoise_set_solver",
              "smg_denoise_sigma_s", "smg_denoise_set_filter", "smg_denoise_filter", "smg_denoise_update", "smg_denoise_run", "smg_denoise_faces_host",
              "smg_debug_denoise", "smg_mesh_face_neighbours")


def test_abi_present(smg_mod):
    L = smg_mod._lib.load()
    for name in DN_SYMBOLS:
        assert hasattr(L, name)
    assert hasattr(smg_mod, "Denoiser") and hasattr(smg_mod, "denoise_params")
    assert L.smg_version() >= 512
    p = smg_mod.denoise_params()
    assert (p.sigma_s, p.sigma_r, p.fidelity, p.normal_iters) == (0.0, 0.35, 1.0, 20)
    assert L.smg_denoise_device_bytes(None) == 0 and L.smg_denoise_sigma_s(None) == 0.0
    X = np.zeros(3)
    for rc in (L.smg_denoise_set_solver(None, 1), L.smg_denoise_set_filter(None, 0.0, 0.0, -1), L.smg_denoise_filter(None, None, 0, None),
               L.smg_denoise_update(None, None, 0, 1, 0.0, None, X.ctypes.data, None, None, None),
               L.smg_denoise_run(None, 0, 1, 0.0, None, X.ctypes.data, None, None, None)):
        assert rc == INVALID


def _create(smg, h, V, F, nV=None, null=None, **params):
    """smg_denoise_create -> (code, message); a successful create is destroyed at once"""
    L = smg._lib.load()
    ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
    V, F = np.ascontiguousarray(V, dtype=np.float64), np.ascontiguousarray(F, dtype=np.int32)
    par = N.params_c(smg, **params)
    out = C.c_void_p(0xdead)
    rc = L.smg_denoise_create(None if null == "h" else h, None if null == "V" else V.ctypes.data_as(dp), V.shape[0] if nV is None else nV,
                              None if null == "F" else F.ctypes.data_as(ip), F.shape[0], None if null == "p" else C.byref(par),
                              None if null == "out" else C.byref(out))
    if rc == 0:
        L.smg_denoise_destroy(out)
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
    cases = [("null %s" % a, (lambda a=a: _create(smg, mg.h, V, F, null=a)), False) for a in ("h", "V", "F", "p", "out")]
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
    for field in ("sigma_r", "fidelity"):
        for tag, bad in (("zero", 0.0), ("negative", -1.0), ("nan", np.nan), ("inf", np.inf)):
            cases.append(("%s %s" % (field, tag), lambda field=field, bad=bad: _create(smg, fake.h, V, F, **{field: bad}), False))
    for tag, bad in (("nan", np.nan), ("inf", np.inf), ("-inf", -np.inf)):
        cases.append(("sigma_s %s" % tag, lambda bad=bad: _create(smg, fake.h, V, F, sigma_s=bad), False))
    cases.append(("normal_iters negative", lambda: _create(smg, fake.h, V, F, normal_iters=-1), False))
    # the object's own checks come in this order: sigma_r, fidelity, sigma_s, normal_iters; all after the mesh's
    cases.append(("order: sigma_r before fidelity", lambda: _create(smg, fake.h, V, F, sigma_r=0.0, fidelity=0.0), False))
    cases.append(("order: fidelity before sigma_s", lambda: _create(smg, fake.h, V, F, fidelity=-1.0, sigma_s=np.nan, normal_iters=-1), False))
    cases.append(("order: sigma_s before normal_iters", lambda: _create(smg, fake.h, V, F, sigma_s=np.inf, normal_iters=-1), False))
    cases.append(("order: mesh before params", lambda: _create(smg, fake.h, Vz, F, sigma_r=0.0), False))
    cases.append(("valid, real hierarchy", lambda: _create(smg, mg.h, V, F), True))
    cases.append(("valid, sigma_s given, no iterations, fake hierarchy", lambda: _create(smg, fake.h, V, F, sigma_s=0.1, normal_iters=0), True))
    return cases, keep


def test_create_refusals_keep_code_and_message(smg_mod):
    """every refusal of smg_denoise_create, with the code and the smg_last_error() text recorded in tests/golden/denoise_refusals.json; all of
    them come before SMG_ERR_NO_DEVICE, which a valid call meets on a box without a GPU"""
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
    own = ("sigma_r zero", "fidelity zero", "sigma_s nan", "normal_iters negative")
    assert len({golden[k][1] for k in own}) == len(own)                                          # each has its own message
    assert golden["order: sigma_r before fidelity"] == golden["sigma_r zero"] and golden["order: fidelity before sigma_s"] == golden["fidelity negative"]
    assert golden["order: sigma_s before normal_iters"] == golden["sigma_s inf"] and golden["order: mesh before params"] == golden["zero area"]
    del keep


def test_host_twin_hook_and_utility_refusals(smg_mod):
    V, F = flat_square(4)
    n, nF = V.shape[0], F.shape[0]
    m = np.tile([0.0, 0.0, 1.0], (nF, 1)).T.reshape(-1)
    L = smg_mod._lib.load()
    for call in (lambda *a, **k: N.faces_host(smg_mod, *a, **k)[0], lambda *a, **k: N.hook(smg_mod, *a, **k)[0]):
        assert call(N.DN_REST, n, F, None, n_out=10 * nF) == INVALID                       # V0 missing
        assert call(N.DN_REST, n, F, V, n_out=0) == INVALID                                # out missing
        assert call(-1, n, F, V, n_out=10 * nF) == INVALID
        assert call(N.DN_FILTER, n, F, V, None, None, n_out=3 * nF, sigma_s=0.1) == INVALID   # the normals missing
        assert call(N.DN_FILTER, n, F, V, None, m, n_out=3 * nF, sigma_s=0.0) == INVALID      # the rule is the object's: the filter takes sigma_s > 0
        assert call(N.DN_FILTER, n, F, V, None, m, n_out=3 * nF, sigma_s=0.1, normal_iters=-1) == INVALID
        assert call(N.DN_PROJECT, n, F, V, None, m, n_out=10 * nF) == INVALID               # the pose missing
        assert call(N.DN_PROJECT, n, F, V, V, None, n_out=10 * nF) == INVALID
        for bad in (n, -1):                                                                 # a face index out of range
            Fo = F.copy()
            Fo[2, 1] = bad
            assert call(N.DN_REST, n, Fo, V, n_out=10 * nF) == INVALID
    assert N.faces_host(smg_mod, N.DN_RHS, n, F, V, V, m, n_out=6 * n)[0] == INVALID        # the twin ends at the per-face pieces
    assert N.hook(smg_mod, N.DN_ENERGY + 1, n, F, V, n_out=1)[0] == INVALID
    assert N.hook(smg_mod, N.DN_RHS, n, F, V, None, None, n_out=6 * n)[0] == INVALID
    assert N.hook(smg_mod, N.DN_ENERGY, n, F, None, None, None, n_out=1)[0] == INVALID
    if L.smg_device_count() == 0:
        assert N.hook(smg_mod, N.DN_REST, n, F, V, n_out=10 * nF)[0] == NO_DEVICE
        assert N.hook(smg_mod, N.DN_ENERGY, n, F, None, None, np.zeros(nF + n), n_out=1)[0] == NO_DEVICE
    ip = C.POINTER(C.c_int)
    Fi = np.ascontiguousarray(F, dtype=np.int32)
    assert L.smg_mesh_face_neighbours(None, nF, n, None, None) == INVALID and L.smg_mesh_face_neighbours(Fi.ctypes.data_as(ip), 0, n, None, None) == INVALID
    assert L.smg_mesh_face_neighbours(Fi.ctypes.data_as(ip), nF, int(F.max()), None, None) == INVALID and b"out of range" in L.smg_last_error()


# ---- the neighbourhoods --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ogre.smgm", "bunny.smgm", "tetrahedron", "fan65"])
def test_face_neighbours_against_sets(smg_mod, name):
    V, F = {"tetrahedron": N.tetrahedron, "fan65": N.fan}[name]() if "." not in name else N.load_mesh(name)
    nV = V.shape[0]
    ptr, idx = N.lib_neighbours(smg_mod, F, nV)
    wp, wi = N.face_neighbours(F, nV)
    assert np.array_equal(ptr, wp) and np.array_equal(idx, wi)
    ln = np.diff(ptr)
    print(name, "nF = %d, entries %d, rows %d .. %d" % (F.shape[0], idx.size, ln.min(), ln.max()))
    if name == "tetrahedron":
        assert np.all(ln == 3)
    if name == "fan65":
        assert np.all(ln == 64)
    if name == "bunny.smgm":                                                                # has boundary
        from oracle import mesh_np as M
        assert len(M.boundary_loop(F)) > 0
    for f in range(0, F.shape[0], max(1, F.shape[0] // 500)):                               # ascending, duplicate-free, without f
        row = idx[ptr[f]:ptr[f + 1]]
        assert np.all(np.diff(row) > 0) and f not in row


# ---- the host twin against the restatement -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", KERNEL_SHAPES)
def test_host_twin_against_restatement(smg_mod, shapes, name):
    V, F = shapes[name]
    nV, nF = V.shape[0], F.shape[0]
    r = N.rest_constants(V, F)
    ptr, idx = N.face_neighbours(F, nV)
    slots = N.row_slots(ptr, idx)
    rc, out = N.faces_host(smg_mod, N.DN_REST, nV, F, V, n_out=10 * nF)
    rl = out.reshape(10, nF).T
    print(name, "rest planes: max error %.2e of the largest entry of the face" % (np.abs(rl - r).max(axis=1) / np.abs(r).max(axis=1)).max())
    assert rc == 0 and np.array_equal(rl, r)
    assert np.all(np.abs(np.sqrt(np.sum(r[:, :3] ** 2, axis=1)) - 1.0) <= 4 * EPS) and np.all(r[:, 3] > 0)
    rc, sp_ = N.faces_host(smg_mod, N.DN_SPACING, nV, F, V, n_out=nF)
    assert rc == 0 and np.array_equal(sp_, N.spacing_terms(r, slots))
    sigma_s = N.sigma_s_rule(r, ptr, slots)
    for iters in (0, 1, 5):
        rc, mo = N.faces_host(smg_mod, N.DN_FILTER, nV, F, V, None, r[:, :3].T.reshape(-1), n_out=3 * nF, sigma_s=sigma_s, normal_iters=iters)
        mo = mo.reshape(3, nF).T
        mn = N.filter_normals(r, slots, r[:, :3], sigma_s, N.DEFAULTS["sigma_r"], iters)
        err = np.abs(mo - mn).max() / EPS
        print("  filter, %d iterations: max |m - m_np| = %.2f eps" % (iters, err))
        assert rc == 0 and (np.array_equal(mo, r[:, :3]) if iters == 0 else err <= FILTER_BOUND[iters])
    X = V + 0.05 * N.mean_edge(V, F) * np.random.default_rng(7).standard_normal(V.shape)
    rc, po = N.faces_host(smg_mod, N.DN_PROJECT, nV, F, V, X, mo.T.reshape(-1), n_out=10 * nF)
    po = po.reshape(10, nF)
    et, share, big = N.project(r, F, X, mo)
    print("  projection: max share error %.2e of the largest term of the face" % (np.abs(po[1:].T - share).max(axis=1) / big).max())
    assert rc == 0 and np.array_equal(po[0], et) and np.array_equal(po[1:].T, share)
    # t is orthogonal to m: the three shares of a face sum to zero, and each is orthogonal to m to rounding
    assert np.all(np.abs(share[:, :3] + share[:, 3:6] + share[:, 6:]) <= 8 * EPS * big[:, None])


def test_weights_assemble_the_cotangent_matrix(shapes):
    """sum_f sum_k w_fk (e_i - e_j)(e_i - e_j)^T = -L: the quadratic part of E is the matrix smg_assemble gives (bound 1e-13 of max |L|)"""
    import scipy.sparse as sp
    from oracle import mesh_np as M
    V, F = shapes["ogre_sim"]
    r = N.rest_constants(V, F)
    I, J, W = [], [], []
    for k in range(3):
        i, j, w = F[:, (k + 1) % 3], F[:, (k + 2) % 3], r[:, 7 + k]
        I += [i, j, i, j]
        J += [i, j, j, i]
        W += [w, w, -w, -w]
    K = sp.coo_matrix((np.concatenate(W), (np.concatenate(I), np.concatenate(J))), shape=(V.shape[0],) * 2).tocsr()
    L = M.cotmatrix(V, F).tocsr()
    err = abs(K + L).max() / abs(L).max()
    print("|sum w d d^T + L| / max |L| = %.2e" % err)
    assert err <= 1e-13


def test_hand_made_rows(smg_mod):
    """face 0 of the mirrored triple has two neighbours of equal weight: with opposite normals the sum is zero and m_0 stays, bit for bit; a field
    of one normal is a fixed point; no iteration returns the input bits"""
    V, F = N.mirrored_triple()
    nF = F.shape[0]
    r = N.rest_constants(V, F)
    ptr, idx = N.lib_neighbours(smg_mod, F, V.shape[0])
    assert list(ptr) == [0, 2, 3, 4] and list(idx) == [1, 2, 0, 0]
    assert r[1, 3] == r[2, 3] and N.dist2(r[:1, 4:7], r[1:2, 4:7]) == N.dist2(r[:1, 4:7], r[2:3, 4:7])
    run = lambda m, iters: N.faces_host(smg_mod, N.DN_FILTER, V.shape[0], F, V, None, m.T.reshape(-1), n_out=3 * nF, sigma_s=1.5,   # noqa: E731
                                        normal_iters=iters)[1].reshape(3, nF).T
    m_in = np.array([[0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [-1.0, 0.0, 0.0]])
    out = run(m_in, 1)
    assert np.array_equal(out[0], m_in[0]) and np.array_equal(out[1], [0.0, 0.0, 1.0]) and np.array_equal(out[2], [0.0, 0.0, 1.0])
    assert np.array_equal(out, N.filter_once(r, N.row_slots(ptr, idx), m_in, 1.5, 0.35))
    m_skew = np.array([[0.0, -0.6, 0.8], [1.0, 0.0, 0.0], [-1.0, 0.0, 0.0]])                 # any m_0 orthogonal to the pair
    assert np.array_equal(run(m_skew, 1)[0], m_skew[0])
    same = np.tile([0.0, 1.0, 0.0], (nF, 1))
    assert np.array_equal(run(same, 3), same)
    tilted = np.tile([0.6, 0.0, 0.8], (nF, 1))
    assert np.all(np.abs(run(tilted, 3) - tilted) <= 2 * EPS)
    odd = np.array([[0.6, 0.8, 0.0], [0.0, 0.28, 0.96], [1.0, 0.0, 0.0]])
    assert np.array_equal(run(odd, 0), odd)


# ---- the restatement itself --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cube", "ogre.smgm"])
def test_energy_never_rises_with_direct_solves(name):
    D, Vn, F, m, X, E = N.reference_run(name)
    print(name, "sigma_s = %.6f" % D.sigma_s, np.array2string(E, precision=6))
    assert np.all(np.isfinite(E)) and np.all(E[1:] <= E[:-1])


def test_normal_error_on_the_noisy_cube():
    """the mean angle between the result's face normals and the clean ones is at most 1 / 4 of the noisy mesh's; the figures of the method's
    prototype: 25.0 degrees noisy, 2.4 filtered, 3.1 after the update, ratio 0.124, E = 0.590, 0.0236, 0.0114, ..., 0.00288"""
    D, Vn, F, m, X, E = N.reference_run("cube")
    Vc = np.asarray(N.cube(4)[0])
    assert Vn.shape == (1538, 3) and F.shape == (3072, 3)
    clean = N.rest_constants(Vc, F)[:, :3]
    noisy_err, out_err = N.normal_error_deg(Vn, F, clean), N.normal_error_deg(X, F, clean)
    filt_err = float(np.degrees(np.mean(np.arccos(np.clip(np.sum(m * clean, axis=1), -1.0, 1.0)))))
    print("noisy %.2f, filtered %.2f, after the update %.2f degrees: ratio %.3f" % (noisy_err, filt_err, out_err, out_err / noisy_err))
    assert out_err <= 0.25 * noisy_err
    assert abs(noisy_err - 25.0) <= 0.1 and abs(filt_err - 2.45) <= 0.05 and abs(out_err / noisy_err - 0.124) <= 0.002
    for t, want in ((0, 0.591), (1, 0.0236), (2, 0.0114), (10, 0.00288)):
        assert abs(E[t] / want - 1.0) <= 5e-3


# ---- the kernels' registers, the host maths under sanitizers -------------------------------------------------------------------------------------
def test_kernels_keep_everything_in_registers():
    """the ISA notes of the four kernels (the build's flags, device side only): no scratch, no spills"""
    from surface_multigrid_code_amd import build as B
    src = os.path.join(B.CSRC, "smg_denoise_device.hip")
    asm = subprocess.check_output([B._hipcc()] + B.FLAGS + ["--cuda-device-only", "-S", src, "-o", "-"], text=True)
    for kernel in ("k_denoise_rest", "k_denoise_spacing", "k_denoise_filter", "k_denoise_project"):
        notes = re.findall(r"\.name:\s+(\S*%s\S*)(.*?)\.wavefront_size" % kernel, asm, flags=re.S)
        assert len(notes) == 1
        body = notes[0][1]
        field = lambda k: int(re.search(r"\.%s:\s+(\d+)" % k, body).group(1))   # noqa: E731
        print("%s: vgpr_count %d, sgpr_count %d, private_segment_fixed_size %d, vgpr_spill_count %d"
              % (kernel, field("vgpr_count"), field("sgpr_count"), field("private_segment_fixed_size"), field("vgpr_spill_count")))
        assert field("private_segment_fixed_size") == 0 and field("vgpr_spill_count") == 0 and field("sgpr_spill_count") == 0
        assert field("vgpr_count") <= 72          # 512 / 72: at least 7 waves per SIMD (58, 26, 70 -- the fp64 exp --, and 44)


def test_host_maths_under_sanitizers(tmp_path):
    """tests/denoise_asan_driver.cpp, a stand-alone program: smg_denoise_faces_host and smg_mesh_face_neighbours on exactly-sized heap arrays
    under AddressSanitizer and UndefinedBehaviorSanitizer (static runtimes: run directly, nothing preloaded, nothing loaded into python)"""
    exe = str(tmp_path / "denoise_asan_driver")
    csrc = os.path.join(ROOT, "surface_multigrid_code_amd", "csrc")
    srcs = [os.path.join(ROOT, "tests", "denoise_asan_driver.cpp"), os.path.join(csrc, "smg_mesh.cpp"), os.path.join(csrc, "smg_sparse.cpp")]
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-ffp-contract=off", "-pthread", "-I" + csrc] + srcs + ["-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    run = subprocess.run([exe], env=env, capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0 and "rows of 64: 65" in run.stdout and "ERROR" not in run.stderr
