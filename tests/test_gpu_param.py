"""GPU (-m gpu): harmonic and as-rigid-as-possible flattening of disk meshes (include/smg.h: smg_param_*).

The host reference is tests/test_param_host.py -- the same method with direct solves, in the kernels' operation order.  The kernels are held
launcher by launcher (smg_debug_param, guarded buffers) to the restatement's expressions: rest constants, covariance, right-hand side, face
energies and det J bit for bit, the rotations to one square root and one division, the singular values to numpy's SVD.

End to end (harmonic map + 5 iterations at inner tolerance 1e-12 s against the restatement's direct solves, both solvers, ogre_sim and
bunny) positions are compared relative to the circle's diameter and energies relatively.  E2E_BOUND = 1e-9 is the bound of
tests/test_gpu_arap.py and tests/test_gpu_membrane.py for the same inner solver at the same relative tolerance.  Measured on an MI355X
(profiles/r16_parent_mesh_object_gpu_tests.log): harmonic <= 1.61e-12 diameters, U_5 <= 1.90e-12 diameters with PCG and
<= 1.88e-11 with the stationary loop (bunny), energies <= 7.42e-13.  The rule "100 x the measured maximum, rounded up to a power of ten" gives
1e-8, which would loosen the bound: it stays 1e-9, 53 x the maximum."""
import ctypes as C
import math

import numpy as np
import pytest

from oracle import mesh_np as M
from test_gpu_parity import smg  # noqa: F401  (fixture)
from test_param_host import (PARAM_COVARIANCE, PARAM_DISTORTION, PARAM_ENERGY, PARAM_FACE_ENERGY, PARAM_REST, PARAM_RHS, PARAM_ROTATIONS, TABLE,
                             circle, covariance, distortion, face_energy, load_mesh, mesh_area, param_hook, reference_run, rest_constants,
                             rhs, rotations)

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
# end to end at tight inner tolerances against the direct solves of the restatement (see the module docstring)
E2E_BOUND = 1e-9
E2E_MESHES = ["ogre_sim.smgm", "bunny.smgm"]


# ---- the smallest inputs that can still go wrong --------------------------------------------------------------------------------------------------
def square2():
    return np.array([[0.0, 0, 0], [1, 0, 0.2], [1.1, 0.9, 0], [-0.1, 1, 0.3]]), np.array([[0, 1, 2], [0, 2, 3]], dtype=np.int32)


def fan(n=65):
    """n faces around vertex 0: its corner list is longer than a wave has lanes, and n is no multiple of 64"""
    t = 2 * np.pi * np.arange(n) / n
    ring = np.stack([(1 + 0.2 * np.cos(3 * t)) * np.cos(t), (1 + 0.2 * np.cos(3 * t)) * np.sin(t), 0.3 * np.sin(2 * t)], axis=1)
    V = np.concatenate([[[0.05, -0.02, 0.4]], ring])
    return V, np.array([[0, 1 + i, 1 + (i + 1) % n] for i in range(n)], dtype=np.int32)


def strip(n):
    """n faces between two rows of vertices"""
    m = n // 2 + 2
    x = np.arange(m, dtype=np.float64)
    V = np.concatenate([np.stack([x, 0.1 * np.sin(x), 0.05 * x * x / m], axis=1), np.stack([x + 0.4, 1 + 0.1 * np.cos(x), 0.2 * np.cos(x)], axis=1)])
    F = []
    for i in range(m - 1):
        F += [[i, i + 1, m + i], [i + 1, m + i + 1, m + i]]
    return V, np.array(F[:n], dtype=np.int32)


def small_cases():
    rng = np.random.default_rng(11)
    out = []
    for label, (V, F) in [("square", square2()), ("fan65", fan(65)), ("strip63", strip(63)), ("strip64", strip(64)), ("strip65", strip(65))]:
        n = int(F.max()) + 1
        V = np.ascontiguousarray(V[:n])
        out.append((label, V, F, [V[:, :2] + 0.3 * rng.standard_normal((n, 2)), rng.standard_normal((n, 2))]))
    return out


@pytest.fixture(scope="module")
def kernel_cases():
    """(label, V, F, [maps]): the small meshes with random maps, the fixtures at the restatement's U_0 (harmonic) and U_3"""
    out = small_cases()
    for name in ("ogre_sim.smgm", "ogre.smgm"):
        P, _, _, its = reference_run(name)
        out.append((name, P.V, P.F, [np.array(its[0]), np.array(its[3])]))
    return {c[0]: c[1:] for c in out}


KERNEL_CASES = ["square", "fan65", "strip63", "strip64", "strip65", "ogre_sim.smgm", "ogre.smgm"]


def hook(smg, op, V, F, UV, R, n_out):
    rc, bad, out = param_hook(smg._lib.load(), op, V.shape[0], F, V, UV, R, n_out)
    assert rc == 0 and bad == 0, (rc, bad)
    return out


# ---- kernels, launcher by launcher ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", KERNEL_CASES)
def test_kernels_against_restatement(smg, kernel_cases, name):
    V, F, maps = kernel_cases[name]
    nV, nF = V.shape[0], F.shape[0]
    r = rest_constants(V, F)
    assert np.array_equal(hook(smg, PARAM_REST, V, F, None, None, 6 * nF).reshape(6, nF).T, r)
    print(name, "nV = %d, nF = %d, longest corner list %d" % (nV, nF, np.bincount(F.ravel()).max()))
    for UV in maps:
        S = covariance(r, F, UV)
        assert np.array_equal(hook(smg, PARAM_COVARIANCE, V, F, UV, None, 4 * nF).reshape(4, nF).T, S)
        cs, sn, h = rotations(S)
        R = hook(smg, PARAM_ROTATIONS, V, F, UV, None, 2 * nF).reshape(2, nF)
        rot_err = max(np.abs(R[0] - cs).max(), np.abs(R[1] - sn).max())
        assert np.all(np.isfinite(R)) and rot_err <= 8 * EPS                       # every face compared: none is left out
        assert np.abs(R[0] * R[0] + R[1] * R[1] - 1.0).max() <= 8 * EPS
        b = hook(smg, PARAM_RHS, V, F, None, (cs, sn), 2 * nV).reshape(2, nV).T
        assert np.array_equal(b, rhs(r, F, nV, cs, sn))
        terms = face_energy(r, F, UV, cs, sn)
        assert np.array_equal(hook(smg, PARAM_FACE_ENERGY, V, F, UV, (cs, sn), nF), terms)
        E1 = hook(smg, PARAM_ENERGY, V, F, UV, (cs, sn), 1)[0]
        E2 = hook(smg, PARAM_ENERGY, V, F, UV, (cs, sn), 1)[0]
        exact = math.fsum(terms)
        bound = 2 * nF * EPS * np.abs(terms).sum()
        assert E1 == E2 and abs(E1 - exact) <= bound
        J, det, s1, s2 = distortion(r, F, UV)
        D = hook(smg, PARAM_DISTORTION, V, F, UV, None, 3 * nF).reshape(3, nF)
        assert np.array_equal(D[0], det) and np.array_equal(D[0] <= 0.0, det <= 0.0)
        sv = np.linalg.svd(J, compute_uv=False)
        sig_err = np.maximum(np.abs(D[1] - sv[:, 0]), np.abs(D[2] - sv[:, 1])) / sv[:, 0]
        print("  rotations %.1f eps, |E - fsum| = %.2e (bound %.2e), sigma %.1f eps sigma1, flipped %d"
              % (rot_err / EPS, abs(E1 - exact), bound, sig_err.max() / EPS, np.sum(det <= 0.0)))
        assert np.all(sig_err <= 16 * EPS)


def test_all_equal_map_gives_the_identity(smg, kernel_cases):
    V, F, _ = kernel_cases["fan65"]
    nF = F.shape[0]
    UV = np.tile([0.25, -3.0], (V.shape[0], 1))
    assert np.all(covariance(rest_constants(V, F), F, UV) == 0.0)                # h == 0 on every face
    R = hook(smg, PARAM_ROTATIONS, V, F, UV, None, 2 * nF).reshape(2, nF)
    assert np.array_equal(R[0], np.ones(nF)) and np.array_equal(R[1], np.zeros(nF))


# ---- end to end -----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def e2e(smg):
    out = {}
    for name in E2E_MESHES:
        V, F = load_mesh(name)
        mg = smg.mg_precompute(V, F, 0.25, 500, 1)
        out[name] = (V, F, mg, smg.Parameterizer(mg, V, F))
    return out


@pytest.mark.parametrize("name", E2E_MESHES)
def test_boundary_and_harmonic_rows(smg, e2e, name):
    V, F, mg, par = e2e[name]
    loop = par.boundary()
    assert np.array_equal(loop, smg.mesh.boundary_loop(F)) and np.array_equal(loop, M.boundary_loop(F)) and loop.size == TABLE[name][1]
    H = par.harmonic()
    assert 0 < par.cycles < 50
    assert np.array_equal(H[loop], circle(V, loop, mesh_area(V, F)))             # the boundary rows are the circle, bit for bit


@pytest.mark.parametrize("pcg", [1, 0])
@pytest.mark.parametrize("name", E2E_MESHES)
def test_tight_solves_against_restatement(smg, e2e, name, pcg):
    """harmonic map and 5 iterations at inner tolerance 1e-12 s against direct solves; prints the figures before it asserts.  Measured maximum
    1.88e-11 (module docstring); bound E2E_BOUND = 1e-9."""
    V, F, mg, par = e2e[name]
    ref, _, _, its = reference_run(name)
    diameter = 2.0 * math.sqrt(mesh_area(V, F) / math.pi)
    par.set_solver(pcg)
    try:
        H = par.harmonic(opts=smg.SolveOpts(tol=1e-12 * ref.harmonic_scale(), max_iter=100))
        c_h = par.cycles
        U, E, cyc = par.flatten(UV0=H, max_iter=5, opts=smg.SolveOpts(tol=1e-12 * ref.scale(), max_iter=100))
    finally:
        par.set_solver(1)
    Un, En, _ = ref.run(U0=its[0], n_iter=5)
    dh = np.abs(H - its[0]).max() / diameter
    du = np.abs(U - Un).max() / diameter
    de = np.abs(E - En) / np.abs(En)
    print("%s pcg=%d: harmonic %.2e diameters (%d cycles), U_5 %.2e diameters, energies %s, cycles %s"
          % (name, pcg, dh, c_h, du, np.array2string(de, precision=2), cyc))
    assert E.shape == (6,) and c_h < 100 and np.all(cyc < 100)
    assert dh <= E2E_BOUND and du <= E2E_BOUND and np.all(de <= E2E_BOUND)


@pytest.mark.parametrize("name", E2E_MESHES)
def test_default_run_and_distortion(smg, e2e, name):
    V, F, mg, par = e2e[name]
    ref = reference_run(name)[0]
    U, E, cyc = par.flatten(max_iter=10)
    print(name, "default opts: E %s, cycles %s" % (np.array2string(E, precision=5), cyc))
    assert E.shape == (11,) and cyc.shape == (10,) and np.all(cyc < 50)
    assert np.all(E[1:] <= E[:-1] * (1.0 + E2E_BOUND))                           # non-increasing, up to the inner solve's freedom
    assert abs(E[10] / TABLE[name][4] - 1.0) <= 5e-3                              # the table's E_10, to 3 digits
    sigma, stats = par.distortion(U)
    _, det, s1, s2 = distortion(ref.r, F, U)
    print(name, stats)
    assert stats["flipped"] == int(np.sum(det <= 0.0))                           # the restatement's count on the same bits
    assert np.array_equal(sigma[:, 0], s1) and np.array_equal(sigma[:, 1], s2)
    A, ok = 0.5 * (ref.r[:, 0] * ref.r[:, 2]), det > 0.0
    want = [np.sum(det <= 0.0), (s1 / s2)[ok].max(), np.sum(A * (s1 / s2)) / A.sum(), np.sum(A * s1 * s2) / A.sum(),
            np.sum((A * (s1 * s1 + s2 * s2 + 1 / (s1 * s1) + 1 / (s2 * s2)))[ok]) / A[ok].sum(), A.sum()]
    got = [stats[k] for k in smg.Parameterizer.STATS]
    assert got[0] == want[0] and got[1] == want[1]
    assert np.allclose(got[2:], want[2:], rtol=1e-12, atol=0.0)                   # sums of nF positive terms in another order: nF eps at most
    assert abs(stats["area"] - 1.0) <= 1e-12                                      # normalize_unit_area


def test_same_bits(smg, e2e):
    import torch
    name = "ogre_sim.smgm"
    V, F, mg, par = e2e[name]
    ref = reference_run(name)[0]
    n = V.shape[0]
    a = par.flatten(max_iter=3)
    before = par.device_bytes()
    b = par.flatten(max_iter=3)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    Ha, Hb = par.harmonic(), par.harmonic()
    assert np.array_equal(Ha, Hb)
    s = ref.scale()
    eager = par.flatten(UV0=Ha, max_iter=3, opts=smg.SolveOpts(tol=1e-8 * s, max_iter=50, use_graph=0))
    graph = par.flatten(UV0=Ha, max_iter=3, opts=smg.SolveOpts(tol=1e-8 * s, max_iter=50, use_graph=1))
    assert all(np.array_equal(x, y) for x, y in zip(eager, graph))
    sh = ref.harmonic_scale()
    assert np.array_equal(par.harmonic(opts=smg.SolveOpts(tol=1e-8 * sh, max_iter=50, use_graph=0)),
                          par.harmonic(opts=smg.SolveOpts(tol=1e-8 * sh, max_iter=50, use_graph=1)))
    par.distortion(a[0])
    assert par.device_bytes() == before                                          # nothing grows after the first call
    # SMG_DEVICE, padded leading dimensions: the same bits, rows past n untouched
    ld_u, ld_u0 = n + 5, n + 2
    Ud = torch.full((2, ld_u), -1.0, dtype=torch.float64, device="cuda")
    U0d = torch.zeros((2, ld_u0), dtype=torch.float64, device="cuda")
    U0d[:, :n] = torch.from_numpy(np.ascontiguousarray(Ha.T))
    Ed, cycd = par.flatten_device(Ud.data_ptr(), ld_uv=ld_u,UV0_ptr=U0d.data_ptr(), ld_uv0=ld_u0, max_iter=3)
    torch.cuda.synchronize()
    Uh, Eh, cych = par.flatten(UV0=Ha, max_iter=3)
    got = Ud.cpu().numpy()
    assert np.array_equal(got[:, :n].T, Uh) and np.all(got[:, n:] == -1.0)
    assert np.array_equal(Ed, Eh) and np.array_equal(cycd, cych)
    Hd = torch.full((2, ld_u), -1.0, dtype=torch.float64, device="cuda")
    par.harmonic_device(Hd.data_ptr(), ld_uv=ld_u)
    torch.cuda.synchronize()
    got = Hd.cpu().numpy()
    assert np.array_equal(got[:, :n].T, Ha) and np.all(got[:, n:] == -1.0)
    # the start computed inside is the harmonic map
    assert all(np.array_equal(x, y) for x, y in zip(par.flatten(max_iter=3), par.flatten(UV0=Ha, max_iter=3)))
    U0, E0, cyc0 = par.flatten(UV0=Ha, max_iter=0)
    assert np.array_equal(U0, Ha) and E0.shape == (1,) and cyc0.size == 0 and E0[0] == a[1][0]


def test_non_finite_start_is_refused_at_iteration_0(smg, e2e):
    """one NaN in UV0 at a vertex that is not the pinned one: E_0 is NaN, so the call ends before any inner solve with SMG_ERR_NONFINITE, n_iter = 0
    and nothing written past energy_his[0]; the object is as usable afterwards as before (the same bits)"""
    V, F, mg, par = e2e["ogre_sim.smgm"]
    n, L = V.shape[0], smg._lib.load()
    before = par.flatten(max_iter=2)
    v = int(np.setdiff1d(np.arange(n), par.boundary())[n // 2])                    # an interior vertex: not loop[0]
    UV0 = np.asfortranarray(par.harmonic())
    UV0[v, 0] = np.nan
    U = np.zeros((n, 2), order="F")
    E, cyc, nit = np.full(4, -7.0), np.full(3, -7, dtype=np.int32), C.c_int(-7)
    rc = L.smg_param_arap(par.p, UV0.ctypes.data, n, 0, 3, 0.0, None, U.ctypes.data, n, E.ctypes.data_as(C.POINTER(C.c_double)),
                          cyc.ctypes.data_as(C.POINTER(C.c_int)), C.byref(nit))
    assert rc == -4 and L.smg_last_error() == b"smg_param_arap: non-finite energy at iteration 0"
    assert nit.value == 0 and np.isnan(E[0]) and np.all(E[1:] == -7.0) and np.all(cyc == -7)
    after = par.flatten(max_iter=2)
    assert all(np.array_equal(x, y) for x, y in zip(before, after))


def test_callers_hierarchy_is_untouched(smg):
    V, F = load_mesh("ogre_sim.smgm")
    mg = smg.mg_precompute(V, F, 0.25, 500, 1)
    A = (M.massmatrix(V, F, "barycentric") - 0.01 * smg.mesh.cotmatrix(V, F)).tocsr()
    mg.precompute(A, None)
    rhs_ = np.asfortranarray(A @ V)
    o = smg.SolveOpts(tol=1e-10, max_iter=30)
    first = mg.solve(rhs_, np.zeros_like(rhs_, order="F"), None, o)
    par = smg.Parameterizer(mg, V, F)
    par.flatten(max_iter=2)
    second = mg.solve(rhs_, np.zeros_like(rhs_, order="F"), None, o)
    assert first[0] and np.array_equal(first[1], second[1]) and np.array_equal(first[2], second[2])


def test_call_refusals(smg, e2e):
    V, F, mg, par = e2e["ogre_sim.smgm"]
    n = V.shape[0]
    with pytest.raises(smg.SmgError) as e:
        par.flatten(max_iter=-1)
    assert e.value.code == -1
    with pytest.raises(smg.SmgError):
        par.flatten(rel_tol=float("nan"))
    L = smg._lib.load()
    U, st = np.zeros((n, 2), order="F"), np.zeros(6)
    assert L.smg_param_harmonic(par.p, 0, None, U.ctypes.data, n - 1, None) == -1
    assert L.smg_param_harmonic(par.p, 7, None, U.ctypes.data, n, None) == -1
    assert L.smg_param_arap(par.p, None, 0, 0, 1, 0.0, None, U.ctypes.data, n - 1, None, None, None) == -1
    assert L.smg_param_distortion(par.p, U.ctypes.data, n, 0, None, None) == -1
    assert L.smg_param_distortion(par.p, U.ctypes.data, n - 1, 0, None, st.ctypes.data_as(C.POINTER(C.c_double))) == -1
