"""GPU (-m gpu): as-rigid-as-possible deformation (include/smg.h: smg_arap_*).

The host reference is tests/test_arap_host.py -- the same method with LAPACK SVDs and direct solves, in the kernels' operation order.  The
kernels are held launcher by launcher (smg_debug_arap, guarded buffers) to the restatement's expressions: covariance, right-hand side and
energy terms bit for bit, the rotations to the perturbation bound of the polar factor.

Measured on an MI355X: rotations max err * gap / eps = 68.7 (bound 256; 63.4 on the edge shapes of
denoise_np.edge_shapes(), 4 to 259 rows and one row of 65 entries), |R^T R - I| <= 9 eps (bound 32);
end to end against the restatement: positions <= 1.11e-12 diagonals, energies <= 1.29e-12 relative (bound E2E_BOUND = 1e-9)."""
import math

import numpy as np
import pytest

from denoise_np import EDGE_SHAPES, edge_shapes, mean_edge
from oracle import mesh_np as M
from pd_np import fixed_sum
from test_arap_host import (ARAP_COVARIANCE, ARAP_ENERGY, ARAP_RHS, ARAP_ROTATIONS, ARAP_VERTEX_ENERGY, ArapNp, ArapRest, arap_hook, bbox_diag,
                            covariance, flat_square, load_mesh, rhs, roll_onto_cylinder, rotation_matrix, rotations_np, twist, vertex_energy)
from test_gpu_parity import smg  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
ROT_BOUND = 256        # |R_gpu - R_np|_F <= ROT_BOUND eps / gap: 4 x what a numpy one-sided Jacobi shows against LAPACK (68)
GAP_MIN = 1e-3         # vertices with a smaller gap may be left out, at most 1 % of a mesh (none on these inputs)
# end to end at tight inner tolerances against the direct solves of the restatement: 100 x the measured maximum (1.29e-12, an energy of the
# 252 834-vertex case; positions 1.11e-12 diagonals there, 1.6e-13 on the small meshes), rounded up to a power of ten
E2E_BOUND = 1e-9

KERNEL_MESHES = ["icosphere5", "bunny.smgm", "ogre.smgm"]


@pytest.fixture(scope="module")
def kernel_cases():
    """per mesh: the rest data and the twist's iterates U_0 and U_3 of the restatement"""
    out = {}
    for name in KERNEL_MESHES:
        V, F = load_mesh(name)
        handles, hp = twist(V)
        arap = ArapNp(M.cotmatrix(V, F), V, handles)
        _, _, its = arap.run(hp, n_iter=3)
        out[name] = (arap.A, [np.ascontiguousarray(its[0]), np.ascontiguousarray(its[3])])
    return out


def hook(smg, op, A, P, R_in, shape):
    out = np.full(shape, np.nan)
    rc, bad = arap_hook(smg._lib.load(), op, A, P, None if R_in is None else np.ascontiguousarray(R_in.reshape(-1)), out)
    assert rc == 0 and bad == 0, (rc, bad)
    return out


# ---- kernels, launcher by launcher ----------------------------------------------------------------------------------------------------------
def check_bitwise(smg, A, Ps, label):
    """covariance, right-hand side and energy terms at the poses Ps bit for bit against the restatement; the reduced energy is the fixed
    sum of the DEVICE's terms in its own order, the same on a second call, and a sum (the fsum bound).  Returns the device's outputs of the
    last pose."""
    n = A.n
    print(label, "n = %d, max degree %d" % (n, A.deg.max()))
    for P in Ps:
        S = covariance(A, P)
        Sd = hook(smg, ARAP_COVARIANCE, A, P, None, 9 * n).reshape(n, 3, 3)
        assert np.array_equal(Sd, S)
        R, _, _ = rotations_np(S)
        b = hook(smg, ARAP_RHS, A, None, R, 3 * n).reshape(3, n).T
        assert np.array_equal(b, rhs(A, R))
        terms = vertex_energy(A, P, R)
        td = hook(smg, ARAP_VERTEX_ENERGY, A, P, R, n)
        assert np.array_equal(td, terms)
        E1 = hook(smg, ARAP_ENERGY, A, P, R, 1)[0]
        E2 = hook(smg, ARAP_ENERGY, A, P, R, 1)[0]
        exact = math.fsum(terms)
        print("  reduced energy %.17g, |E - fsum| = %.2e (bound %.2e)" % (E1, abs(E1 - exact), 2 * n * EPS * np.abs(terms).sum()))
        assert E1 == E2
        assert E1 == fixed_sum(td)                                                   # the fixed sum in its own order
        assert abs(E1 - exact) <= 2 * n * EPS * np.abs(terms).sum()
    return Sd, b, td, E1


@pytest.mark.parametrize("name", KERNEL_MESHES)
def test_covariance_rhs_energy_bitwise(smg, kernel_cases, name):
    A, Ps = kernel_cases[name]
    check_bitwise(smg, A, Ps, name)


def check_rotations(smg, A, P, label, expect_reflections):
    n = A.n
    S = covariance(A, P)
    Rn, gap, d = rotations_np(S)
    R = hook(smg, ARAP_ROTATIONS, A, P, None, 9 * n).reshape(n, 3, 3)
    assert np.all(np.isfinite(R))
    keep = gap >= GAP_MIN
    err = np.linalg.norm((R - Rn).reshape(n, 9), axis=1)
    orth = np.abs(np.einsum("nji,njk->nik", R, R) - np.eye(3)).max()
    print("%s: max err * gap / eps = %.1f, |R^T R - I| = %.1f eps, min gap %.2e, left out %d of %d, reflections %.2f %%"
          % (label, (err * gap / EPS)[keep].max(), orth / EPS, gap.min(), n - keep.sum(), n, 100 * np.mean(d < 0)))
    assert n - keep.sum() <= 0.01 * n
    assert np.all(err[keep] <= ROT_BOUND * EPS / gap[keep])
    assert orth <= 32 * EPS
    assert np.all(np.linalg.det(R) > 0)
    if expect_reflections:
        assert np.any(d < 0)
    return R


@pytest.mark.parametrize("name", KERNEL_MESHES)
def test_rotations_against_lapack(smg, kernel_cases, name):
    A, Ps = kernel_cases[name]
    check_rotations(smg, A, Ps[0], name + " U_0", True)
    check_rotations(smg, A, Ps[1], name + " U_3", False)


def test_rotations_degenerate_inputs(smg):
    V, F = load_mesh("bunny.smgm")
    A = ArapRest(M.cotmatrix(V, F), V)
    P = np.ascontiguousarray(np.tile([0.25, -1.0, 3.0], (A.n, 1)))            # all points equal: S == 0, the identity exactly
    R = hook(smg, ARAP_ROTATIONS, A, P, None, 9 * A.n).reshape(A.n, 3, 3)
    assert np.array_equal(R, np.tile(np.eye(3), (A.n, 1, 1)))
    V, F = flat_square()                                                       # a flat rest pose: rank-2 covariances everywhere
    A = ArapRest(M.cotmatrix(V, F), V)
    P = np.ascontiguousarray(roll_onto_cylinder(V))
    _, gap, _ = rotations_np(covariance(A, P))
    assert gap.min() >= GAP_MIN
    check_rotations(smg, A, P, "flat square on a cylinder", True)


# ---- the same launchers on the edge shapes: fewer rows than a block, rows around a wave and a block, one row of 65 entries ---------------------
@pytest.fixture(scope="module")
def edge_cases():
    """per edge shape: the rest data and two poses -- P1 a rigid image plus 0.05 mean edges of noise, P2 the rest pose stretched by
    (1.3, 0.8, 1.0) plus 0.2 mean edges of noise (default_rng(7) per shape, P1 drawn first)"""
    out = {}
    Rg, tg = rotation_matrix([1.0, 2.0, -0.5], 1.1), np.array([0.3, -0.2, 0.7])
    for name, (V, F) in edge_shapes().items():
        rng = np.random.default_rng(7)
        h = mean_edge(V, F)
        P1 = (V @ Rg.T + tg) + 0.05 * h * rng.standard_normal(V.shape)
        P2 = V * np.array([1.3, 0.8, 1.0]) + 0.2 * h * rng.standard_normal(V.shape)
        out[name] = (ArapRest(M.cotmatrix(V, F), V), [np.ascontiguousarray(P1), np.ascontiguousarray(P2)])
    return out


@pytest.mark.parametrize("name", EDGE_SHAPES)
def test_covariance_rhs_energy_bitwise_on_edge_shapes(smg, edge_cases, name):
    A, Ps = edge_cases[name]
    check_bitwise(smg, A, Ps, name)


@pytest.mark.parametrize("name", EDGE_SHAPES)
def test_rotations_against_lapack_on_edge_shapes(smg, edge_cases, name):
    """the cotangent weights on a boundary are negative: reflections (d < 0) occur on every open shape at both poses, on the closed tetrahedron
    at neither; no vertex has a gap below GAP_MIN (the smallest is 1.2e-2, on the fan), so none is left out"""
    A, Ps = edge_cases[name]
    for label, P in zip(("P1", "P2"), Ps):
        _, gap, _ = rotations_np(covariance(A, P))
        assert gap.min() >= GAP_MIN
        check_rotations(smg, A, P, "%s %s" % (name, label), name != "tetrahedron")


def test_hand_made_rows(smg):
    """a CSR no mesh gives, through the hook's rowptr / col: row 0 is empty, row 1 holds only its diagonal, row 2 stores its diagonal last, row 3
    first, row 4 in the middle, row 5 not at all.  Rows 0 and 1 have no neighbours: S = 0, R = I, b = 0 and an energy term of 0, exactly."""
    rng = np.random.default_rng(11)
    rows = [[], [1], [4, 0, 2], [3, 5, 1, 0], [2, 4, 5], [0, 3]]
    rowptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    col = np.array([j for r in rows for j in r], dtype=np.int32)
    n = len(rows)
    P0 = rng.uniform(-1, 1, (n, 3))
    A = ArapRest.from_csr(rowptr, col, rng.uniform(0.5, 1.5, col.size), P0)
    assert list(A.deg) == [0, 0, 2, 3, 2, 2]
    P = np.ascontiguousarray((P0 @ rotation_matrix([1.0, 2.0, -0.5], 1.1).T + 0.3) + 0.05 * rng.standard_normal((n, 3)))

    def call(op, R_in, shape):
        out = np.full(shape, np.nan)
        rc, bad = arap_hook(smg._lib.load(), op, A, None if op == ARAP_RHS else P, None if R_in is None else np.ascontiguousarray(R_in.reshape(-1)),
                            out, rowptr=rowptr, col=col)
        assert rc == 0 and bad == 0, (rc, bad)
        return out

    S = covariance(A, P)
    Sd = call(ARAP_COVARIANCE, None, 9 * n).reshape(n, 3, 3)
    assert np.array_equal(Sd, S) and not Sd[:2].any() and np.all(np.abs(Sd[2:]).max(axis=(1, 2)) > 0)
    Rn, gap, _ = rotations_np(S)
    assert gap[2:].min() >= GAP_MIN
    Rd = call(ARAP_ROTATIONS, None, 9 * n).reshape(n, 3, 3)
    assert np.array_equal(Rd[:2], np.tile(np.eye(3), (2, 1, 1)))
    err = np.linalg.norm((Rd - Rn).reshape(n, 9), axis=1)
    print("hand-made rows: max err * gap / eps = %.1f" % (err[2:] * gap[2:] / EPS).max())
    assert np.all(err[2:] <= ROT_BOUND * EPS / gap[2:]) and np.all(np.linalg.det(Rd) > 0)
    assert np.abs(np.einsum("nji,njk->nik", Rd, Rd) - np.eye(3)).max() <= 32 * EPS
    b = call(ARAP_RHS, Rn, 3 * n).reshape(3, n).T
    assert np.array_equal(b, rhs(A, Rn)) and not b[:2].any() and np.all(np.abs(b[2:]).max(axis=1) > 0)
    td = call(ARAP_VERTEX_ENERGY, Rn, n)
    assert np.array_equal(td, vertex_energy(A, P, Rn)) and not td[:2].any() and np.all(td[2:] > 0)
    assert call(ARAP_ENERGY, Rn, 1)[0] == fixed_sum(td)


# ---- end to end -----------------------------------------------------------------------------------------------------------------------------
def build(smg, name, n_sub=0):
    if n_sub:
        V, F = load_mesh(name)
        mg, V, F = smg.mg_precompute_subdiv(V, F, n_sub, ratio=0.25, nVCoarsest=1000)
    else:
        V, F = load_mesh(name)
        mg = smg.mg_precompute(V, F, 0.25, 200, 1)
    handles, hp = twist(V)
    return V, F, mg, handles, hp, smg.ArapDeformer(mg, V, F, handles)


@pytest.fixture(scope="module")
def sphere_case(smg):
    return build(smg, "icosphere5")


@pytest.fixture(scope="module")
def bunny_case(smg):
    return build(smg, "bunny.smgm")


@pytest.mark.parametrize("case", ["sphere_case", "bunny_case"])
def test_rigid_image_is_a_fixed_point(smg, request, case):
    V, F, mg, handles, hp, arap = request.getfixturevalue(case)
    rigid = V @ rotation_matrix([1.0, 2.0, -0.5], 1.1).T + np.array([0.3, -0.2, 0.7])
    _, E_twist, _ = arap.deform(hp, max_iter=0)
    U, E, cyc = arap.deform(rigid[handles], U0=rigid, max_iter=2)
    step = np.abs(U - rigid).max() / bbox_diag(V)
    print(case, "step %.2e diagonals, energies %s (twist E_0 %.3e), cycles %s" % (step, E, E_twist[0], cyc))
    assert E.shape == (3,) and cyc.shape == (2,)
    assert step <= 1e-12
    assert np.all(E <= 1e-20 * E_twist[0])
    assert np.all(cyc <= 1)


def check_twist(smg, V, F, handles, hp, arap, n_iter):
    ref = ArapNp(smg.mesh.cotmatrix(V, F), V, handles)                       # the library's own L: the system's bits
    s = ref.A.scale()
    U, E, cyc = arap.deform(hp, max_iter=n_iter, opts=smg.SolveOpts(tol=1e-12 * s, max_iter=100))      # the inner solver is PCG (the default)
    Un, En, _ = ref.run(hp, n_iter=n_iter)
    du = np.abs(U - Un).max() / bbox_diag(V)
    de = np.abs(E - En) / np.abs(En)
    print("n = %d: max |U - U_np| = %.2e diagonals, energy differences %s, cycles %s" % (V.shape[0], du, np.array2string(de, precision=2), cyc))
    assert E.shape == (n_iter + 1,) and np.all(cyc < 100)
    assert du <= E2E_BOUND
    assert np.all(de <= E2E_BOUND)


@pytest.mark.parametrize("case", ["sphere_case", "bunny_case"])
def test_twist_against_restatement(smg, request, case):
    V, F, mg, handles, hp, arap = request.getfixturevalue(case)
    check_twist(smg, V, F, handles, hp, arap, 6)


def test_twist_full_size(smg):
    V, F, mg, handles, hp, arap = build(smg, "bunny_15K_init.smgm", n_sub=2)
    assert V.shape[0] == 252834
    assert arap.device_bytes() > 0
    check_twist(smg, V, F, handles, hp, arap, 3)


@pytest.mark.parametrize("case", ["sphere_case", "bunny_case"])
def test_default_opts_and_stopping_rule(smg, request, case):
    V, F, mg, handles, hp, arap = request.getfixturevalue(case)
    U, E, cyc = arap.deform(hp, max_iter=10)
    print(case, "default opts: cycles %s, relative drops %s" % (cyc, np.array2string((E[:-1] - E[1:]) / E[:-1], precision=3)))
    assert E.shape == (11,) and cyc.shape == (10,)
    assert np.all(E[1:] < E[:-1])
    assert np.all(cyc < 50)                                                  # every inner solve converged
    assert np.array_equal(U[handles], hp)
    U2, E2, cyc2 = arap.deform(hp, max_iter=20, rel_tol=0.2)
    drops = (E2[:-1] - E2[1:]) / np.abs(E2[:-1])
    print(case, "rel_tol = 0.2: n_iter = %d, drops %s" % (cyc2.size, np.array2string(drops, precision=3)))
    assert 1 <= cyc2.size < 20 and E2.size == cyc2.size + 1
    assert drops[-1] <= 0.2 and np.all(drops[:-1] > 0.2)
    assert np.array_equal(E2, E[:E2.size])
    U0, E0, cyc0 = arap.deform(hp, max_iter=0)
    start = V.copy()
    start[handles] = hp
    assert E0.shape == (1,) and cyc0.size == 0 and E0[0] == E[0]
    assert np.array_equal(U0, start)


def test_same_bits(smg, sphere_case):
    import torch
    V, F, mg, handles, hp, arap = sphere_case
    n, nh = V.shape[0], handles.size
    s = ArapRest(M.cotmatrix(V, F), V).scale()
    a = arap.deform(hp, max_iter=4)
    b = arap.deform(hp, max_iter=4)
    before = arap.device_bytes()
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    eager = arap.deform(hp, max_iter=4, opts=smg.SolveOpts(tol=1e-8 * s, max_iter=50, use_graph=0))
    graph = arap.deform(hp, max_iter=4, opts=smg.SolveOpts(tol=1e-8 * s, max_iter=50, use_graph=1))
    assert all(np.array_equal(x, y) for x, y in zip(eager, graph))
    assert arap.device_bytes() == before                                     # nothing grows between the second and later calls
    # SMG_DEVICE, padded leading dimensions: the same bits, rows past n untouched
    ld_u, ld_hp, ld_u0 = n + 5, nh + 3, n + 2
    U0 = a[0] + 0.0
    Ud = torch.full((3, ld_u), -1.0, dtype=torch.float64, device="cuda")
    hpd = torch.zeros((3, ld_hp), dtype=torch.float64, device="cuda")
    hpd[:, :nh] = torch.from_numpy(np.ascontiguousarray(hp.T))
    U0d = torch.zeros((3, ld_u0), dtype=torch.float64, device="cuda")
    U0d[:, :n] = torch.from_numpy(np.ascontiguousarray(U0.T))
    Ed, cycd = arap.deform_device(hpd.data_ptr(), Ud.data_ptr(), ld_u=ld_u, U0_ptr=U0d.data_ptr(), ld_u0=ld_u0, ld_hp=ld_hp, max_iter=3)
    torch.cuda.synchronize()
    Uh, Eh, cych = arap.deform(hp, U0=U0, max_iter=3)
    got = Ud.cpu().numpy()
    assert np.array_equal(got[:, :n].T, Uh) and np.all(got[:, n:] == -1.0)
    assert np.array_equal(Ed, Eh) and np.array_equal(cycd, cych)
    # padded host leading dimensions through the C ABI
    import ctypes as C
    L = smg._lib.load()
    Up = np.full((n + 7, 3), -2.0, order="F")
    hpp = np.zeros((nh + 1, 3), order="F")
    hpp[:nh] = hp
    E = np.zeros(4)
    nit = C.c_int()
    assert L.smg_arap_solve(arap.a, hpp.ctypes.data, nh + 1, None, 0, 0, 3, 0.0, None, Up.ctypes.data, n + 7, E.ctypes.data_as(C.POINTER(C.c_double)),
                            None, C.byref(nit)) == 0
    assert nit.value == 3 and np.array_equal(Up[:n], arap.deform(hp, max_iter=3)[0]) and np.all(Up[n:] == -2.0)


def test_callers_hierarchy_is_untouched(smg):
    V, F = load_mesh("bunny.smgm")
    mg = smg.mg_precompute(V, F, 0.25, 200, 1)
    Lc = smg.mesh.cotmatrix(V, F)
    A = (M.massmatrix(V, F, "barycentric") - 0.01 * Lc).tocsr()
    mg.precompute(A, None)
    rhs_ = np.asfortranarray(A @ V)
    o = smg.SolveOpts(tol=1e-10, max_iter=30)
    first = mg.solve(rhs_, np.zeros_like(rhs_, order="F"), None, o)
    handles, hp = twist(V)
    arap = smg.ArapDeformer(mg, V, F, handles)
    arap.deform(hp, max_iter=2)
    second = mg.solve(rhs_, np.zeros_like(rhs_, order="F"), None, o)
    assert first[0] and np.array_equal(first[1], second[1]) and np.array_equal(first[2], second[2])


def test_solve_refusals(smg, sphere_case):
    V, F, mg, handles, hp, arap = sphere_case
    with pytest.raises(smg.SmgError) as e:
        arap.deform(hp, max_iter=-1)
    assert e.value.code == -1
    with pytest.raises(smg.SmgError):
        arap.deform(hp, rel_tol=-0.5)
    with pytest.raises(smg.SmgError):
        arap.deform(hp, rel_tol=float("nan"))
    L = smg._lib.load()
    hpf = np.asfortranarray(hp)
    U = np.zeros((V.shape[0], 3), order="F")
    assert L.smg_arap_solve(arap.a, hpf.ctypes.data, handles.size - 1, None, 0, 0, 1, 0.0, None, U.ctypes.data, V.shape[0], None, None, None) == -1
    assert L.smg_arap_solve(arap.a, hpf.ctypes.data, handles.size, None, 0, 0, 1, 0.0, None, U.ctypes.data, V.shape[0] - 1, None, None, None) == -1
    assert L.smg_arap_solve(arap.a, hpf.ctypes.data, handles.size, None, 0, 7, 1, 0.0, None, U.ctypes.data, V.shape[0], None, None, None) == -1


def test_non_finite_start_is_refused_at_iteration_0(smg, sphere_case):
    """one NaN in U0 at a vertex that is no handle: E_0 is NaN, so the call ends before any inner solve with SMG_ERR_NONFINITE, n_iter = 0 and
    nothing written past energy_his[0]; the object is as usable afterwards as before (the same bits)"""
    import ctypes as C
    V, F, mg, handles, hp, arap = sphere_case
    n, nh, L = V.shape[0], handles.size, smg._lib.load()
    before = arap.deform(hp, max_iter=2)
    v = int(np.setdiff1d(np.arange(n), handles)[n // 2])
    U0 = np.asfortranarray(V.copy())
    U0[v, 1] = np.nan
    hpf, U = np.asfortranarray(hp), np.zeros((n, 3), order="F")
    E, cyc, nit = np.full(4, -7.0), np.full(3, -7, dtype=np.int32), C.c_int(-7)
    rc = L.smg_arap_solve(arap.a, hpf.ctypes.data, nh, U0.ctypes.data, n, 0, 3, 0.0, None, U.ctypes.data, n, E.ctypes.data_as(C.POINTER(C.c_double)),
                          cyc.ctypes.data_as(C.POINTER(C.c_int)), C.byref(nit))
    assert rc == -4 and L.smg_last_error() == b"smg_arap_solve: non-finite energy at iteration 0"
    assert nit.value == 0 and np.isnan(E[0]) and np.all(E[1:] == -7.0) and np.all(cyc == -7)
    after = arap.deform(hp, max_iter=2)
    assert all(np.array_equal(x, y) for x, y in zip(before, after))


def test_stationary_loop_option(smg, bunny_case):
    V, F, mg, handles, hp, arap = bunny_case
    U_pcg, E_pcg, c_pcg = arap.deform(hp, max_iter=4)
    arap.set_solver(0)
    try:
        U_mg, E_mg, c_mg = arap.deform(hp, max_iter=4)
    finally:
        arap.set_solver(1)
    print("loop entries per solve: PCG %s, stationary %s" % (c_pcg, c_mg))
    # both inner solvers stop at 1e-8 s: the iterates agree to that tolerance, amplified by the iteration (bunny: 2.4 x over 6 iterations)
    assert np.abs(U_pcg - U_mg).max() <= 1e-6 * bbox_diag(V)
    assert np.all(np.abs(E_pcg - E_mg) <= 1e-6 * np.abs(E_pcg))
