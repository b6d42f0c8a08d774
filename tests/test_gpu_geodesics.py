"""GPU (-m gpu): geodesic distance by the heat method (include/smg.h: smg_geodesics_*).

The host reference is tests/test_geodesics_host.py::heat_geodesics_np -- the same discrete method with direct solves -- at the same t and mass
kind.  The kernels are held launcher by launcher (smg_debug_geodesics) to the restatement's expressions in the same order."""
import ctypes as C

import numpy as np
import pytest

import denoise_np as DN
from oracle import mesh_np as M
from test_geodesics_host import (GEO_BASIS, GEO_DIVERGENCE, GEO_SCATTER, GEO_SHIFT, INVALID, corner_lists, geo_hook, grad_basis, great_circle,
                                 heat_geodesics_np, icosphere, indicator, neg_divergence, shift)
from test_gpu_parity import smg  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
# end to end: the iterative solves at the default tolerances against the direct solves of the restatement
E2E_BOUND = 1e-5


@pytest.fixture(scope="module")
def sphere():
    V, F = icosphere(5)
    return V, F


@pytest.fixture(scope="module")
def sphere_geo(smg, sphere):
    V, F = sphere
    mg = smg.mg_precompute(V, F, 0.25, 200, 1)
    return smg.HeatGeodesics(mg, V, F)


# ---- kernels, launcher by launcher --------------------------------------------------------------------------------------------------------
def test_basis_kernel(smg, sphere):
    L = smg._lib.load()
    V, F = sphere
    W = np.full(9 * F.shape[0], np.nan)
    Af = np.full(F.shape[0], np.nan)
    rc, bad = geo_hook(L, GEO_BASIS, V.shape[0], 1, F=F, inp=np.ascontiguousarray(V), W=W, Af=Af)
    assert rc == 0 and bad == 0
    Wn, An = grad_basis(V, F)
    # the same expressions in the same order, correctly rounded operations, no contraction: equal bits
    assert np.array_equal(W.reshape(-1, 3, 3), Wn) and np.array_equal(Af, An)
    # and what it means: sum_i W_fi = 0 (constants have no gradient), W_fi . (x_j - x_i) = -1 for j != i
    assert np.abs(Wn.sum(axis=1)).max() <= 1e-12 * np.abs(Wn).max()


def test_scatter_kernel(smg):
    L = smg._lib.load()
    n = 1000
    sets = [[3], [0, 999, 3], [17, 17, 5], list(range(200, 260))] + [[i] for i in range(60)]
    k = len(sets)
    ptr = np.zeros(k + 1, np.int32)
    ptr[1:] = np.cumsum([len(s) for s in sets])
    src = np.concatenate([np.array(s, np.int32) for s in sets])
    for ld in (n, n + 7):
        out = np.full((ld, k), 7.0, order="F")
        rc, bad = geo_hook(L, GEO_SCATTER, n, k, src_ptr=ptr, src=src, inp=np.zeros(1), out=out, ld_out=ld)
        assert rc == 0 and bad == 0
        assert np.array_equal(out[:n], indicator(n, sets))
        assert np.all(out[n:] == 7.0)                          # rows past n of a padded block are left alone


@pytest.mark.parametrize("k", [1, 3, 8, 64])
def test_divergence_kernel(smg, sphere, k):
    L = smg._lib.load()
    V, F = sphere
    n = V.shape[0]
    rng = np.random.default_rng(k)
    U = np.asfortranarray(rng.uniform(-1, 1, (n, k)))
    U[:, 0] = 0.0                                              # a zero column: grad u == 0 on every face, X = 0
    W, Af = grad_basis(V, F)
    m_ptr, m_idx = corner_lists(F, n)
    out = np.full((n, k), np.nan, order="F")
    rc, bad = geo_hook(L, GEO_DIVERGENCE, n, k, F=F, m_ptr=m_ptr, m_idx=m_idx, inp=U, W=np.ascontiguousarray(W.ravel()), Af=Af, out=out)
    assert rc == 0 and bad == 0
    ref = neg_divergence(F, W, Af, m_ptr, m_idx, U)
    # stated bound: 2 (deg + 8) eps times deg times the largest term magnitude max A_f |W| (|X| = 1): a term is a 3-term gradient, its norm,
    # three quotients, a 3-term dot and one product, deg terms are summed.  In the same operation order the kernel is bit-identical.
    deg = np.diff(m_ptr)
    bound = 2 * (deg.max() + 8) * EPS * np.abs(Af).max() * np.abs(W).max() * deg.max()
    assert np.abs(out - ref).max() <= bound
    assert np.array_equal(out, ref), "not bit-identical to the restatement (within the stated bound)"
    assert np.all(out[:, 0] == 0.0)


def test_shift_kernel(smg):
    L = smg._lib.load()
    n = 777
    rng = np.random.default_rng(5)
    sets = [[4], [0, 776, 4, 4], list(range(100, 400, 3)), [776]]
    k = len(sets)
    ptr = np.zeros(k + 1, np.int32)
    ptr[1:] = np.cumsum([len(s) for s in sets])
    src = np.concatenate([np.array(s, np.int32) for s in sets])
    phi = np.asfortranarray(rng.uniform(-3, 3, (n, k)))
    for ld in (n, n + 5):
        out = np.full((ld, k), -9.0, order="F")
        rc, bad = geo_hook(L, GEO_SHIFT, n, k, src_ptr=ptr, src=src, inp=phi, out=out, ld_out=ld)
        assert rc == 0 and bad == 0
        assert np.array_equal(out[:n], shift(phi, sets))
        assert np.all(out[n:] == -9.0)
        assert out[4, 0] == 0.0 and out[776, 3] == 0.0


# ---- the same launchers on the edge shapes: rows around a wave and a block, a 65-long corner list, meshes smaller than a block ------------------
@pytest.fixture(scope="module")
def edge_shapes():
    return DN.edge_shapes()


@pytest.mark.parametrize("name", DN.EDGE_SHAPES)
def test_basis_kernel_on_edge_shapes(smg, edge_shapes, name):
    L = smg._lib.load()
    V, F = edge_shapes[name]
    W, Af = np.full(9 * F.shape[0], np.nan), np.full(F.shape[0], np.nan)
    rc, bad = geo_hook(L, GEO_BASIS, V.shape[0], 1, F=F, inp=np.ascontiguousarray(V), W=W, Af=Af)
    assert rc == 0 and bad == 0
    Wn, An = grad_basis(V, F)
    assert np.array_equal(W.reshape(-1, 3, 3), Wn) and np.array_equal(Af, An)


def divergence_columns(V, F, seed):
    """n x 3: column 0 all zero (X = 0 everywhere); column 1 random but 0 on the three vertices of a few faces (|grad u| == 0 on those alone:
    the nrm > 0 branch diverges inside a wave) and one value on the vertices of another (a gradient of rounding noise); column 2 random"""
    n, nF = V.shape[0], F.shape[0]
    U = np.asfortranarray(np.random.default_rng(seed).uniform(-1, 1, (n, 3)))
    U[:, 0] = 0.0
    flat = [0, nF // 2] if nF > 4 else [0]
    if nF > 8:
        U[F[nF - 1], 1] = 0.37
    U[F[flat].ravel(), 1] = 0.0
    return U, flat


@pytest.mark.parametrize("name", DN.EDGE_SHAPES)
def test_divergence_kernel_on_edge_shapes(smg, edge_shapes, name):
    L = smg._lib.load()
    V, F = edge_shapes[name]
    n, nF = V.shape[0], F.shape[0]
    W, Af = grad_basis(V, F)
    m_ptr, m_idx = corner_lists(F, n)
    U3, flat = divergence_columns(V, F, nF)
    u = U3[F, 1]                                                 # the partly flat column: exactly those faces have no gradient, the others do
    g = u[:, 0, None] * W[:, 0] + u[:, 1, None] * W[:, 1] + u[:, 2, None] * W[:, 2]
    zero = np.nonzero(np.sqrt(np.sum(g * g, axis=1)) == 0.0)[0]
    assert set(flat) <= set(zero) <= set(flat) | {nF - 1} and zero.size < nF    # (the face with one value: noise, or it rounds to nothing)
    blocks = [U3[:, [c]] for c in range(3)] + [U3]               # k = 1 (each kind of column alone) and k = 3
    if name == "tetrahedron":
        blocks.append(np.tile(U3, (1, 22))[:, :64])             # k = 64 on n = 4
    print(name, "n = %d, nF = %d, longest corner list %d, faces without a gradient in column 1: %s" % (n, nF, np.diff(m_ptr).max(), zero))
    for U in blocks:
        U = np.asfortranarray(U)
        k = U.shape[1]
        ref = neg_divergence(F, W, Af, m_ptr, m_idx, U)
        for ld in (n, n + 3):
            out = np.full((ld, k), -9.0, order="F")
            rc, bad = geo_hook(L, GEO_DIVERGENCE, n, k, F=F, m_ptr=m_ptr, m_idx=m_idx, inp=U, W=np.ascontiguousarray(W.ravel()), Af=Af, out=out, ld_out=ld)
            assert rc == 0 and bad == 0
            assert np.array_equal(out[:n], ref), (k, ld)
            assert np.all(out[n:] == -9.0)                       # the pad rows of a padded block keep what they held
            if k >= 3:
                assert np.all(out[:n, 0] == 0.0) and np.any(out[:n, 1] != 0.0)


def source_sets(n, k, seed):
    """k source sets on n vertices: one of 300 entries and one of 513 (more than one pass of a 256-thread block), a repeated source, the first
    and the last vertex, singletons"""
    rng = np.random.default_rng(seed)
    pick = lambda m: [int(v) for v in (rng.choice(n, m, replace=False) if m <= n else rng.integers(0, n, m))]   # noqa: E731
    sets = [[n - 1], pick(300), [0, n - 1, 0], pick(513), [n // 2, n // 2]]
    sets += [[int(rng.integers(n))] for _ in range(k - len(sets))]
    sets[k - 1] = [n - 1, 0]                                     # the last column, in the second block of k_geo_source_mean
    ptr = np.zeros(k + 1, np.int32)
    ptr[1:] = np.cumsum([len(s) for s in sets])
    return sets, ptr, np.concatenate([np.array(s, np.int32) for s in sets])


# n = 4: g / n decides the column; n k is no multiple of 256 in any case; k = 65 and 130: k_geo_source_mean's second and third block
SCATTER_SHIFT_CASES = [(4, 65), (4, 130), (777, 65), (1001, 130)]


@pytest.mark.parametrize("n,k", SCATTER_SHIFT_CASES)
def test_scatter_kernel_many_columns_and_long_lists(smg, n, k):
    L = smg._lib.load()
    assert (n * k) % 256 != 0
    sets, ptr, src = source_sets(n, k, n + k)
    for ld in (n, n + 7):
        out = np.full((ld, k), 7.0, order="F")
        rc, bad = geo_hook(L, GEO_SCATTER, n, k, src_ptr=ptr, src=src, inp=np.zeros(1), out=out, ld_out=ld)
        assert rc == 0 and bad == 0
        assert np.array_equal(out[:n], indicator(n, sets))
        assert np.all(out[n:] == 7.0)
    if n > 513:
        assert out[:n, 1].sum() == 300 and out[:n, 3].sum() == 513


@pytest.mark.parametrize("n,k", SCATTER_SHIFT_CASES)
def test_shift_kernel_many_columns_and_long_lists(smg, n, k):
    L = smg._lib.load()
    sets, ptr, src = source_sets(n, k, n + k)
    phi = np.asfortranarray(np.random.default_rng(k).uniform(-3, 3, (n, k)))
    ref = shift(phi, sets)
    for ld in (n, n + 5):
        out = np.full((ld, k), -9.0, order="F")
        rc, bad = geo_hook(L, GEO_SHIFT, n, k, src_ptr=ptr, src=src, inp=phi, out=out, ld_out=ld)
        assert rc == 0 and bad == 0
        assert np.array_equal(out[:n], ref)
        assert np.all(out[n:] == -9.0)
        assert out[n - 1, 0] == 0.0 and out[n // 2, 4] == 0.0     # one source, and one source twice: the mean is the value itself


# ---- end to end against the restatement ---------------------------------------------------------------------------------------------------
def check_e2e(geo, V, F, sets, voronoi=False):
    D = geo.distance(sets)
    Dn, t = heat_geodesics_np(V, F, sets, t=geo.t, voronoi=voronoi)
    assert abs(t - geo.t) == 0.0
    err = np.abs(D - Dn).max() / np.abs(Dn).max()
    print("max |D - D_np| / max D_np = %.2e, cycles %s" % (err, geo.cycles))
    assert err <= E2E_BOUND, err
    return D, Dn


def test_icosphere_e2e(smg, sphere, sphere_geo):
    V, F = sphere
    D, _ = check_e2e(sphere_geo, V, F, [[0], [517], [9000, 3]])
    for c, s in enumerate((0, 517)):
        assert np.abs(D[:, c] - great_circle(V, s)).max() <= 1e-2 * np.pi       # analytic: the great-circle distance
        assert D[s, c] == 0.0


def test_icosphere_voronoi_e2e(smg, sphere):
    V, F = sphere
    mg = smg.mg_precompute(V, F, 0.25, 200, 1)
    geo = smg.HeatGeodesics(mg, V, F, voronoi=True)
    del mg                                                                      # the object keeps its own copies
    check_e2e(geo, V, F, [[10]], voronoi=True)


def test_bunny_e2e(smg):
    V, F = M.read_smgm("bunny.smgm")                                           # has a boundary
    V = M.normalize_unit_area(V, F)
    mg = smg.mg_precompute(V, F, 0.25, 200, 1)
    geo = smg.HeatGeodesics(mg, V, F)
    assert len(M.boundary_loop(F)) > 0
    check_e2e(geo, V, F, [[0], [4000, 17]])


def test_bunny_subdiv_e2e(smg):
    V, F = M.read_smgm("bunny_15K_init.smgm")
    V = M.normalize_unit_area(V, F)
    mg, Vf, Ff = smg.mg_precompute_subdiv(V, F, 2, ratio=0.25, nVCoarsest=1000)
    assert Vf.shape[0] > 250000
    geo = smg.HeatGeodesics(mg, Vf, Ff)
    assert geo.device_bytes() > 0
    check_e2e(geo, Vf, Ff, [[12345], [0, 200000]])


def test_explicit_t(smg, sphere):
    V, F = sphere
    mg = smg.mg_precompute(V, F, 0.25, 200, 1)
    geo = smg.HeatGeodesics(mg, V, F, t=0.02)
    assert geo.t == 0.02
    check_e2e(geo, V, F, [[42]])


# ---- batching, determinism ----------------------------------------------------------------------------------------------------------------
def test_batched_matches_single(smg, sphere, sphere_geo):
    V, F = sphere
    n = V.shape[0]
    rng = np.random.default_rng(3)
    sets = [[int(s)] for s in rng.choice(n, 10, replace=False)] + [list(map(int, rng.choice(n, m, replace=False))) for m in (2, 3, 5, 2, 8, 4)]
    D16 = sphere_geo.distance(sets)
    assert D16.shape == (n, 16)
    worst = 0.0
    for c, s in enumerate(sets):
        D1 = sphere_geo.distance([s])[:, 0]
        worst = max(worst, np.abs(D16[:, c] - D1).max() / np.abs(D1).max())
        if len(s) == 1:
            assert D16[s[0], c] == 0.0 and D1[s[0]] == 0.0
    print("k = 16 against k = 1: max relative difference %.2e" % worst)
    # the two solves stop on the Frobenius norm over all columns: a batch and a single column stop after different cycle counts, so the
    # columns agree to the solves' tolerance, not to rounding
    assert worst <= 1e-8


def test_deterministic(smg, sphere, sphere_geo):
    sets = [[1], [2, 3000]]
    a = sphere_geo.distance(sets)
    b = sphere_geo.distance(sets)
    assert np.array_equal(a, b)
    eager = smg.SolveOpts(tol=1e-11 * np.sqrt(3), max_iter=100, use_graph=0)
    graph = smg.SolveOpts(tol=1e-11 * np.sqrt(3), max_iter=100, use_graph=1)
    po = smg.SolveOpts(tol=1e-11 * np.sqrt(2 * 4 * np.pi), max_iter=100)
    assert np.array_equal(sphere_geo.distance(sets, eager, po), sphere_geo.distance(sets, graph, po))


def test_device_memspace(smg, sphere, sphere_geo):
    import torch
    V, _ = sphere
    n = V.shape[0]
    sets = [[7], [8, 9]]
    ld = n + 3
    Dd = torch.full((2, ld), -1.0, dtype=torch.float64, device="cuda")       # column-major n x 2 with leading dimension ld
    sphere_geo.distance_device(sets, Dd.data_ptr(), ld)
    torch.cuda.synchronize()
    Dh = Dd.cpu().numpy()
    ref = sphere_geo.distance(sets)
    assert np.array_equal(Dh[:, :n].T, ref) and np.all(Dh[:, n:] == -1.0)


def test_stationary_loop_option(smg, sphere, sphere_geo):
    V, F = sphere
    sets = [[100]]
    pcg = sphere_geo.distance(sets)
    c_pcg = sphere_geo.cycles
    sphere_geo.set_solver(0, 0)
    try:
        mg = sphere_geo.distance(sets)
        c_mg = sphere_geo.cycles
    finally:
        sphere_geo.set_solver(1, 1)
    print("cycles: PCG %s, stationary %s" % (c_pcg, c_mg))
    assert np.abs(pcg - mg).max() <= 2 * E2E_BOUND * np.abs(pcg).max()


def test_solve_refusals(smg, sphere_geo):
    n = sphere_geo.n
    for bad in ([[]], [[0], []], [[n]], [[-1]], []):
        with pytest.raises(smg.SmgError) as e:
            sphere_geo.distance(bad)
        assert e.value.code == INVALID
    L = smg._lib.load()
    D = np.zeros(n)
    ptr, src = np.array([0, 1], np.int32), np.array([0], np.int32)
    ip = C.POINTER(C.c_int)
    assert L.smg_geodesics_solve(sphere_geo.g, 1, ptr.ctypes.data_as(ip), src.ctypes.data_as(ip), 0, None, None, D.ctypes.data, n - 1, None) == INVALID
    assert L.smg_geodesics_solve(sphere_geo.g, 1, ptr.ctypes.data_as(ip), src.ctypes.data_as(ip), 5, None, None, D.ctypes.data, n, None) == INVALID
