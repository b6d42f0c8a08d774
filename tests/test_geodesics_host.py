"""CPU: geodesic distance by the heat method (include/smg.h: smg_geodesics_*) -- the ABI and its refusals without a GPU, and the numpy / scipy
restatement of the discrete method (direct solves) that tests/test_gpu_geodesics.py checks the device against.  The restatement follows the
kernels of csrc/smg_geodesics_device.hip operation by operation (gradient basis, corner order of the divergence, list order of the shift)."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from oracle import mesh_np as M

INVALID, NO_DEVICE = -1, -2
GEO_BASIS, GEO_SCATTER, GEO_DIVERGENCE, GEO_SHIFT = 0, 1, 2, 3


# ---- meshes -------------------------------------------------------------------------------------------------------------------------------
def icosphere(level):
    """unit sphere: the icosahedron, `level` times split at edge mid-points projected to the sphere (level 5: 10 242 vertices)"""
    p = (1.0 + 5 ** 0.5) / 2
    V = [[-1, p, 0], [1, p, 0], [-1, -p, 0], [1, -p, 0], [0, -1, p], [0, 1, p], [0, -1, -p], [0, 1, -p], [p, 0, -1], [p, 0, 1], [-p, 0, -1], [-p, 0, 1]]
    F = [[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2], [10, 7, 6], [7, 1, 8],
         [3, 9, 4], [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11], [6, 2, 10], [8, 6, 7], [9, 8, 1]]
    V = [np.array(v, dtype=np.float64) / np.linalg.norm(v) for v in V]
    for _ in range(level):
        mid, NF = {}, []

        def m(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                x = V[a] + V[b]
                V.append(x / np.linalg.norm(x))
                mid[key] = len(V) - 1
            return mid[key]
        for a, b, c in F:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            NF += [[a, ab, ca], [b, bc, ab], [c, ca, bc], [ab, bc, ca]]
        F = NF
    return np.array(V), np.array(F, dtype=np.int32)


def flat_square(n=24, seed=0):
    """[0, 1]^2, an n x n grid with jittered interior vertices and random diagonals: an irregular triangulation with boundary"""
    rng = np.random.default_rng(seed)
    x, y = np.meshgrid(np.linspace(0, 1, n + 1), np.linspace(0, 1, n + 1), indexing="ij")
    V = np.stack([x.ravel(), y.ravel(), np.zeros(x.size)], axis=1)
    inner = (V[:, 0] > 0) & (V[:, 0] < 1) & (V[:, 1] > 0) & (V[:, 1] < 1)
    V[inner, :2] += rng.uniform(-0.3, 0.3, (inner.sum(), 2)) / n
    F = []
    for i in range(n):
        for j in range(n):
            a, b, c, d = i * (n + 1) + j, (i + 1) * (n + 1) + j, (i + 1) * (n + 1) + j + 1, i * (n + 1) + j + 1
            F += [[a, b, c], [a, c, d]] if rng.random() < 0.5 else [[a, b, d], [b, c, d]]
    return V, np.array(F, dtype=np.int32)


# ---- the heat method in numpy (the kernels' expressions, in their order) ----------------------------------------------------------------
def default_t(V):
    """t = (bounding-box diagonal / 12)^2"""
    diag = np.sqrt(np.sum((V.max(axis=0) - V.min(axis=0)) ** 2))
    return (diag / 12.0) * (diag / 12.0)


def grad_basis(V, F):
    """W (nF x 3 x 3): W[f, i] = (N x e_i) / (2A), e_i the edge opposite corner i (counter-clockwise); Af = A (k_geo_basis)"""
    a, b, c = V[F[:, 0]], V[F[:, 1]], V[F[:, 2]]
    u, v = b - a, c - a
    w = np.stack([u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1], u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2], u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]], axis=1)
    dA = np.sqrt(w[:, 0] * w[:, 0] + w[:, 1] * w[:, 1] + w[:, 2] * w[:, 2])
    nrm = w / dA[:, None]
    W = np.zeros((F.shape[0], 3, 3))
    for i, e in enumerate((c - b, a - c, b - a)):
        W[:, i, 0] = (nrm[:, 1] * e[:, 2] - nrm[:, 2] * e[:, 1]) / dA
        W[:, i, 1] = (nrm[:, 2] * e[:, 0] - nrm[:, 0] * e[:, 2]) / dA
        W[:, i, 2] = (nrm[:, 0] * e[:, 1] - nrm[:, 1] * e[:, 0]) / dA
    return W, dA * 0.5


def corner_lists(F, n):
    """m_ptr, m_idx: the corners t = 3f + j of every vertex, faces ascending (AssemblyPlan::m_ptr / m_idx)"""
    t = np.arange(3 * F.shape[0])
    order = np.argsort(F.ravel(), kind="stable")
    m_ptr = np.zeros(n + 1, dtype=np.int32)
    m_ptr[1:] = np.cumsum(np.bincount(F.ravel(), minlength=n))
    return m_ptr, t[order].astype(np.int32)


def neg_divergence(F, W, Af, m_ptr, m_idx, U):
    """out[v, c] = sum over v's corners in list order of A_f (W_fj . X_fc), X = -grad u / |grad u| (0 where grad u == 0) (k_geo_divergence)"""
    U = np.asarray(U, dtype=np.float64).reshape(U.shape[0], -1)
    u0, u1, u2 = U[F[:, 0]], U[F[:, 1]], U[F[:, 2]]                          # nF x k
    g = [u0 * W[:, 0, d, None] + u1 * W[:, 1, d, None] + u2 * W[:, 2, d, None] for d in range(3)]
    nrm = np.sqrt(g[0] * g[0] + g[1] * g[1] + g[2] * g[2])
    pos = nrm > 0.0
    safe = np.where(pos, nrm, 1.0)
    X = [np.where(pos, -gd / safe, 0.0) for gd in g]
    n, k = m_ptr.shape[0] - 1, U.shape[1]
    out = np.zeros((n, k))
    deg = np.diff(m_ptr)
    for p in range(deg.max()):                       # corner slot p of every vertex that has one: the sequential sum, vectorised
        vs = np.nonzero(deg > p)[0]
        t = m_idx[m_ptr[vs] + p]
        f, j = t // 3, t % 3
        dot = W[f, j, 0, None] * X[0][f] + W[f, j, 1, None] * X[1][f] + W[f, j, 2, None] * X[2][f]
        out[vs] += Af[f, None] * dot
    return out


def indicator(n, sets):
    B = np.zeros((n, len(sets)), order="F")
    for c, s in enumerate(sets):
        B[list(s), c] = 1.0
    return B


def shift(phi, sets):
    """D = phi - the mean of phi over each column's sources, summed in list order (k_geo_source_mean / k_geo_shift)"""
    D = np.empty_like(phi)
    for c, s in enumerate(sets):
        acc = 0.0
        for v in s:
            acc += phi[v, c]
        D[:, c] = phi[:, c] - acc / len(s)
    return D


def heat_geodesics_np(V, F, sets, t=None, voronoi=False, heat_noise=0.0, seed=0):
    """the discrete heat method with direct solves: returns (D, t).  heat_noise: uniform noise of that size relative to max |u| added to
    the heat solution (a stand-in for an iterative solve's error)."""
    n = V.shape[0]
    t = default_t(V) if t is None else t
    L = M.cotmatrix(V, F).tocsc()
    Mm = M.massmatrix(V, F, "voronoi" if voronoi else "barycentric")
    U = spla.splu((Mm - t * L).tocsc()).solve(indicator(n, sets))
    if heat_noise:
        U = U + heat_noise * np.abs(U).max() * np.random.default_rng(seed).uniform(-1, 1, U.shape)
    W, Af = grad_basis(V, F)
    m_ptr, m_idx = corner_lists(F, n)
    b = neg_divergence(F, W, Af, m_ptr, m_idx, U)
    K = (-L).tocsc()[1:, 1:]                        # vertex 0 pinned at 0
    phi = np.zeros_like(b)
    phi[1:] = spla.splu(K.tocsc()).solve(b[1:])
    return shift(phi, sets), t


def great_circle(V, s):
    return np.arccos(np.clip(V @ V[s], -1.0, 1.0))


# ---- the restatement against exact distances ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sphere5():
    return icosphere(5)


def test_icosphere_default_t_against_great_circle(sphere5):
    V, F = sphere5
    assert V.shape[0] == 10242
    srcs = [0, 517, 9000]
    D, t = heat_geodesics_np(V, F, [[s] for s in srcs])
    assert abs(t - (2 * np.sqrt(3) / 12) ** 2) < 1e-3       # the bounding box of the unit sphere is nearly the cube [-1, 1]^3
    for c, s in enumerate(srcs):
        err = np.abs(D[:, c] - great_circle(V, s)).max()
        assert D[s, c] == 0.0
        assert err <= 1e-2 * np.pi, (s, err / np.pi)


def test_icosphere_default_t_tolerates_solver_noise(sphere5):
    """the reason for the default t: at t = h^2 a relative error of 1e-10 in u ruins the far side; at the default it does not"""
    V, F = sphere5
    h = np.mean(np.linalg.norm(V[F[:, 0]] - V[F[:, 1]], axis=1))
    exact = great_circle(V, 0)
    D_small, _ = heat_geodesics_np(V, F, [[0]], t=h * h, heat_noise=1e-10)
    D_dflt, _ = heat_geodesics_np(V, F, [[0]], heat_noise=1e-10)
    assert np.abs(D_small[:, 0] - exact).max() > 0.1 * np.pi
    assert np.abs(D_dflt[:, 0] - exact).max() <= 1e-2 * np.pi


def test_flat_square_against_euclidean():
    V, F = flat_square(24)
    s = int(np.argmin(np.linalg.norm(V[:, :2] - 0.5, axis=1)))
    D, _ = heat_geodesics_np(V, F, [[s]])
    exact = np.linalg.norm(V - V[s], axis=1)
    err = np.abs(D[:, 0] - exact).max()
    # measured: 0.067 of the largest distance from the centre, 0.049 from a corner, at the default t (the Neumann heat step bends the
    # distance near the boundary; at t = h^2 0.049 / 0.031)
    assert err <= 0.08 * exact.max(), err / exact.max()
    D2, _ = heat_geodesics_np(V, F, [[0]])          # a corner source: the same bound
    exact2 = np.linalg.norm(V - V[0], axis=1)
    assert np.abs(D2[:, 0] - exact2).max() <= 0.08 * exact2.max()


def test_multi_source_is_distance_to_the_nearest(sphere5):
    V, F = sphere5
    D, _ = heat_geodesics_np(V, F, [[0, 3]])
    exact = np.minimum(great_circle(V, 0), great_circle(V, 3))
    assert np.abs(D[:, 0] - exact).max() <= 1e-2 * np.pi        # measured 2.1e-3 pi at the default t


# ---- the ABI without a GPU ----------------------------------------------------------------------------------------------------------------
def _create(L, h, V, F, t=0.0, voronoi=0, nV=None):
    out = C.c_void_p()
    V = np.ascontiguousarray(V, dtype=np.float64)
    F = np.ascontiguousarray(F, dtype=np.int32)
    rc = L.smg_geodesics_create(h, V.ctypes.data_as(C.POINTER(C.c_double)), V.shape[0] if nV is None else nV,
                                F.ctypes.data_as(C.POINTER(C.c_int)), F.shape[0], t, voronoi, C.byref(out))
    if rc == 0:
        L.smg_geodesics_destroy(out)
    return rc


def _fake_hierarchy(smg, n):
    """a 2-level handle whose level 0 has n rows: the create checks read nothing else of it"""
    H = smg.Hierarchy(2)
    H.set_prolong(1, sp.csr_matrix(np.ones((n, 1))))
    return H


def test_abi_present(smg_mod):
    L = smg_mod._lib.load()
    for name in ("smg_geodesics_create", "smg_geodesics_destroy", "smg_geodesics_time", "smg_geodesics_set_solver", "smg_geodesics_device_bytes",
                 "smg_geodesics_solve", "smg_debug_geodesics"):
        assert hasattr(L, name)
    assert hasattr(smg_mod, "HeatGeodesics")
    assert L.smg_geodesics_time(None) == 0.0 and L.smg_geodesics_device_bytes(None) == 0
    assert L.smg_geodesics_set_solver(None, 1, 1) == INVALID


def test_create_refusals(smg_mod):
    smg = smg_mod
    L = smg._lib.load()
    V, F = icosphere(3)
    n = V.shape[0]
    mg = smg.mg_precompute(V, F, 0.25, 50, 1)
    assert mg.n_levels == 2
    assert _create(L, None, V, F) == INVALID                                      # null arguments
    out = C.c_void_p()
    assert L.smg_geodesics_create(mg.h, None, n, F.ctypes.data_as(C.POINTER(C.c_int)), F.shape[0], 0.0, 0, C.byref(out)) == INVALID
    assert L.smg_geodesics_create(mg.h, V.ctypes.data_as(C.POINTER(C.c_double)), n, None, F.shape[0], 0.0, 0, C.byref(out)) == INVALID
    assert L.smg_geodesics_create(mg.h, V.ctypes.data_as(C.POINTER(C.c_double)), n, F.ctypes.data_as(C.POINTER(C.c_int)), F.shape[0], 0.0, 0,
                                  None) == INVALID
    assert _create(L, mg.h, V[:-1], F, nV=n - 1) == INVALID                        # nV != rows of level 0
    for t in (float("nan"), float("inf"), -1.0):                                  # t not finite (or negative)
        assert _create(L, mg.h, V, F, t=t) == INVALID
    blk = smg.mg_precompute_block(V, F, 0.25, 50, 1)                              # block (3-DOF) hierarchy, with and without the row match
    assert _create(L, blk.h, V, F) == INVALID
    V3 = np.concatenate([V, V + 3.0, V + 6.0])
    F3 = np.concatenate([F, F + n, F + 2 * n])
    assert _create(L, blk.h, V3, F3) == INVALID
    un = smg.Hierarchy.union([mg, mg])                                             # union handle
    V2, F2 = np.concatenate([V, V + 3.0]), np.concatenate([F, F + n])
    assert _create(L, un.h, V2, F2) == INVALID
    two = _fake_hierarchy(smg, 2 * n)                                              # two connected components
    assert _create(L, two.h, V2, F2) == INVALID
    iso = _fake_hierarchy(smg, n + 1)                                              # a vertex in no face
    assert _create(L, iso.h, np.concatenate([V, [[5.0, 5.0, 5.0]]]), F) == INVALID
    fake = _fake_hierarchy(smg, n)
    Fz = F.copy()
    Vz = V.copy()
    Vz[F[0, 1]] = Vz[F[0, 0]]                                                      # a face with zero double area
    assert _create(L, fake.h, Vz, Fz) == INVALID
    Fo = F.copy()
    Fo[3, 2] = n                                                                   # a face index out of range
    assert _create(L, fake.h, V, Fo) == INVALID
    if L.smg_device_count() == 0:
        assert _create(L, mg.h, V, F) == NO_DEVICE                                 # valid arguments: the device is what is missing
        assert _create(L, fake.h, V, F, t=0.5, voronoi=1) == NO_DEVICE


def test_solve_refusals_without_object(smg_mod):
    L = smg_mod._lib.load()
    ptr = np.array([0, 1], dtype=np.int32)
    src = np.array([0], dtype=np.int32)
    D = np.zeros(4)
    assert L.smg_geodesics_solve(None, 1, ptr.ctypes.data_as(C.POINTER(C.c_int)), src.ctypes.data_as(C.POINTER(C.c_int)), 0, None, None,
                                 D.ctypes.data, 4, None) == INVALID


def geo_hook(L, op, n, k=1, F=None, m_ptr=None, m_idx=None, src_ptr=None, src=None, inp=None, W=None, Af=None, out=None, ld_out=None):
    """one call of smg_debug_geodesics; returns (rc, guard_bad)"""
    ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
    arr = lambda a, t: None if a is None else a.ctypes.data_as(t)   # noqa: E731
    bad = C.c_int(-1)
    nF = 0 if F is None else F.shape[0]
    rc = L.smg_debug_geodesics(op, n, nF, k, arr(F, ip), arr(m_ptr, ip), arr(m_idx, ip), arr(src_ptr, ip), arr(src, ip), arr(inp, dp), arr(W, dp),
                               arr(Af, dp), arr(out, dp), ld_out if ld_out is not None else n, C.byref(bad))
    return rc, bad.value


def test_hook_refusals(smg_mod):
    L = smg_mod._lib.load()
    V, F = icosphere(1)
    n = V.shape[0]
    m_ptr, m_idx = corner_lists(F, n)
    W, Af = np.zeros(9 * F.shape[0]), np.zeros(F.shape[0])
    out = np.zeros((n, 2), order="F")
    ok_ptr, ok_src = np.array([0, 1, 3], np.int32), np.array([0, 4, 5], np.int32)
    U = np.zeros((n, 2), order="F")
    assert geo_hook(L, 7, n, 2, src_ptr=ok_ptr, src=ok_src, inp=U, out=out)[0] == INVALID                     # unknown op
    assert geo_hook(L, GEO_SCATTER, n, 0, src_ptr=ok_ptr, src=ok_src, inp=U, out=out)[0] == INVALID           # k < 1
    assert geo_hook(L, GEO_SCATTER, n, 2, src_ptr=np.array([0, 1, 1], np.int32), src=ok_src, inp=U, out=out)[0] == INVALID   # empty set
    assert geo_hook(L, GEO_SCATTER, n, 2, src_ptr=ok_ptr, src=np.array([0, n, 1], np.int32), inp=U, out=out)[0] == INVALID   # out of range
    assert geo_hook(L, GEO_SHIFT, n, 2, src_ptr=ok_ptr, src=np.array([-1, 2, 1], np.int32), inp=U, out=out)[0] == INVALID
    assert geo_hook(L, GEO_SHIFT, n, 2, src_ptr=ok_ptr, src=ok_src, inp=U, out=out, ld_out=n - 1)[0] == INVALID  # ld_out < n
    Fb = F.copy()
    Fb[0, 0] = n
    assert geo_hook(L, GEO_DIVERGENCE, n, 2, F=Fb, m_ptr=m_ptr, m_idx=m_idx, inp=U, W=W, Af=Af, out=out)[0] == INVALID
    mb = m_idx.copy()
    mb[0] = 3 * F.shape[0]
    assert geo_hook(L, GEO_DIVERGENCE, n, 2, F=F, m_ptr=m_ptr, m_idx=mb, inp=U, W=W, Af=Af, out=out)[0] == INVALID
    assert geo_hook(L, GEO_BASIS, n, 1, F=F, inp=V.copy(), W=None, Af=Af)[0] == INVALID
    if L.smg_device_count() == 0:
        assert geo_hook(L, GEO_SCATTER, n, 2, src_ptr=ok_ptr, src=ok_src, inp=U, out=out)[0] == NO_DEVICE
        assert geo_hook(L, GEO_BASIS, n, 1, F=F, inp=np.ascontiguousarray(V), W=W, Af=Af)[0] == NO_DEVICE


def test_python_sources_layout(smg_mod):
    k, ptr, src = smg_mod.HeatGeodesics._sources(5)
    assert k == 1 and list(ptr) == [0, 1] and list(src) == [5]
    k, ptr, src = smg_mod.HeatGeodesics._sources([3, [1, 2, 2], [7]])
    assert k == 3 and list(ptr) == [0, 1, 4, 5] and list(src) == [3, 1, 2, 2, 7]
