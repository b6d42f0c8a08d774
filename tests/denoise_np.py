"""The numpy / scipy restatement of feature-preserving denoising (include/smg.h: smg_denoise_*), with direct solves, written from the method's
formulas: the bilateral normal filter over the faces that share a vertex (Zheng, Fu, Au, Tai 2011, local scheme) and the alternating
minimisation of  E(X, t) = 1/2 sum_f sum_k w_fk |(x_i - x_j) - t_fk|^2 + fidelity / 2 sum_v M_v |x_v - V_v|^2  with t_fk orthogonal to m_f.

Sums over a neighbourhood or a corner list run in list order, one slot of every row at a time, so the floating-point order is the method's.
tests/test_denoise_host.py checks the restatement and the library's host twin; tests/test_gpu_denoise.py checks the device against it."""
import ctypes as C
import functools

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from oracle import mesh_np as M
from pd_np import EPS, corner_lists, corner_sum, fixed_sum, load_mesh  # noqa: F401  (shared with the tests)

DN_REST, DN_SPACING, DN_FILTER, DN_PROJECT, DN_RHS, DN_ENERGY = range(6)
DEFAULTS = dict(sigma_s=0.0, sigma_r=0.35, fidelity=1.0, normal_iters=20)


# ---- shapes ------------------------------------------------------------------------------------------------------------------------------------
def strip(n):
    """n faces between two rows of vertices; no vertex without a face"""
    m = n // 2 + 2
    x = np.arange(m, dtype=np.float64)
    V = np.concatenate([np.stack([x, 0.1 * np.sin(x), 0.05 * x * x / m], axis=1), np.stack([x + 0.4, 1 + 0.1 * np.cos(x), 0.2 * np.cos(x)], axis=1)])
    F = []
    for i in range(m - 1):
        F += [[i, i + 1, m + i], [i + 1, m + i + 1, m + i]]
    F = np.array(F[:n], dtype=np.int32)
    used = np.unique(F)
    return np.ascontiguousarray(V[used]), np.searchsorted(used, F).astype(np.int32)


def fan(n=65):
    """n faces around vertex 0, closed: every face shares the hub with the n - 1 others"""
    t = 2 * np.pi * np.arange(n) / n
    ring = np.stack([(1 + 0.2 * np.cos(3 * t)) * np.cos(t), (1 + 0.2 * np.cos(3 * t)) * np.sin(t), 0.3 * np.sin(2 * t)], axis=1)
    return np.concatenate([[[0.05, -0.02, 0.4]], ring]), np.array([[0, 1 + i, 1 + (i + 1) % n] for i in range(n)], dtype=np.int32)


def tetrahedron():
    V = np.array([[0.0, 0.0, 0.0], [1.0, 0.1, 0.0], [0.2, 0.9, 0.1], [0.3, 0.2, 0.8]])
    return V, np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [2, 0, 3]], dtype=np.int32)


def square2():
    V = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.1], [1.1, 0.9, 0.0], [0.0, 1.0, 0.2]])
    return V, np.array([[0, 1, 2], [0, 2, 3]], dtype=np.int32)


def edge_shapes():
    """label -> (V, F), the awkward shapes a launcher is held on: strips with one row more or fewer than a wave (63 / 64 / 65 faces) and than a
    256-thread block (strip(n) has n faces and n + 2 vertices: 253 / 254 / 255 put the vertices, 255 / 256 / 257 the faces around 256), a fan
    whose hub has 65 corners and 65 neighbours, and two meshes smaller than any block"""
    out = {"strip%d" % n: strip(n) for n in (63, 64, 65, 253, 254, 255, 256, 257)}
    out.update(fan65=fan(65), tetrahedron=tetrahedron(), square=square2())
    return out


EDGE_SHAPES = ["strip63", "strip64", "strip65", "strip253", "strip254", "strip255", "strip256", "strip257", "fan65", "tetrahedron", "square"]


def mirrored_triple():
    """three faces: face 0 shares one vertex with face 1 and one with face 2, which is face 1 mirrored in the plane x = 0 (corner by corner):
    A_1 = A_2 and |c_0 - c_1| = |c_0 - c_2| to the bit"""
    V = np.array([[-1.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [3.0, 0.0, 0.0], [2.0, 1.0, 0.0], [-3.0, 0.0, 0.0], [-2.0, 1.0, 0.0]])
    return V, np.array([[0, 1, 2], [1, 3, 4], [0, 5, 6]], dtype=np.int32)


@functools.lru_cache(maxsize=None)
def cube(n_sub=4):
    """the unit cube, midpoint-subdivided n_sub times: (V, F, prolongations); 4 gives 1 538 vertices and 3 072 faces"""
    V = np.array([[x, y, z] for x in (0.0, 1.0) for y in (0.0, 1.0) for z in (0.0, 1.0)])
    F = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4], [1, 5, 7], [1, 7, 3]],
                 dtype=np.int32)
    V, F, Ps = M.subdivision_hierarchy(V, F, n_sub)
    V.setflags(write=False)
    F.setflags(write=False)
    return V, F, Ps


def mean_edge(V, F):
    return float(np.mean([np.linalg.norm(V[F[:, i]] - V[F[:, (i + 1) % 3]], axis=1) for i in range(3)]))


def noisy(V, F, amp=0.2, seed=0):
    """V + amp x mean edge x N(0, 1) per coordinate"""
    return V + amp * mean_edge(V, F) * np.random.default_rng(seed).standard_normal(V.shape)


# ---- the fixed quantities of the input mesh ----------------------------------------------------------------------------------------------------
def rest_constants(V, F):
    """nF x 10: n (3), A, c (3), w (3); w_k = half the cotangent at corner k = (l_i^2 + l_j^2 - l_k^2) / |N| / 4 (igl::cotmatrix_entries)"""
    p0, p1, p2 = V[F[:, 0]], V[F[:, 1]], V[F[:, 2]]
    N = np.cross(p1 - p0, p2 - p0)
    dbl = np.sqrt((N[:, 0] * N[:, 0] + N[:, 1] * N[:, 1]) + N[:, 2] * N[:, 2])
    c = ((p0 + p1) + p2) / 3.0
    sq = lambda e: (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]   # noqa: E731
    l0, l1, l2 = sq(p1 - p2), sq(p2 - p0), sq(p0 - p1)
    w = np.stack([((l1 + l2) - l0) / dbl / 4.0, ((l2 + l0) - l1) / dbl / 4.0, ((l0 + l1) - l2) / dbl / 4.0], axis=1)
    return np.concatenate([N / dbl[:, None], (0.5 * dbl)[:, None], c, w], axis=1)


def face_neighbours(F, nV):
    """N(f) by sets: (ptr, idx), rows ascending"""
    at = [[] for _ in range(nV)]
    for f, tri in enumerate(F):
        for v in tri:
            at[v].append(f)
    rows = [sorted(set(g for v in tri for g in at[v]) - {f}) for f, tri in enumerate(F)]
    ptr = np.zeros(len(rows) + 1, dtype=np.int32)
    ptr[1:] = np.cumsum([len(r) for r in rows])
    return ptr, np.array([g for r in rows for g in r], dtype=np.int32)


def row_slots(ptr, idx):
    """[(faces, neighbours)] slot by slot: slot k holds the k-th neighbour of every face that has one"""
    ln = np.diff(ptr)
    return [(np.nonzero(ln > k)[0], idx[ptr[:-1][ln > k] + k]) for k in range(int(ln.max()) if ln.size else 0)]


def dist2(a, b):
    d = a - b
    return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


def spacing_terms(r, slots):
    acc = np.zeros(r.shape[0])
    for fs, gs in slots:
        acc[fs] = acc[fs] + np.sqrt(dist2(r[fs, 4:7], r[gs, 4:7]))
    return acc


def sigma_s_rule(r, ptr, slots):
    """the mean of |c_f - c_g| over the ordered pairs, summed as the library sums it"""
    return fixed_sum(spacing_terms(r, slots)) / float(ptr[-1])


# ---- the normal filter -------------------------------------------------------------------------------------------------------------------------
def filter_once(r, slots, m, sigma_s, sigma_r):
    two_ss, two_rr = 2.0 * (sigma_s * sigma_s), 2.0 * (sigma_r * sigma_r)
    s = np.zeros_like(m)
    for fs, gs in slots:
        wgt = r[gs, 3] * np.exp(0.0 - (dist2(r[fs, 4:7], r[gs, 4:7]) / two_ss + dist2(m[fs], m[gs]) / two_rr))
        s[fs] = s[fs] + wgt[:, None] * m[gs]
    ln = np.sqrt((s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2])
    ok = (ln > 0.0) & np.isfinite(ln)
    out = m.copy()
    out[ok] = s[ok] / ln[ok, None]
    return out


def filter_normals(r, slots, m, sigma_s, sigma_r, iters):
    for _ in range(iters):
        m = filter_once(r, slots, m, sigma_s, sigma_r)
    return m


def filter_largest_term(r, slots, m, sigma_s, sigma_r):
    """per face the largest |weight| of its row and |s_f|: what a filter error is measured against"""
    two_ss, two_rr = 2.0 * (sigma_s * sigma_s), 2.0 * (sigma_r * sigma_r)
    big, s = np.zeros(m.shape[0]), np.zeros_like(m)
    for fs, gs in slots:
        wgt = r[gs, 3] * np.exp(0.0 - (dist2(r[fs, 4:7], r[gs, 4:7]) / two_ss + dist2(m[fs], m[gs]) / two_rr))
        big[fs] = np.maximum(big[fs], wgt)
        s[fs] = s[fs] + wgt[:, None] * m[gs]
    return big, np.sqrt(np.sum(s * s, axis=1))


# ---- the vertex update -------------------------------------------------------------------------------------------------------------------------
def project(r, F, X, m):
    """(energy terms nF, corner shares nF x 9, the largest |w_k (x_i - x_j)| of each face)"""
    w = r[:, 7:10]
    x = [X[F[:, 0]], X[F[:, 1]], X[F[:, 2]]]
    t, h, big = [], [], np.zeros(F.shape[0])
    for k in range(3):
        d = x[(k + 1) % 3] - x[(k + 2) % 3]
        hk = (d[:, 0] * m[:, 0] + d[:, 1] * m[:, 1]) + d[:, 2] * m[:, 2]
        h.append(hk)
        t.append(w[:, k, None] * (d - hk[:, None] * m))
        big = np.maximum(big, np.abs(w[:, k]) * np.sqrt(np.sum(d * d, axis=1)))
    share = np.concatenate([t[2] - t[1], t[0] - t[2], t[1] - t[0]], axis=1)
    et = 0.5 * ((w[:, 0] * (h[0] * h[0]) + w[:, 1] * (h[1] * h[1])) + w[:, 2] * (h[2] * h[2]))
    return et, share, big


def vertices(share, lists, m0, fidelity, V, X):
    """(B nV x 3, fidelity terms nV, |B_v|^2 nV): b_v = (fidelity M_v) V_v + the corner shares in list order"""
    acc = corner_sum(share, lists, m0.size)
    w = fidelity * m0
    B = w[:, None] * V + acc
    dq = X - V
    iterm = (0.5 * w) * ((dq[:, 0] * dq[:, 0] + dq[:, 1] * dq[:, 1]) + dq[:, 2] * dq[:, 2])
    return B, iterm, (B[:, 0] * B[:, 0] + B[:, 1] * B[:, 1]) + B[:, 2] * B[:, 2]


class DenoiseNp:
    def __init__(self, V, F, **params):
        p = dict(DEFAULTS)
        p.update(params)
        self.p = p
        self.V = np.ascontiguousarray(V, dtype=np.float64)
        self.F = np.ascontiguousarray(F, dtype=np.int32)
        self.nV, self.nF = self.V.shape[0], self.F.shape[0]
        self.r = rest_constants(self.V, self.F)
        self.ptr, self.idx = face_neighbours(self.F, self.nV)
        self.slots = row_slots(self.ptr, self.idx)
        self.sigma_s = p["sigma_s"] if p["sigma_s"] > 0.0 else sigma_s_rule(self.r, self.ptr, self.slots)
        self.m0 = M.massmatrix(self.V, self.F, "voronoi").diagonal()
        self.lists = corner_lists(self.F, self.nV)
        self.A = (sp.diags(p["fidelity"] * self.m0) - M.cotmatrix(self.V, self.F)).tocsc()
        self.lu = spla.splu(self.A)
        self.m = self.r[:, :3].copy()

    def filter(self, normals=None, iters=None):
        m = self.r[:, :3] if normals is None else np.asarray(normals, dtype=np.float64)
        self.m = filter_normals(self.r, self.slots, m, self.sigma_s, self.p["sigma_r"], self.p["normal_iters"] if iters is None else iters)
        return self.m

    def local(self, X):
        """(E, B, |B|_F) at the iterate X"""
        et, share, _ = project(self.r, self.F, X, self.m)
        B, iterm, bsq = vertices(share, self.lists, self.m0, self.p["fidelity"], self.V, X)
        return float(np.sum(et) + np.sum(iterm)), B, float(np.sqrt(np.sum(bsq)))

    def update(self, X0=None, n_iter=10):
        """(X, energy_his with n_iter + 1 entries) with direct solves"""
        X = self.V.copy() if X0 is None else np.array(X0, dtype=np.float64)
        E = []
        for _ in range(n_iter):
            e, B, _ = self.local(X)
            E.append(e)
            X = self.lu.solve(B)
        E.append(self.local(X)[0])
        return X, np.array(E)

    def run(self, n_iter=10):
        self.filter()
        return self.update(None, n_iter)


def normal_error_deg(V, F, clean_normals):
    """the mean angle in degrees between the face normals of (V, F) and clean_normals"""
    n = rest_constants(V, F)[:, :3]
    return float(np.degrees(np.mean(np.arccos(np.clip(np.sum(n * clean_normals, axis=1), -1.0, 1.0)))))


@functools.lru_cache(maxsize=None)
def reference_run(name, n_iter=10):
    """(DenoiseNp, noisy V, F, filtered normals, X, energy_his) of the default run on a noisy fixture ("cube", or a mesh file normalised to unit
    area): computed once per session and left unchanged by its users"""
    if name == "cube":
        Vc, F, _ = cube(4)
    else:
        Vc, F = load_mesh(name)
    Vn = noisy(Vc, F)
    D = DenoiseNp(Vn, F)
    X, E = D.run(n_iter)
    for a in (Vn, D.m, X, E):
        a.setflags(write=False)
    return D, Vn, F, D.m, X, E


# ---- the library's side, shared with tests/test_gpu_denoise.py -----------------------------------------------------------------------------------
def params_c(smg, **params):
    p = dict(DEFAULTS)
    p.update(params)
    return smg.denoise_params(**p)


def _call(fn, op, nV, F, V0, P, inp, par, n_out, with_guard):
    ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
    F = np.ascontiguousarray(F, dtype=np.int32)
    keep = [None if a is None else np.ascontiguousarray(a, dtype=np.float64) for a in (V0, P, inp)]
    arr = lambda a: None if a is None else a.ctypes.data_as(dp)   # noqa: E731
    out = np.full(max(n_out, 1), np.nan)
    bad = C.c_int(-1)
    args = [op, nV, F.shape[0], F.ctypes.data_as(ip), arr(keep[0]), arr(keep[1]), arr(keep[2]), C.byref(par), out.ctypes.data_as(dp) if n_out else None]
    rc = fn(*args, C.byref(bad)) if with_guard else fn(*args)
    return rc, bad.value, out


def faces_host(smg, op, nV, F, V0=None, P=None, inp=None, n_out=0, **params):
    """one call of smg_denoise_faces_host; returns (rc, out)"""
    rc, _, out = _call(smg._lib.load().smg_denoise_faces_host, op, nV, F, V0, P, inp, params_c(smg, **params), n_out, False)
    return rc, out


def hook(smg, op, nV, F, V0=None, P=None, inp=None, n_out=0, **params):
    """one call of smg_debug_denoise; returns (rc, guard hits, out)"""
    return _call(smg._lib.load().smg_debug_denoise, op, nV, F, V0, P, inp, params_c(smg, **params), n_out, True)


def lib_neighbours(smg, F, nV):
    """smg_mesh_face_neighbours by its two calls -> (ptr, idx)"""
    L = smg._lib.load()
    ip = C.POINTER(C.c_int)
    F = np.ascontiguousarray(F, dtype=np.int32)
    nnz = L.smg_mesh_face_neighbours(F.ctypes.data_as(ip), F.shape[0], nV, None, None)
    assert nnz >= 0
    ptr, idx = np.full(F.shape[0] + 1, -1, dtype=np.int32), np.full(max(nnz, 1), -1, dtype=np.int32)
    assert L.smg_mesh_face_neighbours(F.ctypes.data_as(ip), F.shape[0], nV, ptr.ctypes.data_as(ip), idx.ctypes.data_as(ip)) == nnz
    return ptr, idx[:nnz]
