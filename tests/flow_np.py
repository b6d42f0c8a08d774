"""The numpy / scipy restatement of the conformalized mean-curvature flow (include/smg.h: smg_flow_*), in the kernels' operation order, with direct
solves for the steps; the ctypes wrappers of smg_flow_host and smg_debug_flow.

    step:        a = the barycentric masses of U;  (diag(a) - delta L_0) U' = a U;  U <- normalize_unit_area(U')
    sphericity:  c = sum a U / sum a,  r_i = |U_i - c|,  rbar = sum a r / sum a,  sqrt(sum a (r - rbar)^2 / sum a) / rbar
    sphere map:  S_i = (U_i - c) / r_i;  per face the singular values of the 3 x 2 Jacobian rest face -> sphere face in closed form

A vertex's mass is summed over its corner list, faces ascending, one slot of every vertex at a time, so the floating-point order is the kernels';
every other sum is pd_np.fixed_sum, the order of launch_fixed_sum.  Only +, -, *, / and sqrt occur: the library's host twin and its kernels are
held to this file bit for bit.  Positions are n x 3 arrays here; the library's blocks are column-major, so the wrappers pass them Fortran-ordered."""
import ctypes as C
import functools

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import morph_np
from oracle import mesh_np as M
from pd_np import EPS, corner_lists, fixed_sum  # noqa: F401  (shared with the tests)

FLOW_SYSTEM, FLOW_NORMALIZE, FLOW_SPHERICITY, FLOW_SPHERE = range(4)
LAUNCHER_MESHES = ("icosphere1", "icosphere3", "torus", "square", "bunny.smgm")     # tests/test_gpu_flow.py's table
DELTA = 0.01


# ---- meshes --------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def shape(name):
    """(V, F) of a test mesh; computed once and left unchanged by its users.  squashed: icosphere(3) with axes 1, 0.6, 0.35"""
    if name == "squashed":
        V, F = morph_np.shape("icosphere3")
        V = V * np.array([1.0, 0.6, 0.35])
    else:
        V, F = morph_np.shape(name)
    V, F = np.ascontiguousarray(V, dtype=np.float64), np.ascontiguousarray(F, dtype=np.int32)
    V.setflags(write=False)
    F.setflags(write=False)
    return V, F


def wobbled(name):
    """a state that is not the rest mesh: every vertex moved along a smooth field, nothing normalised"""
    V, _ = shape(name)
    return np.ascontiguousarray(1.7 * V + 0.05 * np.sin(3.0 * V[:, [1, 2, 0]]) + np.array([0.3, -0.2, 0.9]))


@functools.lru_cache(maxsize=None)
def cotan_csr(name):
    """(rowptr, col, L0) of the mesh's cotangent matrix with sorted rows, the stand-in for the object's L_0"""
    V, F = shape(name)
    L = sp.csr_matrix(M.cotmatrix(V, F))
    L.sort_indices()
    return L.indptr.astype(np.int32), L.indices.astype(np.int32), np.ascontiguousarray(L.data, dtype=np.float64)


# ---- the kernels' expressions ----------------------------------------------------------------------------------------------------------------------
def darea(U, F):
    a, b, c = U[F[:, 0]], U[F[:, 1]], U[F[:, 2]]
    u, v = b - a, c - a
    wx, wy, wz = u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1], u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2], u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]
    return np.sqrt(wx * wx + wy * wy + wz * wz)


def mass(U, F):
    q = darea(U, F) / 6.0
    acc = np.zeros(U.shape[0])
    for vs, ts in corner_lists(np.asarray(F), U.shape[0]):
        acc[vs] = acc[vs] + q[ts // 3]
    return acc


def diagonal(rowptr, col):
    rows = np.repeat(np.arange(rowptr.size - 1), np.diff(rowptr))
    return np.flatnonzero(col == rows)


def system(U, F, rowptr, col, L0, delta):
    """(mass, B as n x 3, val) of k_flow_system"""
    m = mass(U, F)
    val = (-delta) * L0
    d = diagonal(rowptr, col)
    val[d] = m + val[d]
    return m, m[:, None] * U, val


def normalize(U, F):
    """k_flow_normalize: divide first, then the means and the minimum of the divided columns (src/normalize_unit_area.cpp)"""
    n = U.shape[0]
    scale = np.sqrt(fixed_sum(darea(U, F)) / 2.0)
    X = U / scale
    mx, my = fixed_sum(X[:, 0]) / float(n), fixed_sum(X[:, 1]) / float(n)
    zmin = 0.0 - np.max(0.0 - X[:, 2])
    return np.stack([X[:, 0] - mx, X[:, 1] - my, X[:, 2] - zmin], axis=1)


def radius(U, c):
    d = U - c
    return np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])


def sphericity(U, F):
    """the 7 doubles of k_flow_sphericity: the sphericity, sum a, sum a U (3), sum a r, sum a (r - rbar)^2"""
    a = mass(U, F)
    s = np.zeros(7)
    s[1] = fixed_sum(a)
    for d in range(3):
        s[2 + d] = fixed_sum(a * U[:, d])
    r = radius(U, s[2:5] / s[1])
    s[5] = fixed_sum(a * r)
    rbar = s[5] / s[1]
    dev = r - rbar
    s[6] = fixed_sum(a * (dev * dev))
    s[0] = np.sqrt(s[6] / s[1]) / rbar
    return s


def dot3(a, b):
    return a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1] + a[:, 2] * b[:, 2]


def cross3(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)


def sigma_closed(V0, S, F):
    """(sigma as nF x 2, flipped as nF) of flow_sigma"""
    a, b, c = V0[F[:, 0]], V0[F[:, 1]], V0[F[:, 2]]
    p, q, r = S[F[:, 0]], S[F[:, 1]], S[F[:, 2]]
    e1, e2, s1, s2 = b - a, c - a, q - p, r - p
    x1 = np.sqrt(dot3(e1, e1))
    x2 = dot3(e1, e2) / x1
    y2 = darea(V0, F) / x1
    j1 = s1 / x1[:, None]
    j2 = (s2 - x2[:, None] * j1) / y2[:, None]
    E, G, Fm = dot3(j1, j1), dot3(j2, j2), dot3(j1, j2)
    h, g = (E + G) * 0.5, (E - G) * 0.5
    cr = cross3(j1, j2)
    sig1 = np.sqrt(h + np.sqrt(g * g + Fm * Fm))
    sig2 = np.sqrt(dot3(cr, cr)) / sig1
    nrm = cross3(s1, s2)
    cen = (p + q) + r
    return np.stack([sig1, sig2], axis=1), (dot3(nrm, cen) <= 0.0).astype(np.float64)


def sigma_svd(V0, S, F):
    """the same singular values by LAPACK: the Jacobian on an orthonormal basis of the rest face"""
    a, b, c = V0[F[:, 0]], V0[F[:, 1]], V0[F[:, 2]]
    p, q, r = S[F[:, 0]], S[F[:, 1]], S[F[:, 2]]
    e1, e2 = b - a, c - a
    t1 = e1 / np.linalg.norm(e1, axis=1)[:, None]
    nn = np.cross(e1, e2)
    t2 = np.cross(nn / np.linalg.norm(nn, axis=1)[:, None], t1)
    R = np.stack([np.stack([np.einsum("ij,ij->i", e1, t1), np.einsum("ij,ij->i", e2, t1)], axis=1),
                  np.stack([np.einsum("ij,ij->i", e1, t2), np.einsum("ij,ij->i", e2, t2)], axis=1)], axis=1)     # nF x 2 x 2: rest edges in the plane
    Sx = np.stack([q - p, r - p], axis=2)                                                                          # nF x 3 x 2: sphere edges
    return np.linalg.svd(Sx @ np.linalg.inv(R), compute_uv=False)


def sphere(U, V0, F):
    """(S, sigma as nF x 2, terms as 4 x nF, stats) of the sphere map"""
    s = sphericity(U, F)
    c = s[2:5] / s[1]
    S = (U - c) / radius(U, c)[:, None]
    sig, fl = sigma_closed(V0, S, F)
    A = darea(V0, F) * 0.5
    ratio = sig[:, 0] / sig[:, 1]
    terms = np.stack([A * ratio, A, ratio, fl])
    stats = np.array([fixed_sum(terms[0]) / fixed_sum(terms[1]), float(np.max(ratio)), fixed_sum(fl), s[0]])
    return S, sig, terms, stats


# ---- the method with direct solves -----------------------------------------------------------------------------------------------------------------
class FlowNp:
    """the flow with scipy.sparse.linalg.splu; L: the cotangent matrix of the (normalised) rest mesh, numpy's or the library's own bits"""

    def __init__(self, V, F, delta=DELTA, normalize_=True, L=None):
        self.F = np.asarray(F)
        self.V0 = normalize(np.asarray(V, dtype=np.float64), self.F) if normalize_ else np.array(V, dtype=np.float64)
        self.L = sp.csr_matrix(M.cotmatrix(self.V0, self.F) if L is None else L)
        self.delta, self.normalize_ = delta, normalize_
        self.U = self.V0.copy()

    def step(self, n=1):
        """n steps; returns the sphericity before every step and after the last one"""
        his = []
        for _ in range(n):
            his.append(sphericity(self.U, self.F)[0])
            a = mass(self.U, self.F)
            A = (sp.diags(a) - self.delta * self.L).tocsc()
            Z = spla.splu(A).solve(a[:, None] * self.U)
            self.U = normalize(Z, self.F) if self.normalize_ else Z
        his.append(sphericity(self.U, self.F)[0])
        return np.array(his)

    def sphere(self):
        return sphere(self.U, self.V0, self.F)


# ---- the library's side, shared with tests/test_gpu_flow.py ------------------------------------------------------------------------------------------
def out_size(op, nV, nF, nnz):
    return {FLOW_SYSTEM: 4 * nV + nnz, FLOW_NORMALIZE: 3 * nV, FLOW_SPHERICITY: 7, FLOW_SPHERE: 3 * nV + 6 * nF + 4}.get(op, 3 * nV)


def unpack(op, out, nV, nF):
    """SYSTEM: (mass, B as nV x 3, val); NORMALIZE: U as nV x 3; SPHERICITY: the 7 doubles; SPHERE: (S as nV x 3, sigma as nF x 2, terms as 4 x nF, stats)"""
    if op == FLOW_SYSTEM:
        return out[:nV], out[nV:4 * nV].reshape(3, nV).T, out[4 * nV:]
    if op == FLOW_NORMALIZE:
        return out.reshape(3, nV).T
    if op == FLOW_SPHERICITY:
        return out
    return (out[:3 * nV].reshape(3, nV).T, out[3 * nV:3 * nV + 2 * nF].reshape(2, nF).T, out[3 * nV + 2 * nF:3 * nV + 6 * nF].reshape(4, nF),
            out[3 * nV + 6 * nF:])


SENTINEL = -7.25e300


def _call(fn, with_guard, op, U, F, V0=None, csr=None, delta=DELTA, over=None, pad=64):
    """`pad` doubles of sentinel follow the op's extent in `out`: nothing past the extent may be written"""
    ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
    nV, nF = U.shape[0], F.shape[0]
    F = np.ascontiguousarray(F, dtype=np.int32)
    cols = lambda a: None if a is None else np.ascontiguousarray(np.asarray(a, dtype=np.float64).T).reshape(-1)   # noqa: E731  (column-major)
    keep = [cols(U), cols(V0)]
    rowptr, col, L0 = csr if csr is not None else (None, None, None)
    arr = lambda a, ty=dp: None if a is None else a.ctypes.data_as(ty)   # noqa: E731
    size = out_size(op, nV, nF, 0 if col is None else col.size)
    out = np.full(size + pad, SENTINEL)
    bad = C.c_int(-1)
    a = dict(nV=nV, nF=nF, F=arr(F, ip), U=arr(keep[0]), V0=arr(keep[1]), rowptr=arr(rowptr, ip), col=arr(col, ip), L0=arr(L0), delta=delta, out=arr(out))
    a.update(over or {})
    args = [op] + [a[key] for key in ("nV", "nF", "F", "U", "V0", "rowptr", "col", "L0", "delta", "out")]
    rc = fn(*args, C.byref(bad)) if with_guard else fn(*args)
    if rc == 0:
        assert np.all(out[size:] == SENTINEL), "op %d wrote past its extent" % op
        assert not np.any(out[:size] == SENTINEL), "op %d left a part of its extent unwritten" % op
    return rc, bad.value, out[:size]


def host(smg, op, U, F, **kw):
    """one call of smg_flow_host; returns (rc, out)"""
    rc, _, out = _call(smg._lib.load().smg_flow_host, False, op, U, F, **kw)
    return rc, out


def hook(smg, op, U, F, **kw):
    """one call of smg_debug_flow; returns (rc, guard hits, out)"""
    return _call(smg._lib.load().smg_debug_flow, True, op, U, F, **kw)


def check_launchers(run, name):
    """every op of `run(op, U, F, **operands) -> out` on one mesh against the restatement, bit for bit; shared by the host twin's and the device's tests"""
    V, F = shape(name)
    U = wobbled(name)
    n, nF = V.shape[0], F.shape[0]
    rowptr, col, L0 = cotan_csr(name)
    m, B, val = unpack(FLOW_SYSTEM, run(FLOW_SYSTEM, U, F, csr=(rowptr, col, L0), delta=0.0125), n, nF)
    mn, Bn, valn = system(U, F, rowptr, col, L0, 0.0125)
    assert np.array_equal(m, mn) and np.array_equal(B, Bn) and np.array_equal(val, valn)
    Un = normalize(U, F)
    assert np.array_equal(unpack(FLOW_NORMALIZE, run(FLOW_NORMALIZE, U, F), n, nF), Un)
    assert np.array_equal(run(FLOW_SPHERICITY, U, F), sphericity(U, F))
    S, sig, terms, stats = unpack(FLOW_SPHERE, run(FLOW_SPHERE, U, F, V0=V), n, nF)
    Sn, sign, termsn, statsn = sphere(U, V, F)
    assert np.array_equal(S, Sn) and np.array_equal(sig, sign) and np.array_equal(terms, termsn) and np.array_equal(stats, statsn)
    return m, Un, sig, S
