"""The numpy / scipy restatement of the Helmholtz-Hodge decomposition of per-face fields (include/smg.h: smg_hodge_*), in the kernels' operation
order, with direct solves for the two Poisson systems; the ctypes wrappers of smg_hodge_host and smg_debug_hodge.

    Xt = G + R + H,   G_f = sum_i u_i W_fi,   R_f = n_f x sum_i v_i W_fi,   H = (Xt - G) - R
    (-L) u = b,  b_i = (1/2) sum (n_f x e_fi) . X_f;     (-L) v = c,  c_i = -(1/2) sum e_fi . X_f
    u: vertex 0 known and 0;  v: the same on a closed mesh, every boundary vertex known and 0 on a mesh with boundary

The sums over a corner list run in list order, one slot of every vertex at a time, so the floating-point order is the kernels'; the energies are
pd_np.fixed_sum, the order of launch_fixed_sum.  Only +, -, *, / and sqrt occur: the library's host twin and its kernels are held to this file bit
for bit.  Fields are k x nF x 3 arrays and potentials nV x k arrays here; the library's potential blocks are column-major."""
import ctypes as C
import functools

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import morph_np
from morph_np import rest_faces
from oracle import mesh_np as M
from pd_np import EPS, corner_lists, fixed_sum  # noqa: F401  (shared with the tests)

HODGE_RHS, HODGE_PARTS, HODGE_FIELD = range(3)
LAUNCHER_MESHES = ("icosphere1", "icosphere3", "torus", "square", "bunny.smgm")


# ---- meshes and fields ---------------------------------------------------------------------------------------------------------------------------
def double_pyramid(nV):
    """a closed double pyramid: a ring of nV - 2 vertices on a wavy ellipse, one apex above and one below (tests/hodge_asan_driver.cpp's mesh)"""
    ring = nV - 2
    a = 2.0 * np.pi * np.arange(ring) / ring
    V = np.zeros((nV, 3))
    V[:ring] = np.stack([1.3 * np.cos(a), 0.8 * np.sin(a), 0.1 * np.sin(3.0 * a)], axis=1)
    V[nV - 2, 2], V[nV - 1, 2] = 0.9, -0.7
    i = np.arange(ring)
    j = (i + 1) % ring
    F = np.stack([np.stack([i, j, np.full(ring, nV - 2)], axis=1), np.stack([j, i, np.full(ring, nV - 1)], axis=1)], axis=1).reshape(-1, 3)
    return V, F


@functools.lru_cache(maxsize=None)
def shape(name):
    """(V, F) of a test mesh; computed once and left unchanged by its users.  pyramidN: double_pyramid(N); else morph_np.shape"""
    if name.startswith("pyramid"):
        V, F = double_pyramid(int(name[len("pyramid"):]))
    else:
        V, F = morph_np.shape(name)
    V, F = np.ascontiguousarray(V, dtype=np.float64), np.ascontiguousarray(F, dtype=np.int32)
    V.setflags(write=False)
    F.setflags(write=False)
    return V, F


def centroids(V, F):
    return (V[F[:, 0]] + V[F[:, 1]] + V[F[:, 2]]) / 3.0


def smooth_field(V, F, k=1):
    """k x nF x 3: omega_s x c_f + a_s + 0.3 sin((2 + s) c_f[[1, 2, 0]]) at the face centroids c_f; it is not tangent"""
    c = centroids(V, F)
    out = []
    for s in range(k):
        omega = np.array([0.3 + 0.2 * s, -0.5, 0.8 - 0.1 * s])
        a = np.array([0.2, 0.1 * s, -0.3])
        out.append(np.cross(omega, c) + a + 0.3 * np.sin((2.0 + s) * c[:, [1, 2, 0]]))
    return np.ascontiguousarray(np.stack(out))


def dalpha_field(V, F):
    """1 x nF x 3: (-y, x, 0) / (x^2 + y^2) at the centroids, the harmonic 1-form d alpha of a torus about the z axis"""
    c = centroids(V, F)
    r2 = c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]
    return np.ascontiguousarray(np.stack([-c[:, 1] / r2, c[:, 0] / r2, np.zeros(c.shape[0])], axis=1)[None])


def potentials(V, k=1, seed=None):
    """(u0, v0), nV x k each: smooth functions of the positions, or with a seed standard normal values"""
    if seed is not None:
        rng = np.random.default_rng(seed)
        return rng.standard_normal((V.shape[0], k)), rng.standard_normal((V.shape[0], k))
    s = np.arange(k)[None, :]
    u = np.sin((3.0 + s) * V[:, [0]]) + V[:, [1]] * V[:, [2]] + 0.1 * s
    v = np.cos((2.0 + s) * V[:, [1]]) - 0.5 * V[:, [0]] * V[:, [2]]
    return np.ascontiguousarray(u), np.ascontiguousarray(v)


def boundary_vertices(F):
    """the vertices of the edges that one face alone holds, ascending"""
    e = np.sort(np.concatenate([F[:, [0, 1]], F[:, [1, 2]], F[:, [2, 0]]]), axis=1)
    uniq, cnt = np.unique(e, axis=0, return_counts=True)
    return np.unique(uniq[cnt == 1])


# ---- the kernels' expressions ----------------------------------------------------------------------------------------------------------------------
def dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def cross3(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def rhs(V, F, X):
    """(b, c as nV x k, bsq as 2 x k x nV) of k_hodge_rhs"""
    nV, k = V.shape[0], X.shape[0]
    _, nrm, _ = rest_faces(V, F)
    a, b, c = V[F[:, 0]], V[F[:, 1]], V[F[:, 2]]
    E = np.stack([c - b, a - c, b - a], axis=1)                      # nF x 3 (corner) x 3
    NE = cross3(nrm[:, None, :], E)
    tb = dot3(NE[None], X[:, :, None, :]).reshape(k, -1)             # k x 3 nF: corner t = 3 f + j
    tc = dot3(E[None], X[:, :, None, :]).reshape(k, -1)
    accb, accc = np.zeros((k, nV)), np.zeros((k, nV))
    for vs, ts in corner_lists(np.asarray(F), nV):
        accb[:, vs] = accb[:, vs] + tb[:, ts]
        accc[:, vs] = accc[:, vs] + tc[:, ts]
    bv, cv = 0.5 * accb, -0.5 * accc
    return np.ascontiguousarray(bv.T), np.ascontiguousarray(cv.T), np.stack([bv * bv, cv * cv])


def grad(W, F, u):
    """k x nF x 3: sum_i u_i W_fi, i in order"""
    u0, u1, u2 = u[F[:, 0]].T[:, :, None], u[F[:, 1]].T[:, :, None], u[F[:, 2]].T[:, :, None]      # k x nF x 1
    return (u0 * W[None, :, 0, :] + u1 * W[None, :, 1, :]) + u2 * W[None, :, 2, :]


def parts(V, F, X, u, v):
    """(parts as k x nF x 9, terms as 4 k x nF, energy as 4 k) of k_hodge_parts and the sums"""
    W, nrm, A = rest_faces(V, F)
    xn = dot3(X, nrm[None])
    Xt = X - xn[:, :, None] * nrm[None]
    G = grad(W, F, u)
    R = cross3(nrm[None], grad(W, F, v))
    H = (Xt - G) - R
    terms = np.stack([A[None] * dot3(q, q) for q in (Xt, G, R, H)], axis=1).reshape(-1, F.shape[0])     # plane 4 s + e
    return np.concatenate([G, R, H], axis=2), terms, np.array([fixed_sum(t) for t in terms])


def field(V, F, u, v):
    """k x nF x 3: grad u + n x grad v"""
    W, nrm, _ = rest_faces(V, F)
    return grad(W, F, u) + cross3(nrm[None], grad(W, F, v))


def inner(A, P, Q):
    """the area inner products of two k x nF x 3 fields, per set"""
    return np.array([np.sum(A * np.einsum("fd,fd->f", p, q)) for p, q in zip(P, Q)])


# ---- the method with direct solves -----------------------------------------------------------------------------------------------------------------
class HodgeNp:
    """the whole query with scipy.sparse.linalg.splu on -L with the known rows removed; L: the cotangent matrix, numpy's or the library's own bits"""

    def __init__(self, V, F, L=None):
        self.V, self.F = np.asarray(V, dtype=np.float64), np.asarray(F)
        n = self.V.shape[0]
        self.A = sp.csr_matrix(-(M.cotmatrix(self.V, self.F) if L is None else L))
        self.bnd = boundary_vertices(self.F)
        self.closed = self.bnd.size == 0
        self.Iu = np.arange(1, n)
        self.Iv = self.Iu if self.closed else np.setdiff1d(np.arange(n), self.bnd)
        self.Auu = self.A[self.Iu][:, self.Iu].tocsc()
        self.Avv = self.Auu if self.closed else self.A[self.Iv][:, self.Iv].tocsc()
        self.lu_u = spla.splu(self.Auu)
        self.lu_v = self.lu_u if self.closed else spla.splu(self.Avv)

    def lam_min(self):
        """the smallest eigenvalues of -L over the unknown rows of the u and of the v system"""
        one = lambda A: float(spla.eigsh(A, k=1, sigma=0.0, which="LM", return_eigenvectors=False)[0])   # noqa: E731
        lu = one(self.Auu)
        return lu, (lu if self.closed else one(self.Avv))

    def solve(self, b, c):
        """(u, v, |b - (-L) u|_2 and |c - (-L) v|_2 over the unknown rows, per set)"""
        n, k = b.shape
        u, v = np.zeros((n, k)), np.zeros((n, k))
        u[self.Iu] = self.lu_u.solve(b[self.Iu])
        v[self.Iv] = self.lu_v.solve(c[self.Iv])
        ru = np.linalg.norm(b[self.Iu] - self.Auu @ u[self.Iu], axis=0)
        rv = np.linalg.norm(c[self.Iv] - self.Avv @ v[self.Iv], axis=0)
        return u, v, ru, rv

    def decompose(self, X):
        """X: k x nF x 3 -> dict(u, v, parts, terms, energy, b, c, ru, rv)"""
        b, c, _ = rhs(self.V, self.F, X)
        u, v, ru, rv = self.solve(b, c)
        P, terms, energy = parts(self.V, self.F, X, u, v)
        return dict(u=u, v=v, parts=P, terms=terms, energy=energy.reshape(-1, 4), b=b, c=c, ru=ru, rv=rv)


# ---- the library's side, shared with tests/test_gpu_hodge.py -----------------------------------------------------------------------------------------
def out_size(op, nV, nF, k):
    return {HODGE_RHS: 4 * nV * k, HODGE_PARTS: 13 * nF * k + 4 * k, HODGE_FIELD: 3 * nF * k}.get(op, 3 * nF * k)


def unpack(op, out, nV, nF, k):
    """RHS: (b, c as nV x k, bsq as 2 x k x nV); PARTS: (parts as k x nF x 9, terms as 4 k x nF, energy as 4 k); FIELD: X as k x nF x 3"""
    if op == HODGE_RHS:
        return out[:nV * k].reshape(k, nV).T, out[nV * k:2 * nV * k].reshape(k, nV).T, out[2 * nV * k:].reshape(2, k, nV)
    if op == HODGE_PARTS:
        return out[:9 * nF * k].reshape(k, nF, 9), out[9 * nF * k:13 * nF * k].reshape(4 * k, nF), out[13 * nF * k:]
    return out.reshape(k, nF, 3)


SENTINEL = -7.25e300


def _call(fn, with_guard, op, V, F, k=1, X=None, u=None, v=None, over=None, pad=64):
    """`pad` doubles of sentinel follow the op's extent in `out`: nothing past the extent may be written"""
    ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
    nV, nF = V.shape[0], F.shape[0]
    F = np.ascontiguousarray(F, dtype=np.int32)
    rows = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64).reshape(-1)                 # noqa: E731
    cols = lambda a: None if a is None else np.ascontiguousarray(np.asarray(a, dtype=np.float64).T).reshape(-1)   # noqa: E731  (column-major)
    keep = [rows(V), rows(X), cols(u), cols(v)]
    arr = lambda a, ty=dp: None if a is None else a.ctypes.data_as(ty)   # noqa: E731
    size = out_size(op, nV, nF, max(k, 0))
    out = np.full(size + pad, SENTINEL)
    bad = C.c_int(-1)
    a = dict(nV=nV, nF=nF, k=k, F=arr(F, ip), V=arr(keep[0]), X=arr(keep[1]), u=arr(keep[2]), v=arr(keep[3]), out=arr(out))
    a.update(over or {})
    args = [op] + [a[key] for key in ("nV", "nF", "k", "F", "V", "X", "u", "v", "out")]
    rc = fn(*args, C.byref(bad)) if with_guard else fn(*args)
    if rc == 0:
        assert np.all(out[size:] == SENTINEL), "op %d wrote past its extent" % op
        assert not np.any(out[:size] == SENTINEL), "op %d left a part of its extent unwritten" % op
    return rc, bad.value, out[:size]


def host(smg, op, V, F, **kw):
    """one call of smg_hodge_host; returns (rc, out)"""
    rc, _, out = _call(smg._lib.load().smg_hodge_host, False, op, V, F, **kw)
    return rc, out


def hook(smg, op, V, F, **kw):
    """one call of smg_debug_hodge; returns (rc, guard hits, out)"""
    return _call(smg._lib.load().smg_debug_hodge, True, op, V, F, **kw)


def check_launchers(run, name, k):
    """every op of `run(op, V, F, **operands) -> out` on one mesh against the restatement, bit for bit; shared by the host twin's and the device's
    tests.  Returns the outputs for a comparison of the two."""
    V, F = shape(name)
    n, nF = V.shape[0], F.shape[0]
    X = smooth_field(V, F, k)
    u0, v0 = potentials(V, k)
    outs = [run(HODGE_RHS, V, F, k=k, X=X), run(HODGE_PARTS, V, F, k=k, X=X, u=u0, v=v0), run(HODGE_FIELD, V, F, k=k, u=u0, v=v0)]
    b, c, bsq = unpack(HODGE_RHS, outs[0], n, nF, k)
    bn, cn, bsqn = rhs(V, F, X)
    assert np.array_equal(b, bn) and np.array_equal(c, cn) and np.array_equal(bsq, bsqn), name
    P, terms, energy = unpack(HODGE_PARTS, outs[1], n, nF, k)
    Pn, termsn, energyn = parts(V, F, X, u0, v0)
    assert np.array_equal(P, Pn) and np.array_equal(terms, termsn) and np.array_equal(energy, energyn), name
    assert np.array_equal(unpack(HODGE_FIELD, outs[2], n, nF, k), field(V, F, u0, v0)), name
    return outs
