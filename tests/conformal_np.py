"""The numpy / scipy restatement of the discrete conformal metric (include/smg.h: smg_conformal_*; Springborn, Schroeder, Pinkall 2008), in the
kernels' operation order, with direct solves for the Newton steps; the unfolding of a flat metric; the mesh table of the tests; the ctypes
wrappers of smg_conformal_host and smg_debug_conformal.

    rest     l0[f][c] = the length of the edge opposite corner c (the expressions of k_face_terms)
    scale    s = exp(-u / 2)
    face     a_c = l0[f][c] s[F[f][c]];  S = a + b + c, s0 = b + c - a, s1 = a + c - b, s2 = a + b - c;
             angle 0 = 2 atan2(sqrt(s1 s2), sqrt(S s0)), half cotangent 0 = (b b + c c - a a) / sqrt(S s0 s1 s2) / 2, cyclically, formed as
             (b b + c c - a a) / (dA0 r) / 4: dA0 = twice the rest area by the cross product (smg_mesh_cotmatrix's dA), r = sqrt(S s0 s1 s2)
             over the same root of the rest lengths, exactly 1 at s = 1, where the values are smg_mesh_cotmatrix's own bits;
             some s_c <= 0: broken, the angle opposite the too-long edge pi, the others 0, the half cotangents 0
    rows     angle sum over the corner list, faces ascending; g = sum - Theta, 0 on fixed rows; -L~ in smg_mesh_cotmatrix's CSR and term order
    Newton   (-L~)_uu d = g_u;  t = 1, 1/2, ...: accepted when |g(u + t d)|_2 <= (1 - 1e-4 t) |g(u)|_2;  stop at max |g| <= grad_tol

Given the same s, half cotangents, flags, lengths and matrix values are +, -, *, / and sqrt in one order on every side: bit for bit.  exp and
atan2 come from the platform's libm here and from the device's library there: held to bounds (tests/test_conformal_host.py).  The norms are
pd_np.fixed_sum, the order of launch_fixed_sum."""
import ctypes as C
import functools

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import flow_np
from pd_np import EPS, corner_lists, fixed_sum  # noqa: F401  (shared with the tests)
from test_geodesics_host import flat_square

SCALE, FACES, ROWS = range(3)
LAUNCHER_MESHES = ("icosphere1", "icosphere3", "torus", "square", "bunny.smgm")
SENTINEL = -7.25e300
PI = float(np.pi)


# ---- meshes --------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def shape(name):
    """(V, F) of a test mesh; computed once and left unchanged.  squashed: icosphere(3) with axes 1, 0.6, 0.35 (flow_np); bumped: flat_square(12)
    with z = 0.3 sin(2.5 x) cos(2 y); flat: flat_square(12) itself"""
    if name == "bumped" or name == "flat":
        V, F = flat_square(12)
        V = np.array(V, dtype=np.float64)
        if name == "bumped":
            V[:, 2] = 0.3 * np.sin(2.5 * V[:, 0]) * np.cos(2.0 * V[:, 1])
    else:
        V, F = flow_np.shape(name)
    V, F = np.ascontiguousarray(V, dtype=np.float64), np.ascontiguousarray(F, dtype=np.int32)
    V.setflags(write=False)
    F.setflags(write=False)
    return V, F


def boundary_vertices(F):
    e = np.concatenate([F[:, [1, 2]], F[:, [2, 0]], F[:, [0, 1]]])
    e = np.sort(e, axis=1)
    uniq, cnt = np.unique(e, axis=0, return_counts=True)
    return np.unique(uniq[cnt == 1]).astype(np.int32)


def nearest(V, dirs):
    """the vertex nearest to every direction, on the normalised positions"""
    Vn = V / np.linalg.norm(V, axis=1)[:, None]
    D = np.asarray(dirs, dtype=np.float64)
    D = D / np.linalg.norm(D, axis=1)[:, None]
    return np.argmax(Vn @ D.T, axis=0).astype(np.int32)


CUBE = [[a, b, c] for a in (-1, 1) for b in (-1, 1) for c in (-1, 1)]
TETRA = [[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]]


def smooth_u(V):
    """a smooth non-zero u for the launcher tests and the known-u* case: 0.3 sin(3 x) + 0.8 y z"""
    return 0.3 * np.sin(3.0 * V[:, 0]) + 0.8 * V[:, 1] * V[:, 2]


@functools.lru_cache(maxsize=None)
def case(name):
    """(mesh name, fixed, Theta, expected Newton steps) of the end-to-end table; known: Theta is the angle sums of u* = smooth_u shifted to u*_0 = 0"""
    if name == "known":
        mesh, steps = "squashed", 3
        V, F = shape(mesh)
        fixed = np.array([0], np.int32)
        ustar = smooth_u(V)
        ustar = ustar - ustar[0]
        Theta = ConformalNp(V, F, fixed).evaluate(ustar, np.zeros(V.shape[0]))["sum"]
    elif name == "torus":
        mesh, steps = "torus", 3
        V, F = shape(mesh)
        fixed, Theta = np.array([0], np.int32), np.full(V.shape[0], 2.0 * PI)
    elif name in ("cones8", "cones4", "cones4_ico2"):
        mesh = "icosphere2" if name.endswith("ico2") else "icosphere3"
        steps = 4 if name == "cones8" else 5
        V, F = shape(mesh)
        cones = nearest(V, CUBE if name == "cones8" else TETRA)
        Theta = np.full(V.shape[0], 2.0 * PI)
        Theta[cones] = 1.5 * PI if name == "cones8" else PI
        fixed = np.array([min(set(range(V.shape[0])) - set(cones.tolist()))], np.int32)
    else:
        mesh, steps = (name, 3) if name == "bumped" else ("bunny.smgm", 4)
        V, F = shape(mesh)
        fixed, Theta = boundary_vertices(F), np.full(V.shape[0], 2.0 * PI)
    Theta.setflags(write=False)
    fixed.setflags(write=False)
    return mesh, fixed, Theta, steps


# ---- the kernels' expressions ----------------------------------------------------------------------------------------------------------------------
def rest_lengths(V, F):
    a, b, c = V[F[:, 0]], V[F[:, 1]], V[F[:, 2]]
    out = []
    for d in (b - c, c - a, a - b):
        out.append(np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]))
    return np.stack(out, axis=1)


def rest_area2(V, F):
    """twice the rest area of every face: the cross product's norm, the dA of k_face_terms and smg_mesh_cotmatrix"""
    return flow_np.darea(V, F)


def heron(a, b, c):
    S, s0, s1, s2 = a + b + c, b + c - a, a + c - b, a + b - c
    return np.sqrt(S * s0 * s1 * s2)


def scale(u):
    return np.exp((0.0 - u) / 2.0)


def faces(F, l0, area2, s):
    """(angles nF x 3, half cotangents nF x 3, broken nF) of k_conformal_faces"""
    a, b, c = l0[:, 0] * s[F[:, 0]], l0[:, 1] * s[F[:, 1]], l0[:, 2] * s[F[:, 2]]
    S, s0, s1, s2 = a + b + c, b + c - a, a + c - b, a + b - c
    bad = (s0 <= 0.0) | (s1 <= 0.0) | (s2 <= 0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        ang = np.stack([2.0 * np.arctan2(np.sqrt(s1 * s2), np.sqrt(S * s0)), 2.0 * np.arctan2(np.sqrt(s2 * s0), np.sqrt(S * s1)),
                        2.0 * np.arctan2(np.sqrt(s0 * s1), np.sqrt(S * s2))], axis=1)
        dA = area2 * (np.sqrt(S * s0 * s1 * s2) / heron(l0[:, 0], l0[:, 1], l0[:, 2]))
        hc = np.stack([(b * b + c * c - a * a) / dA / 4.0, (c * c + a * a - b * b) / dA / 4.0, (a * a + b * b - c * c) / dA / 4.0], axis=1)
    big = np.where(s0 <= 0.0, 0, np.where(s1 <= 0.0, 1, 2))
    ang[bad] = np.where(np.arange(3)[None, :] == big[bad][:, None], PI, 0.0)
    hc[bad] = 0.0
    return ang, hc, bad.astype(np.float64)


def lengths(F, l0, s):
    s0, s1, s2 = s[F[:, 0]], s[F[:, 1]], s[F[:, 2]]
    return np.stack([l0[:, 0] / (s1 * s2), l0[:, 1] / (s2 * s0), l0[:, 2] / (s0 * s1)], axis=1)


def angle_sums(ang, lists, nV):
    acc = np.zeros(nV)
    flat = ang.reshape(-1)
    for vs, ts in lists:
        acc[vs] = acc[vs] + flat[ts]
    return acc


class Plan:
    """the CSR pattern of smg_mesh_cotmatrix and, per stored entry, its signed terms in cotmatrix()'s insertion order (csrc/smg_mesh.cpp:
    make_assembly_plan): face by face, edge e = 0, 1, 2 from corner e + 1 to corner e + 2, the four triplets (s, d, +), (d, s, +), (s, s, -),
    (d, d, -); a stable sort of every row by column merges duplicates in that order"""

    def __init__(self, F, nV):
        F = np.asarray(F)
        es, ed = np.array([1, 2, 0]), np.array([2, 0, 1])
        s, d = F[:, es], F[:, ed]                                       # nF x 3
        rows = np.stack([s, d, s, d], axis=2).reshape(-1)               # global order (f, e, k)
        cols = np.stack([d, s, s, d], axis=2).reshape(-1)
        term = np.repeat(np.arange(3 * F.shape[0]), 4)
        sgn = np.tile(np.array([1.0, 1.0, -1.0, -1.0]), 3 * F.shape[0])
        order = np.lexsort((np.arange(rows.size), cols, rows))          # by row, then column, then insertion
        rows, cols, self.term, self.sgn = rows[order], cols[order], term[order], sgn[order]
        first = np.ones(rows.size, bool)
        first[1:] = (rows[1:] != rows[:-1]) | (cols[1:] != cols[:-1])
        self.entry = np.cumsum(first) - 1                               # the stored entry of every term
        start = np.flatnonzero(first)
        self.rank = np.arange(rows.size) - start[self.entry]
        self.col = cols[start].astype(np.int32)
        self.rowptr = np.concatenate([[0], np.cumsum(np.bincount(rows[start], minlength=nV))]).astype(np.int32)
        self.nnz = start.size

    def values(self, hc):
        """-L~: every entry's terms summed one after the other, the first assigning, then times -1"""
        flat = hc.reshape(-1)
        L = np.zeros(self.nnz)
        for k in range(int(self.rank.max()) + 1):
            m = self.rank == k
            x = self.sgn[m] * flat[self.term[m]]
            L[self.entry[m]] = x if k == 0 else L[self.entry[m]] + x
        return -1.0 * L


# ---- the method with direct solves -----------------------------------------------------------------------------------------------------------------
class ConformalNp:
    def __init__(self, V, F, fixed):
        self.F = np.asarray(F)
        self.n = V.shape[0]
        self.l0 = rest_lengths(np.asarray(V, dtype=np.float64), self.F)
        self.area2 = rest_area2(np.asarray(V, dtype=np.float64), self.F)
        self.lists = corner_lists(self.F, self.n)
        self.plan = Plan(self.F, self.n)
        self.fixed = np.asarray(fixed, dtype=np.int64)
        self.mask = np.zeros(self.n, bool)
        self.mask[self.fixed] = True
        self.free = np.flatnonzero(~self.mask)
        self.u = np.zeros(self.n)
        self.broken_max = 0

    def evaluate(self, u, Theta, s=None):
        s = scale(u) if s is None else s
        ang, hc, br = faces(self.F, self.l0, self.area2, s)
        a = angle_sums(ang, self.lists, self.n)
        g = np.where(self.mask, 0.0, a - Theta)
        return dict(s=s, ang=ang, hc=hc, broken=br, sum=a, g=g, norm=float(np.sqrt(fixed_sum(g * g))), max=float(np.max(np.abs(g))),
                    n_broken=int(br.sum()))

    def matrix(self, hc):
        return sp.csr_matrix((self.plan.values(hc), self.plan.col, self.plan.rowptr), shape=(self.n, self.n))

    def solve(self, Theta, u_fixed=None, grad_tol=1e-10, max_newton=50):
        """Newton from self.u; returns (grad_his, step_his, converged)"""
        u = self.u.copy()
        u[self.fixed] = 0.0 if u_fixed is None else u_fixed
        e = self.evaluate(u, Theta)
        self.broken_max = e["n_broken"]
        his, steps, conv = [e["max"]], [], False
        for t in range(max_newton + 1):
            if not np.isfinite(e["norm"]):
                raise FloatingPointError("non-finite gradient norm at Newton step %d" % t)
            if e["max"] <= grad_tol:
                conv = True
                break
            if t == max_newton:
                break
            A = self.matrix(e["hc"])[self.free][:, self.free].tocsc()
            d = np.zeros(self.n)
            d[self.free] = spla.splu(A).solve(e["g"][self.free])
            step, trial = 1.0, None
            while step >= 2.0 ** -20:
                trial = self.evaluate(u + step * d, Theta)
                self.broken_max = max(self.broken_max, trial["n_broken"])
                if trial["norm"] <= (1.0 - 1e-4 * step) * e["norm"]:
                    break
                step, trial = step * 0.5, None
            if trial is None:
                break
            u, e = u + step * d, trial
            his.append(e["max"])
            steps.append(step)
        self.u, self.last = u, e
        return np.array(his), np.array(steps), conv


# ---- the unfolding -----------------------------------------------------------------------------------------------------------------------------------
def unfold(F, lt, nV):
    """smg_mesh_unfold: breadth-first from face 0, the neighbours across the edges opposite corners 0, 1, 2 in turn; returns (X, mismatch, flipped)"""
    F = np.asarray(F)
    half = {(int(F[f, (c + 1) % 3]), int(F[f, (c + 2) % 3])): (f, c) for f in range(F.shape[0]) for c in range(3)}
    X, placed, seen = np.zeros((nV, 2)), np.zeros(nV, bool), np.zeros(F.shape[0], bool)

    def place(f, c):
        A, B = F[f, (c + 1) % 3], F[f, (c + 2) % 3]
        L, dA, dB = lt[f, c], lt[f, (c + 2) % 3], lt[f, (c + 1) % 3]
        ex, ey = X[B] - X[A]
        el = np.sqrt(ex * ex + ey * ey)
        x = (dA * dA - dB * dB + L * L) / (2.0 * L)
        y = np.sqrt(max(dA * dA - x * x, 0.0))
        X[F[f, c]] = X[A, 0] + x * (ex / el) - y * (ey / el), X[A, 1] + x * (ey / el) + y * (ex / el)
        placed[F[f, c]] = True

    X[F[0, 1]] = lt[0, 2], 0.0
    placed[F[0, :2]] = True
    place(0, 2)
    queue, seen[0] = [0], True
    for f in queue:
        for c in range(3):
            hit = half.get((int(F[f, (c + 2) % 3]), int(F[f, (c + 1) % 3])))
            if hit is None or seen[hit[0]]:
                continue
            seen[hit[0]] = True
            if not placed[F[hit]]:
                place(*hit)
            queue.append(hit[0])
    assert len(queue) == F.shape[0]
    P = X[F]
    laid = np.stack([np.linalg.norm(P[:, 2] - P[:, 1], axis=1), np.linalg.norm(P[:, 0] - P[:, 2], axis=1), np.linalg.norm(P[:, 1] - P[:, 0], axis=1)], axis=1)
    e1, e2 = P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]
    area2 = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
    return X, float((np.abs(laid - lt) / lt).max()), int(np.sum(~(area2 > 0.0)))


def rigid_distance(X, Y):
    """max |R X + t - Y| over the best proper rigid motion of the plane"""
    Xc, Yc = X - X.mean(axis=0), Y - Y.mean(axis=0)
    U, _, Vt = np.linalg.svd(Xc.T @ Yc)
    R = U @ np.diag([1.0, np.linalg.det(U @ Vt)]) @ Vt
    return float(np.abs(Xc @ R - Yc).max())


# ---- the library's side, shared with tests/test_gpu_conformal.py -----------------------------------------------------------------------------------
def out_size(op, nV, nF, nnz):
    return {SCALE: 2 * nV, FACES: 10 * nF, ROWS: 4 * nV + 3 + nnz}.get(op, 2 * nV)


def unpack(op, out, nV, nF):
    """SCALE: (s, u + t d); FACES: (angles, half cotangents, broken, l~); ROWS: (sums, g, g^2, |g|, the 3 reductions, val)"""
    if op == SCALE:
        return out[:nV], out[nV:]
    if op == FACES:
        return out[:3 * nF].reshape(nF, 3), out[3 * nF:6 * nF].reshape(nF, 3), out[6 * nF:7 * nF], out[7 * nF:].reshape(nF, 3)
    return out[:nV], out[nV:2 * nV], out[2 * nV:3 * nV], out[3 * nV:4 * nV], out[4 * nV:4 * nV + 3], out[4 * nV + 3:]


def _call(fn, with_guard, op, nV, F, l0=None, area2=None, u=None, d=None, t=0.0, s=None, Theta=None, fixed=None, nnz=0, over=None, pad=64):
    """`pad` doubles of sentinel follow the op's extent in `out`: nothing past the extent may be written"""
    ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
    F = np.ascontiguousarray(F, dtype=np.int32)
    nF = F.shape[0]
    vec = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64).reshape(-1)   # noqa: E731
    keep = [vec(l0), vec(u), vec(d), vec(s), vec(Theta), None if fixed is None else np.ascontiguousarray(fixed, dtype=np.int32), vec(area2)]
    arr = lambda a, ty=dp: None if a is None else a.ctypes.data_as(ty)   # noqa: E731
    size = out_size(op, nV, nF, nnz)
    out = np.full(size + pad, SENTINEL)
    bad = C.c_int(-1)
    a = dict(nV=nV, nF=nF, F=arr(F, ip), l0=arr(keep[0]), area2=arr(keep[6]), u=arr(keep[1]), d=arr(keep[2]), t=t, s=arr(keep[3]), Theta=arr(keep[4]), fixed=arr(keep[5], ip),
             n_fixed=0 if keep[5] is None else keep[5].size, out=arr(out))
    a.update(over or {})
    args = [op] + [a[key] for key in ("nV", "nF", "F", "l0", "area2", "u", "d", "t", "s", "Theta", "fixed", "n_fixed", "out")]
    rc = fn(*args, C.byref(bad)) if with_guard else fn(*args)
    if rc == 0:
        assert np.all(out[size:] == SENTINEL), "op %d wrote past its extent" % op
        assert not np.any(out[:size] == SENTINEL), "op %d left a part of its extent unwritten" % op
    return rc, bad.value, out[:size]


def host(smg, op, nV, F, **kw):
    """one call of smg_conformal_host; returns (rc, out)"""
    rc, _, out = _call(smg._lib.load().smg_conformal_host, False, op, nV, F, **kw)
    return rc, out


def hook(smg, op, nV, F, **kw):
    """one call of smg_debug_conformal; returns (rc, guard hits, out)"""
    return _call(smg._lib.load().smg_debug_conformal, True, op, nV, F, **kw)


@functools.lru_cache(maxsize=None)
def launcher_inputs(name):
    """(V, F, restatement object, [u = 0, a smooth u, a u with vertex 20 at +6], Theta, fixed) of a launcher mesh.  The spike lengthens the edges
    at vertex 20 twentyfold: a face there breaks when its two long edges differ by more than the short one (every mesh of the table has such
    faces at vertex 20; a vertex of the icosahedron itself, whose edges are all equal, would break none)"""
    V, F = shape(name)
    ref = ConformalNp(V, F, [0, 5])
    spike = np.zeros(V.shape[0])
    spike[20] = 6.0
    Theta = np.full(V.shape[0], 2.0 * PI) - 0.01 * np.cos(5.0 * V[:, 0])
    return V, F, ref, (np.zeros(V.shape[0]), smooth_u(V), spike), Theta, np.array([0, 5], np.int32)


def check_launchers(run, name):
    """FACES and ROWS of `run(op, nV, F, **operands) -> out` on one mesh against the restatement, bit for bit, when both sides are handed the
    restatement's s (the angles of unbroken faces excepted); s, the angles and the sums are returned for the caller's bounds"""
    V, F, ref, us, Theta, fixed = launcher_inputs(name)
    n, nF = V.shape[0], F.shape[0]
    got = []
    for u in us:
        e = ref.evaluate(u, Theta)
        s, ut = unpack(SCALE, run(SCALE, n, F, u=u), n, nF)
        assert np.array_equal(ut, u)
        ang, hc, br, lt = unpack(FACES, run(FACES, n, F, l0=ref.l0, area2=ref.area2, s=e["s"]), n, nF)
        assert np.array_equal(hc, e["hc"]) and np.array_equal(br, e["broken"]) and np.array_equal(lt, lengths(F, ref.l0, e["s"]))
        assert np.array_equal(ang[br == 1.0], e["ang"][br == 1.0])
        sums, g, gsq, gabs, red, val = unpack(ROWS, run(ROWS, n, F, l0=ref.l0, area2=ref.area2, s=e["s"], Theta=Theta, fixed=fixed, nnz=ref.plan.nnz), n, nF)
        assert np.array_equal(val, ref.plan.values(e["hc"])) and red[2] == e["n_broken"]
        assert np.all(g[fixed] == 0.0) and np.array_equal(gsq, g * g) and np.array_equal(gabs, np.abs(g))
        assert red[0] == fixed_sum(gsq) and red[1] == np.max(gabs)
        got.append(dict(s=s, ang=ang, sums=sums, g=g, e=e))
    d = 0.25 * np.cos(2.0 * V[:, 1])
    s, ut = unpack(SCALE, run(SCALE, n, F, u=us[1], d=d, t=0.5), n, nF)
    assert np.array_equal(ut, us[1] + 0.5 * d)
    return got
