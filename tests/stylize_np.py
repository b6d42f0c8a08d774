"""The numpy / scipy restatement of cubic and normal-driven stylization (include/smg.h: smg_stylize_*), with LAPACK SVDs and direct solves, written
from the method's formulas in the order the header gives them:

    E(R, U) = sum_i [ 1/2 sum_j w_ij |e'_ij - R_i e_ij|^2 + lambda_i a_i |Q R_i n_i|_1 ]        (normal-driven: lambda_i a_i |R_i n_i - t_i|^2)

Sums over a row of L or a corner list run in stored order, one slot of every row at a time, so the floating-point order is the method's.
tests/test_stylize_host.py checks the restatement and the library's host twin; tests/test_gpu_stylize.py checks the device against both."""
import ctypes as C
import functools

import numpy as np

from oracle import mesh_np as M
from denoise_np import strip, tetrahedron
from pd_np import EPS, corner_lists, fixed_sum  # noqa: F401  (shared with the tests)
from test_arap_host import ArapNp, ArapRest, covariance, rhs, rotations_np, vertex_energy
from test_geodesics_host import icosphere

STY_NORMALS, STY_ADMM_ONE, STY_LOCAL, STY_LOCAL_TARGETS, STY_ENERGY = range(5)
DEFAULTS = dict(lambda_=0.2, rho0=1e-4, abs_tol=1e-5, rel_tol=1e-3, mu=10.0, tau=2.0, admm_iters=100)
KERNEL_SHAPES = ["icosphere2", "icosphere3", "icosphere4", "bunny.smgm", "strip255", "strip256", "strip257", "tetrahedron"]


# ---- shapes ------------------------------------------------------------------------------------------------------------------------------------
def unit_box(V):
    """V moved and scaled so that the longest side of its bounding box is [0, 1]"""
    lo, hi = V.min(axis=0), V.max(axis=0)
    return np.ascontiguousarray((V - lo) / (hi - lo).max())


def flat_strip(nV):
    """an open strip of nV vertices (denoise_np.strip with nV - 2 faces) pressed into the plane z = 0: every covariance has rank 2"""
    V, F = strip(nV - 2)
    assert V.shape[0] == nV
    V = V.copy()
    V[:, 2] = 0.0
    return V, F


@functools.lru_cache(maxsize=None)
def shape(name):
    """(V, F) of a test shape, V scaled to a unit bounding-box side; computed once and left unchanged by its users"""
    if name.startswith("icosphere"):
        V, F = icosphere(int(name[len("icosphere"):]))
    elif name.startswith("strip"):
        V, F = flat_strip(int(name[len("strip"):]))
    elif name == "tetrahedron":
        V, F = tetrahedron()
    else:
        V, F = M.read_smgm(name)
    V, F = unit_box(np.asarray(V, dtype=np.float64)), np.ascontiguousarray(F, dtype=np.int32)
    V.setflags(write=False)
    F.setflags(write=False)
    return V, F


@functools.lru_cache(maxsize=None)
def rest(name):
    """ArapRest (the CSR of the numpy cotangent matrix and the rest positions) of a shape"""
    V, F = shape(name)
    return ArapRest(M.cotmatrix(V, F), V)


def noisy_pose(V, amp=0.02, seed=0):
    """the prototype's pose: V + amp x standard_normal, the seed fixed"""
    return np.ascontiguousarray(V + amp * np.random.default_rng(seed).standard_normal(V.shape))


# ---- rest data ---------------------------------------------------------------------------------------------------------------------------------
def dot3(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def norm3(a):
    return np.sqrt(dot3(a, a))


def vertex_normals_areas(V, F):
    """(n nV x 3, a nV): the normalised sum of (p1 - p0) x (p2 - p0) over the vertex's faces, faces ascending; the sum of the double areas over 6"""
    nV = V.shape[0]
    a, b = V[F[:, 1]] - V[F[:, 0]], V[F[:, 2]] - V[F[:, 0]]
    c = np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)
    dbl = norm3(c)
    total, area = np.zeros((nV, 3)), np.zeros(nV)
    for vs, ts in corner_lists(F, nV):
        total[vs] = total[vs] + c[ts // 3]
        area[vs] = area[vs] + dbl[ts // 3]
    ln = norm3(total)
    ok = ln > 0.0
    n = np.zeros((nV, 3))
    n[ok] = total[ok] / ln[ok, None]
    return n, area / 6.0


def cubeness(V, F):
    """the area-weighted mean of the L1 norm of the unit face normals: 1 for an axis-aligned box, sqrt(3) at the worst"""
    c = np.cross(V[F[:, 1]] - V[F[:, 0]], V[F[:, 2]] - V[F[:, 0]])
    dbl = np.linalg.norm(c, axis=1)
    return float(np.sum(np.abs(c).sum(axis=1)) / np.sum(dbl))


def nearest_axis(n):
    """per row the signed coordinate axis closest to it"""
    t = np.zeros_like(n)
    k = np.argmax(np.abs(n), axis=1)
    t[np.arange(n.shape[0]), k] = np.where(n[np.arange(n.shape[0]), k] < 0, -1.0, 1.0)
    return t


# ---- the local step ----------------------------------------------------------------------------------------------------------------------------
def shrink(x, k):
    return np.where(x > k, x - k, np.where(x < -k, x + k, 0.0))


def rotated_normal(Q, R, n):
    """y = Q (R n)"""
    rn = np.stack([dot3(R[:, a, :], n) for a in range(3)], axis=1)
    return np.stack([(Q[a, 0] * rn[:, 0] + Q[a, 1] * rn[:, 1]) + Q[a, 2] * rn[:, 2] for a in range(3)], axis=1)


def admm_matrix(S, n, Q, z, u, rho):
    """M = S + rho n (Q^T (z - u))^T"""
    d = z - u
    v = np.stack([(Q[0, c] * d[:, 0] + Q[1, c] * d[:, 1]) + Q[2, c] * d[:, 2] for c in range(3)], axis=1)
    return S + (rho[:, None] * n)[:, :, None] * v[:, None, :]


def admm_after_fit(R, n, Q, la, p, z, u, rho):
    """steps 3 .. 11 from a given rotation: (z, u, rho, done, dict(y, r, s))"""
    y = rotated_normal(Q, R, n)
    k = la / rho
    z_new = shrink(y + u, k[:, None])
    u_new = u + (y - z_new)
    r, s = norm3(z_new - y), rho * norm3(z_new - z)
    up = r > p["mu"] * s
    down = ~up & (s > p["mu"] * r)
    rho_new = np.where(up, rho * p["tau"], np.where(down, rho / p["tau"], rho))
    u_new = np.where(up[:, None], u_new / p["tau"], np.where(down[:, None], u_new * p["tau"], u_new))
    floor = np.sqrt(3.0) * p["abs_tol"]
    done = (r < floor + p["rel_tol"] * np.maximum(norm3(y), norm3(z_new))) & (s < floor + p["rel_tol"] * (rho_new * norm3(u_new)))
    return z_new, u_new, rho_new, done, dict(y=y, r=r, s=s)


def admm_one(S, n, Q, la, p, z, u, rho):
    """one iteration: (R, z, u, rho, done, dict(y, r, s, gap))"""
    R, gap, _ = rotations_np(admm_matrix(S, n, Q, z, u, rho))
    z, u, rho, done, aux = admm_after_fit(R, n, Q, la, p, z, u, rho)
    aux["gap"] = gap
    return R, z, u, rho, done, aux


def params(**over):
    p = dict(DEFAULTS)
    p.update(over)
    return p


def start_state(nV, p):
    return np.zeros((nV, 3)), np.zeros((nV, 3)), np.full(nV, p["rho0"])


def energy_terms(A, P, R, n, la, Q=None, targets=None):
    """1/2 sum_j w_ij |e'_ij - R_i e_ij|^2 + la |Q R n|_1, or + la |R n - t|^2 with targets"""
    Q = np.eye(3) if Q is None else Q
    if targets is None:
        y = rotated_normal(Q, R, n)
        pen = la * ((np.abs(y[:, 0]) + np.abs(y[:, 1])) + np.abs(y[:, 2]))
    else:
        d = np.stack([dot3(R[:, a, :], n) for a in range(3)], axis=1) - targets
        pen = la * dot3(d, d)
    return 0.5 * vertex_energy(A, P, R) + pen


def local(A, P, n, area, p, lam=None, Q=None, state=None):
    """the cubic local step: (R, (z, u, rho), iters, energy terms); the vertices iterate until their own stopping test holds"""
    Q = np.eye(3) if Q is None else Q
    la = (p["lambda_"] if lam is None else lam) * area
    S = covariance(A, P)
    z, u, rho = [a.copy() for a in (start_state(A.n, p) if state is None else state)]
    R = np.zeros((A.n, 3, 3))
    iters = np.zeros(A.n, dtype=np.int32)
    active = np.ones(A.n, dtype=bool)
    for _ in range(p["admm_iters"]):
        i = np.nonzero(active)[0]
        if i.size == 0:
            break
        R[i], z[i], u[i], rho[i], done, _ = admm_one(S[i], n[i], Q, la[i], p, z[i], u[i], rho[i])
        iters[i] += 1
        active[i[done]] = False
    return R, (z, u, rho), iters, energy_terms(A, P, R, n, la, Q)


def local_targets(A, P, n, area, p, targets, lam=None):
    """the normal-driven local step: (R, energy terms, gap)"""
    la = (p["lambda_"] if lam is None else lam) * area
    R, gap, _ = rotations_np(covariance(A, P) + ((2.0 * la)[:, None] * n)[:, :, None] * targets[:, None, :])
    return R, energy_terms(A, P, R, n, la, None, targets), gap


class StylizeNp:
    """the restatement with direct solves: (-L)_uu factored once (ArapNp), one local / global step per outer iteration"""

    def __init__(self, V, F, pins=None, L=None, **over):
        self.V, self.F = np.ascontiguousarray(V, dtype=np.float64), np.ascontiguousarray(F, dtype=np.int32)
        self.pins = np.array([0] if pins is None else pins, dtype=np.int64)
        self.arap = ArapNp(M.cotmatrix(self.V, self.F) if L is None else L, self.V, self.pins)      # L: the library's own, the system's bits
        self.A = self.arap.A
        self.n, self.area = vertex_normals_areas(self.V, self.F)
        self.p = params(**over)
        self.lam = self.Q = self.targets = None

    def run(self, pin_pos=None, U0=None, n_iter=10):
        """(U, energy_his with n_iter + 1 entries, the ADMM iteration counts of every local step)"""
        pin_pos = self.V[self.pins] if pin_pos is None else np.asarray(pin_pos, dtype=np.float64)
        U = self.arap.start(pin_pos, U0)
        E, counts, state = [], [], None
        for t in range(n_iter + 1):
            if self.targets is None:
                R, state, iters, terms = local(self.A, U, self.n, self.area, self.p, self.lam, self.Q, state)
            else:
                R, terms, _ = local_targets(self.A, U, self.n, self.area, self.p, self.targets, self.lam)
                iters = np.zeros(self.A.n, dtype=np.int32)
            E.append(float(np.sum(terms)))
            counts.append(iters)
            if t == n_iter:
                break
            b = rhs(self.A, R)
            Un = U.copy()
            Un[self.arap.unknown] = self.arap.lu.solve(b[self.arap.unknown] - self.arap.Kuk @ pin_pos)
            U = Un
        return U, np.array(E), counts


@functools.lru_cache(maxsize=None)
def reference_run(name, mode="cubic", lambda_=0.2, n_iter=10):
    """(StylizeNp, U, energy_his, counts) of the restatement on a shape, vertex 0 pinned: computed once per session and left unchanged"""
    V, F = shape(name)
    S = StylizeNp(V, F, lambda_=lambda_)
    if mode == "targets":
        S.targets = nearest_axis(S.n)
    U, E, counts = S.run(n_iter=n_iter)
    U.setflags(write=False)
    E.setflags(write=False)
    return S, U, E, counts


# ---- the library's side, shared with tests/test_gpu_stylize.py -----------------------------------------------------------------------------------
def params_c(smg, **over):
    return smg.stylize_params(**params(**over))


OUT_SIZE = {STY_NORMALS: 4, STY_ADMM_ONE: 17, STY_LOCAL: 17, STY_LOCAL_TARGETS: 10, STY_ENERGY: 1}


def pack_state(state):
    """(z, u, rho) -> the 7 planes the library keeps"""
    z, u, rho = state
    return np.ascontiguousarray(np.concatenate([z.T.reshape(-1), u.T.reshape(-1), rho]))


def unpack(op, out, n):
    """the library's `out` of an op as arrays: NORMALS (n, a); ADMM_ONE / LOCAL (R, terms, (z, u, rho)); LOCAL_TARGETS (R, terms); ENERGY terms"""
    if op == STY_NORMALS:
        return out[:3 * n].reshape(n, 3), out[3 * n:4 * n]
    if op == STY_ENERGY:
        return out[:n]
    R, terms = out[:9 * n].reshape(n, 3, 3), out[9 * n:10 * n]
    if op == STY_LOCAL_TARGETS:
        return R, terms
    st = out[10 * n:17 * n].reshape(7, n)
    return R, terms, (st[0:3].T.copy(), st[3:6].T.copy(), st[6].copy())


def _call(fn, with_guard, op, A, F, P, lam, Q, targets, state_in, R_in, par, over):
    ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
    n = A.n
    F = np.ascontiguousarray(F, dtype=np.int32)
    keep = [None if a is None else np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(-1)) for a in (A.P0, P, lam, Q, targets, state_in, R_in)]
    arr = lambda a, t=dp: None if a is None else a.ctypes.data_as(t)   # noqa: E731
    size = OUT_SIZE.get(op, 17) * n + (1 if op == STY_ENERGY and with_guard else 0)
    out = np.full(size, np.nan)
    iters = np.full(n, -1, dtype=np.int32)
    bad = C.c_int(-1)
    a = dict(nV=n, nF=F.shape[0], F=arr(F, ip), rowptr=arr(A.rowptr, ip), col=arr(A.col, ip), w=arr(A.w), V0=arr(keep[0]), P=arr(keep[1]),
             lam=arr(keep[2]), Q=arr(keep[3]), targets=arr(keep[4]), state_in=arr(keep[5]), R_in=arr(keep[6]), p=C.byref(par), out=arr(out),
             iters=arr(iters, ip))
    a.update(over)
    args = [op] + [a[k] for k in ("nV", "nF", "F", "rowptr", "col", "w", "V0", "P", "lam", "Q", "targets", "state_in", "R_in", "p", "out", "iters")]
    rc = fn(*args, C.byref(bad)) if with_guard else fn(*args)
    return rc, bad.value, out, iters


def local_host(smg, op, A, F, P=None, lam=None, Q=None, targets=None, state_in=None, R_in=None, over=None, **par):
    """one call of smg_stylize_local_host on the rest data A (ArapRest); returns (rc, out, iters).  over: raw arguments that replace the built ones"""
    rc, _, out, iters = _call(smg._lib.load().smg_stylize_local_host, False, op, A, F, P, lam, Q, targets, state_in, R_in, params_c(smg, **par), over or {})
    return rc, out, iters


def hook(smg, op, A, F, P=None, lam=None, Q=None, targets=None, state_in=None, R_in=None, over=None, **par):
    """one call of smg_debug_stylize; returns (rc, guard hits, out, iters)"""
    return _call(smg._lib.load().smg_debug_stylize, True, op, A, F, P, lam, Q, targets, state_in, R_in, params_c(smg, **par), over or {})
