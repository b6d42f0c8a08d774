"""The numpy / scipy restatement of two-species reaction-diffusion on a surface (include/smg.h: smg_rd_*), in the kernels' operation order, with
direct solves for the diffusion; the ctypes wrappers of smg_rd_host and smg_debug_rd.

    cubic   uu = u u; uv = u v; vv = v v;  r = c0;  r = r + c1 u;  r = r + c2 v;  r = r + c3 uu;  r = r + c4 uv;  r = r + c5 vv;
            r = r + c6 (uu u);  r = r + c7 (uu v);  r = r + c8 (u vv);  r = r + c9 (vv v)
    react   h = dt / substeps;  `substeps` times:  ru = cubic(R_u; u, v);  rv = cubic(R_v; u, v);  u = u + h ru;  v = v + h rv;
            then the right-hand sides m u*, m v* and their squares
    solve   (M + dt Du (-L)) u' = m u*,  (M + dt Dv (-L)) v' = m v*;  Dv == 0: v' = v*
    close   the terms m u', m v' and max(|u' - u|, |v' - v|); sums per column in the order of launch_fixed_sum, maxima in any order

Only +, -, *, max and fabs occur in the kernels: the library's host twin and its kernels are held to this file bit for bit.  u and v are nV x k
arrays here (the library's blocks are column-major); term planes are (planes) x nV; a coefficient table is k x 20, R_u's ten first, over the
monomials 1, u, v, u^2, uv, v^2, u^3, u^2 v, u v^2, v^3."""
import ctypes as C

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import fluid_np
from fluid_np import LAUNCHER_MESHES, PYRAMIDS, SENTINEL, mass, shape  # noqa: F401  (shared with the tests)
from oracle import mesh_np as M
from pd_np import EPS, fixed_sum  # noqa: F401

RD_REACT, RD_CLOSE = 0, 1
DEFAULTS = dict(Du=1.0, Dv=1.0, dt=1.0, react_substeps=1, stop_change=0.0)


# ---- the kernels' expressions --------------------------------------------------------------------------------------------------------------------
def cubic(c, u, v):
    """c: k x 10; u, v: nV x k -> nV x k, the order of rd_cubic"""
    c = np.asarray(c, dtype=np.float64)
    uu, uv, vv = u * u, u * v, v * v
    r = c[None, :, 0] + np.zeros(u.shape)
    r = r + c[None, :, 1] * u
    r = r + c[None, :, 2] * v
    r = r + c[None, :, 3] * uu
    r = r + c[None, :, 4] * uv
    r = r + c[None, :, 5] * vv
    r = r + c[None, :, 6] * (uu * u)
    r = r + c[None, :, 7] * (uu * v)
    r = r + c[None, :, 8] * (u * vv)
    r = r + c[None, :, 9] * (vv * v)
    return r


def substeps(coeff, u, v, dt, n_sub):
    """(u*, v*): n_sub Euler steps of length dt / n_sub of the reaction alone, both rates from the same (u, v)"""
    coeff = np.asarray(coeff, dtype=np.float64).reshape(-1, 20)
    h = dt / n_sub
    for _ in range(n_sub):
        ru, rv = cubic(coeff[:, :10], u, v), cubic(coeff[:, 10:], u, v)
        u, v = u + h * ru, v + h * rv
    return u, v


def react(m, u, v, coeff, dt, n_sub):
    """(R nV x 2k: m u* then m v*, rsq 2k x nV, v* nV x k, the two sums of the squares) of k_rd_react and its reductions"""
    us, vs = substeps(coeff, u, v, dt, n_sub)
    R = np.concatenate([m[:, None] * us, m[:, None] * vs], axis=1)
    rsq = np.ascontiguousarray((R * R).T)
    k = u.shape[1]
    return R, rsq, vs, np.array([fixed_sum(rsq[:k].reshape(-1)), fixed_sum(rsq[k:].reshape(-1))])


def close(m, u, v, un, vn):
    """(mt 2k x nV: m u' then m v', chg k x nV, the sums 2k, the maxima k) of k_rd_close and its reductions"""
    mt = np.ascontiguousarray(np.concatenate([m[:, None] * un, m[:, None] * vn], axis=1).T)
    chg = np.ascontiguousarray(np.maximum(np.abs(un - u), np.abs(vn - v)).T)
    return mt, chg, np.array([fixed_sum(t) for t in mt]), chg.max(axis=1)


def test_state(V, F, k, seed=0):
    """(u, v, un, vn as nV x k, coeff k x 20): smooth fields of the positions and random coefficient tables of mixed signs and sizes"""
    rng = np.random.default_rng(1000 * seed + 7 * k + V.shape[0])
    a, b = fluid_np.hodge_np.potentials(V, k)
    u, v = np.array(a), np.array(b)
    un = np.ascontiguousarray(u + 0.25 * np.cos(3.0 * V[:, [2]] + np.arange(k)[None, :]))
    vn = np.ascontiguousarray(v - 0.125 * np.sin(2.0 * V[:, [0]] - np.arange(k)[None, :]))
    coeff = rng.standard_normal((k, 20)) * 10.0 ** rng.integers(-2, 2, size=(k, 20))
    return u, v, un, vn, coeff


# ---- the method with direct solves ---------------------------------------------------------------------------------------------------------------
class RdNp:
    """the whole step with scipy.sparse.linalg.splu on M + dt D (-L); L: the cotangent matrix, numpy's or the library's own bits.  After a step
    self.res holds the direct solves' residual 2-norms per column (2k: u's then v's, 0 where nothing is solved)"""

    def __init__(self, V, F, L=None, **params):
        self.V, self.F = np.asarray(V, dtype=np.float64), np.asarray(F)
        self.p = dict(DEFAULTS, **params)
        self.A = sp.csr_matrix(-(M.cotmatrix(self.V, self.F) if L is None else L))
        self.m, self.msum = mass(self.V, self.F)
        self.case = "v alone" if self.p["Dv"] == 0.0 else "one" if self.p["Du"] == self.p["Dv"] else "two"
        self.lu, self.mat = {}, {}
        self.u = self.v = self.coeff = self.res = None

    def matrix(self, D):
        c = self.p["dt"] * D
        if c not in self.mat:
            self.mat[c] = (sp.diags(self.m) + c * self.A).tocsc()
            self.lu[c] = spla.splu(self.mat[c])
        return self.mat[c], self.lu[c]

    def set_state(self, u, v, coeff):
        n = self.V.shape[0]
        self.u, self.v = np.array(np.asarray(u, dtype=np.float64).reshape(n, -1)), np.array(np.asarray(v, dtype=np.float64).reshape(n, -1))
        k = self.u.shape[1]
        coeff = np.asarray(coeff, dtype=np.float64)
        self.coeff = np.array(np.broadcast_to(coeff, (k, 20)) if coeff.ndim == 1 else coeff.reshape(k, 20))

    def step(self, n_steps=1):
        """-> (mass n_done x 2k, change n_done x k); ends early as the library does"""
        p, k = self.p, self.u.shape[1]
        masses, changes = [], []
        for _ in range(n_steps):
            R, _, vs, _ = react(self.m, self.u, self.v, self.coeff, p["dt"], p["react_substeps"])
            Au, lu = self.matrix(p["Du"])
            un = lu.solve(R[:, :k])
            res = [np.linalg.norm(R[:, :k] - Au @ un, axis=0), np.zeros(k)]
            if p["Dv"] == 0.0:
                vn = vs
            else:
                Av, lv = self.matrix(p["Dv"])
                vn = lv.solve(R[:, k:])
                res[1] = np.linalg.norm(R[:, k:] - Av @ vn, axis=0)
            self.res = np.concatenate(res)
            _, _, sums, mx = close(self.m, self.u, self.v, un, vn)
            self.u, self.v = un, vn
            masses.append(sums)
            changes.append(mx)
            if p["stop_change"] > 0.0 and np.all(mx <= p["stop_change"]):
                break
        return np.stack(masses), np.stack(changes)


# ---- how far two runs of the method can drift apart: CHAIN of tests/test_gpu_rd.py, used by both test files -------------------------------------
def jacobians(coeff, u, v):
    """(J nV x k x 2 x 2: the reaction's Jacobian at (u, v); H nV x k: the sum over both cubics of the absolute second derivatives)"""
    c = np.asarray(coeff, dtype=np.float64).reshape(-1, 20)[None, :, :]
    J, H = np.zeros(u.shape + (2, 2)), np.zeros(u.shape)
    au, av = np.abs(u), np.abs(v)
    for r, off in ((0, 0), (1, 10)):
        q = lambda j: c[:, :, off + j]   # noqa: E731
        J[..., r, 0] = q(1) + 2 * q(3) * u + q(4) * v + 3 * q(6) * u * u + 2 * q(7) * u * v + q(8) * v * v
        J[..., r, 1] = q(2) + q(4) * u + 2 * q(5) * v + q(7) * u * u + 2 * q(8) * u * v + 3 * q(9) * v * v
        H += (2 * np.abs(q(3)) + 6 * np.abs(q(6)) * au + 2 * np.abs(q(7)) * av) + 2 * (np.abs(q(4)) + 2 * np.abs(q(7)) * au + 2 * np.abs(q(8)) * av) \
            + (2 * np.abs(q(5)) + 2 * np.abs(q(8)) * au + 6 * np.abs(q(9)) * av)
    return J, H


class Chain:
    """The distance between the restatement `ref` and another run of the same steps from the same start whose solves stop at the absolute
    residual `tol` (0: exact answers).  E is the M-norm sqrt(sum m (du^2 + dv^2)) of one column's difference:

        E' = g E + sqrt(max m) sqrt(b_u^2 + b_v^2) + 64 s eps g' |(u, v)|_M + dt H g'^2 E^2 / min m,      |d(u, v)|_2 <= E / sqrt(min m)
        b = (10 tol + res_np) / min m + extra  per species and column (0 for v when Dv == 0)
        g = the product over the s sub-steps of max_i sigma_max(I + (dt / s) J_i) at that sub-step's state,  g' = max(g, 1)

    before() reads g, H and the size from ref's state at the step's start; step ref; after(extra_u, extra_v) -> the 2-norm bound per column."""

    def __init__(self, ref, tol):
        self.ref, self.tol = ref, tol
        self.E = np.zeros(ref.u.shape[1])
        self.mmin, self.mmax = float(ref.m.min()), float(ref.m.max())

    def one_step(self, extra_u=0.0, extra_v=0.0):
        k = self.ref.u.shape[1]
        b = (10.0 * self.tol + self.ref.res) / self.mmin
        b[:k] += extra_u
        b[k:] = 0.0 if self.ref.p["Dv"] == 0.0 else b[k:] + extra_v
        return b

    def before(self):
        ref = self.ref
        n_sub, h = ref.p["react_substeps"], ref.p["dt"] / ref.p["react_substeps"]
        u, v = ref.u, ref.v
        self.g, self.H, self.size = np.ones(u.shape[1]), np.zeros(u.shape[1]), np.zeros(u.shape[1])
        for _ in range(n_sub):                                                # every sub-step is one pointwise map I + h J at its own state
            J, H = jacobians(ref.coeff, u, v)
            G = np.eye(2)[None, None] + h * J
            self.g = self.g * np.linalg.norm(G, ord=2, axis=(2, 3)).max(axis=0)
            self.H = np.maximum(self.H, H.max(axis=0))
            self.size = np.maximum(self.size, np.sqrt(np.sum(ref.m[:, None] * (u ** 2 + v ** 2), axis=0)))
            u, v = substeps(ref.coeff, u, v, h, 1)

    def after(self, extra_u=0.0, extra_v=0.0):
        k, n_sub = self.ref.u.shape[1], self.ref.p["react_substeps"]
        b = self.one_step(extra_u, extra_v)
        gg = np.maximum(self.g, 1.0)                                          # the later sub-steps carry the earlier ones' rounding and remainder
        self.E = (self.g * self.E + np.sqrt(self.mmax) * np.sqrt(b[:k] ** 2 + b[k:] ** 2) + 64 * n_sub * EPS * gg * self.size
                  + self.ref.p["dt"] * self.H * gg ** 2 * self.E ** 2 / self.mmin)
        return self.E / np.sqrt(self.mmin)


def row_sum_defect(A):
    """|A 1|_2 of a stored cotangent matrix, whose row sums vanish only up to the rounding of its entries: every row summed by math.fsum (correctly
    rounded), so this is the stored matrix's own defect and no model of it"""
    import math
    A = sp.csr_matrix(A)
    return float(np.linalg.norm([math.fsum(A.data[A.indptr[i]:A.indptr[i + 1]]) for i in range(A.shape[0])]))


def distance(u, v, ref_u, ref_v):
    """the 2-norm of one column's difference, both species together"""
    return np.sqrt(np.sum((u - ref_u) ** 2 + (v - ref_v) ** 2, axis=0))


# ---- the library's side, shared with tests/test_gpu_rd.py ------------------------------------------------------------------------------------------
def out_size(op, nV, k):
    return 5 * nV * k + 2 if op == RD_REACT else 3 * nV * k + 3 * k


def unpack(op, out, nV, k):
    """the outputs of an op in the restatement's shapes"""
    nk = nV * k
    if op == RD_REACT:
        return out[:2 * nk].reshape(2 * k, nV).T, out[2 * nk:4 * nk].reshape(2 * k, nV), out[4 * nk:5 * nk].reshape(k, nV).T, out[5 * nk:]
    return out[:2 * nk].reshape(2 * k, nV), out[2 * nk:3 * nk].reshape(k, nV), out[3 * nk:3 * nk + 2 * k], out[3 * nk + 2 * k:]


def _call(fn, with_guard, op, V, F, k=1, u=None, v=None, coeff=None, dt=0.5, substeps=1, un=None, vn=None, over=None, pad=64):
    """`pad` doubles of sentinel follow the op's extent in `out`: nothing past the extent may be written"""
    ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
    nV, nF = V.shape[0], F.shape[0]
    F = np.ascontiguousarray(F, dtype=np.int32)
    rows = lambda x: None if x is None else np.ascontiguousarray(x, dtype=np.float64).reshape(-1)                 # noqa: E731
    cols = lambda x: None if x is None else np.ascontiguousarray(np.asarray(x, dtype=np.float64).T).reshape(-1)   # noqa: E731  (column-major)
    keep = [rows(V), cols(u), cols(v), rows(coeff), cols(un), cols(vn)]
    arr = lambda x, ty=dp: None if x is None else x.ctypes.data_as(ty)   # noqa: E731
    size = out_size(op, nV, max(k, 0))
    out = np.full(size + pad, SENTINEL)
    bad = C.c_int(-1)
    q = dict(nV=nV, nF=nF, k=k, F=arr(F, ip), V=arr(keep[0]), u=arr(keep[1]), v=arr(keep[2]), coeff=arr(keep[3]), dt=float(dt), substeps=int(substeps),
             un=arr(keep[4]), vn=arr(keep[5]), out=arr(out))
    q.update(over or {})
    args = [op] + [q[key] for key in ("nV", "nF", "k", "F", "V", "u", "v", "coeff", "dt", "substeps", "un", "vn", "out")]
    rc = fn(*args, C.byref(bad)) if with_guard else fn(*args)
    if rc == 0:
        assert np.all(out[size:] == SENTINEL), "op %d wrote past its extent" % op
        assert not np.any(out[:size] == SENTINEL), "op %d left a part of its extent unwritten" % op
    return rc, bad.value, out[:size]


def host(smg, op, V, F, **kw):
    """one call of smg_rd_host; returns (rc, out)"""
    rc, _, out = _call(smg._lib.load().smg_rd_host, False, op, V, F, **kw)
    return rc, out


def hook(smg, op, V, F, **kw):
    """one call of smg_debug_rd; returns (rc, guard hits, out)"""
    return _call(smg._lib.load().smg_debug_rd, True, op, V, F, **kw)


def check_launchers(run, name, k, n_sub):
    """both ops of `run(op, V, F, **operands) -> out` on one mesh against the restatement, bit for bit; shared by the host twin's and the device's
    tests.  Returns the outputs for a comparison of the two."""
    V, F = shape(name)
    n = V.shape[0]
    u, v, un, vn, coeff = test_state(V, F, k)
    m = mass(V, F)[0]
    dt = 0.03
    eq = np.array_equal
    outs = [run(RD_REACT, V, F, k=k, u=u, v=v, coeff=coeff, dt=dt, substeps=n_sub)]
    want = react(m, u, v, coeff, dt, n_sub)
    assert np.all(np.isfinite(want[0])) and not eq(want[2], v)
    for got, w_ in zip(unpack(RD_REACT, outs[-1], n, k), want):
        assert eq(got, w_), (name, k, n_sub)
    outs.append(run(RD_CLOSE, V, F, k=k, u=u, v=v, un=un, vn=vn))
    for got, w_ in zip(unpack(RD_CLOSE, outs[-1], n, k), close(m, u, v, un, vn)):
        assert eq(got, w_), (name, k)
    return outs
