"""The numpy / scipy restatement of the wave equation on a surface (include/smg.h: smg_wave_*), in the kernels' operation order, with direct solves;
the ctypes wrappers of smg_wave_host and smg_debug_wave; the dense step map and the bound on two runs' distance.

    planes    mt = m / (speed speed);  s2 = 2.0 + sigma dt;  a = 0.25 dt dt;  q2 = 2.0 / dt
    rhs       b = mt (s2 u + dt v);  rsq = b b (0.0 on a known row);  z = 2.0 u + dt v
    sources   b = b + a (sig0 + sig1);  rsq = b b            at the source vertices
    solve     A w = b,  A = diag(0.5 s2 mt) + a C,  C = -L;  clamped: the boundary rows of w are 0 and A is its interior block
    advance   u' = w - u;  d = u' - u;  v' = q2 d - v;  ke = 0.5 ((mt v') v');  then rhs of (u', v')
    energy    kinetic: the fixed-order sum of ke per column;  potential: the fixed-order sum of k_fluid_velocity's face terms 0.5 (A_f |grad u'|^2)

Only +, - and * occur in the kernels: the library's host twin and its kernels are held to this file bit for bit.  u, v, w, b and z are nV x k
arrays here (the library's blocks are column-major); term planes are k x nV; signals and traces are rows of (vertex of the list) x column."""
import ctypes as C

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import fluid_np
from fluid_np import LAUNCHER_MESHES, PYRAMIDS, mass, shape  # noqa: F401  (shared with the tests)
from hodge_np import boundary_vertices
from oracle import mesh_np as M
from pd_np import EPS, fixed_sum  # noqa: F401
from rd_np import SENTINEL

WAVE_RHS, WAVE_SOURCES, WAVE_ADVANCE, WAVE_RECORD = range(4)
DEFAULTS = dict(dt=1.0, damping=0.0, clamped=0)


# ---- the kernels' expressions --------------------------------------------------------------------------------------------------------------------
def planes(m, speed, sigma, dt):
    """(mt, s2) of wave_host_planes; speed, sigma: nV values, a scalar, or None (1 and 0)"""
    n = m.shape[0]
    mt = m if speed is None else m / (np.broadcast_to(np.asarray(speed, dtype=np.float64), (n,)) * np.broadcast_to(np.asarray(speed, dtype=np.float64), (n,)))
    s2 = np.full(n, 2.0) if sigma is None else 2.0 + np.broadcast_to(np.asarray(sigma, dtype=np.float64), (n,)) * dt
    return np.array(mt), np.array(s2)


def known_mask(F, nV, clamped):
    known = np.zeros(nV, dtype=bool)
    if clamped:
        known[boundary_vertices(np.asarray(F))] = True
    return known


def rhs(mt, s2, known, dt, u, v):
    """(b nV x k, rsq k x nV, z nV x k, the sum of rsq) of k_wave_rhs and its reduction"""
    b = mt[:, None] * (s2[:, None] * u + dt * v)
    z = 2.0 * u + dt * v
    rsq = np.ascontiguousarray((b * b).T)
    rsq[:, known] = 0.0
    return b, rsq, z, fixed_sum(rsq.reshape(-1))


def sources(b, rsq, idx, sig0, sig1, a):
    """(b, rsq, the sum of rsq) after k_wave_sources; sig0, sig1: n_src x k"""
    b, rsq = np.array(b), np.array(rsq)
    x = b[idx] + a * (sig0 + sig1)
    b[idx] = x
    rsq[:, idx] = (x * x).T
    return b, rsq, fixed_sum(rsq.reshape(-1))


def advance(mt, q2, w, u, v):
    """(u', v' nV x k, ke k x nV, the sums of ke) of k_wave_advance and its reductions"""
    un = w - u
    d = un - u
    vn = q2 * d - v
    ke = np.ascontiguousarray((0.5 * ((mt[:, None] * vn) * vn)).T)
    return un, vn, ke, np.array([fixed_sum(t) for t in ke])


def potential(V, F, u):
    """the k potential energies: the fixed-order sums of k_fluid_velocity's face terms"""
    return fluid_np.velocity(V, F, u)[2]


def test_state(V, F, k, clamped=False):
    """(u, v, w as nV x k): smooth fields of the positions; 0 on the boundary when clamped"""
    u, v = fluid_np.hodge_np.potentials(V, k)
    u, v = np.array(u), np.array(v)
    w = np.ascontiguousarray(2.0 * u + 0.25 * np.cos(3.0 * V[:, [2]] + np.arange(k)[None, :]))
    if clamped:
        bnd = boundary_vertices(np.asarray(F))
        u[bnd], v[bnd], w[bnd] = 0.0, 0.0, 0.0
    return u, v, w


def test_lists(V, F, count, clamped=False):
    """`count` distinct vertices that contain the first and the last usable vertex (interior ones when clamped)"""
    n = V.shape[0]
    ok = np.setdiff1d(np.arange(n), boundary_vertices(np.asarray(F))) if clamped else np.arange(n)
    pick = [ok[0], ok[-1], ok[len(ok) // 2]][:count] if count > 1 else [ok[-1]]
    return np.array(pick, dtype=np.int32)


# ---- the method with direct solves ---------------------------------------------------------------------------------------------------------------
class WaveNp:
    """the whole step with scipy.sparse.linalg.splu on A; L: the cotangent matrix, numpy's or the library's own bits.  After a step self.res holds
    the direct solve's residual 2-norms per column (over the unknown rows), self.b the right-hand side and self.w the solve's answer"""

    def __init__(self, V, F, L=None, speed=None, sigma=None, **params):
        self.V, self.F = np.asarray(V, dtype=np.float64), np.asarray(F)
        self.p = dict(DEFAULTS, **params)
        self.C = sp.csr_matrix(-(M.cotmatrix(self.V, self.F) if L is None else L))
        self.m = mass(self.V, self.F)[0]
        self.speed, self.sigma = speed, sigma
        self.known = known_mask(self.F, self.V.shape[0], self.p["clamped"])
        self.free = np.flatnonzero(~self.known)
        self.src = np.zeros(0, dtype=np.int32)
        self.rec = np.zeros(0, dtype=np.int32)
        self.u = self.v = self.res = self.b = self.w = None
        self.system()

    def system(self):
        dt = self.p["dt"]
        self.mt, self.s2 = planes(self.m, self.speed, self.p["damping"] if self.sigma is None else self.sigma, dt)
        self.a, self.q2 = 0.25 * dt * dt, 2.0 / dt
        self.A = (sp.diags(0.5 * self.s2 * self.mt) + self.a * self.C).tocsr()
        self.Auu = self.A[self.free][:, self.free].tocsc()
        self.lu = spla.splu(self.Auu)
        self.mu = float(np.min(0.5 * self.s2 * self.mt))

    def set_params(self, **params):
        self.p.update(params)
        self.system()

    def set_state(self, u, v):
        n = self.V.shape[0]
        self.u, self.v = np.array(np.asarray(u, dtype=np.float64).reshape(n, -1)), np.array(np.asarray(v, dtype=np.float64).reshape(n, -1))

    def right_hand_side(self, f0=None, f1=None):
        """(b, the sum of its squares, the warm start) of the current state; f0, f1: n_src x k forces at the step's two ends"""
        b, rsq, z, ss = rhs(self.mt, self.s2, self.known, self.p["dt"], self.u, self.v)
        if f0 is not None:
            b, rsq, ss = sources(b, rsq, self.src, f0, f1, self.a)
        return b, ss, z

    def solve(self, b):
        w = np.zeros(b.shape)
        w[self.free] = self.lu.solve(b[self.free])
        return w, np.linalg.norm(b[self.free] - self.Auu @ w[self.free], axis=0)

    def step(self, n_steps=1, signal=None):
        """-> (energy n_steps x 2k, traces n_steps x n_rec x k); signal: (n_steps + 1) x n_src x k"""
        E, T = [], []
        for t in range(n_steps):
            f0, f1 = (None, None) if signal is None else (signal[t], signal[t + 1])
            self.b, self.ss, _ = self.right_hand_side(f0, f1)
            self.w, self.res = self.solve(self.b)
            self.u0, self.v0 = self.u, self.v
            self.u, self.v, _, ke = advance(self.mt, self.q2, self.w, self.u, self.v)
            E.append(np.concatenate([ke, potential(self.V, self.F, self.u)]))
            T.append(self.u[self.rec])
        return np.stack(E), np.stack(T)

    def energy(self, u=None, v=None):
        """(kinetic, potential) per column as the library reports them"""
        u, v = (self.u, self.v) if u is None else (u, v)
        ke = np.ascontiguousarray((0.5 * ((self.mt[:, None] * v) * v)).T)
        return np.array([fixed_sum(t) for t in ke]), potential(self.V, self.F, u)

    # ---- exact-arithmetic quantities of the identities, in plain numpy (not the kernels' order) ----------------------------------------------
    def E(self, u, v):
        """0.5 v' Mt v + 0.5 u' C u per column"""
        return 0.5 * np.sum(v * (self.mt[:, None] * v), axis=0) + 0.5 * np.sum(u * (self.C @ u), axis=0)

    def E_abs(self, u, v):
        """the same sum with every term's absolute value: the scale of E's own rounding"""
        return 0.5 * np.sum(v * (self.mt[:, None] * v), axis=0) + 0.5 * np.sum(np.abs(u) * (abs(self.C) @ np.abs(u)), axis=0)

    def residual(self, w, b):
        """r = A w - b on the unknown rows, 0 on the known ones"""
        r = self.A @ w - b
        r[self.known] = 0.0
        return r

    def step_map(self):
        """the dense 2 nV x 2 nV matrix S with (u', v') = S (u, v) for an unforced step, exact solves"""
        n = self.V.shape[0]
        Ainv = np.zeros((n, n))
        Ainv[np.ix_(self.free, self.free)] = np.linalg.inv(self.Auu.toarray())
        W = np.concatenate([Ainv * (self.mt * self.s2)[None, :], Ainv * (self.mt * self.p["dt"])[None, :]], axis=1)
        eye, zero = np.eye(n), np.zeros((n, n))
        return np.concatenate([W - np.concatenate([eye, zero], axis=1), self.q2 * W - np.concatenate([2.0 * self.q2 * eye, eye], axis=1)], axis=0)


# ---- how far two runs of the method can drift apart: CHAIN of tests/test_gpu_wave.py --------------------------------------------------------------
def power_norms(S, steps):
    """[|S^0|_2, ..., |S^(steps - 1)|_2] from numpy"""
    out, P = [1.0], np.eye(S.shape[0])
    for _ in range(1, steps):
        P = S @ P
        out.append(float(np.linalg.norm(P, 2)))
    return np.array(out)


class Chain:
    """The distance between the restatement `ref` and another run of the same steps from the same start whose solves stop at the absolute residual
    `tol` (0: exact answers), | | the 2-norm of one column's (u, v) together: after n steps at most sum_j |S^(n - j)|_2 delta_j with

        beta_j  = (10 tol + res_np) / min_i(0.5 s2_i mt_i) + 8 eps |mt (|s2 u| + dt |v|) + a |f0 + f1||_2 / min_i(0.5 s2_i mt_i)
        delta_j = sqrt(1 + q2^2) beta_j + 2 eps sqrt(|u'|^2 + (q2 |u'| + 2 q2 |u' - u| + |v'|)^2)

    (the derivation: CHAIN in tests/test_gpu_wave.py).  after() is called once the restatement has stepped; extra: added to beta_j."""

    def __init__(self, ref, tol, norms):
        self.ref, self.tol, self.norms, self.deltas = ref, tol, norms, []

    def after(self, f0=None, f1=None, extra=0.0):
        r = self.ref
        mag = r.mt[:, None] * (np.abs(r.s2[:, None] * r.u0) + r.p["dt"] * np.abs(r.v0))
        if f0 is not None:
            mag[r.src] += r.a * np.abs(f0 + f1)
        beta = (10.0 * self.tol + r.res) / r.mu + 8.0 * EPS * np.linalg.norm(mag, axis=0) / r.mu + extra
        nu, nd, nv = np.linalg.norm(r.u, axis=0), np.linalg.norm(r.u - r.u0, axis=0), np.linalg.norm(r.v, axis=0)
        self.deltas.append(np.sqrt(1.0 + r.q2 ** 2) * beta + 2.0 * EPS * np.sqrt(nu ** 2 + (r.q2 * nu + 2.0 * r.q2 * nd + nv) ** 2))
        n = len(self.deltas)
        return sum(self.norms[n - 1 - j] * self.deltas[j] for j in range(n))


def distance(u, v, ref_u, ref_v):
    """the 2-norm of one column's difference, u and v together"""
    return np.sqrt(np.sum((u - ref_u) ** 2 + (v - ref_v) ** 2, axis=0))


# ---- the library's side, shared with tests/test_gpu_wave.py ------------------------------------------------------------------------------------------
def out_size(op, nV, k, n_idx):
    return n_idx * k if op == WAVE_RECORD else 9 * nV * k + 2 * k + 1 if op == WAVE_ADVANCE else 3 * nV * k + 1


def unpack(op, out, nV, k, n_idx):
    """the outputs of an op in the restatement's shapes"""
    nk = nV * k
    col = lambda j: out[j * nk:(j + 1) * nk].reshape(k, nV).T   # noqa: E731
    pl = lambda j: out[j * nk:(j + 1) * nk].reshape(k, nV)      # noqa: E731
    if op == WAVE_RECORD:
        return (out.reshape(n_idx, k),)
    if op == WAVE_ADVANCE:
        return (col(0), col(1), pl(2), col(3), col(4), pl(5), col(6), pl(7), col(8), out[9 * nk:9 * nk + k], out[9 * nk + k:9 * nk + 2 * k], out[9 * nk + 2 * k])
    return col(0), pl(1), col(2), out[3 * nk]


def _call(fn, with_guard, op, V, F, k=1, speed=None, sigma=None, clamped=0, dt=0.5, u=None, v=None, w=None, idx=None, sig0=None, sig1=None, over=None,
          pad=64):
    """`pad` doubles of sentinel follow the op's extent in `out`: nothing past the extent may be written"""
    ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
    nV, nF = V.shape[0], F.shape[0]
    F = np.ascontiguousarray(F, dtype=np.int32)
    rows = lambda x: None if x is None else np.ascontiguousarray(x, dtype=np.float64).reshape(-1)                 # noqa: E731
    cols = lambda x: None if x is None else np.ascontiguousarray(np.asarray(x, dtype=np.float64).T).reshape(-1)   # noqa: E731  (column-major)
    ints = None if idx is None else np.ascontiguousarray(idx, dtype=np.int32).reshape(-1)
    keep = [rows(V), rows(speed), rows(sigma), cols(u), cols(v), cols(w), rows(sig0), rows(sig1)]
    arr = lambda x, ty=dp: None if x is None else x.ctypes.data_as(ty)   # noqa: E731
    n_idx = 0 if ints is None else ints.size
    size = out_size(op, nV, max(k, 0), n_idx)
    out = np.full(size + pad, SENTINEL)
    bad = C.c_int(-1)
    q = dict(nV=nV, nF=nF, k=k, F=arr(F, ip), V=arr(keep[0]), speed=arr(keep[1]), sigma=arr(keep[2]), clamped=int(clamped), dt=float(dt), u=arr(keep[3]),
             v=arr(keep[4]), w=arr(keep[5]), idx=arr(ints, ip), n_idx=n_idx, sig0=arr(keep[6]), sig1=arr(keep[7]), out=arr(out))
    q.update(over or {})
    args = [op] + [q[key] for key in ("nV", "nF", "k", "F", "V", "speed", "sigma", "clamped", "dt", "u", "v", "w", "idx", "n_idx", "sig0", "sig1", "out")]
    rc = fn(*args, C.byref(bad)) if with_guard else fn(*args)
    if rc == 0:
        assert np.all(out[size:] == SENTINEL), "op %d wrote past its extent" % op
        assert not np.any(out[:size] == SENTINEL), "op %d left a part of its extent unwritten" % op
    return rc, bad.value, out[:size]


def host(smg, op, V, F, **kw):
    """one call of smg_wave_host; returns (rc, out)"""
    rc, _, out = _call(smg._lib.load().smg_wave_host, False, op, V, F, **kw)
    return rc, out


def hook(smg, op, V, F, **kw):
    """one call of smg_debug_wave; returns (rc, guard hits, out)"""
    return _call(smg._lib.load().smg_debug_wave, True, op, V, F, **kw)


def nonuniform(V):
    """(speed, sigma) that vary smoothly over the mesh: speed in [0.75, 1.25], sigma in [0, 0.4]"""
    return 1.0 + 0.25 * np.sin(2.0 * V[:, 0] + V[:, 1]), 0.2 * (1.0 + np.cos(3.0 * V[:, 2] - V[:, 0]))


def check_launchers(run, name, k, clamped, count):
    """all four ops of `run(op, V, F, **operands) -> out` on one mesh against the restatement, bit for bit; ADVANCE's next right-hand side against
    RHS of (u', v'); shared by the host twin's and the device's tests.  Returns the outputs for a comparison of the two."""
    V, F = shape(name)
    n = V.shape[0]
    u, v, w = test_state(V, F, k, clamped)
    speed, sigma = nonuniform(V)
    m = mass(V, F)[0]
    dt = 0.03
    mt, s2 = planes(m, speed, sigma, dt)
    a, q2 = 0.25 * dt * dt, 2.0 / dt
    known = known_mask(F, n, clamped)
    idx = test_lists(V, F, count, clamped)
    assert idx.size == count and (clamped or (n - 1 in idx and (count == 1 or 0 in idx)))
    rng = np.random.default_rng(n + 10 * k + count)
    sig0, sig1 = rng.standard_normal((count, k)), rng.standard_normal((count, k))
    eq = np.array_equal
    common = dict(k=k, speed=speed, sigma=sigma, clamped=int(clamped), dt=dt)
    outs = [run(WAVE_RHS, V, F, u=u, v=v, **common)]
    want = rhs(mt, s2, known, dt, u, v)
    for got, w_ in zip(unpack(WAVE_RHS, outs[-1], n, k, 0), want):
        assert eq(got, w_), (name, k, clamped, "rhs")
    assert not clamped or (np.all(want[1][:, known] == 0.0) and np.all(want[0][known] == 0.0))
    outs.append(run(WAVE_SOURCES, V, F, u=u, v=v, idx=idx, sig0=sig0, sig1=sig1, **common))
    b2, rsq2, ss2 = sources(want[0], want[1], idx, sig0, sig1, a)
    assert not eq(b2, want[0])
    for got, w_ in zip(unpack(WAVE_SOURCES, outs[-1], n, k, count), (b2, rsq2, want[2], ss2)):
        assert eq(got, w_), (name, k, clamped, "sources")
    outs.append(run(WAVE_ADVANCE, V, F, u=u, v=v, w=w, **common))
    un, vn, ke, kes = advance(mt, q2, w, u, v)
    nb, nrsq, nz, nss = rhs(mt, s2, known, dt, un, vn)
    got = unpack(WAVE_ADVANCE, outs[-1], n, k, 0)
    for g_, w_ in zip(got, (un, vn, ke, un, vn, ke, nb, nrsq, nz, kes, potential(V, F, un), nss)):
        assert eq(g_, w_), (name, k, clamped, "advance")
    assert not clamped or (np.all(un[known] == 0.0) and np.all(vn[known] == 0.0)), "exact zeros on the clamped rows"
    again = unpack(WAVE_RHS, run(WAVE_RHS, V, F, u=un, v=vn, **common), n, k, 0)           # the fused right-hand side is RHS of (u', v')
    assert eq(got[6], again[0]) and eq(got[7], again[1]) and eq(got[8], again[2]) and got[11] == again[3]
    outs.append(run(WAVE_RECORD, V, F, k=k, u=u, idx=np.concatenate([idx, idx[:1]])))     # receivers may repeat
    assert eq(unpack(WAVE_RECORD, outs[-1], n, k, count + 1)[0], u[np.concatenate([idx, idx[:1]])])
    return outs
