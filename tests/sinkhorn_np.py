"""The numpy / scipy restatement of heat-kernel optimal transport on a mesh (include/smg.h: smg_sinkhorn_*; Solomon et al. 2015, Convolutional
Wasserstein Distances), in the operation order of csrc/smg_sinkhorn_inl.hpp, with direct solves for the heat kernel; the ctypes wrapper of smg_sinkhorn_host.

    m the barycentric vertex masses, A = sum m, C~ the cotangent matrix with its negative weights clamped, S = diag(m) + (t / s) C~
    y = K(r):   y^1 = S^-1 r,  y^j = S^-1 (m y^(j-1)),  y_eff = max(y^s, 0) + (floor * sum r) / A
    distance:   r_w = m;  per iteration  y = K(r_w);  e0 = sum |r_v y_eff - mu0|;  r_v = mu0 / y_eff;  z = K(r_v);  r_w = mu1 / z_eff
                value = (4 t) sum (mu0 ln(r_v / m) + mu1 ln(r_w / m))
    barycentre: r_v = m;  per iteration  y = K(r_v);  r_w = MU / y_eff;  z = K(r_w);  d_c = (r_v,c / m) z_eff,c;
                mu = exp(sum_c alpha_c ln d_c);  r_v,c = (m mu) / z_eff,c

Every sum of a plane is pd_np.fixed_sum, the order of launch_fixed_sum.  SCALE and SUBSTEP are +, -, *, /, max and abs alone: the library's host
twin is held to this file bit for bit; VALUE and GEOMEAN go through log and exp and are held to a bound.  Blocks are nV x k
arrays here (the library's are column-major); planes of terms are k x nV."""
import ctypes as C

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import fluid_np
import hodge_np
from oracle import mesh_np as M
from pd_np import EPS, fixed_sum  # noqa: F401  (shared with the tests)

SK_SCALE, SK_SUBSTEP, SK_VALUE, SK_GEOMEAN = range(4)
LAUNCHER_MESHES = ("icosphere1", "icosphere3", "torus", "regular12", "bunny.smgm")
PYRAMIDS = ("pyramid255", "pyramid256", "pyramid257")
DEFAULTS = dict(t=0.0, substeps=1, tol=1e-6, max_iter=500, check_every=5, kernel_floor=1e-10, inner_rel_tol=1e-12, clamp_weights=1)
NEGATIVE = 1e-12      # a weight below -NEGATIVE times the largest weight counts as negative


# ---- meshes and distributions ----------------------------------------------------------------------------------------------------------------------
def regular_square(n):
    """[0, 1]^2 as the unjittered (n + 1)^2 grid; cell (i, j) is split along a-c when (i + j) % 2 == 0 and along b-d otherwise, so that no
    cotangent weight is negative"""
    x, y = np.meshgrid(np.linspace(0, 1, n + 1), np.linspace(0, 1, n + 1), indexing="ij")
    V = np.stack([x.ravel(), y.ravel(), np.zeros(x.size)], axis=1)
    F = []
    for i in range(n):
        for j in range(n):
            a, b, c, d = i * (n + 1) + j, (i + 1) * (n + 1) + j, (i + 1) * (n + 1) + j + 1, i * (n + 1) + j + 1
            F += [[a, b, c], [a, c, d]] if (i + j) % 2 == 0 else [[a, b, d], [b, c, d]]
    return V, np.array(F, dtype=np.int32)


_regular = {}


def shape(name):
    """(V, F) of a test mesh, computed once; regularN: regular_square(N); else hodge_np.shape"""
    if name.startswith("regular"):
        if name not in _regular:
            V, F = regular_square(int(name[len("regular"):]))
            V.setflags(write=False)
            F.setflags(write=False)
            _regular[name] = (V, F)
        return _regular[name]
    return hodge_np.shape(name)


def blob(V, F, centre, width=0.1):
    """emd_np.blob: a mass-weighted Gaussian around vertex `centre` of total mass 1"""
    s = width * np.max(V.max(axis=0) - V.min(axis=0))
    d2 = np.sum((V - V[centre]) ** 2, axis=1)
    mu = fluid_np.mass(V, F)[0] * np.exp(-d2 / (2.0 * s * s))
    return mu / mu.sum()


def pairs(V, F, k):
    """(mu0, mu1), nV x k each: blob pairs; column 1 (where there is one) has exact zeros in both, and its sums still agree"""
    n = V.shape[0]
    c0 = [blob(V, F, (7 * s + 1) % n) for s in range(k)]
    c1 = [blob(V, F, (n // 2 + 11 * s) % n) for s in range(k)]
    mu0, mu1 = np.stack(c0, axis=1), np.stack(c1, axis=1)
    if k > 1:
        for mu in (mu0, mu1):
            mu[::3, 1] = 0.0
            mu[:, 1] /= mu[:, 1].sum()
        mu1[:, 1] *= mu0[:, 1].sum() / mu1[:, 1].sum()
    return mu0, mu1


# ---- the matrix ------------------------------------------------------------------------------------------------------------------------------------
def clamped(C_in):
    """(C~ csr, the number of negative edges, the most negative weight): off-diagonals min(C_ij, 0) of C = -L, the diagonal minus the row sum;
    an edge is negative when its weight -C_ij is below -NEGATIVE times the largest weight"""
    Cm = sp.coo_matrix(C_in)
    off = Cm.row != Cm.col
    r, c, v = Cm.row[off], Cm.col[off], Cm.data[off]
    wmax = float(np.max(-v))
    neg = (v > NEGATIVE * wmax) & (r < c)
    Co = sp.csr_matrix((np.minimum(v, 0.0), (r, c)), shape=Cm.shape)
    Ct = (Co - sp.diags(np.asarray(Co.sum(axis=1)).ravel())).tocsr()
    return Ct, int(neg.sum()), float(min(0.0, np.min(-v)))


def default_t(area):
    return (0.05 * 0.05) * area


# ---- the library's expressions -----------------------------------------------------------------------------------------------------------------------
def sums(planes):
    return np.array([fixed_sum(p) for p in planes])


def effective(y, sr, floor, A):
    """y_eff of a block y (nV x k) whose kernel input summed to sr (k)"""
    return np.maximum(y, 0.0) + ((floor * np.asarray(sr)) / A)[None, :]


def scale(y, r, mu, sr, floor, A):
    """(r' nV x k, the error planes k x nV, the squares k x nV, sum r' k, e0 k, sum of all squares) of the scale op; mu has k_in columns and
    column c reads mu's column c % k_in"""
    k = y.shape[1]
    MU = mu[:, np.arange(k) % mu.shape[1]]
    ye = effective(y, sr, floor, A)
    err = np.abs(r * ye - MU)
    with np.errstate(divide="ignore", invalid="ignore"):
        rn = np.where(MU == 0.0, 0.0, MU / ye)
    rsq = rn * rn
    return rn, np.ascontiguousarray(err.T), np.ascontiguousarray(rsq.T), sums(rn.T), sums(err.T), fixed_sum(rsq.T.reshape(-1))


def substep(y, m):
    """(m y nV x k, the squares k x nV, their sum) of the substep op"""
    r = m[:, None] * y
    rsq = r * r
    return r, np.ascontiguousarray(rsq.T), fixed_sum(rsq.T.reshape(-1))


def value_terms(mu0, mu1, rv, rw, m):
    """(terms k x nV, ln v nV x k, ln w nV x k, their sums k) of the value op"""
    with np.errstate(divide="ignore", invalid="ignore"):
        lv = np.where(mu0 == 0.0, -np.inf, np.log(rv / m[:, None]))
        lw = np.where(mu1 == 0.0, -np.inf, np.log(rw / m[:, None]))
        t0 = np.where(mu0 == 0.0, 0.0, mu0 * lv)
        t1 = np.where(mu1 == 0.0, 0.0, mu1 * lw)
    terms = np.ascontiguousarray((t0 + t1).T)
    return terms, lv, lw, sums(terms)


def geomean(z, rv, prev, sr, alphas, floor, A, m):
    """(r_v' nV x G k_in, the barycentre masses nV x G, the change planes G x nV, the squares G k_in x nV, sum r_v' per column, the change and
    the mass per group, the sum of all squares, the exponent's magnitude sum_c |alpha_c ln d_c| nV x G) of the geomean op"""
    G, kin = alphas.shape
    n = z.shape[0]
    ze = effective(z, sr, floor, A)
    d = (rv / m[:, None]) * ze
    acc, mag, dead = np.zeros((n, G)), np.zeros((n, G)), np.zeros((n, G), dtype=bool)
    for g in range(G):
        for c in range(kin):
            a = alphas[g, c]
            if a > 0.0:
                dc = d[:, g * kin + c]
                pos = dc > 0.0
                with np.errstate(divide="ignore", invalid="ignore"):
                    term = a * np.log(np.where(pos, dc, 1.0))
                acc[:, g] = np.where(pos, acc[:, g] + term, acc[:, g])
                mag[:, g] += np.abs(term)
                dead[:, g] |= ~pos
    mu = np.where(dead, 0.0, np.exp(acc))
    bm = m[:, None] * mu
    with np.errstate(divide="ignore", invalid="ignore"):
        rn = np.repeat(bm, kin, axis=1) / ze
    chg = np.abs(bm - prev)
    rsq = rn * rn
    return (rn, bm, np.ascontiguousarray(chg.T), np.ascontiguousarray(rsq.T), sums(rn.T), sums(chg.T), sums(bm.T), fixed_sum(rsq.T.reshape(-1)), mag)


# ---- the method with direct solves -------------------------------------------------------------------------------------------------------------------
class SinkhornNp:
    """the calls of smg_sinkhorn_* with scipy.sparse.linalg.splu on S; C: the matrix -L, numpy's or the library's own bits.  solve(B) -> X
    replaces the direct solve (a CG stand-in for the device's)"""

    def __init__(self, V, F, C_mat=None, solve=None, **params):
        self.V, self.F = np.asarray(V, dtype=np.float64), np.asarray(F)
        self.p = dict(DEFAULTS, **params)
        self.m, self.A = fluid_np.mass(self.V, self.F)
        self.C = sp.csr_matrix(-M.cotmatrix(self.V, self.F) if C_mat is None else C_mat)
        self.Ct, self.n_clamped, self.w_min = clamped(self.C)
        if not self.p["clamp_weights"]:
            if self.n_clamped:
                raise ValueError("negative cotangent weights")
            self.Ct = self.C
        self.t = self.p["t"] if self.p["t"] > 0.0 else default_t(self.A)
        self.S = (sp.diags(self.m) + (self.t / self.p["substeps"]) * self.Ct).tocsc()
        self.lu = spla.splu(self.S)
        self.solve = solve or (lambda B: self.lu.solve(np.ascontiguousarray(B)))
        self.half_steps = []

    def apply(self, r, eff=True):
        """K(r) -> y_eff (eff) or the raw y^s"""
        r = np.asarray(r, dtype=np.float64).reshape(self.m.size, -1)
        y = self.solve(r)
        for _ in range(1, self.p["substeps"]):
            y = self.solve(substep(y, self.m)[0])
        return effective(y, sums(r.T), self.p["kernel_floor"], self.A) if eff else y

    def _raw(self, r):
        y = self.solve(r)
        for _ in range(1, self.p["substeps"]):
            y = self.solve(substep(y, self.m)[0])
        return y

    def distance(self, mu0, mu1, n_iter=None, check_every=None, **params):
        """the distance loop.  n_iter: exactly that many iterations and no early end.  Returns dict(value, marginal_err,
        iterations, log_v, log_w, r_v, r_w)."""
        p = dict(self.p, **params)
        n = self.m.size
        mu0, mu1 = np.asarray(mu0, dtype=np.float64).reshape(n, -1), np.asarray(mu1, dtype=np.float64).reshape(n, -1)
        k = mu0.shape[1]
        every = p["check_every"] if check_every is None else check_every
        max_iter = p["max_iter"] if n_iter is None else n_iter
        fl, A, m = p["kernel_floor"], self.A, self.m
        rw, rv = np.repeat(m[:, None], k, axis=1), np.zeros((n, k))
        srw = sums(rw.T)
        e0, it = np.full(k, np.inf), 0
        tot = sums(mu0.T)
        for it in range(1, max_iter + 1):
            y = self._raw(rw)
            rv, _, _, srv, e0, _ = scale(y, rv, mu0, srw, fl, A)
            if it > 1 and n_iter is None and (it % every == 0 or it == max_iter) and np.all(e0 <= p["tol"] * tot):
                break
            if it == max_iter:
                break
            z = self._raw(rv)
            rw, _, _, srw, _, _ = scale(z, rw, mu1, srv, fl, A)
        terms, lv, lw, s = value_terms(mu0, mu1, rv, rw, m) if it else (None, None, None, np.zeros(k))
        return dict(value=(4.0 * self.t) * s, marginal_err=e0, iterations=it, log_v=lv, log_w=lw, r_v=rv, r_w=rw, terms=terms)

    def debiased(self, mu0, mu1, **kw):
        d = self.distance(np.concatenate([mu0, mu0, mu1], axis=1), np.concatenate([mu1, mu0, mu1], axis=1), **kw)
        k = mu0.shape[1]
        v = d["value"]
        return v[:k] - 0.5 * v[k:2 * k] - 0.5 * v[2 * k:], d

    def barycenter(self, mus, alphas, n_iter=None, check_every=None, **params):
        """the barycentre loop.  Returns dict(bary nV x G, change, mass, iterations, his: per iteration the
        changes and the largest change of the density mu per group)."""
        p = dict(self.p, **params)
        n = self.m.size
        mus = np.asarray(mus, dtype=np.float64).reshape(n, -1)
        alphas = np.atleast_2d(np.asarray(alphas, dtype=np.float64))
        alphas = alphas / np.array([np.cumsum(a)[-1] for a in alphas])[:, None]
        G, kin = alphas.shape
        every = p["check_every"] if check_every is None else check_every
        max_iter = p["max_iter"] if n_iter is None else n_iter
        fl, A, m = p["kernel_floor"], self.A, self.m
        rv = np.repeat(m[:, None], G * kin, axis=1)
        rw = np.zeros((n, G * kin))
        srv = sums(rv.T)
        bm, chg, mass, it = np.zeros((n, G)), np.full(G, np.inf), np.zeros(G), 0
        his = []
        for it in range(1, max_iter + 1):
            y = self._raw(rv)
            rw, _, _, srw, _, _ = scale(y, rw, mus, srv, fl, A)
            z = self._raw(rw)
            prev = bm
            rv, bm, _, _, srv, chg, mass, _, _ = geomean(z, rv, bm, srw, alphas, fl, A, m)
            his.append((chg, np.abs((bm - prev) / m[:, None]).max(axis=0)))
            if n_iter is None and (it % every == 0 or it == max_iter) and np.all(chg <= p["tol"] * mass):
                break
        return dict(bary=bm, change=chg, mass=mass, iterations=it, his=his)

    def interpolate(self, mu0, mu1, ts, **kw):
        ts = np.asarray(ts, dtype=np.float64)
        return self.barycenter(np.stack([mu0, mu1], axis=1), np.stack([1.0 - ts, ts], axis=1), **kw)


def cg_solver(S, rel=1e-12):
    """solve(B) by scipy's CG to a relative residual `rel`, column by column, from zero: what a solve of that accuracy costs the reference"""
    def solve(B):
        B = np.asarray(B).reshape(S.shape[0], -1)
        X = np.zeros_like(B)
        for c in range(B.shape[1]):
            X[:, c], info = spla.cg(S, B[:, c], rtol=rel, atol=0.0, maxiter=10000)
            assert info == 0
        return X
    return solve


# ---- the library's side -----------------------------------------------------------------------------------------------------------------------------
def out_size(op, nV, k, kin):
    nk = nV * k
    return {SK_SCALE: 3 * nk + 2 * k + 1, SK_SUBSTEP: 2 * nk + 1, SK_VALUE: 3 * nk + k,
            SK_GEOMEAN: 2 * nk * kin + 2 * nk + k * kin + 2 * k + 1}.get(op, nk)


def unpack(op, out, nV, k, kin):
    """the outputs of an op in the restatement's shapes and order"""
    nk = nV * k
    if op == SK_SCALE:
        return (out[:nk].reshape(k, nV).T, out[nk:2 * nk].reshape(k, nV), out[2 * nk:3 * nk].reshape(k, nV), out[3 * nk:3 * nk + k],
                out[3 * nk + k:3 * nk + 2 * k], out[3 * nk + 2 * k])
    if op == SK_SUBSTEP:
        return out[:nk].reshape(k, nV).T, out[nk:2 * nk].reshape(k, nV), out[2 * nk]
    if op == SK_VALUE:
        return out[:nk].reshape(k, nV), out[nk:2 * nk].reshape(k, nV).T, out[2 * nk:3 * nk].reshape(k, nV).T, out[3 * nk:]
    K = k * kin
    nK = nV * K
    o = [0, nK, nK + nk, nK + 2 * nk, 2 * nK + 2 * nk, 2 * nK + 2 * nk + K, 2 * nK + 2 * nk + K + k, 2 * nK + 2 * nk + K + 2 * k]
    return (out[o[0]:o[1]].reshape(K, nV).T, out[o[1]:o[2]].reshape(k, nV).T, out[o[2]:o[3]].reshape(k, nV), out[o[3]:o[4]].reshape(K, nV),
            out[o[4]:o[5]], out[o[5]:o[6]], out[o[6]:o[7]], out[o[7]])


SENTINEL = -7.25e300


def _call(fn, with_guard, op, V, F, k=1, kin=1, y=None, r=None, mu=None, mu1=None, sr=None, alphas=None, floor=1e-10, over=None, pad=64):
    """`pad` doubles of sentinel follow the op's extent in `out`: nothing past the extent may be written.  k: the columns (GEOMEAN: the groups);
    kin: the columns of mu (SCALE) or of a group (GEOMEAN)"""
    ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
    nV, nF = V.shape[0], F.shape[0]
    F = np.ascontiguousarray(F, dtype=np.int32)
    rows = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64).reshape(-1)                 # noqa: E731
    cols = lambda a: None if a is None else np.ascontiguousarray(np.asarray(a, dtype=np.float64).T).reshape(-1)   # noqa: E731  (column-major)
    keep = [rows(V), cols(y), cols(r), cols(mu), cols(mu1), rows(sr), rows(alphas)]
    arr = lambda a, ty=dp: None if a is None else a.ctypes.data_as(ty)   # noqa: E731
    size = out_size(op, nV, max(k, 0), max(kin, 0))
    out = np.full(size + pad, SENTINEL)
    bad = C.c_int(-1)
    a = dict(nV=nV, nF=nF, k=k, kin=kin, F=arr(F, ip), V=arr(keep[0]), y=arr(keep[1]), r=arr(keep[2]), mu=arr(keep[3]), mu1=arr(keep[4]), sr=arr(keep[5]),
             alphas=arr(keep[6]), floor=float(floor), out=arr(out))
    a.update(over or {})
    args = [op] + [a[key] for key in ("nV", "nF", "k", "kin", "F", "V", "y", "r", "mu", "mu1", "sr", "alphas", "floor", "out")]
    rc = fn(*args, C.byref(bad)) if with_guard else fn(*args)
    if rc == 0:
        assert np.all(out[size:] == SENTINEL), "op %d wrote past its extent" % op
        assert not np.any(out[:size] == SENTINEL), "op %d left a part of its extent unwritten" % op
    return rc, bad.value, out[:size]


def host(smg, op, V, F, **kw):
    """one call of smg_sinkhorn_host; returns (rc, out)"""
    rc, _, out = _call(smg._lib.load().smg_sinkhorn_host, False, op, V, F, **kw)
    return rc, out


def test_state(V, F, K, seed=3):
    """(y, r) nV x K: a positive smooth field with a few non-positive entries (the clamp's branch) and a positive scaling"""
    rng = np.random.default_rng(seed)
    n = V.shape[0]
    m = fluid_np.mass(V, F)[0]
    y = np.exp(rng.uniform(-12.0, 0.0, (n, K)))
    y[5 % n::17] *= -1e-9
    y[3 % n, :] = 0.0
    r = m[:, None] * np.exp(rng.uniform(-3.0, 3.0, (n, K)))
    return y, r


def close(a, w, bound):
    """|a - w| <= bound elementwise, equal infinities and zeros allowed"""
    a, w = np.asarray(a), np.asarray(w)
    same = a == w
    with np.errstate(invalid="ignore"):
        return bool(np.all(same | (np.abs(a - w) <= bound)))


def check_launchers(run, name, k, kin=2, G=1):
    """every op of `run(op, V, F, **operands) -> out` (the host twin) on one mesh against the restatement: SCALE and SUBSTEP bit for bit, VALUE to
    16 eps sum |terms| (per term: 16 eps |term|), GEOMEAN to a relative 16 eps (1 + sum_c |alpha_c ln d_c|); the sums of planes that are not
    bit-equal are held to the fixed-order sum of the run's own plane.  Returns (the outputs held bit for bit, the others)."""
    V, F = shape(name)
    n = V.shape[0]
    m, A = fluid_np.mass(V, F)
    mu0, mu1 = pairs(V, F, k)
    y, r = test_state(V, F, k)
    sr, fl = sums(r.T), 1e-10
    eq = np.array_equal
    outs, approx = [], []
    # SCALE with mu's columns = k (the distance) and, where k splits, with fewer (the barycentre's first half step)
    for mc in sorted({k, 1}):
        out = run(SK_SCALE, V, F, k=k, kin=mc, y=y, r=r, mu=mu0[:, :mc], sr=sr, floor=fl)
        outs.append(out)
        for a, w in zip(unpack(SK_SCALE, out, n, k, mc), scale(y, r, mu0[:, :mc], sr, fl, A)):
            assert eq(a, w), (name, "scale", mc)
    out = run(SK_SCALE, V, F, k=k, kin=k, y=y, r=r, mu=mu0, sr=sr, floor=0.0)          # no floor: a non-positive y gives an infinite or NaN r
    outs.append(out)
    for a, w in zip(unpack(SK_SCALE, out, n, k, k), scale(y, r, mu0, sr, 0.0, A)):
        assert eq(a, w, equal_nan=True), (name, "scale without floor")
    out = run(SK_SUBSTEP, V, F, k=k, y=y)
    outs.append(out)
    for a, w in zip(unpack(SK_SUBSTEP, out, n, k, 1), substep(y, m)):
        assert eq(a, w), (name, "substep")
    # VALUE on the scalings of one half step
    rv = scale(y, r, mu0, sr, fl, A)[0]
    rw = scale(np.abs(y[::-1]) + 1e-30, r, mu1, sr, fl, A)[0]
    out = run(SK_VALUE, V, F, k=k, y=rw, r=rv, mu=mu0, mu1=mu1)
    approx.append(out)
    terms, lv, lw, s = unpack(SK_VALUE, out, n, k, 1)
    wt, wlv, wlw, ws = value_terms(mu0, mu1, rv, rw, m)
    assert close(lv, wlv, 16 * EPS * (1.0 + np.abs(np.where(np.isfinite(wlv), wlv, 0.0)))) and close(lw, wlw, 16 * EPS * (1.0 + np.abs(np.where(np.isfinite(wlw), wlw, 0.0))))
    assert eq(np.isneginf(lv), mu0 == 0.0) and eq(np.isneginf(lw), mu1 == 0.0)
    with np.errstate(invalid="ignore"):
        mag = np.where(mu0 == 0.0, 0.0, np.abs(mu0 * wlv)) + np.where(mu1 == 0.0, 0.0, np.abs(mu1 * wlw))
    assert close(terms.T, wt.T, 16 * EPS * mag), (name, "value terms")
    assert eq(s, sums(terms)) and np.all(np.abs(s - ws) <= 16 * EPS * mag.sum(axis=0)), (name, "value")
    # GEOMEAN
    K = G * kin
    z, rvg = test_state(V, F, K, seed=9)
    srg = sums(rvg.T)
    alphas = np.random.default_rng(4).uniform(0.1, 1.0, (G, kin))
    alphas[0, 0] = 0.0 if kin > 1 else 1.0                                             # a zero alpha removes its column
    alphas = alphas / alphas.sum(axis=1)[:, None]
    prev = np.abs(test_state(V, F, G, seed=11)[1])
    out = run(SK_GEOMEAN, V, F, k=G, kin=kin, y=z, r=rvg, mu=prev, sr=srg, alphas=alphas, floor=fl)
    approx.append(out)
    rn, bm, chg, rsq, srn, change, mass, tot = unpack(SK_GEOMEAN, out, n, G, kin)
    wrn, wbm, wchg, wrsq, _, _, _, _, mag = geomean(z, rvg, prev, srg, alphas, fl, A, m)
    rel = 16 * EPS * (1.0 + mag)
    assert close(bm, wbm, rel * np.abs(wbm)), (name, "geomean masses")
    assert close(rn, wrn, np.repeat(rel, kin, axis=1) * np.abs(wrn) * 1.5), (name, "geomean scalings")
    assert close(chg.T, wchg.T, rel * np.abs(wbm) + EPS * wchg.T), (name, "geomean change")          # the mass's error and the subtraction's rounding
    assert eq(srn, sums(rn.T)) and eq(change, sums(chg)) and eq(mass, sums(bm.T)) and tot == fixed_sum(rsq.reshape(-1)) and eq(rsq.T, rn * rn)
    if kin > 1:                                                                        # the column of the zero alpha does not enter group 0's masses
        z2 = z.copy()
        z2[:, 0] = 1.0
        out2 = run(SK_GEOMEAN, V, F, k=G, kin=kin, y=z2, r=rvg, mu=prev, sr=srg, alphas=alphas, floor=fl)
        assert eq(unpack(SK_GEOMEAN, out2, n, G, kin)[1], bm), (name, "zero alpha")
    return outs, approx
