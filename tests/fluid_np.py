"""The numpy / scipy restatement of incompressible flow on a surface in vorticity form (include/smg.h: smg_fluid_*), in the kernels' operation order,
with direct solves for the two systems; the ctypes wrappers of smg_fluid_host and smg_debug_fluid.

    (-L) psi = -m (w - wbar);   wbar = sum(m w) / sum(m) and psi_0 = 0 on a closed mesh;   wbar = 0 and psi = 0 on the boundary otherwise
    corner of vertex i in face (i, j, k):  c = ((psi_i + psi_j) + psi_k) / 3.0;  Phi_ij = 0.5 (psi_i + psi_j) - c;  Phi_ik = c - 0.5 (psi_i + psi_k)
    adv_i = 0.0 - (sum_segments (0.5 (Phi - theta |Phi|)) (w_nbr - w_i)) / m_i;     rate_i = (sum_segments max(Phi, 0.0)) / m_i
    stage:  out = a w_n + b (w_s + dt adv(w_s));   (a, b) = (0, 1) | (0, 1), (1/2, 1/2) | (0, 1), (3/4, 1/4), (1/3, 2/3)
    viscosity:  (M + viscosity dt (-L)) w_new = m w*, no known rows

The sums over a corner list run in list order, one slot of every vertex at a time and segment ij before ik, so the floating-point order is the
kernels'; sums of per-vertex and per-face terms are pd_np.fixed_sum, the order of launch_fixed_sum; a maximum is the same in any order.  Only +, -, *,
/, max and fabs occur: the library's host twin and its kernels are held to this file bit for bit.  Vorticity and stream function are nV x k arrays
here (the library's blocks are column-major); term planes are k x nV, velocities k x nF x 3."""
import ctypes as C

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import hodge_np
from hodge_np import boundary_vertices, cross3, dot3
from morph_np import rest_faces
from oracle import mesh_np as M
from pd_np import EPS, corner_lists, fixed_sum  # noqa: F401  (shared with the tests)

FLUID_RHS, FLUID_ADVECT, FLUID_VELOCITY, FLUID_DIAG, FLUID_DT = range(5)
LAUNCHER_MESHES = ("icosphere1", "icosphere3", "torus", "square", "bunny.smgm")
PYRAMIDS = ("pyramid255", "pyramid256", "pyramid257")
DEFAULTS = dict(theta=0.0, stages=3, viscosity=0.0, dt=0.0, cfl=0.5)
PAIRS = {1: ((0.0, 1.0),), 2: ((0.0, 1.0), (0.5, 0.5)), 3: ((0.0, 1.0), (0.75, 0.25), (1.0 / 3.0, 2.0 / 3.0))}
shape = hodge_np.shape


# ---- the kernels' expressions --------------------------------------------------------------------------------------------------------------------
def mass(V, F):
    """(m nV, its fixed-order sum) of k_fluid_mass: a third of the areas around every vertex, summed in corner-list order"""
    _, _, A = rest_faces(V, F)
    acc = np.zeros(V.shape[0])
    for vs, ts in corner_lists(np.asarray(F), V.shape[0]):
        acc[vs] = acc[vs] + A[ts // 3]
    m = acc / 3.0
    return m, fixed_sum(m)


def known_rows(F, nV):
    """(mask of the rows whose psi is given, the number of boundary vertices): the boundary, or vertex 0 on a closed mesh"""
    bnd = boundary_vertices(np.asarray(F))
    known = np.zeros(nV, dtype=bool)
    known[bnd if bnd.size else 0] = True
    return known, int(bnd.size)


def diag(m, w):
    """(m w and (1/2) m w^2 as k x nV, their sums k each) of k_fluid_diag"""
    mw = m[:, None] * w
    ew = 0.5 * (mw * w)
    mw, ew = np.ascontiguousarray(mw.T), np.ascontiguousarray(ew.T)
    return mw, ew, np.array([fixed_sum(t) for t in mw]), np.array([fixed_sum(t) for t in ew])


def rhs(V, F, w, m=None, no_known=False):
    """(m, msum, mw k x nV, mwsum k, r nV x k, rsq k x nV, the one sum of rsq) of k_fluid_diag, the sums and k_fluid_rhs"""
    m, msum = mass(V, F) if m is None else m
    known, nb = known_rows(F, V.shape[0])
    mw, _, mwsum, _ = diag(m, w)
    wbar = mwsum / msum if nb == 0 else np.zeros(w.shape[1])
    r = 0.0 - m[:, None] * (w - wbar[None, :])
    rsq = np.ascontiguousarray((r * r).T)
    if not no_known:
        rsq[:, known] = 0.0
    return m, msum, mw, mwsum, r, rsq, fixed_sum(rsq.reshape(-1))


def fluxes(F, psi):
    """(Phi_ij, Phi_ik), 3 nF x k each, row t = 3 f + i: the two segments of corner i of face f"""
    F = np.asarray(F)
    vi, vj, vk = F.reshape(-1), F[:, [1, 2, 0]].reshape(-1), F[:, [2, 0, 1]].reshape(-1)
    pi, pj, pk = psi[vi], psi[vj], psi[vk]
    c = ((pi + pj) + pk) / 3.0
    return 0.5 * (pi + pj) - c, c - 0.5 * (pi + pk)


def rates(V, F, psi, m=None):
    """(rate k x nV, their maxima k) of k_fluid_advect<true>"""
    m = mass(V, F)[0] if m is None else m
    fij, fik = fluxes(F, psi)
    rij, rik = np.maximum(fij, 0.0), np.maximum(fik, 0.0)
    racc = np.zeros(psi.shape)
    for vs, ts in corner_lists(np.asarray(F), V.shape[0]):
        racc[vs] = racc[vs] + rij[ts]
        racc[vs] = racc[vs] + rik[ts]
    rate = np.ascontiguousarray((racc / m[:, None]).T)
    return rate, rate.max(axis=1)


def advect(V, F, psi, w, wn, a, b, dt, theta, m=None, lists=None):
    """(out nV x k, rate k x nV, mw k x nV, the rates' maxima k, the sums of mw k) of k_fluid_advect<false> and the reductions"""
    m = mass(V, F)[0] if m is None else m
    F = np.asarray(F)
    vi, vj, vk = F.reshape(-1), F[:, [1, 2, 0]].reshape(-1), F[:, [2, 0, 1]].reshape(-1)
    fij, fik = fluxes(F, psi)
    tij = (0.5 * (fij - theta * np.abs(fij))) * (w[vj] - w[vi])
    tik = (0.5 * (fik - theta * np.abs(fik))) * (w[vk] - w[vi])
    rij, rik = np.maximum(fij, 0.0), np.maximum(fik, 0.0)
    acc, racc = np.zeros(w.shape), np.zeros(w.shape)
    for vs, ts in (corner_lists(F, V.shape[0]) if lists is None else lists):
        acc[vs] = acc[vs] + tij[ts]
        acc[vs] = acc[vs] + tik[ts]
        racc[vs] = racc[vs] + rij[ts]
        racc[vs] = racc[vs] + rik[ts]
    rate = np.ascontiguousarray((racc / m[:, None]).T)
    adv = 0.0 - acc / m[:, None]
    out = a * wn + b * (w + np.asarray(dt, dtype=np.float64)[None, :] * adv)
    mw = np.ascontiguousarray((m[:, None] * out).T)
    return out, rate, mw, rate.max(axis=1), np.array([fixed_sum(t) for t in mw])


def velocity(V, F, psi):
    """(U k x nF x 3, the terms (1/2) A |grad psi|^2 as k x nF, their sums k) of k_fluid_velocity"""
    W, nrm, A = rest_faces(V, F)
    g = hodge_np.grad(W, F, psi)
    U = cross3(nrm[None], g)
    terms = 0.5 * (A[None] * dot3(g, g))
    return U, terms, np.array([fixed_sum(t) for t in terms])


def step_dt(cfl, rmax3, time_in):
    """(dt, the step's cfl, the times after it) of k_fluid_dt on the maxima of three stages (3 x k)"""
    with np.errstate(divide="ignore"):
        dt = np.where(rmax3[0] > 0.0, cfl / np.where(rmax3[0] > 0.0, rmax3[0], 1.0), 0.0)
    return dt, dt * np.maximum(np.maximum(rmax3[0], rmax3[1]), rmax3[2]), time_in + dt


def test_state(V, F, k):
    """(psi, w, wn as nV x k, dt k): smooth fields; psi vanishes on the boundary of a mesh that has one"""
    psi, w = hodge_np.potentials(V, k)
    psi, w = np.array(psi), np.array(w)
    known, nb = known_rows(F, V.shape[0])
    if nb:
        psi[known] = 0.0
    wn = np.ascontiguousarray(w + 0.25 * np.cos(3.0 * V[:, [2]] + np.arange(k)[None, :]))
    return psi, w, wn, 0.01 * (1.0 + np.arange(k))


# ---- the method with direct solves ---------------------------------------------------------------------------------------------------------------
class FluidNp:
    """the whole step with scipy.sparse.linalg.splu on -L without the known rows and on M + viscosity dt (-L); L: the cotangent matrix, numpy's or
    the library's own bits"""

    def __init__(self, V, F, L=None, **params):
        self.V, self.F = np.asarray(V, dtype=np.float64), np.asarray(F)
        self.p = dict(DEFAULTS, **params)
        n = self.V.shape[0]
        self.A = sp.csr_matrix(-(M.cotmatrix(self.V, self.F) if L is None else L))
        self.known, self.nb = known_rows(self.F, n)
        self.I = np.flatnonzero(~self.known)
        self.Auu = self.A[self.I][:, self.I].tocsc()
        self.lu = spla.splu(self.Auu)
        self.m, self.msum = mass(self.V, self.F)
        self.lists = corner_lists(self.F, n)
        self.lu_v = None
        self.w, self.time = None, None

    def lam_min(self):
        return float(spla.eigsh(self.Auu, k=1, sigma=0.0, which="LM", return_eigenvectors=False)[0])

    def set_vorticity(self, w):
        self.w = np.array(np.asarray(w, dtype=np.float64).reshape(self.V.shape[0], -1))
        self.time = np.zeros(self.w.shape[1])

    def stream(self, w=None, solve=None):
        """psi of w (default: the state); solve(r) -> psi replaces the direct solve"""
        w = self.w if w is None else w
        r = rhs(self.V, self.F, w, m=(self.m, self.msum))[4]
        if solve is not None:
            return solve(r)
        psi = np.zeros(w.shape)
        psi[self.I] = self.lu.solve(r[self.I])
        return psi

    def stage(self, w, wn, a, b, dt, psi=None):
        psi = self.stream(w) if psi is None else psi
        return advect(self.V, self.F, psi, w, wn, a, b, dt, self.p["theta"], m=self.m, lists=self.lists)

    def step(self, n_steps=1, solve=None):
        """-> (cfl n_steps x k, time n_steps x k)"""
        p, k = self.p, self.w.shape[1]
        cfls, times = [], []
        for _ in range(n_steps):
            wn, w, rmax = self.w, self.w, []
            dt = np.full(k, p["dt"])
            for s, (a, b) in enumerate(PAIRS[p["stages"]]):
                psi = self.stream(w, solve)
                if s == 0 and p["dt"] == 0.0:
                    r0 = rates(self.V, self.F, psi, m=self.m)[1]
                    with np.errstate(divide="ignore"):
                        dt = np.where(r0 > 0.0, p["cfl"] / np.where(r0 > 0.0, r0, 1.0), 0.0)
                w, _, _, rm, _ = self.stage(w, wn, a, b, dt, psi)
                rmax.append(rm)
            if p["viscosity"] > 0.0:
                if self.lu_v is None:
                    self.lu_v = spla.splu((sp.diags(self.m) + (p["viscosity"] * p["dt"]) * self.A).tocsc())
                w = self.lu_v.solve(self.m[:, None] * w)
            self.w = w
            self.time = self.time + dt
            cfls.append(dt * np.max(np.stack(rmax), axis=0))
            times.append(self.time)
        return np.stack(cfls), np.stack(times)

    def diagnostics(self):
        _, _, circ, enst = diag(self.m, self.w)
        energy = velocity(self.V, self.F, self.stream())[2]
        return dict(circulation=circ, enstrophy=enst, energy=energy, wbar=circ / self.msum if self.nb == 0 else np.zeros(circ.size))


# ---- the library's side, shared with tests/test_gpu_fluid.py ---------------------------------------------------------------------------------------
def out_size(op, nV, nF, k, rates_only=False):
    return {FLUID_RHS: nV + 1 + 3 * nV * k + k + 1, FLUID_ADVECT: nV * k + k if rates_only else 3 * nV * k + 2 * k, FLUID_VELOCITY: 4 * nF * k + k,
            FLUID_DIAG: 2 * nV * k + 2 * k, FLUID_DT: 3 * k}.get(op, nV * k)


def unpack(op, out, nV, nF, k, rates_only=False):
    """the outputs of an op in the restatement's shapes"""
    nk, fk = nV * k, nF * k
    if op == FLUID_RHS:
        o = nV + 1
        return (out[:nV], out[nV], out[o:o + nk].reshape(k, nV), out[o + nk:o + nk + k], out[o + nk + k:o + 2 * nk + k].reshape(k, nV).T,
                out[o + 2 * nk + k:o + 3 * nk + k].reshape(k, nV), out[o + 3 * nk + k])
    if op == FLUID_ADVECT and rates_only:
        return out[:nk].reshape(k, nV), out[nk:]
    if op == FLUID_ADVECT:
        return out[:nk].reshape(k, nV).T, out[nk:2 * nk].reshape(k, nV), out[2 * nk:3 * nk].reshape(k, nV), out[3 * nk:3 * nk + k], out[3 * nk + k:]
    if op == FLUID_VELOCITY:
        return out[:3 * fk].reshape(k, nF, 3), out[3 * fk:4 * fk].reshape(k, nF), out[4 * fk:]
    if op == FLUID_DIAG:
        return out[:nk].reshape(k, nV), out[nk:2 * nk].reshape(k, nV), out[2 * nk:2 * nk + k], out[2 * nk + k:]
    return out[:k], out[k:2 * k], out[2 * k:]


SENTINEL = -7.25e300


def _call(fn, with_guard, op, V, F, k=1, w=None, psi=None, wn=None, a=0.0, b=1.0, dt=None, theta=0.0, rates_only=False, over=None, pad=64):
    """`pad` doubles of sentinel follow the op's extent in `out`: nothing past the extent may be written.  FLUID_DT: w = the maxima (3 x k), psi = the
    times (k), a = cfl"""
    ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
    nV, nF = V.shape[0], F.shape[0]
    F = np.ascontiguousarray(F, dtype=np.int32)
    rows = lambda x: None if x is None else np.ascontiguousarray(x, dtype=np.float64).reshape(-1)                 # noqa: E731
    cols = lambda x: None if x is None else np.ascontiguousarray(np.asarray(x, dtype=np.float64).T).reshape(-1)   # noqa: E731  (column-major)
    block = rows if op == FLUID_DT else cols
    keep = [rows(V), block(w), block(psi), cols(wn), rows(dt)]
    arr = lambda x, ty=dp: None if x is None else x.ctypes.data_as(ty)   # noqa: E731
    size = out_size(op, nV, nF, max(k, 0), rates_only)
    out = np.full(size + pad, SENTINEL)
    bad = C.c_int(-1)
    q = dict(nV=nV, nF=nF, k=k, F=arr(F, ip), V=arr(keep[0]), w=arr(keep[1]), psi=arr(keep[2]), wn=arr(keep[3]), a=float(a), b=float(b), dt=arr(keep[4]),
             theta=float(theta), rates_only=int(bool(rates_only)), out=arr(out))
    q.update(over or {})
    args = [op] + [q[key] for key in ("nV", "nF", "k", "F", "V", "w", "psi", "wn", "a", "b", "dt", "theta", "rates_only", "out")]
    rc = fn(*args, C.byref(bad)) if with_guard else fn(*args)
    if rc == 0:
        assert np.all(out[size:] == SENTINEL), "op %d wrote past its extent" % op
        assert not np.any(out[:size] == SENTINEL), "op %d left a part of its extent unwritten" % op
    return rc, bad.value, out[:size]


def host(smg, op, V, F, **kw):
    """one call of smg_fluid_host; returns (rc, out)"""
    rc, _, out = _call(smg._lib.load().smg_fluid_host, False, op, V, F, **kw)
    return rc, out


def hook(smg, op, V, F, **kw):
    """one call of smg_debug_fluid; returns (rc, guard hits, out)"""
    return _call(smg._lib.load().smg_debug_fluid, True, op, V, F, **kw)


def check_launchers(run, name, k, theta):
    """every op of `run(op, V, F, **operands) -> out` on one mesh against the restatement, bit for bit: the right-hand side, both forms of the
    transport with each of the three (a, b) pairs, the velocity, the diagnostics' terms and the step's closing arithmetic; shared by the host
    twin's and the device's tests.  Returns the outputs for a comparison of the two."""
    V, F = shape(name)
    n, nF = V.shape[0], F.shape[0]
    psi, w, wn, dt = test_state(V, F, k)
    eq = np.array_equal
    outs = [run(FLUID_RHS, V, F, k=k, w=w)]
    for got, want in zip(unpack(FLUID_RHS, outs[-1], n, nF, k), rhs(V, F, w)):
        assert eq(got, want), name
    outs.append(run(FLUID_ADVECT, V, F, k=k, psi=psi, rates_only=True))
    rate, rmax = rates(V, F, psi)
    got = unpack(FLUID_ADVECT, outs[-1], n, nF, k, True)
    assert eq(got[0], rate) and eq(got[1], rmax), name
    assert np.all(rmax > 0.0)
    for a, b in PAIRS[3]:
        outs.append(run(FLUID_ADVECT, V, F, k=k, psi=psi, w=w, wn=wn, a=a, b=b, dt=dt, theta=theta))
        want = advect(V, F, psi, w, wn, a, b, dt, theta)
        for g_, w_ in zip(unpack(FLUID_ADVECT, outs[-1], n, nF, k), want):
            assert eq(g_, w_), (name, a, b)
        assert eq(want[1], rate), "both forms of the kernel give the same rates"
    outs.append(run(FLUID_VELOCITY, V, F, k=k, psi=psi))
    for g_, w_ in zip(unpack(FLUID_VELOCITY, outs[-1], n, nF, k), velocity(V, F, psi)):
        assert eq(g_, w_), name
    outs.append(run(FLUID_DIAG, V, F, k=k, w=w))
    for g_, w_ in zip(unpack(FLUID_DIAG, outs[-1], n, nF, k), diag(mass(V, F)[0], w)):
        assert eq(g_, w_), name
    rm3 = np.stack([rmax, 1.5 * rmax[::-1], 0.5 * rmax])
    rm3[0, 0] = 0.0 if k > 1 else rm3[0, 0]                               # a column at rest: dt = 0
    t_in = 0.125 + np.arange(k)
    outs.append(run(FLUID_DT, V, F, k=k, w=rm3, psi=t_in, a=0.5))
    for g_, w_ in zip(unpack(FLUID_DT, outs[-1], n, nF, k), step_dt(0.5, rm3, t_in)):
        assert eq(g_, w_), name
    return outs
