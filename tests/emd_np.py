"""The numpy / scipy restatement of the earth mover's distance on a mesh (include/smg.h: smg_emd_*; Solomon, Rustamov, Guibas, Butscher 2014, in
Beckmann form by ADMM), in the kernels' operation order, with direct solves for the Poisson system; the ctypes wrappers of smg_emd_host and
smg_debug_emd.

    minimise sum_f A_f |J_f|  subject to  sum_f A_f W2_fi . J_f = b_i;    dual: maximise b . psi subject to |grad psi_f| <= 1
    per iteration:  Y = Z - U;  r_i = sum_corners A_f (W2_fi . Y_f) - b_i;  (-L) phi = r, phi_0 = 0;  J = Y - grad phi;
                    T = (alpha J + (1 - alpha) Z) + U;  Z = max(0, 1 - (1 / rho) / |T|) T;  U = T - Z
    bounds:         upper = sum_f A_f |J_f|;  potential = (-rho / max(1, gmax)) phi, gmax^2 = max_f rho^2 |grad phi_f|^2;  lower = b . potential

Per-face vectors are 2-vectors in the face's frame t1 = (p1 - p0) / |p1 - p0|, t2 = n x t1.  The sums over a corner list run in list order, one slot
of every vertex at a time, so the floating-point order is the kernels'; upper, lower and the residual's squares are pd_np.fixed_sum, the order of
launch_fixed_sum; gmax^2 goes through the same tree with the maximum.  Only +, -, *, /, sqrt and max occur: the library's host twin and its kernels
are held to this file bit for bit.  Masses and potentials are nV x k arrays here (the library's blocks are column-major); the state ZU is
k x nF x 4 (Z then U), a frame field k x nF x 2."""
import ctypes as C
import functools

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import hodge_np
from hodge_np import cross3, dot3
from morph_np import rest_faces
from oracle import mesh_np as M
from pd_np import EPS, corner_lists, fixed_sum, fixed_sum_groups  # noqa: F401  (shared with the tests)

EMD_GEOMETRY, EMD_RHS, EMD_UPDATE, EMD_DUAL, EMD_FLOW, EMD_RESIDUAL = range(6)
LAUNCHER_MESHES = ("icosphere1", "icosphere3", "torus", "square", "bunny.smgm")
PYRAMIDS = ("pyramid255", "pyramid256", "pyramid257")
DEFAULTS = dict(gap_tol=1e-2, max_iter=2000, check_every=10, alpha=1.7, rho_scale=0.1, inner_rel_tol=1e-8)
shape = hodge_np.shape


# ---- distributions -------------------------------------------------------------------------------------------------------------------------------
def vertex_mass(V, F):
    """the barycentric (lumped) mass of every vertex: a third of the area of its faces"""
    _, _, A = rest_faces(V, F)
    m = np.zeros(V.shape[0])
    np.add.at(m, np.asarray(F).reshape(-1), np.repeat(A / 3.0, 3))
    return m


def deltas(V, F, i=None, j=None):
    """(mu0, mu1): unit masses at vertices i (default 1) and j (default nV / 2)"""
    n = V.shape[0]
    mu0, mu1 = np.zeros(n), np.zeros(n)
    mu0[1 if i is None else i] = 1.0
    mu1[n // 2 if j is None else j] = 1.0
    return mu0, mu1


def blob(V, F, centre, width=0.1):
    """a mass-weighted Gaussian around vertex `centre` whose width is `width` times the bounding box's longest side, of total mass 1"""
    s = width * np.max(V.max(axis=0) - V.min(axis=0))
    d2 = np.sum((V - V[centre]) ** 2, axis=1)
    mu = vertex_mass(V, F) * np.exp(-d2 / (2.0 * s * s))
    return mu / mu.sum()


def blobs(V, F, i=None, j=None):
    n = V.shape[0]
    return blob(V, F, 1 if i is None else i), blob(V, F, n // 2 if j is None else j)


def pairs(V, F, k):
    """(mu0, mu1), nV x k each: the delta pair, the blob pair, then blob pairs around other vertices"""
    n = V.shape[0]
    cols = [deltas(V, F), blobs(V, F)] + [blobs(V, F, (7 * s + 3) % n, (n // 3 + 11 * s) % n) for s in range(max(0, k - 2))]
    return np.stack([c[0] for c in cols[:k]], axis=1), np.stack([c[1] for c in cols[:k]], axis=1)


def test_state(V, F, k, seed=5):
    """(phi nV x k, ZU k x nF x 4, rho k, alpha): smooth potentials and a state with faces on both sides of the shrink's threshold"""
    rng = np.random.default_rng(seed)
    phi = np.ascontiguousarray(hodge_np.potentials(V, k)[0])
    ZU = rng.standard_normal((k, F.shape[0], 4)) * np.array([3.0, 3.0, 0.5, 0.5])
    ZU[:, 0] = 0.0
    phi[F[0]] = 0.0                                                    # face 0: |T| = 0
    rho = 0.5 + 0.75 * np.arange(k)
    return phi, ZU, rho, 1.7


# ---- the kernels' expressions --------------------------------------------------------------------------------------------------------------------
def frames(V, F):
    """(t1, t2, nF x 3 each) of emd_frame"""
    _, nrm, _ = rest_faces(V, F)
    e = V[F[:, 1]] - V[F[:, 0]]
    t1 = e / np.sqrt(dot3(e, e))[:, None]
    return t1, cross3(nrm, t1)


def geometry(V, F):
    """(W2 as nF x 3 x 2, A as nF, the total area) of k_emd_geometry and its sum"""
    W, _, A = rest_faces(V, F)
    t1, t2 = frames(V, F)
    W2 = np.stack([dot3(W, t1[:, None, :]), dot3(W, t2[:, None, :])], axis=2)
    return W2, A, fixed_sum(A)


def divergence(V, F, X2, b):
    """nV x k: sum over every vertex's corners of A_f (W2_fi . X_f), minus b; X2: k x nF x 2"""
    W2, A, _ = geometry(V, F)
    nV, k = b.shape
    t = (A[None, :, None] * (W2[None, :, :, 0] * X2[:, :, None, 0] + W2[None, :, :, 1] * X2[:, :, None, 1])).reshape(k, -1)   # corner 3 f + i
    acc = np.zeros((k, nV))
    for vs, ts in corner_lists(np.asarray(F), nV):
        acc[:, vs] = acc[:, vs] + t[:, ts]
    return np.ascontiguousarray((acc - b.T).T)


def rhs(V, F, b, ZU):
    """r (nV x k) of k_emd_rhs"""
    return divergence(V, F, ZU[:, :, :2] - ZU[:, :, 2:], b)


def residual(V, F, b, J2):
    """(d nV x k, dsq k x nV with row 0 zeroed, their sums) of k_emd_rhs on J: the weak divergence of J minus b"""
    d = divergence(V, F, J2, b)
    dsq = np.ascontiguousarray((d * d).T)
    dsq[:, 0] = 0.0
    return d, dsq, np.array([fixed_sum(t) for t in dsq])


def grad2(W2, F, phi):
    """k x nF x 2: sum_i phi_i W2_fi, i in order"""
    p0, p1, p2 = phi[F[:, 0]].T[:, :, None], phi[F[:, 1]].T[:, :, None], phi[F[:, 2]].T[:, :, None]
    return (p0 * W2[None, :, 0, :] + p1 * W2[None, :, 1, :]) + p2 * W2[None, :, 2, :]


def fixed_max(term):
    """launch_fixed_max's tree; a maximum is the same in any order"""
    return float(np.max(term))


def update(V, F, phi, ZU, rho, alpha):
    """(ZU' k x nF x 4, J k x nF x 2, the planes A |J| and rho^2 |grad phi|^2 as k x nF, upper k, gmax^2 k) of k_emd_update and the reductions"""
    W2, A, _ = geometry(V, F)
    rho = np.asarray(rho, dtype=np.float64)[:, None, None]
    Z, U = ZU[:, :, :2], ZU[:, :, 2:]
    Y = Z - U
    g = grad2(W2, F, phi)
    J = Y - g
    T = (alpha * J + (1.0 - alpha) * Z) + U
    nT = np.sqrt(T[:, :, 0] * T[:, :, 0] + T[:, :, 1] * T[:, :, 1])
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.where(nT > 0.0, np.maximum(0.0, 1.0 - (1.0 / rho[:, :, 0]) / nT), 0.0)
    Zn = s[:, :, None] * T
    Un = T - Zn
    up = A[None] * np.sqrt(J[:, :, 0] * J[:, :, 0] + J[:, :, 1] * J[:, :, 1])
    gq = (rho[:, :, 0] * rho[:, :, 0]) * (g[:, :, 0] * g[:, :, 0] + g[:, :, 1] * g[:, :, 1])
    return np.concatenate([Zn, Un], axis=2), J, up, gq, np.array([fixed_sum(t) for t in up]), np.array([fixed_max(t) for t in gq])


def dual(b, phi, rho, gmax2):
    """(potential nV x k, terms k x nV, lower k) of k_emd_dual: potential = (-rho / max(1, sqrt(gmax2))) phi, terms b_i potential_i"""
    s = -np.asarray(rho, dtype=np.float64) / np.maximum(1.0, np.sqrt(gmax2))
    pot = s[None, :] * phi
    terms = np.ascontiguousarray((b * pot).T)
    return pot, terms, np.array([fixed_sum(t) for t in terms])


def flow(V, F, J2):
    """k x nF x 3: J0 t1 + J1 t2"""
    t1, t2 = frames(V, F)
    return J2[:, :, [0]] * t1[None] + J2[:, :, [1]] * t2[None]


def seq_sum(x):
    """the sum in index order"""
    return float(np.cumsum(x)[-1]) if x.size else 0.0


def column_setup(b, area, rho_scale):
    """(m, rho, |b|_2 per column) as the library forms them: sums in index order; a zero column has rho = 1"""
    k = b.shape[1]
    m = np.array([0.5 * seq_sum(np.abs(b[:, c])) for c in range(k)])
    nb = np.array([np.sqrt(seq_sum(b[:, c] * b[:, c])) for c in range(k)])
    rho = np.array([rho_scale * np.sqrt(area) / m[c] if m[c] > 0.0 else 1.0 for c in range(k)])
    return m, rho, nb


# ---- the method with direct solves ---------------------------------------------------------------------------------------------------------------
class EmdNp:
    """the whole query with scipy.sparse.linalg.splu on -L with row 0 removed; L: the cotangent matrix, numpy's or the library's own bits"""

    def __init__(self, V, F, L=None, **params):
        self.V, self.F = np.asarray(V, dtype=np.float64), np.asarray(F)
        self.p = dict(DEFAULTS, **params)
        self.Auu = sp.csr_matrix(-(M.cotmatrix(self.V, self.F) if L is None else L))[1:][:, 1:].tocsc()
        self.lu = spla.splu(self.Auu)
        self.W2, self.A, self.area = geometry(self.V, self.F)
        self.state = None

    def lam_min(self):
        return float(spla.eigsh(self.Auu, k=1, sigma=0.0, which="LM", return_eigenvectors=False)[0])

    def solve(self, mu0, mu1, warm=False, n_iter=None, history=False, solve=None, **params):
        """the loop of smg_emd_solve on nV x k masses.  n_iter: run exactly that many iterations and check at the last alone.  history: the bounds
        of every iteration.  solve(r, phi) -> phi replaces the direct solve.  Returns dict(upper, lower, iterations, residual (relative to |b|_2),
        res_abs, potential, J, T, his)."""
        p = dict(self.p, **params)
        V, F, n = self.V, self.F, self.V.shape[0]
        b = np.ascontiguousarray(np.asarray(mu1, dtype=np.float64).reshape(n, -1) - np.asarray(mu0, dtype=np.float64).reshape(n, -1))
        k, nF = b.shape[1], F.shape[0]
        m, rho, nb = column_setup(b, self.area, p["rho_scale"])
        if not (warm and self.state is not None and self.state[0].shape[1] == k):
            self.state = (np.zeros((n, k)), np.zeros((k, nF, 4)))
        phi, ZU = self.state
        max_iter = p["max_iter"] if n_iter is None else n_iter
        upper, lower = np.where(m > 0.0, np.inf, 0.0), np.zeros(k)
        out = dict(upper=upper, lower=lower, iterations=0, residual=np.zeros(k), res_abs=np.zeros(k), potential=np.zeros((n, k)),
                   J=np.zeros((k, nF, 2)), gmax=np.zeros(k), his=[])
        if not np.any(m > 0.0):
            return out
        for t in range(1, max_iter + 1):
            r = rhs(V, F, b, ZU)
            if solve is None:
                phi = np.zeros((n, k))
                phi[1:] = self.lu.solve(r[1:])
            else:
                phi = solve(r, phi)
            check = t == max_iter if n_iter is not None else (t % p["check_every"] == 0 or t == max_iter)
            ZU, J, up, gq, upper, gmax2 = update(V, F, phi, ZU, rho, p["alpha"])
            if check or history:
                pot, _, lower = dual(b, phi, rho, gmax2)
                _, _, dss = residual(V, F, b, J)
                upper, lower = np.where(m > 0.0, upper, 0.0), np.where(m > 0.0, lower, 0.0)
                res = np.sqrt(dss)
                if history:
                    out["his"].append((upper, lower, res, np.linalg.norm(pot, axis=0)))
            if check:
                out.update(upper=upper, lower=lower, iterations=t, res_abs=res, residual=np.where(nb > 0.0, res / np.where(nb > 0.0, nb, 1.0), 0.0),
                           potential=pot, J=J, gmax=np.sqrt(gmax2))
                if n_iter is None and np.all(upper - lower <= p["gap_tol"] * upper):
                    break
        self.state = (phi, ZU)
        out["T"] = ZU[:, :, :2] + ZU[:, :, 2:]
        return out


# ---- the library's side, shared with tests/test_gpu_emd.py -----------------------------------------------------------------------------------------
def out_size(op, nV, nF, k):
    return {EMD_GEOMETRY: 7 * nF + 1, EMD_RHS: nV * k, EMD_UPDATE: 8 * nF * k + 2 * k, EMD_DUAL: 2 * nV * k + k, EMD_FLOW: 3 * nF * k,
            EMD_RESIDUAL: 2 * nV * k + k}.get(op, nV * k)


def unpack(op, out, nV, nF, k):
    """the outputs of an op in the restatement's shapes"""
    nk, fk = nV * k, nF * k
    if op == EMD_GEOMETRY:
        return out[:6 * nF].reshape(nF, 3, 2), out[6 * nF:7 * nF], out[7 * nF]
    if op == EMD_RHS:
        return out.reshape(k, nV).T
    if op == EMD_UPDATE:
        return (out[:4 * fk].reshape(k, nF, 4), out[4 * fk:6 * fk].reshape(k, nF, 2), out[6 * fk:7 * fk].reshape(k, nF), out[7 * fk:8 * fk].reshape(k, nF),
                out[8 * fk:8 * fk + k], out[8 * fk + k:])
    if op == EMD_DUAL:
        return out[:nk].reshape(k, nV).T, out[nk:2 * nk].reshape(k, nV), out[2 * nk:]
    if op == EMD_FLOW:
        return out.reshape(k, nF, 3)
    return out[:nk].reshape(k, nV).T, out[nk:2 * nk].reshape(k, nV), out[2 * nk:]


SENTINEL = -7.25e300


def _call(fn, with_guard, op, V, F, k=1, b=None, phi=None, state=None, rho=None, alpha=1.7, over=None, pad=64):
    """`pad` doubles of sentinel follow the op's extent in `out`: nothing past the extent may be written.  state: ZU (k x nF x 4), a frame field
    (k x nF x 2, FLOW and RESIDUAL) or gmax^2 (k, DUAL)"""
    ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
    nV, nF = V.shape[0], F.shape[0]
    F = np.ascontiguousarray(F, dtype=np.int32)
    rows = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64).reshape(-1)                 # noqa: E731
    cols = lambda a: None if a is None else np.ascontiguousarray(np.asarray(a, dtype=np.float64).T).reshape(-1)   # noqa: E731  (column-major)
    keep = [rows(V), cols(b), cols(phi), rows(state), rows(rho)]
    arr = lambda a, ty=dp: None if a is None else a.ctypes.data_as(ty)   # noqa: E731
    size = out_size(op, nV, nF, max(k, 0))
    out = np.full(size + pad, SENTINEL)
    bad = C.c_int(-1)
    a = dict(nV=nV, nF=nF, k=k, F=arr(F, ip), V=arr(keep[0]), b=arr(keep[1]), phi=arr(keep[2]), state=arr(keep[3]), rho=arr(keep[4]), alpha=float(alpha),
             out=arr(out))
    a.update(over or {})
    args = [op] + [a[key] for key in ("nV", "nF", "k", "F", "V", "b", "phi", "state", "rho", "alpha", "out")]
    rc = fn(*args, C.byref(bad)) if with_guard else fn(*args)
    if rc == 0:
        assert np.all(out[size:] == SENTINEL), "op %d wrote past its extent" % op
        assert not np.any(out[:size] == SENTINEL), "op %d left a part of its extent unwritten" % op
    return rc, bad.value, out[:size]


def host(smg, op, V, F, **kw):
    """one call of smg_emd_host; returns (rc, out)"""
    rc, _, out = _call(smg._lib.load().smg_emd_host, False, op, V, F, **kw)
    return rc, out


def hook(smg, op, V, F, **kw):
    """one call of smg_debug_emd; returns (rc, guard hits, out)"""
    return _call(smg._lib.load().smg_debug_emd, True, op, V, F, **kw)


def check_launchers(run, name, k):
    """every op of `run(op, V, F, **operands) -> out` on one mesh against the restatement, bit for bit; shared by the host twin's and the device's
    tests.  Returns the outputs for a comparison of the two."""
    V, F = shape(name)
    n, nF = V.shape[0], F.shape[0]
    mu0, mu1 = pairs(V, F, k)
    b = np.ascontiguousarray(mu1 - mu0)
    phi, ZU, rho, alpha = test_state(V, F, k)
    ZUn, Jn, upn, gqn, uppern, gmax2n = update(V, F, phi, ZU, rho, alpha)
    outs = [run(EMD_GEOMETRY, V, F, k=1), run(EMD_RHS, V, F, k=k, b=b, state=ZU), run(EMD_UPDATE, V, F, k=k, phi=phi, state=ZU, rho=rho, alpha=alpha),
            run(EMD_DUAL, V, F, k=k, b=b, phi=phi, state=gmax2n, rho=rho), run(EMD_FLOW, V, F, k=k, state=Jn), run(EMD_RESIDUAL, V, F, k=k, b=b, state=Jn)]
    eq = np.array_equal
    W2, A, area = unpack(EMD_GEOMETRY, outs[0], n, nF, 1)
    W2n, An, arean = geometry(V, F)
    assert eq(W2, W2n) and eq(A, An) and area == arean, name
    assert eq(unpack(EMD_RHS, outs[1], n, nF, k), rhs(V, F, b, ZU)), name
    got = unpack(EMD_UPDATE, outs[2], n, nF, k)
    for a, w in zip(got, (ZUn, Jn, upn, gqn, uppern, gmax2n)):
        assert eq(a, w), name
    assert np.any(ZUn[:, :, :2] == 0.0) and np.any(ZUn[:, :, :2] != 0.0), "the state must put faces on both sides of the shrink"
    for a, w in zip(unpack(EMD_DUAL, outs[3], n, nF, k), dual(b, phi, rho, gmax2n)):
        assert eq(a, w), name
    assert eq(unpack(EMD_FLOW, outs[4], n, nF, k), flow(V, F, Jn)), name
    for a, w in zip(unpack(EMD_RESIDUAL, outs[5], n, nF, k), residual(V, F, b, Jn)):
        assert eq(a, w), name
    return outs
