"""CPU: the neo-Hookean membrane time step (include/smg.h: smg_membrane_*) -- the numpy / LAPACK / scipy restatement of the
method that tests/test_gpu_membrane.py checks the device against, its own checks (finite differences, anchors of the reference's
configuration), the ABI and its refusals without a GPU, the contribution lists, and the shared per-face maths compiled for the host.
PARITY UNPINNED: the reference's 06 example needs Eigen and libigl, so nothing here is compared with its binaries.

Per face f with corners q0, q1, q2, e1 = q1 - q0, e2 = q2 - q0:  a = [[e1.e1, e1.e2], [e1.e2, e2.e2]], abar = a of the rest pose,
lnJ = log(det a / det abar) / 2,  W_f = coeff (beta (tr(abar^-1 a) - 2 - 2 lnJ) + alpha lnJ^2),  coeff = h sqrt(det abar) / 4.
With T = beta abar^-1 + t1 a^-1, t1 = -beta + alpha lnJ, and the rows r0, r1 (= r2), r3 of d vec(a) / d (q0, q1, q2):
    G_f = coeff (T00 r0 + 2 T01 r1 + T11 r3)
    H_f = coeff ((alpha / 2 - t1) p p^T + (t1 / det a) (r3 r0^T + r0 r3^T - 2 r1 r1^T) + S (x) I_3),   p = the same combination with a^-1
    S   = 2 T00 [[1,-1,0],[-1,1,0],[0,0,0]] + 2 T01 [[2,-1,-1],[-1,0,1],[-1,1,0]] + 2 T11 [[1,0,-1],[0,0,0],[-1,0,1]]
The per-face eigenvalue fix replaces every eigenvalue below eig_floor by eig_value (numpy.linalg.eigh)."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from oracle import mesh_np as M

DEFAULTS = dict(young=6e6, poisson=0.5, thickness=0.1, mass_scale=1000.0, dt=1e-3, pressure=1e6, newton_iters=10,
                ls_c=1e-8, ls_shrink=0.5, ls_min_alpha=1e-8, eig_floor=1e-6, eig_value=1e-3)

TRIU = np.triu_indices(9)          # the 45 stored entries of H_f, row by row


def fundamental_form(P, F):
    e1, e2 = P[F[:, 1]] - P[F[:, 0]], P[F[:, 2]] - P[F[:, 0]]
    dot = lambda u, v: (u[:, 0] * v[:, 0] + u[:, 1] * v[:, 1]) + u[:, 2] * v[:, 2]   # noqa: E731
    return e1, e2, dot(e1, e1), dot(e1, e2), dot(e2, e2)


def eig_fix(H, floor, value):
    """Q fix(Lambda) Q^T of every 9 x 9 (or 6 x 6) block; returns (fixed blocks, eigenvalues before the fix)"""
    lam, Q = np.linalg.eigh(H)
    lam2 = np.where(lam < floor, value, lam)
    return np.einsum("fij,fj,fkj->fik", Q, lam2, Q), lam


class MembraneNp:
    def __init__(self, V0, F, **params):
        p = dict(DEFAULTS)
        p.update(params)
        self.p = p
        self.V0 = np.ascontiguousarray(V0, dtype=np.float64)
        self.F = np.ascontiguousarray(F, dtype=np.int32)
        self.nV, self.nF = self.V0.shape[0], self.F.shape[0]
        E, nu = p["young"], p["poisson"]
        self.alpha = E * nu / (1.0 - nu * nu)
        self.beta = E / 2.0 / (1.0 + nu)
        _, _, a00, a01, a11 = fundamental_form(self.V0, self.F)
        det = a00 * a11 - a01 * a01
        self.detabar = det
        self.abinv = np.stack([a11 / det, -a01 / det, a00 / det], axis=1)          # (00, 01, 11) of abar^-1
        self.coeff = p["thickness"] * np.sqrt(det) / 4.0
        self.mass0 = M.massmatrix(self.V0, self.F, "voronoi").diagonal()
        self.Md = np.repeat(p["mass_scale"] * self.mass0, 3)
        # the scalar pattern (adjacency + I) (x) 1_{3x3}, from the 9 vertex pairs of every face
        fi = np.repeat(self.F, 3, axis=1).reshape(-1)                                 # corner j of pair (j, k)
        fj = np.tile(self.F, (1, 3)).reshape(-1)                                      # corner k
        self.pair_i, self.pair_j = fi, fj

    # ---- per-face quantities ---------------------------------------------------------------------------------------------------------------
    def faces(self, P, derivs=True, fix=True):
        """W_f; with derivs also G_f (nF x 9), H_f (nF x 9 x 9; fixed when fix) and the eigenvalues of the unfixed H_f"""
        e1, e2, a00, a01, a11 = fundamental_form(P, self.F)
        det = a00 * a11 - a01 * a01
        al, be, bi, co = self.alpha, self.beta, self.abinv, self.coeff
        with np.errstate(invalid="ignore", divide="ignore"):
            lnJ = np.log(det / self.detabar) / 2.0
        tr = (bi[:, 0] * a00 + 2.0 * (bi[:, 1] * a01)) + bi[:, 2] * a11
        W = co * (be * ((tr - 2.0) - 2.0 * lnJ) + al * (lnJ * lnJ))
        W = np.where(det > 0.0, W, np.inf)
        if not derivs:
            return W
        t1 = al * lnJ - be
        ai = np.stack([a11 / det, -a01 / det, a00 / det], axis=1)                    # a^-1
        T = be * bi + t1[:, None] * ai

        def comb(c):                                                                  # c00 r0 + 2 c01 r1 + c11 r3 = 2 [-(u + v), u, v]
            u = 2.0 * (c[:, 0, None] * e1 + c[:, 1, None] * e2)
            v = 2.0 * (c[:, 1, None] * e1 + c[:, 2, None] * e2)
            return np.concatenate([-(u + v), u, v], axis=1)

        G = co[:, None] * comb(T)
        p = comb(ai)
        z = np.zeros_like(e1)
        r0 = np.concatenate([-2.0 * e1, 2.0 * e1, z], axis=1)
        r1 = np.concatenate([-(e1 + e2), e2, e1], axis=1)
        r3 = np.concatenate([-2.0 * e2, z, 2.0 * e2], axis=1)
        outer = lambda x, y: x[:, :, None] * y[:, None, :]   # noqa: E731
        H = (0.5 * al - t1)[:, None, None] * outer(p, p)
        H += (t1 / det)[:, None, None] * ((outer(r3, r0) + outer(r0, r3)) - 2.0 * outer(r1, r1))
        T00, T01, T11 = 2.0 * T[:, 0], 2.0 * T[:, 1], 2.0 * T[:, 2]
        S = np.empty((self.nF, 3, 3))
        S[:, 0, 0] = (T00 + 2.0 * T01) + T11
        S[:, 1, 1], S[:, 2, 2] = T00, T11
        S[:, 0, 1] = S[:, 1, 0] = -(T00 + T01)
        S[:, 0, 2] = S[:, 2, 0] = -(T01 + T11)
        S[:, 1, 2] = S[:, 2, 1] = T01
        H += np.einsum("fjk,lm->fjlkm", S, np.eye(3)).reshape(self.nF, 9, 9)
        H *= co[:, None, None]
        lam = None
        if fix:
            H, lam = eig_fix(H, self.p["eig_floor"], self.p["eig_value"])
        return W, G, H, lam

    # ---- assembly ------------------------------------------------------------------------------------------------------------------------------
    def gradient(self, G):
        g = np.zeros((self.nV, 3))
        for j in range(3):
            np.add.at(g, self.F[:, j], G[:, 3 * j:3 * j + 3])
        return g.reshape(-1)

    def stiffness(self, H):
        """K (3 nV x 3 nV, CSR) from the per-face blocks"""
        rows = (3 * self.F[:, :, None] + np.arange(3)).reshape(self.nF, 9)
        I = np.repeat(rows, 9, axis=1).reshape(-1)
        J = np.tile(rows, (1, 9)).reshape(-1)
        K = sp.coo_matrix((H.reshape(-1), (I, J)), shape=(3 * self.nV, 3 * self.nV)).tocsr()
        K.sum_duplicates()
        K.sort_indices()
        return K

    def system(self, P, qdot, qdot0, fext):
        """(W, H = M + dt^2 K, b, eigenvalues of the unfixed face blocks) at the pose P"""
        dt = self.p["dt"]
        Wf, G, H, lam = self.faces(P)
        K = self.stiffness(H)
        Hm = (sp.diags(self.Md) + (dt * dt) * K).tocsr()
        Hm.sort_indices()
        b = -((self.Md * (qdot - qdot0) + dt * self.gradient(G)) + dt * fext)
        return float(np.sum(Wf)), Hm, b, lam

    def pressure_force(self, P):
        """fExt_v = -pressure m_v(P) n_v(P): Voronoi mass of the CURRENT pose, area-weighted unit vertex normal"""
        m = M.massmatrix(P, self.F, "voronoi").diagonal()
        e1, e2 = P[self.F[:, 1]] - P[self.F[:, 0]], P[self.F[:, 2]] - P[self.F[:, 0]]
        c = np.cross(e1, e2)
        N = np.zeros((self.nV, 3))
        for j in range(3):
            np.add.at(N, self.F[:, j], c)
        N /= np.linalg.norm(N, axis=1, keepdims=True)
        return (-(self.p["pressure"] * m)[:, None] * N).reshape(-1)

    def objective(self, t, qdot0, pos0, fext):
        P = pos0 + self.p["dt"] * t.reshape(-1, 3)
        d = t - qdot0
        return float(np.dot(P.reshape(-1), fext) + 0.5 * np.dot(d, self.Md * d) + np.sum(self.faces(P, derivs=False)))

    # ---- the time step -------------------------------------------------------------------------------------------------------------------------
    def step(self, pos, qdot, newton_iters=None, solve=None, record=None):
        """One implicit-Euler step from (pos, qdot) with direct solves (or solve(H, b)).  Returns (pos, qdot, info); info holds per Newton
        iteration |b|, alpha, W after the iteration, the objective history, and with record=True the iterates and systems."""
        p = self.p
        n_it = p["newton_iters"] if newton_iters is None else newton_iters
        dt = p["dt"]
        pos0, qdot0 = pos.copy(), qdot.copy()
        fext = self.pressure_force(pos)
        info = dict(bnorm=[], alpha=[], W=[], objective=[], neg=[], band=[], poses=[pos.copy()], fext=fext, systems=[])
        for _ in range(n_it):
            W, H, b, lam = self.system(pos, qdot, qdot0, fext)
            info["bnorm"].append(float(np.linalg.norm(b)))
            info["neg"].append(int(np.sum(lam < -1e-6)))
            info["band"].append(int(np.sum((lam >= 1e-8) & (lam <= 1e-4))))
            dx = spla.spsolve(H.tocsc(), b) if solve is None else solve(H, b)
            if record:
                info["systems"].append((H, b, dx))
            f0 = self.objective(qdot, qdot0, pos0, fext)
            info["objective"].append(f0)
            s = f0 + p["ls_c"] * float(np.dot(b, dx))
            alpha, taken = 1.0, 0.0
            while alpha > p["ls_min_alpha"]:
                if self.objective(qdot + alpha * dx, qdot0, pos0, fext) <= s:
                    qdot = qdot + alpha * dx
                    taken = alpha
                    break
                alpha *= p["ls_shrink"]
            info["alpha"].append(taken)
            pos = pos0 + dt * qdot.reshape(-1, 3)
            info["poses"].append(pos.copy())
            info["W"].append(float(np.sum(self.faces(pos, derivs=False))))
        info["objective"].append(self.objective(qdot, qdot0, pos0, fext))
        return pos, qdot, info


def perturbed_pose(V, F, seed=0, amount=0.02):
    """rest + amount sqrt(mean double area) N(0, 1)"""
    s = np.sqrt(np.mean(M.doublearea(V, F)))
    return V + amount * s * np.random.default_rng(seed).standard_normal(V.shape)


def load_mesh(name):
    return M.read_smgm(name)


# ---- the library's side, shared with tests/test_gpu_membrane.py ---------------------------------------------------------------------------------
INVALID, NO_DEVICE = -1, -2
MEM_REST, MEM_FACES_RAW, MEM_FACES, MEM_ENERGY, MEM_PRESSURE, MEM_MATRIX, MEM_GRADIENT, MEM_OBJECTIVE = range(8)


def unpack_upper(Hp):
    """(45, nF) planes of the upper triangle -> (nF, 9, 9) symmetric blocks"""
    H = np.zeros((Hp.shape[1], 9, 9))
    H[:, TRIU[0], TRIU[1]] = Hp.T
    H[:, TRIU[1], TRIU[0]] = Hp.T
    return H


def pack_upper(H):
    return np.ascontiguousarray(H[:, TRIU[0], TRIU[1]].T)


def faces_host(smg, V0, P, F, fix, **params):
    """smg_membrane_faces_host: (W, G as nF x 9, H as nF x 9 x 9)"""
    L = smg._lib.load()
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    V0, P, F = np.ascontiguousarray(V0), np.ascontiguousarray(P), np.ascontiguousarray(F, dtype=np.int32)
    nF = F.shape[0]
    W, G, H = np.zeros(nF), np.zeros((9, nF)), np.zeros((45, nF))
    prm = smg.membrane_params(**params)
    rc = L.smg_membrane_faces_host(V0.ctypes.data_as(dp), P.ctypes.data_as(dp), V0.shape[0], F.ctypes.data_as(ip), nF, C.byref(prm), int(fix),
                                   W.ctypes.data_as(dp), G.ctypes.data_as(dp), H.ctypes.data_as(dp))
    assert rc == 0, L.smg_last_error()
    return W, G.T.copy(), unpack_upper(H)


def lists(smg, F, nV):
    """smg_membrane_lists: (bptr, bcol, c_ptr, c_src)"""
    L = smg._lib.load()
    ip = C.POINTER(C.c_int)
    F = np.ascontiguousarray(F, dtype=np.int32)
    nb, nc = C.c_int(0), C.c_int(0)
    assert L.smg_membrane_lists(F.ctypes.data_as(ip), F.shape[0], nV, C.byref(nb), C.byref(nc), None, None, None, None) == 0
    bptr, bcol = np.zeros(nV + 1, dtype=np.int32), np.zeros(nb.value, dtype=np.int32)
    c_ptr, c_src = np.zeros(nb.value + 1, dtype=np.int32), np.zeros(nc.value, dtype=np.int32)
    assert L.smg_membrane_lists(F.ctypes.data_as(ip), F.shape[0], nV, None, None, bptr.ctypes.data_as(ip), bcol.ctypes.data_as(ip),
                                c_ptr.ctypes.data_as(ip), c_src.ctypes.data_as(ip)) == 0
    return bptr, bcol, c_ptr, c_src


def scalar_pattern(bptr, bcol):
    """(rowptr, col) of the 3 nV x 3 nV matrix in the order k_membrane_matrix writes: row 3 i + l = the blocks of block row i, three columns each"""
    nV = bptr.shape[0] - 1
    cnt = np.diff(bptr)
    rowptr = np.zeros(3 * nV + 1, dtype=np.int64)
    rowptr[1:] = np.cumsum(np.repeat(3 * cnt, 3))
    col = np.empty(9 * bcol.shape[0], dtype=np.int64)
    for i in range(nV):
        c = (3 * bcol[bptr[i]:bptr[i + 1], None] + np.arange(3)).reshape(-1)
        for l in range(3):
            col[rowptr[3 * i + l]:rowptr[3 * i + l + 1]] = c
    return rowptr.astype(np.int32), col.astype(np.int32)


def matrix_values_np(Hp, mass0, lsts, dt, mass_scale):
    """the sum k_membrane_matrix takes, operation by operation: per block the sub-blocks in list order, times dt^2, the mass last"""
    bptr, bcol, c_ptr, c_src = lsts
    nB, nF = bcol.shape[0], Hp.shape[1]
    H = unpack_upper(Hp)
    f, a, b = c_src // 9, (c_src % 9) // 3, c_src % 3
    sub = H[f[:, None, None], (3 * a)[:, None, None] + np.arange(3)[None, :, None], (3 * b)[:, None, None] + np.arange(3)[None, None, :]]
    acc = np.zeros((nB, 3, 3))
    cnt = np.diff(c_ptr)
    for k in range(int(cnt.max())):
        sel = np.nonzero(cnt > k)[0]
        acc[sel] += sub[c_ptr[sel] + k]
    vals = (dt * dt) * acc
    brow = np.repeat(np.arange(bptr.shape[0] - 1), np.diff(bptr))
    dg = np.nonzero(bcol == brow)[0]
    mv = mass_scale * mass0
    for l in range(3):
        vals[dg, l, l] += mv[brow[dg]]
    out = np.empty(9 * nB)
    first, n = bptr[brow], np.diff(bptr)[brow]
    q = np.arange(nB)
    for l in range(3):
        for m in range(3):
            out[9 * first + l * 3 * n + 3 * (q - first) + m] = vals[:, l, m]
    return out


def corner_lists(F, nV):
    """per vertex its corners t = 3 f + j, faces ascending; as slot arrays for sequential sums"""
    t = np.arange(3 * F.shape[0])
    v = F.reshape(-1)
    order = np.argsort(v, kind="stable")
    v, t = v[order], t[order]
    rank = np.arange(t.size) - np.searchsorted(v, np.arange(nV))[v]
    return [(v[rank == k], t[rank == k]) for k in range(int(rank.max()) + 1)]


def hook(smg, op, V0, F, P=None, inp=None, n_out=0, **params):
    """one call of smg_debug_membrane; returns (rc, guard hits, out)"""
    L = smg._lib.load()
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    arr = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64).ctypes.data_as(dp)   # noqa: E731
    F = np.ascontiguousarray(F, dtype=np.int32)
    keep = [None if a is None else np.ascontiguousarray(a, dtype=np.float64) for a in (V0, P, inp)]
    out = np.full(max(n_out, 1), np.nan)
    bad = C.c_int(-1)
    prm = smg.membrane_params(**params)
    nV = (keep[0] if keep[0] is not None else keep[1]).shape[0] if (keep[0] is not None or keep[1] is not None) else int(F.max()) + 1
    rc = L.smg_debug_membrane(op, nV, F.shape[0], F.ctypes.data_as(ip), arr(keep[0]), arr(keep[1]), arr(keep[2]), C.byref(prm),
                              out.ctypes.data_as(dp) if n_out else None, C.byref(bad))
    return rc, bad.value, out


# ---- 1, 2: the restatement against finite differences; symmetry, the fix, positive definiteness ------------------------------------------------
MESHES = ["ogre_sim.smgm", "bunny_15K_init.smgm"]


@pytest.mark.parametrize("name", MESHES)
def test_restatement_against_finite_differences(name):
    """central differences, h = 1e-6 sqrt(mean double area): the bound 1e-6 is the O(h^2) + eps / h error of the quotient with two decades of room"""
    V, F = load_mesh(name)
    mb = MembraneNp(V, F)
    P = perturbed_pose(V, F)
    h = 1e-6 * np.sqrt(np.mean(M.doublearea(V, F)))
    d = np.random.default_rng(1).standard_normal(V.shape)
    _, G, H, _ = mb.faces(P, fix=False)
    g, K = mb.gradient(G), mb.stiffness(H)
    Wp, Wm = np.sum(mb.faces(P + h * d, derivs=False)), np.sum(mb.faces(P - h * d, derivs=False))
    gd = float(g @ d.reshape(-1))
    eW = abs((Wp - Wm) / (2 * h) - gd) / abs(gd)
    gp, gm = mb.gradient(mb.faces(P + h * d, fix=False)[1]), mb.gradient(mb.faces(P - h * d, fix=False)[1])
    Kd = K @ d.reshape(-1)
    eG = np.linalg.norm((gp - gm) / (2 * h) - Kd) / np.linalg.norm(Kd)
    print(name, "dW against g.d %.2e, dg against K d %.2e" % (eW, eG))
    assert eW <= 1e-6 and eG <= 1e-6


@pytest.mark.parametrize("name", MESHES)
def test_face_hessians_fix_and_cholesky(name):
    import scipy.linalg as sla
    V, F = load_mesh(name)
    mb = MembraneNp(V, F)
    P = perturbed_pose(V, F)
    _, _, Hraw, _ = mb.faces(P, fix=False)
    assert np.abs(Hraw - Hraw.transpose(0, 2, 1)).max() <= 1e-12 * np.abs(Hraw).max()
    assert np.abs(Hraw.reshape(-1, 3, 3, 3, 3).sum(axis=3)).max() <= 1e-9 * np.abs(Hraw).max()      # translations are annihilated
    _, _, Hfix, lam = mb.faces(P)
    assert not np.any((lam >= 1e-8) & (lam <= 1e-4))
    assert np.linalg.eigvalsh(Hfix).min() >= mb.p["eig_floor"]
    _, Hm, _, _ = mb.system(P, np.zeros(3 * mb.nV), np.zeros(3 * mb.nV), np.zeros(3 * mb.nV))
    assert abs(Hm - Hm.T).max() <= 1e-12 * abs(Hm).max()
    if name == "ogre_sim.smgm":                                     # dense Cholesky of the 7 836 x 7 836 matrix
        sla.cholesky(Hm.toarray(), lower=True)
    else:                                                           # sparse: the LU of a symmetric positive definite matrix has a positive diagonal
        lu = spla.splu(Hm.tocsc(), permc_spec="MMD_AT_PLUS_A", diag_pivot_thresh=0.0, options=dict(SymmetricMode=True))
        assert np.all(lu.U.diagonal() > 0) and np.array_equal(lu.perm_r, lu.perm_c)


# ---- 3, 4: the restated step, the anchors, the condition of every comparison ---------------------------------------------------------------------
ANCHORS = {   # |b| over Newton iterations 0-3, W after iteration 0, max displacement after the step, (iterations run)
    "ogre_sim.smgm": dict(bnorm=[(50.47, 4), (0.1442, 4), (1.64e-3, 3), (7.6e-5, 2)], W=33.543, disp=1.014e-3, neg=3576, n_eig=45648, iters=10),
    "bunny_15K_init.smgm": dict(bnorm=[(7.852, 4), (1.619, 4), (4.77e-2, 3), (9.2e-3, 2)], W=26.599, disp=1.218e-3, neg=None, n_eig=284436, iters=10),
}


def agrees(x, ref, digits):
    """x rounds to ref at the digits ref is given with (at least 3 where the anchor has them)"""
    return abs(x - ref) <= 0.5 * 10.0 ** (np.floor(np.log10(abs(ref))) - (digits - 1)) * 1.0000001


@pytest.mark.parametrize("name", MESHES)
def test_restated_step_and_anchors(name):
    V, F = load_mesh(name)
    A = ANCHORS[name]
    mb = MembraneNp(V, F)
    pos, qdot, info = mb.step(V.copy(), np.zeros(3 * V.shape[0]), newton_iters=A["iters"])
    obj, alpha = np.array(info["objective"]), np.array(info["alpha"])
    print(name, "|b|", info["bnorm"][:4], "W", info["W"][0], "disp", np.abs(pos - V).max(), "alpha", alpha, "neg", info["neg"], "band", info["band"])
    assert 9 * F.shape[0] == A["n_eig"]
    for k, (ref, digits) in enumerate(A["bnorm"]):
        assert agrees(info["bnorm"][k], ref, digits), (k, info["bnorm"][k], ref)
    assert agrees(info["W"][0], A["W"], 5) and agrees(np.abs(pos - V).max(), A["disp"], 4)
    if A["neg"] is not None:
        assert info["neg"][0] == 0 and all(n == A["neg"] for n in info["neg"][1:])
    else:
        assert np.all(alpha[:4] == 1.0)
    acc = np.nonzero(alpha > 0)[0]
    assert np.all(obj[acc + 1] <= obj[acc])                        # the objective does not increase over accepted steps
    assert np.all(obj[1:] <= obj[:-1])
    assert sum(info["band"]) == 0                                  # no face eigenvalue of any compared pose lies in [1e-8, 1e-4]
    if name == "ogre_sim.smgm":                                    # ... nor in step 1
        _, _, info1 = mb.step(pos, qdot, newton_iters=3)
        assert sum(info1["band"]) == 0


# ---- 5: the ABI without a GPU, the lists, the shared maths on the host, the registers ------------------------------------------------------------
def test_abi_present(smg_mod):
    L = smg_mod._lib.load()
    for name in ("smg_membrane_params_default", "smg_membrane_create", "smg_membrane_destroy", "smg_membrane_device_bytes", "smg_membrane_set_state",
                 "smg_membrane_get_state", "smg_membrane_set_solver", "smg_membrane_step", "smg_membrane_lists", "smg_membrane_faces_host",
                 "smg_debug_membrane"):
        assert hasattr(L, name)
    assert hasattr(smg_mod, "MembraneSim")
    p = smg_mod.membrane_params()
    got = [getattr(p, k) for k, _ in p._fields_]
    assert got == [6e6, 0.5, 0.1, 1000.0, 1e-3, 1e6, 10, 1e-8, 0.5, 1e-8, 1e-6, 1e-3]
    assert L.smg_membrane_device_bytes(None) == 0
    assert L.smg_membrane_set_solver(None, 1) == INVALID
    assert L.smg_membrane_step(None, None, None, None, None, None) == INVALID
    assert L.smg_membrane_get_state(None, None, None, 0) == INVALID and L.smg_membrane_set_state(None, None, None, 0) == INVALID
    assert L.smg_version() >= 507


def _create(smg, h, V, F, nV=None, **params):
    L = smg._lib.load()
    out = C.c_void_p(1)
    V = np.ascontiguousarray(V, dtype=np.float64)
    F = np.ascontiguousarray(F, dtype=np.int32)
    prm = smg.membrane_params(**params)
    rc = L.smg_membrane_create(h, V.ctypes.data_as(C.POINTER(C.c_double)), V.shape[0] if nV is None else nV, F.ctypes.data_as(C.POINTER(C.c_int)),
                               F.shape[0], C.byref(prm), C.byref(out))
    if rc == 0:
        L.smg_membrane_destroy(out)
    else:
        assert out.value is None, "a refused create must leave *out == NULL"
        assert len(L.smg_last_error()) > 0
    return rc


def _fake_block_hierarchy(smg, n):
    """a 2-level block handle whose level 0 has 3 n rows: the create checks read nothing else of it"""
    H = smg.Hierarchy(2)
    H.set_prolong(1, sp.kron(sp.csr_matrix(np.ones((n, 1))), sp.identity(3)).tocsr())
    return H


def test_create_refusals(smg_mod):
    from test_geodesics_host import icosphere
    smg = smg_mod
    L = smg._lib.load()
    V, F = icosphere(3)
    n = V.shape[0]
    blk = smg.mg_precompute_block(V, F, 0.25, 50, 1)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    out = C.c_void_p()
    prm = smg.membrane_params()
    assert _create(smg, None, V, F) == INVALID                                        # null arguments
    assert L.smg_membrane_create(blk.h, None, n, F.ctypes.data_as(ip), F.shape[0], C.byref(prm), C.byref(out)) == INVALID
    assert L.smg_membrane_create(blk.h, V.ctypes.data_as(dp), n, None, F.shape[0], C.byref(prm), C.byref(out)) == INVALID
    assert L.smg_membrane_create(blk.h, V.ctypes.data_as(dp), n, F.ctypes.data_as(ip), F.shape[0], None, C.byref(out)) == INVALID
    assert L.smg_membrane_create(blk.h, V.ctypes.data_as(dp), n, F.ctypes.data_as(ip), F.shape[0], C.byref(prm), None) == INVALID
    mg = smg.mg_precompute(V, F, 0.25, 50, 1)                                         # a scalar hierarchy, with and without the row match
    assert _create(smg, mg.h, V, F) == INVALID
    assert _create(smg, mg.h, V[:n // 3 * 3 // 3], F) == INVALID
    un = smg.Hierarchy.union([mg, mg])                                                # a union handle
    V2, F2 = np.concatenate([V, V + 3.0]), np.concatenate([F, F + n])
    assert _create(smg, un.h, V2, F2) == INVALID
    assert _create(smg, blk.h, V[:-1], F, nV=n - 1) == INVALID                        # 3 nV != rows of level 0
    two = _fake_block_hierarchy(smg, 2 * n)                                           # two connected components
    assert _create(smg, two.h, V2, F2) == INVALID
    fake = _fake_block_hierarchy(smg, n)
    Vz = V.copy()
    Vz[F[0, 1]] = Vz[F[0, 0]]                                                         # a face with zero double area
    assert _create(smg, fake.h, Vz, F) == INVALID
    Fo = F.copy()
    Fo[3, 2] = n                                                                      # a face index out of range
    assert _create(smg, fake.h, V, Fo) == INVALID
    for bad in (np.nan, np.inf):                                                      # a non-finite coordinate
        Vn = V.copy()
        Vn[n - 1, 1] = bad
        assert _create(smg, fake.h, Vn, F) == INVALID
    for bad in (dict(dt=0.0), dict(dt=-1e-3), dict(poisson=1.0), dict(poisson=-1.5), dict(young=0.0), dict(thickness=0.0), dict(mass_scale=-1.0),
                dict(newton_iters=-1), dict(eig_value=0.0), dict(dt=float("nan"))):
        assert _create(smg, blk.h, V, F, **bad) == INVALID, bad
    if L.smg_device_count() == 0:
        assert _create(smg, blk.h, V, F) == NO_DEVICE                                 # valid arguments: the device is what is missing
        assert _create(smg, fake.h, V, F, newton_iters=0) == NO_DEVICE


def test_hook_refusals(smg_mod):
    from test_geodesics_host import icosphere
    V, F = icosphere(1)
    n, nF = V.shape[0], F.shape[0]
    P = V * 1.1
    assert hook(smg_mod, 8, V, F, P, None, 5 * nF)[0] == INVALID                       # unknown op
    assert hook(smg_mod, -1, V, F, P, None, 5 * nF)[0] == INVALID
    assert hook(smg_mod, MEM_FACES, V, F, None, None, 55 * nF)[0] == INVALID           # the pose missing
    assert hook(smg_mod, MEM_REST, None, F, P, None, 5 * nF)[0] == INVALID             # the rest pose missing
    assert hook(smg_mod, MEM_MATRIX, V, F, P, None, 9 * n)[0] == INVALID               # the input missing
    assert hook(smg_mod, MEM_REST, V, F, P, None, 0)[0] == INVALID                     # out missing
    Fo = F.copy()
    Fo[2, 1] = n
    assert hook(smg_mod, MEM_REST, V, Fo, P, None, 5 * nF)[0] == INVALID
    if smg_mod._lib.load().smg_device_count() == 0:
        assert hook(smg_mod, MEM_REST, V, F, P, None, 5 * nF)[0] == NO_DEVICE
        assert hook(smg_mod, MEM_FACES, V, F, P, None, 55 * nF)[0] == NO_DEVICE


@pytest.mark.parametrize("name", MESHES)
def test_contribution_lists(smg_mod, name):
    V, F = load_mesh(name)
    nV, nF = V.shape[0], F.shape[0]
    bptr, bcol, c_ptr, c_src = lists(smg_mod, F, nV)
    nB = bcol.shape[0]
    assert bptr[0] == 0 and bptr[-1] == nB and c_ptr[0] == 0 and c_ptr[-1] == 9 * nF and np.all(np.diff(c_ptr) >= 1)
    assert np.array_equal(np.sort(c_src), np.arange(9 * nF))                          # every face corner pair appears exactly once
    brow = np.repeat(np.arange(nV), np.diff(bptr))
    blk = np.repeat(np.arange(nB), np.diff(c_ptr))
    f, a, b = c_src // 9, (c_src % 9) // 3, c_src % 3
    assert np.array_equal(F[f, a], brow[blk]) and np.array_equal(F[f, b], bcol[blk])     # ... in the block of its vertex pair
    inner = np.ones(9 * nF, dtype=bool)
    inner[c_ptr[:-1]] = False
    assert np.all(np.diff(f)[inner[1:]] > 0)                                          # faces ascending within a block
    key = brow.astype(np.int64) * nV + bcol
    assert np.all(np.diff(key) > 0)                                                   # block columns ascending, no block twice
    A = sp.coo_matrix((np.ones(9 * nF), (F[f, a], F[f, b])), shape=(nV, nV)).tocsr()
    A.sort_indices()
    assert np.array_equal(A.indptr, bptr) and np.array_equal(A.indices, bcol)         # the pattern is adjacency + I
    rowptr, col = scalar_pattern(bptr, bcol)
    K = MembraneNp(V, F).stiffness(np.ones((nF, 9, 9)))
    assert np.array_equal(K.indptr, rowptr) and np.array_equal(K.indices, col)        # and its scalar form is the CSR of K, sorted


@pytest.mark.parametrize("name", MESHES)
def test_shared_maths_on_the_host(smg_mod, name):
    """smg_membrane_inl.hpp compiled for the host against the restatement: W, G, the unfixed H to rounding; the 6 x 6 Jacobi fix against LAPACK's
    Q fix(Lambda) Q^T of the SAME unfixed blocks.  Scale: coeff beta |a|, the size of the terms that are summed."""
    V, F = load_mesh(name)
    mb = MembraneNp(V, F)
    for pose in (V, perturbed_pose(V, F), mb.step(V.copy(), np.zeros(3 * V.shape[0]), newton_iters=2)[2]["poses"][2]):
        W, G, H, _ = mb.faces(pose, fix=False)
        Wl, Gl, Hl = faces_host(smg_mod, V, pose, F, 0)
        _, _, a00, _, a11 = fundamental_form(pose, F)
        scale = mb.coeff * mb.beta * (a00 + a11) / np.sqrt(mb.detabar)
        eW, eG = np.abs(Wl - W).max() / scale.max(), (np.abs(Gl - G).max(axis=1) / (scale / np.sqrt(a00 + a11))).max()
        eH = (np.abs(Hl - H).max(axis=(1, 2)) / (scale / (a00 + a11))).max()
        ref, lam = eig_fix(Hl, mb.p["eig_floor"], mb.p["eig_value"])
        _, _, Hf = faces_host(smg_mod, V, pose, F, 1)
        eF = (np.linalg.norm(Hf - ref, axis=(1, 2)) / np.linalg.norm(ref, axis=(1, 2))).max()
        lmin = np.linalg.eigvalsh(Hf).min()
        print(name, "W %.2e G %.2e H %.2e fix %.2e lambda_min %.3e" % (eW, eG, eH, eF, lmin))
        assert not np.any((lam >= 1e-8) & (lam <= 1e-4))
        assert eW <= 1e-12 and eG <= 1e-11 and eH <= 1e-11             # rounding of ~20 operations on terms of that size, lnJ cancelling at the rest pose
        assert eF <= 1e-12 and lmin >= mb.p["eig_floor"] * (1 - 1e-9)


def test_faces_kernel_keeps_everything_in_registers():
    """the ISA notes of k_membrane_faces with the fix (the build's flags, device side only): no scratch, no spills, 3 waves per SIMD"""
    import os
    import re
    import subprocess
    from surface_multigrid_code_amd import build as B
    src = os.path.join(B.CSRC, "smg_membrane_device.hip")
    asm = subprocess.check_output([B._hipcc()] + B.FLAGS + ["--cuda-device-only", "-S", src, "-o", "-"], text=True)
    for mode, cap in ((0, 64), (2, 168)):
        notes = re.findall(r"\.name:\s+(\S*k_membrane_facesILi%dE\S*)(.*?)\.wavefront_size" % mode, asm, flags=re.S)
        assert len(notes) == 1
        body = notes[0][1]
        field = lambda k: int(re.search(r"\.%s:\s+(\d+)" % k, body).group(1))   # noqa: E731
        print("k_membrane_faces<%d>: vgpr_count %d, private_segment_fixed_size %d, vgpr_spill_count %d"
              % (mode, field("vgpr_count"), field("private_segment_fixed_size"), field("vgpr_spill_count")))
        assert field("private_segment_fixed_size") == 0 and field("vgpr_spill_count") == 0
        assert field("vgpr_count") <= cap      # 512 / 168 = 3 waves per SIMD with the fix (154), 8 for the energy alone (45)


def test_example_compiles():
    """examples/06_balloon_sim.cpp against the C++ mirror: syntax check with the host compiler (as the adapter's)"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = os.path.join(root, "examples", "06_balloon_sim.cpp")
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + os.path.join(root, "include"),
                           "-I" + os.path.join(root, "surface_multigrid_code_amd", "csrc"), src])
