"""The numpy restatement of the StVK and tension-field StVK membrane materials (include/smg.h: smg_membrane_set_material),
shared by tests/test_membrane_materials_host.py and tests/test_gpu_membrane_materials.py, and the ctypes wrappers of the entry points that take
a material.

The restatement follows the reference's StVKMaterial.cpp:11-60 and TensionFieldStVKMaterial.cpp:11-171 TERM BY TERM: the 4 x 9 derivative of
vec(a) (rows r0, r1, r1, r3), its four constant 9 x 9 second derivatives, the 2 x 2 matrices M = abar^-1 (a - abar), temp, Mainv, mat, inner, and
every `*hessian +=` as one numpy statement.  The library instead builds both materials from d psi / d a and a 6-entry table of second
derivatives with one shared tail (csrc/smg_membrane_inl.hpp), so the two derivations check each other.

Beside each sum the restatement records the largest magnitude among the terms that enter it (per face): the scale the comparisons of W, G and
the unfixed H are relative to.  For a wrinkled face that includes the 1 / denom^3 term."""
import ctypes as C

import numpy as np

from test_membrane_host import MembraneNp, eig_fix, fundamental_form, unpack_upper

NEO_HOOKEAN, STVK, TENSION_FIELD = 0, 1, 2
MATERIAL_NAMES = {STVK: "stvk", TENSION_FIELD: "tension_field"}
PURE, SLACK, WRINKLED = 0, 1, 2

I3 = np.eye(3)
# the second derivatives of a00, a01, a10, a11 with respect to (q0, q1, q2)
AHESS = np.stack([np.kron(np.array(S, dtype=np.float64), I3) for S in (
    [[2, -2, 0], [-2, 2, 0], [0, 0, 0]],
    [[2, -1, -1], [-1, 0, 1], [-1, 1, 0]],
    [[2, -1, -1], [-1, 0, 1], [-1, 1, 0]],
    [[2, 0, -2], [0, 0, 0], [-2, 0, 2]])])


def outer(x, y):
    return x[:, :, None] * y[:, None, :]


class Sum:
    """a running sum of per-face terms and the largest magnitude among them"""

    def __init__(self, shape):
        self.total = np.zeros(shape)
        self.scale = np.zeros(shape[0])

    def add(self, term):
        self.total = self.total + term
        self.scale = np.maximum(self.scale, np.abs(term).reshape(term.shape[0], -1).max(axis=1))

    def times(self, factor):
        f = factor.reshape((-1,) + (1,) * (self.total.ndim - 1))
        self.total = self.total * f
        self.scale = self.scale * np.abs(factor)


class MaterialNp(MembraneNp):
    """MembraneNp with the faces of StVK (material 1) or tension-field StVK (material 2)"""

    def __init__(self, V0, F, material, **params):
        super().__init__(V0, F, **params)
        assert material in (STVK, TENSION_FIELD)
        self.material = material
        _, _, self.ab00, self.ab01, self.ab11 = fundamental_form(self.V0, self.F)
        self.last = None

    # ---- the pieces both materials share -------------------------------------------------------------------------------------------------------
    def _forms(self, P):
        e1, e2, a00, a01, a11 = fundamental_form(P, self.F)
        z = np.zeros_like(e1)
        r0 = np.concatenate([-2.0 * e1, 2.0 * e1, z], axis=1)
        r1 = np.concatenate([-(e1 + e2), e2, e1], axis=1)
        r3 = np.concatenate([-2.0 * e2, z, 2.0 * e2], axis=1)
        aderiv = [r0, r1, r1, r3]                                              # rows of d vec(a) (a00, a10, a01, a11: column-major)
        bi = {(0, 0): self.abinv[:, 0], (0, 1): self.abinv[:, 1], (1, 0): self.abinv[:, 1], (1, 1): self.abinv[:, 2]}
        d = {(0, 0): a00 - self.ab00, (0, 1): a01 - self.ab01, (1, 0): a01 - self.ab01, (1, 1): a11 - self.ab11}       # a - abar
        Mm = {(i, j): bi[i, 0] * d[0, j] + bi[i, 1] * d[1, j] for i in range(2) for j in range(2)}                       # abar^-1 (a - abar)
        return aderiv, bi, d, Mm

    VEC = [(0, 0), (1, 0), (0, 1), (1, 1)]                                    # Eigen's column-major order of a 2 x 2 as a 4-vector

    def _stvk(self, aderiv, bi, Mm, derivs):
        al, be = self.alpha, self.beta
        coeff = self.p["thickness"] / 4.0
        dA = 0.5 * np.sqrt(self.detabar)
        trM = Mm[0, 0] + Mm[1, 1]
        MM = [Mm[0, 0] * Mm[0, 0], Mm[0, 1] * Mm[1, 0], Mm[1, 0] * Mm[0, 1], Mm[1, 1] * Mm[1, 1]]                            # the terms of tr(M M)
        W = Sum((self.nF,))
        W.add(0.5 * al * trM ** 2)
        for t in MM:
            W.add(be * t)
        W.times(coeff * dA)
        if not derivs:
            return W, None, None
        Mainv = {(i, j): Mm[i, 0] * bi[0, j] + Mm[i, 1] * bi[1, j] for i in range(2) for j in range(2)}
        temp = {ij: al * trM * bi[ij] + 2.0 * be * Mainv[ij] for ij in bi}
        G = Sum((self.nF, 9))
        for row, ij in zip(aderiv, self.VEC):
            G.add(temp[ij][:, None] * row)
        G.times(coeff * dA)
        H = Sum((self.nF, 9, 9))
        inner = sum(bi[ij][:, None] * row for row, ij in zip(aderiv, self.VEC))
        H.add(al * outer(inner, inner))
        for k, ij in enumerate(self.VEC):
            H.add((al * trM * bi[ij] + 2.0 * be * Mainv[ij])[:, None, None] * AHESS[k][None])
        inner00 = bi[0, 0][:, None] * aderiv[0] + bi[0, 1][:, None] * aderiv[2]
        inner01 = bi[0, 0][:, None] * aderiv[1] + bi[0, 1][:, None] * aderiv[3]
        inner10 = bi[1, 0][:, None] * aderiv[0] + bi[1, 1][:, None] * aderiv[2]
        inner11 = bi[1, 0][:, None] * aderiv[1] + bi[1, 1][:, None] * aderiv[3]
        H.add(2.0 * be * outer(inner00, inner00))
        H.add(2.0 * be * (outer(inner01, inner10) + outer(inner10, inner01)))
        H.add(2.0 * be * outer(inner11, inner11))
        H.times(coeff * dA)
        return W, G, H

    def branches(self, P):
        """per face: (branch, lambda1, lambda2, denom, transition) of the tension-field test"""
        _, _, _, Mm = self._forms(P)
        return self._branches(Mm)

    def _branches(self, Mm):
        al, be = self.alpha, self.beta
        coeff = self.p["thickness"] / 4.0
        T = Mm[0, 0] + Mm[1, 1]
        D = Mm[0, 0] * Mm[1, 1] - Mm[0, 1] * Mm[1, 0]
        root = np.sqrt(np.maximum(0.0, T * T / 4.0 - D))
        l1, l2 = T / 2.0 + root, T / 2.0 - root
        swap = l2 > l1
        l1, l2 = np.where(swap, l2, l1), np.where(swap, l1, l2)
        sign = np.where(swap, -1.0, 1.0)
        k1, k2 = 0.5 * coeff * al, coeff * be
        trans = -k1 / (k1 + k2)
        pure = (l1 >= 0) & (l2 >= trans * l1)
        branch = np.where(pure, PURE, np.where(l1 < 0, SLACK, WRINKLED))
        with np.errstate(invalid="ignore"):
            denom = np.sqrt(T * T / 4.0 - D)
        return branch, l1, l2, denom, trans, sign, T, k1, k2

    def margins_ok(self, P, rel=1e-6):
        """no face within a relative `rel` of a branch boundary: |l1|, |l2 - transition l1| and denom all >= rel max(|l1|, |l2|)"""
        _, l1, l2, denom, trans, *_ = self.branches(P)
        s = np.maximum(np.abs(l1), np.abs(l2))
        with np.errstate(invalid="ignore"):
            ok = (np.abs(l1) >= rel * s) & (np.abs(l2 - trans * l1) >= rel * s) & ((denom >= rel * s) | (s == 0.0))
        return bool(np.all(ok)), float(np.min(np.where(s > 0, denom / np.where(s > 0, s, 1.0), np.inf)))

    def _wrinkled(self, aderiv, bi, d, br, derivs):
        _, l1, _, denom, _, sign, T, k1, k2 = br
        dA = 0.5 * np.sqrt(self.detabar)
        detAbarinv = bi[0, 0] * bi[1, 1] - bi[0, 1] * bi[1, 0]
        lam = l1
        ks = k1 + k2 - k1 * k1 / (k1 + k2)
        W = Sum((self.nF,))
        W.add(ks * dA * lam * lam)
        if not derivs:
            return W, None, None
        adj = {(0, 0): d[1, 1], (1, 1): d[0, 0], (0, 1): -d[1, 0], (1, 0): -d[0, 1]}
        with np.errstate(invalid="ignore", divide="ignore"):
            inner = {ij: T / 4.0 * bi[ij] - 1.0 / 2.0 * detAbarinv * adj[ij] for ij in bi}
            mat = {ij: 0.5 * bi[ij] + sign / denom * inner[ij] for ij in bi}
            K2 = 2.0 * ks * dA
            G = Sum((self.nF, 9))
            for row, ij in zip(aderiv, [(0, 0), (0, 1), (1, 0), (1, 1)]):
                G.add((K2 * lam * mat[ij])[:, None] * row)
            H = Sum((self.nF, 9, 9))
            rankone = sum(mat[ij][:, None] * row for row, ij in zip(aderiv, [(0, 0), (0, 1), (1, 0), (1, 1)]))
            H.add(K2[:, None, None] * outer(rankone, rankone))
            for k, ij in enumerate([(0, 0), (0, 1), (1, 0), (1, 1)]):
                H.add((K2 * lam * mat[ij])[:, None, None] * AHESS[k][None])
            f = K2 * sign * lam / denom * (-1.0 / 2.0 * detAbarinv)
            H.add(f[:, None, None] * outer(aderiv[3], aderiv[0]))
            H.add((f * -1)[:, None, None] * outer(aderiv[2], aderiv[1]))
            H.add((f * -1)[:, None, None] * outer(aderiv[1], aderiv[2]))
            H.add(f[:, None, None] * outer(aderiv[0], aderiv[3]))
            abarinvterm = sum(bi[ij][:, None] * row for row, ij in zip(aderiv, [(0, 0), (0, 1), (1, 0), (1, 1)]))
            H.add((K2 * sign * lam / denom / 4.0)[:, None, None] * outer(abarinvterm, abarinvterm))
            innerVec = sum(inner[ij][:, None] * row for row, ij in zip(aderiv, [(0, 0), (0, 1), (1, 0), (1, 1)]))
            H.add((2.0 * ks * -dA * sign * lam / denom / denom / denom)[:, None, None] * outer(innerVec, innerVec))
        return W, G, H

    # ---- MembraneNp's interface ----------------------------------------------------------------------------------------------------------------
    def faces(self, P, derivs=True, fix=True):
        """as MembraneNp.faces; self.last keeps the branch per face and the scales of the sums of W, G and the unfixed H"""
        aderiv, bi, d, Mm = self._forms(P)
        W, G, H = self._stvk(aderiv, bi, Mm, derivs)
        branch = np.zeros(self.nF, dtype=np.int64)
        if self.material == TENSION_FIELD:
            br = self._branches(Mm)
            branch = br[0]
            Ww, Gw, Hw = self._wrinkled(aderiv, bi, d, br, derivs)
            for S, Sw in ((W, Ww), (G, Gw), (H, Hw)):
                if S is None:
                    continue
                sel = branch.reshape((-1,) + (1,) * (S.total.ndim - 1))
                S.total = np.where(sel == PURE, S.total, np.where(sel == SLACK, 0.0, Sw.total))
                S.scale = np.where(branch == PURE, S.scale, np.where(branch == SLACK, 0.0, Sw.scale))
        if not derivs:
            return W.total
        self.last = dict(branch=branch, scW=W.scale, scG=G.scale, scH=H.scale)
        Hm, lam = H.total, None
        if fix:
            Hm, lam = eig_fix(Hm, self.p["eig_floor"], self.p["eig_value"])
        return W.total, G.total, Hm, lam

    def candidates(self, P):
        """the unfixed H of every face by the pure-tension (StVK) formula and by the wrinkled formula, whatever branch the face is in (entries of
        the wrinkled one are not finite where denom is 0 or not a number)"""
        aderiv, bi, d, Mm = self._forms(P)
        Hp = self._stvk(aderiv, bi, Mm, True)[2]
        Hw = self._wrinkled(aderiv, bi, d, self._branches(Mm), True)[2]
        return Hp.total, Hw.total

    def faces_detail(self, P):
        """(W, G, unfixed H, branch, scale of W, of G, of H)"""
        W, G, H, _ = self.faces(P, fix=False)
        L = self.last
        return W, G, H, L["branch"], L["scW"], L["scG"], L["scH"]


def relative_errors(got, ref, scale):
    """max over the faces of |got - ref| / scale, faces whose scale is 0 (every term is 0) must agree exactly"""
    diff = np.abs(got - ref).reshape(ref.shape[0], -1).max(axis=1)
    zero = scale == 0.0
    assert not np.any(diff[zero] != 0.0), "a face all of whose terms are 0 differs"
    return float((diff[~zero] / scale[~zero]).max()) if np.any(~zero) else 0.0


def infer_branch(mb, P, W, H, scale):
    """the branch every face of a tension-field output (W, unfixed H) took: slack where W == 0 and H == 0 exactly; else the one of the
    restatement's two formulas (MaterialNp.candidates) that H is nearer to, per face relative to `scale`.  Returns (branch, the distance to the
    nearer formula, the distance to the other one)."""
    Hp, Hw = mb.candidates(P)
    with np.errstate(invalid="ignore", divide="ignore"):
        sc = np.where(scale > 0, scale, 1.0)
        dp = np.abs(H - Hp).reshape(H.shape[0], -1).max(axis=1) / sc
        dw = np.abs(H - Hw).reshape(H.shape[0], -1).max(axis=1) / sc
    dw = np.where(np.isfinite(dw), dw, np.inf)
    slack = (W == 0.0) & (np.abs(H).reshape(H.shape[0], -1).max(axis=1) == 0.0)
    branch = np.where(slack, SLACK, np.where(dp <= dw, PURE, WRINKLED))
    return branch, np.where(slack, 0.0, np.minimum(dp, dw)), np.where(slack, np.inf, np.maximum(dp, dw))


# ---- hand-made meshes whose poses send consecutive faces through the three branches (chosen on the CPU: MaterialNp.margins_ok holds) ----------------
FAN_A, FAN_B = (1.42, 0.70, 0.67), (1.02, 0.82, 0.90)


def strip_mesh(n):
    """a zig-zag strip of n faces over n + 2 vertices"""
    k = np.arange(n + 2)
    V = np.stack([0.5 * k, (k % 2).astype(float), 0.05 * np.sin(0.9 * k)], axis=1)
    F = np.array([[i, i + 1, i + 2] if i % 2 == 0 else [i + 1, i, i + 2] for i in range(n)], dtype=np.int32)
    return V, F


def strip_pose(V, a=(0.67, 1.16, 1.41), b=(0.93, 0.91, 0.84)):
    """the spacing along the strip and its width scaled with period 3 in the vertex index: faces cycle slack, pure, wrinkled"""
    k = np.arange(V.shape[0])
    x = np.concatenate([[0.0], np.cumsum(0.5 * np.asarray(a)[k[:-1] % 3])])
    return np.stack([x, V[:, 1] * np.asarray(b)[k % 3], V[:, 2] * 1.1 + 0.02 * np.cos(1.3 * k)], axis=1)


def fan_mesh(n):
    """n faces around vertex 0; the rim winds three times around it (rising), so that 65 faces are not 65 slivers: a sliver's large abar^-1 would
    lift the rounding of the null eigenvalues of H_f, |H_f| eps, into the band [1e-8, 1e-4] that the comparison of fixed blocks keeps empty"""
    k = np.arange(n + 1)
    th = 6 * np.pi * k / (n + 5)
    V = np.concatenate([[[0, 0, 0.3]], np.stack([np.cos(th), np.sin(th), 0.01 * k], axis=1)])
    F = np.array([[0, i + 1, i + 2] for i in range(n)], dtype=np.int32)
    return V, F


def fan_pose(V, a=FAN_A, b=FAN_B):
    """the angles between the spokes and their lengths scaled with period 3: consecutive faces are in three different branches"""
    n = V.shape[0] - 1
    k = np.arange(n)
    th0 = 6 * np.pi / (n + 4)
    th = np.concatenate([[0.0], np.cumsum(th0 * np.asarray(a)[k[:-1] % 3])])
    r = np.asarray(b)[k % 3]
    return np.concatenate([[[0, 0, 0.25]], np.stack([r * np.cos(th), r * np.sin(th), 0.011 * k + 0.03 * np.sin(2.0 * k)], axis=1)])


# ---- the library's side ---------------------------------------------------------------------------------------------------------------------------
def faces_host_material(smg, V0, P, F, material, fix, derivs=True, **params):
    """smg_membrane_faces_host_material: (W, G as nF x 9, H as nF x 9 x 9); derivs=False: W alone"""
    L = smg._lib.load()
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    V0, P, F = np.ascontiguousarray(V0, dtype=np.float64), np.ascontiguousarray(P, dtype=np.float64), np.ascontiguousarray(F, dtype=np.int32)
    nF = F.shape[0]
    W, G, H = np.zeros(nF), np.zeros((9, nF)), np.zeros((45, nF))
    prm = smg.membrane_params(**params)
    rc = L.smg_membrane_faces_host_material(V0.ctypes.data_as(dp), P.ctypes.data_as(dp), V0.shape[0], F.ctypes.data_as(ip), nF, C.byref(prm), int(material),
                                            int(fix), W.ctypes.data_as(dp), G.ctypes.data_as(dp) if derivs else None, H.ctypes.data_as(dp) if derivs else None)
    assert rc == 0, L.smg_last_error()
    return (W, G.T.copy(), unpack_upper(H)) if derivs else W


def hook_material(smg, material, op, V0, F, P=None, inp=None, n_out=0, **params):
    """one call of smg_debug_membrane_material; returns (rc, guard hits, out)"""
    L = smg._lib.load()
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    arr = lambda a: None if a is None else a.ctypes.data_as(dp)   # noqa: E731
    F = np.ascontiguousarray(F, dtype=np.int32)
    keep = [None if a is None else np.ascontiguousarray(a, dtype=np.float64) for a in (V0, P, inp)]
    out = np.full(max(n_out, 1), np.nan)
    bad = C.c_int(-1)
    prm = smg.membrane_params(**params)
    nV = (keep[0] if keep[0] is not None else keep[1]).shape[0] if (keep[0] is not None or keep[1] is not None) else int(F.max()) + 1
    rc = L.smg_debug_membrane_material(int(material), op, nV, F.shape[0], F.ctypes.data_as(ip), arr(keep[0]), arr(keep[1]), arr(keep[2]), C.byref(prm),
                                       out.ctypes.data_as(dp) if n_out else None, C.byref(bad))
    return rc, bad.value, out
