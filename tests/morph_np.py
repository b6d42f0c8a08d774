"""The numpy / scipy restatement of gradient-domain morphing (include/smg.h: smg_morph_*), in the kernels' operation order, with LAPACK SVDs for the
polar factors and direct solves for the Poisson systems; the ctypes wrappers of smg_morph_faces_host and smg_debug_morph.

    J_f = T_f + N_f n_f^T,  T_f = sum_i x_i W_fi^T;   J_f = R_f S_f;   omega_f = log R_f;   J_f(t) = exp(t omega_f) (I + t (S_f - I));
    (-L U)_i = sum over the corners (f, j) of vertex i, faces ascending, of A_f J_f W_fj, the pinned rows known

Sums over a corner list run in list order, one slot of every vertex at a time, so the floating-point order is the kernels'.  Everything but the
SVD, sin, cos and atan2 is correctly rounded +, -, *, / and sqrt in one order on both sides.

Deformation transfer from an affine source.  The source's rest pose is S0 = V A^T + a and its pose is S1 = S0 B^T + b.  A source face has the
unit normal n_s (a function of A and the target's normal n_t) and the pose face the unit normal N = cof(B) n_s / |cof(B) n_s|, so
J_f = B (I - n_s n_s^T) + N n_s^T: B on the source face's plane.  The target sees J_f on ITS face's plane.  When A = s I (a uniform scale and a
translation) the two planes are parallel, J_f w = B w for every tangent w of the target face, the field is the gradient of V B^T and the transfer
returns V B^T moved so that the pins stay: exact_transfer() below.  For a general A the planes differ from face to face, the field J_f restricted
to the target's planes is not a gradient, and the result is the least-squares fit the direct solve gives (transfer() below): the tests hold
the device to that value and check the closed form only where it exists."""
import ctypes as C
import functools

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from oracle import mesh_np as M
from pd_np import EPS, corner_lists, fixed_sum  # noqa: F401  (shared with the tests)
from test_arap_host import ArapNp, roll_onto_cylinder, rotation_matrix, rotations_np, twist
from test_geodesics_host import flat_square, icosphere

MORPH_FACE_GRADIENT, MORPH_FACE_POLAR, MORPH_RHS_GRADIENT, MORPH_RHS_INTERP, MORPH_PINS = range(5)
CASES = [("icosphere1", "stretch"), ("icosphere3", "twist"), ("torus", "stretch"), ("bunny.smgm", "twist"), ("square", "roll")]   # (mesh, pose)
SET_COUNTS = (1, 2, 5)                                 # 3, 6 and 15 columns: the raw, the padded-to-8 and the padded-to-16 widths of the solve
TIMES = (0.25, 0.5, 1.5, 0.0, 1.0)                     # the first k of them are a case's times


# ---- meshes and poses --------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def shape(name):
    """(V, F) of a test mesh; computed once and left unchanged by its users.  torus: smg_mesh_torus at 24 x 12, built by the library's host code"""
    if name.startswith("icosphere"):
        V, F = icosphere(int(name[len("icosphere"):]))
    elif name == "torus":
        from surface_multigrid_code_amd import mesh
        V, F = mesh.torus(24, 12)
    elif name == "square":
        V, F = flat_square(12)
    else:
        V, F = M.read_smgm(name)
        V = M.normalize_unit_area(V, F)
    V, F = np.ascontiguousarray(V, dtype=np.float64), np.ascontiguousarray(F, dtype=np.int32)
    V.setflags(write=False)
    F.setflags(write=False)
    return V, F


@functools.lru_cache(maxsize=None)
def pose(name, kind):
    """the pose of a case: "twist" = three iterations of the ARAP restatement under test_arap_host.twist's handles (60 degrees and a shift),
    "stretch" = diag(1.5, 0.7, 1.2) after a rotation of 2 radians about (1, 2, -0.5), "roll" = roll_onto_cylinder (up to 2 radians)"""
    V, F = shape(name)
    if kind == "twist":
        handles, hp = twist(V)
        X = ArapNp(M.cotmatrix(V, F), V, handles).run(hp, n_iter=3)[0]
    elif kind == "stretch":
        X = (V @ rotation_matrix([1.0, 2.0, -0.5], 2.0).T) * np.array([1.5, 0.7, 1.2])
    else:
        X = roll_onto_cylinder(V)
    X = np.ascontiguousarray(X, dtype=np.float64)
    X.setflags(write=False)
    return X


# ---- per face ------------------------------------------------------------------------------------------------------------------------------------
def rest_faces(V, F):
    """W (nF x 3 x 3: W[f, i] = (n x e_i) / (2A)), n (nF x 3), A (nF): k_geo_basis' expressions (morph_basis)"""
    a, b, c = V[F[:, 0]], V[F[:, 1]], V[F[:, 2]]
    u, v = b - a, c - a
    w = np.stack([u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1], u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2], u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]], axis=1)
    dA = np.sqrt(w[:, 0] * w[:, 0] + w[:, 1] * w[:, 1] + w[:, 2] * w[:, 2])
    nrm = w / dA[:, None]
    W = np.zeros((F.shape[0], 3, 3))
    for i, e in enumerate((c - b, a - c, b - a)):
        W[:, i, 0] = (nrm[:, 1] * e[:, 2] - nrm[:, 2] * e[:, 1]) / dA
        W[:, i, 1] = (nrm[:, 2] * e[:, 0] - nrm[:, 0] * e[:, 2]) / dA
        W[:, i, 2] = (nrm[:, 0] * e[:, 1] - nrm[:, 1] * e[:, 0]) / dA
    return W, nrm, dA * 0.5


def gradient(V0, F, X):
    """J (nF x 3 x 3) of the pose X on the rest mesh (V0, F) (morph_gradient)"""
    W, nrm, _ = rest_faces(V0, F)
    x0, x1, x2 = X[F[:, 0]], X[F[:, 1]], X[F[:, 2]]
    u, v = x1 - x0, x2 - x0
    w = np.stack([u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1], u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2], u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]], axis=1)
    d = np.sqrt(w[:, 0] * w[:, 0] + w[:, 1] * w[:, 1] + w[:, 2] * w[:, 2])
    N = np.where((d > 0.0)[:, None], w / np.where(d > 0.0, d, 1.0)[:, None], 0.0)
    J = np.zeros((F.shape[0], 3, 3))
    for a in range(3):
        for b in range(3):
            T = x0[:, a] * W[:, 0, b] + x1[:, a] * W[:, 1, b] + x2[:, a] * W[:, 2, b]
            J[:, a, b] = T + N[:, a] * nrm[:, b]
    return J


def polar(J):
    """(R, S, gap, sigma): J = R S by LAPACK, R = U D V^T with the flip on the smallest singular value, S = sym(R^T J); gap = (sigma_2 + d sigma_3) / sigma_1"""
    Rt, gap, _ = rotations_np(J)                         # the rotation that maximises tr(R_a J) is R^T
    R = np.ascontiguousarray(Rt.transpose(0, 2, 1))
    Mx = np.einsum("nji,njk->nik", R, J)
    return R, 0.5 * (Mx + Mx.transpose(0, 2, 1)), gap, np.linalg.svd(J, compute_uv=False)


def stretch_of(R, J):
    """S6 (nF x 6: 00, 01, 02, 11, 12, 22) from given rotations, in morph_polar's order"""
    Mx = np.zeros_like(J)
    for a in range(3):
        for b in range(3):
            Mx[:, a, b] = R[:, 0, a] * J[:, 0, b] + R[:, 1, a] * J[:, 1, b] + R[:, 2, a] * J[:, 2, b]
    return np.stack([Mx[:, 0, 0], 0.5 * (Mx[:, 0, 1] + Mx[:, 1, 0]), 0.5 * (Mx[:, 0, 2] + Mx[:, 2, 0]), Mx[:, 1, 1], 0.5 * (Mx[:, 1, 2] + Mx[:, 2, 1]),
                     Mx[:, 2, 2]], axis=1)


def sym6(S):
    return np.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], axis=1)


def log_rotation(R):
    """omega (nF x 3): Shepperd's branch, w >= 0, theta = 2 atan2(|v|, w), omega = (theta / |v|) v (morph_log)"""
    r = lambda a, b: R[:, a, b]   # noqa: E731
    tr = r(0, 0) + r(1, 1) + r(2, 2)
    c0 = (tr >= r(0, 0)) & (tr >= r(1, 1)) & (tr >= r(2, 2))
    c1 = ~c0 & (r(0, 0) >= r(1, 1)) & (r(0, 0) >= r(2, 2))
    c2 = ~c0 & ~c1 & (r(1, 1) >= r(2, 2))
    cases = [(1.0 + tr, None, r(2, 1) - r(1, 2), r(0, 2) - r(2, 0), r(1, 0) - r(0, 1)),
             (((1.0 + r(0, 0)) - r(1, 1)) - r(2, 2), r(2, 1) - r(1, 2), None, r(0, 1) + r(1, 0), r(0, 2) + r(2, 0)),
             (((1.0 - r(0, 0)) + r(1, 1)) - r(2, 2), r(0, 2) - r(2, 0), r(0, 1) + r(1, 0), None, r(1, 2) + r(2, 1)),
             (((1.0 - r(0, 0)) - r(1, 1)) + r(2, 2), r(1, 0) - r(0, 1), r(0, 2) + r(2, 0), r(1, 2) + r(2, 1), None)]
    sel = [c0, c1, c2, ~c0 & ~c1 & ~c2]
    q = np.zeros((R.shape[0], 4))
    for m, (t, *wxyz) in zip(sel, cases):
        h = 0.5 / np.sqrt(np.where(m, t, 1.0))
        for e, val in enumerate(wxyz):
            q[:, e] = np.where(m, (t if val is None else val) * h, q[:, e])
    q = np.where((q[:, 0] < 0.0)[:, None], -q, q)
    vn = np.sqrt(q[:, 1] * q[:, 1] + q[:, 2] * q[:, 2] + q[:, 3] * q[:, 3])
    pos = vn > 0.0
    g = (2.0 * np.arctan2(vn, q[:, 0])) / np.where(pos, vn, 1.0)
    return np.where(pos[:, None], g[:, None] * q[:, 1:], 0.0)


def interp(omega, S6, t, dtype=np.float64):
    """J(t) (nF x 3 x 3) = Rodrigues(t omega) (I + t (S - I)) in morph_interp's order; dtype = numpy.longdouble evaluates it in extended precision"""
    om, S6 = omega.astype(dtype), S6.astype(dtype)
    t, one = dtype(t), dtype(1.0)
    ax, ay, az = t * om[:, 0], t * om[:, 1], t * om[:, 2]
    th = np.sqrt(ax * ax + ay * ay + az * az)
    pos = th > 0
    safe = np.where(pos, th, one)
    kx, ky, kz = ax / safe, ay / safe, az / safe
    s, c = np.sin(th), np.cos(th)
    v = one - c
    R = np.zeros((om.shape[0], 3, 3), dtype=dtype)
    R[:, 0, 0], R[:, 0, 1], R[:, 0, 2] = c + v * (kx * kx), v * (kx * ky) - s * kz, v * (kx * kz) + s * ky
    R[:, 1, 0], R[:, 1, 1], R[:, 1, 2] = v * (kx * ky) + s * kz, c + v * (ky * ky), v * (ky * kz) - s * kx
    R[:, 2, 0], R[:, 2, 1], R[:, 2, 2] = v * (kx * kz) - s * ky, v * (ky * kz) + s * kx, c + v * (kz * kz)
    R[~pos] = np.eye(3, dtype=dtype)
    St = np.zeros_like(R)
    St[:, 0, 0], St[:, 1, 1], St[:, 2, 2] = one + t * (S6[:, 0] - one), one + t * (S6[:, 3] - one), one + t * (S6[:, 5] - one)
    St[:, 0, 1] = St[:, 1, 0] = t * S6[:, 1]
    St[:, 0, 2] = St[:, 2, 0] = t * S6[:, 2]
    St[:, 1, 2] = St[:, 2, 1] = t * S6[:, 4]
    J = np.zeros_like(R)
    for a in range(3):
        for b in range(3):
            J[:, a, b] = R[:, a, 0] * St[:, 0, b] + R[:, a, 1] * St[:, 1, b] + R[:, a, 2] * St[:, 2, b]
    return J, St


# ---- per vertex ----------------------------------------------------------------------------------------------------------------------------------
def rhs(V0, F, Js):
    """(B as nV x 3k, bsq as k x nV) from Js (k x nF x 3 x 3): b_v = sum over v's corners in list order of A_f (J_f W_fj) (k_morph_rhs)"""
    W, _, Af = rest_faces(V0, F)
    Js = np.asarray(Js)
    n, k = V0.shape[0], Js.shape[0]
    acc = np.zeros((k, n, 3), dtype=Js.dtype)
    for vs, q in corner_lists(np.asarray(F), n):
        f, j = q // 3, q % 3
        w = W[f, j]
        for c in range(k):
            Jf = Js[c][f]
            for a in range(3):
                acc[c, vs, a] += Af[f] * (Jf[:, a, 0] * w[:, 0] + Jf[:, a, 1] * w[:, 1] + Jf[:, a, 2] * w[:, 2])
    B = np.ascontiguousarray(acc.transpose(1, 0, 2).reshape(n, 3 * k))
    return B, acc[:, :, 0] * acc[:, :, 0] + acc[:, :, 1] * acc[:, :, 1] + acc[:, :, 2] * acc[:, :, 2]


def rhs_scale(V0, F, Sts):
    """sum over v's corners of A_f |S_f(t_c)|_F |W_fj|: the scale of the error bound of k_morph_rhs<true>; nV x k"""
    W, _, Af = rest_faces(V0, F)
    n, k = V0.shape[0], len(Sts)
    out = np.zeros((n, k))
    wn = np.linalg.norm(W, axis=2)
    for f in range(F.shape[0]):
        for j in range(3):
            for c in range(k):
                out[F[f, j], c] += Af[f] * float(np.linalg.norm(Sts[c][f].astype(np.float64))) * wn[f, j]
    return out


def blend(V0, X, t):
    return (1.0 - t) * V0 + t * X


def pins_and_start(V0, X, ts, pins, k):
    """(hp as n_pins x 3k, U as nV x 3k): the default pin positions and the default start with its pinned rows set (k_morph_pins / _start / _set_pins)"""
    sets = [V0 if X is None else blend(V0, X, ts[c]) for c in range(k)]
    U = np.concatenate(sets, axis=1)
    return np.ascontiguousarray(U[pins]), np.ascontiguousarray(U)


# ---- the method with direct solves -----------------------------------------------------------------------------------------------------------------
class MorphNp:
    """(-L)_uu factored once; L = the cotangent matrix of the rest mesh (the numpy one, or the library's own bits)"""

    def __init__(self, V, F, pins=(0,), L=None):
        self.V, self.F = np.asarray(V, dtype=np.float64), np.asarray(F)
        self.n = self.V.shape[0]
        self.pins = np.asarray(pins, dtype=np.int64)
        K = (-sp.csr_matrix(M.cotmatrix(self.V, self.F) if L is None else L)).tocsr()
        mask = np.ones(self.n, dtype=bool)
        mask[self.pins] = False
        self.unknown = np.nonzero(mask)[0]
        self.lu = spla.splu(K[self.unknown][:, self.unknown].tocsc())
        self.Kuk = K[self.unknown][:, self.pins]

    def solve(self, B, hp):
        U = np.zeros_like(B)
        U[self.pins] = hp
        U[self.unknown] = self.lu.solve(B[self.unknown] - self.Kuk @ hp)
        return U

    def sets(self, U):
        return np.ascontiguousarray(U.reshape(self.n, -1, 3).transpose(1, 0, 2))

    def reconstruct(self, Js, pin_pos=None):
        """Js: k x nF x 3 x 3; pin_pos: k x n_pins x 3 or None = the rest positions.  Returns (U as k x n x 3, B)"""
        Js = np.asarray(Js).reshape(-1, self.F.shape[0], 3, 3)
        k = Js.shape[0]
        B, _ = rhs(self.V, self.F, Js)
        hp = pins_and_start(self.V, None, None, self.pins, k)[0] if pin_pos is None else np.concatenate(list(pin_pos), axis=1)
        return self.sets(self.solve(B, hp)), B

    def factors(self, X):
        """(omega, S6) of the pose X: LAPACK's polar factors and the kernel's logarithm"""
        J = gradient(self.V, self.F, X)
        R, S, _, _ = polar(J)
        return log_rotation(R), sym6(S)

    def interpolate(self, X, ts, pin_pos=None):
        om, S6 = self.factors(X)
        Js = np.stack([interp(om, S6, t)[0] for t in ts])
        B, _ = rhs(self.V, self.F, Js)
        hp = pins_and_start(self.V, X, ts, self.pins, len(ts))[0] if pin_pos is None else np.concatenate(list(pin_pos), axis=1)
        return self.sets(self.solve(B, hp)), B

    def transfer(self, S0, S1s, Fs=None, pin_pos=None):
        Fs = self.F if Fs is None else Fs
        S1s = np.asarray(S1s).reshape(-1, S0.shape[0], 3)
        return self.reconstruct(np.stack([gradient(S0, Fs, S1) for S1 in S1s]), pin_pos)


def exact_transfer(V, pins, B):
    """the transfer of the affine pose x -> B x + b of a source S0 = s V + a (s > 0): V B^T moved so that pin 0 keeps its rest position"""
    U = V @ B.T
    return U + (V[pins[0]] - U[pins[0]])


# ---- the library's side, shared with tests/test_gpu_morph.py ---------------------------------------------------------------------------------------
def out_size(op, nV, nF, k, n_pins):
    return {MORPH_FACE_GRADIENT: 9 * nF * k, MORPH_FACE_POLAR: 18 * nF, MORPH_RHS_GRADIENT: 4 * nV * k, MORPH_RHS_INTERP: 4 * nV * k,
            MORPH_PINS: 3 * k * (nV + n_pins)}.get(op, 18 * nF)


def unpack(op, out, nV, nF, k, n_pins=0):
    """GRADIENT: J (k x nF x 3 x 3); POLAR: (R, omega, S6); RHS_*: (B as nV x 3k, bsq as k x nV); PINS: (hp as n_pins x 3k, U as nV x 3k)"""
    if op == MORPH_FACE_GRADIENT:
        return out[:9 * nF * k].reshape(k, nF, 3, 3)
    if op == MORPH_FACE_POLAR:
        return out[:9 * nF].reshape(nF, 3, 3), out[9 * nF:12 * nF].reshape(nF, 3), out[12 * nF:18 * nF].reshape(nF, 6)
    if op == MORPH_PINS:
        return out[:3 * k * n_pins].reshape(3 * k, n_pins).T, out[3 * k * n_pins:3 * k * (n_pins + nV)].reshape(3 * k, nV).T
    return out[:3 * nV * k].reshape(3 * k, nV).T, out[3 * nV * k:4 * nV * k].reshape(k, nV)


SENTINEL = -7.25e300


def _call(fn, with_guard, op, V0, F, k=1, X=None, t=None, inp=None, pins=None, over=None, pad=64):
    """`pad` doubles of sentinel follow the op's extent in `out`: nothing past the extent may be written"""
    ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
    nV, nF = V0.shape[0], F.shape[0]
    F = np.ascontiguousarray(F, dtype=np.int32)
    keep = [None if a is None else np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(-1)) for a in (V0, X, t, inp)]
    pins = None if pins is None else np.ascontiguousarray(pins, dtype=np.int32)
    arr = lambda a, ty=dp: None if a is None else a.ctypes.data_as(ty)   # noqa: E731
    n_pins = 0 if pins is None else pins.shape[0]
    size = out_size(op, nV, nF, max(k, 1), n_pins)
    out = np.full(size + pad, SENTINEL)
    bad = C.c_int(-1)
    a = dict(nV=nV, nF=nF, k=k, F=arr(F, ip), V0=arr(keep[0]), X=arr(keep[1]), t=arr(keep[2]), inp=arr(keep[3]), pins=arr(pins, ip), n_pins=n_pins,
             out=arr(out))
    a.update(over or {})
    args = [op] + [a[key] for key in ("nV", "nF", "k", "F", "V0", "X", "t", "inp", "pins", "n_pins", "out")]
    rc = fn(*args, C.byref(bad)) if with_guard else fn(*args)
    if rc == 0:
        assert np.all(out[size:] == SENTINEL), "op %d wrote past its extent" % op
    return rc, bad.value, out[:size]


def faces_host(smg, op, V0, F, **kw):
    """one call of smg_morph_faces_host; returns (rc, out)"""
    rc, _, out = _call(smg._lib.load().smg_morph_faces_host, False, op, V0, F, **kw)
    return rc, out


def hook(smg, op, V0, F, **kw):
    """one call of smg_debug_morph; returns (rc, guard hits, out)"""
    return _call(smg._lib.load().smg_debug_morph, True, op, V0, F, **kw)
