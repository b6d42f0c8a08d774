"""The numpy / scipy restatement of the projective-dynamics membrane step (include/smg.h: smg_pd_*), with direct solves.

The face maths follow csrc/smg_pd_inl.hpp operation by operation (every sum one accumulator in the header's order), the right-hand side sums
in corner-list order as k_pd_vertices does, and fixed_sum restates launch_fixed_sum's order.  The projection is ALSO available through
numpy.linalg.svd (project_svd), so the closed form is held to LAPACK.  tests/test_pd_host.py checks the restatement and the library's host
twin; tests/test_gpu_pd.py checks the device against it."""
import ctypes as C
import functools

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from oracle import mesh_np as M

EPS = 2.0 ** -52
RANK_GUARD = 2.0 ** -80
PD_REST, PD_FACES, PD_FACES_STEP, PD_MASS, PD_PREDICT, PD_VERTICES, PD_ENERGY, PD_FINISH, PD_STRAIN = range(9)
DEFAULTS = dict(dt=1e-2, density=1.0, stiffness=1.0, sigma_min=1.0, sigma_max=1.0, pressure=0.0, gravity=(0.0, 0.0, 0.0))


# ---- the face maths (smg_pd_inl.hpp, in its order) ---------------------------------------------------------------------------------------------
def rest_constants(V, F):
    """nF x 4: a, b, c, A_f (pd_rest)"""
    p0, p1, p2 = V[F[:, 0]], V[F[:, 1]], V[F[:, 2]]
    e1x, e1y, e1z = (p1 - p0).T
    e2x, e2y, e2z = (p2 - p0).T
    a = np.sqrt(e1x * e1x + e1y * e1y + e1z * e1z)
    dot = e1x * e2x + e1y * e2y + e1z * e2z
    wx, wy, wz = e1y * e2z - e1z * e2y, e1z * e2x - e1x * e2z, e1x * e2y - e1y * e2x
    b, c = dot / a, np.sqrt(wx * wx + wy * wy + wz * wz) / a
    return np.stack([a, b, c, 0.5 * (a * c)], axis=1)


def gradient(r, F, P):
    """nF x 6: f1x, f1y, f1z, f2x, f2y, f2z (pd_gradient)"""
    q0, q1, q2 = P[F[:, 0]], P[F[:, 1]], P[F[:, 2]]
    f1 = (q1 - q0) / r[:, 0, None]
    f2 = ((q2 - q0) - r[:, 1, None] * f1) / r[:, 2, None]
    return np.concatenate([f1, f2], axis=1)


def clamp(s, lo, hi):
    return np.where(s < lo, lo, np.where(s > hi, hi, s))


def project(Fg, smin, smax):
    """(sigma nF x 2, T nF x 6, guard nF bool) by the closed form of pd_project"""
    with np.errstate(invalid="ignore", divide="ignore"):
        f1, f2 = Fg[:, :3], Fg[:, 3:]
        c11 = (f1[:, 0] * f1[:, 0] + f1[:, 1] * f1[:, 1]) + f1[:, 2] * f1[:, 2]
        c12 = (f1[:, 0] * f2[:, 0] + f1[:, 1] * f2[:, 1]) + f1[:, 2] * f2[:, 2]
        c22 = (f2[:, 0] * f2[:, 0] + f2[:, 1] * f2[:, 1]) + f2[:, 2] * f2[:, 2]
        m, d = 0.5 * (c11 + c22), 0.5 * (c11 - c22)
        r = np.sqrt(d * d + c12 * c12)
        l1, l2 = m + r, np.fmax(m - r, 0.0)
        s1, s2 = np.sqrt(l1), np.sqrt(l2)
        t1, t2 = clamp(s1, smin, smax), clamp(s2, smin, smax)
        x, y = np.where(d >= 0.0, r + d, c12), np.where(d >= 0.0, c12, r - d)
        n = np.sqrt(x * x + y * y)
        v1x, v1y = np.where(n > 0.0, x / n, 1.0), np.where(n > 0.0, y / n, 0.0)
        v2x, v2y = 0.0 - v1y, v1x
        u1 = (f1 * v1x[:, None] + f2 * v1y[:, None]) / s1[:, None]
        u2 = (f1 * v2x[:, None] + f2 * v2y[:, None]) / s2[:, None]
        point = l1 == 0.0
        rank = ~point & (l2 <= RANK_GUARD * l1)
        if np.any(rank):
            a = np.abs(u1[rank])
            j = np.where((a[:, 0] <= a[:, 1]) & (a[:, 0] <= a[:, 2]), 0, np.where(a[:, 1] <= a[:, 2], 1, 2))
            uj = u1[rank][np.arange(j.size), j]
            w = np.eye(3)[j] - uj[:, None] * u1[rank]
            ln = np.sqrt((w[:, 0] * w[:, 0] + w[:, 1] * w[:, 1]) + w[:, 2] * w[:, 2])
            u2[rank] = w / ln[:, None]
        s1x, s1y, s2x, s2y = t1 * v1x, t1 * v1y, t2 * v2x, t2 * v2y
        T = np.concatenate([s1x[:, None] * u1 + s2x[:, None] * u2, s1y[:, None] * u1 + s2y[:, None] * u2], axis=1)
        if np.any(point):
            T[point] = 0.0
            T[point, 0] = t1[point]
            T[point, 4] = t1[point]
    return np.stack([s1, s2], axis=1), T, point | rank


def project_svd(Fg, smin, smax):
    """(sigma, T) through numpy.linalg.svd of the 3 x 2 matrices: the reference the closed form is held to"""
    A = np.stack([Fg[:, :3], Fg[:, 3:]], axis=2)                   # nF x 3 x 2
    U, s, Vt = np.linalg.svd(A, full_matrices=False)
    Tm = np.einsum("fik,fk,fkj->fij", U, np.clip(s, smin, smax), Vt)
    return s, np.concatenate([Tm[:, :, 0], Tm[:, :, 1]], axis=1)


def distance2(Fg, T):
    acc = np.zeros(Fg.shape[0])
    for e in range(6):
        x = Fg[:, e] - T[:, e]
        acc = acc + x * x
    return acc


def face_energy(r, k, Fg, T):
    return 0.5 * ((k * r[:, 3]) * distance2(Fg, T))


def corner_shares(r, k, T):
    """nF x 9: entry 3 i + l = k A_f (T g_i)_l (pd_corner_shares)"""
    kA = k * r[:, 3]
    g1x, g1y, g2y = 1.0 / r[:, 0], 0.0 - r[:, 1] / (r[:, 0] * r[:, 2]), 1.0 / r[:, 2]
    t1 = T[:, :3] * g1x[:, None] + T[:, 3:] * g1y[:, None]
    t2 = T[:, 3:] * g2y[:, None]
    return np.concatenate([kA[:, None] * ((0.0 - t1) - t2), kA[:, None] * t1, kA[:, None] * t2], axis=1)


def strain_terms(r, Fg, sigma, T, smin, smax):
    """nF x 5: sigma1, -sigma2, outside the band, A_f |F - T|^2, A_f (k_pd_strain_terms)"""
    out = ((sigma[:, 0] > smax) | (sigma[:, 1] < smin)).astype(np.float64)
    return np.stack([sigma[:, 0], 0.0 - sigma[:, 1], out, r[:, 3] * distance2(Fg, T), r[:, 3]], axis=1)


def clamp_outcomes(sigma, smin, smax):
    """(faces inside the band, faces with sigma1 above it, faces with sigma2 below it)"""
    above, below = sigma[:, 0] > smax, sigma[:, 1] < smin
    return int(np.sum(~above & ~below)), int(np.sum(above)), int(np.sum(below))


# ---- the vertex side ---------------------------------------------------------------------------------------------------------------------------
def corner_lists(F, nV):
    """per vertex its corners t = 3 f + i, faces ascending; as slot arrays [(vertices, corners)] for sequential sums"""
    t = np.arange(3 * F.shape[0])
    v = F.reshape(-1)
    order = np.argsort(v, kind="stable")
    v, t = v[order], t[order]
    rank = np.arange(t.size) - np.searchsorted(v, np.arange(nV))[v]
    return [(v[rank == k], t[rank == k]) for k in range(int(rank.max()) + 1)]


def corner_sum(share, lists, nV):
    """nV x 3: the sum over every vertex's corners, in list order, of the corner shares (one accumulator from 0)"""
    acc = np.zeros((nV, 3))
    flat = share.reshape(-1, 3)                                    # row 3 f + i
    for vs, ts in lists:
        acc[vs] = acc[vs] + flat[ts]
    return acc


def vertices(share, lists, m0, c_mass, S, Q):
    """(B nV x 3, inertia terms nV, |B_v|^2 nV) of k_pd_vertices"""
    acc = corner_sum(share, lists, m0.size)
    w = c_mass * m0
    B = w[:, None] * S + acc
    dq = Q - S
    iterm = (0.5 * w) * ((dq[:, 0] * dq[:, 0] + dq[:, 1] * dq[:, 1]) + dq[:, 2] * dq[:, 2])
    return B, iterm, (B[:, 0] * B[:, 0] + B[:, 1] * B[:, 1]) + B[:, 2] * B[:, 2]


def pressure_fext(P, F, pressure):
    """what launch_membrane_pressure writes: (-(pressure m_v(P))) n_v(P), nV x 3"""
    m = M.massmatrix(P, F, "voronoi").diagonal()
    c = np.cross(P[F[:, 1]] - P[F[:, 0]], P[F[:, 2]] - P[F[:, 0]])
    N = np.zeros_like(P)
    for j in range(3):
        np.add.at(N, F[:, j], c)
    ln = np.sqrt((N[:, 0] * N[:, 0] + N[:, 1] * N[:, 1]) + N[:, 2] * N[:, 2])
    return (-(pressure * m))[:, None] * (N / ln[:, None])


def predict(x, v, fext, m0, h, rho, g):
    """S of k_pd_predict"""
    rm = rho * m0
    fv = (0.0 - fext) + rm[:, None] * np.asarray(g, dtype=np.float64)[None, :]
    return (x + h * v) + ((h * h) * fv) / rm[:, None]


def fixed_sum_groups(n):
    return int(max(1, min((n + 2047) // 2048, 1024)))


def fixed_sum(term):
    """launch_fixed_sum's order: row chunks, 256 strided accumulators per chunk, a halving tree, 64 strided accumulators over the chunks, a
    halving tree"""
    term = np.asarray(term, dtype=np.float64)
    n = term.size
    groups = fixed_sum_groups(n)
    rpc = (n + groups - 1) // groups
    part = np.zeros(groups)
    for g in range(groups):
        rows = term[g * rpc:min(n, (g + 1) * rpc)]
        pad = np.zeros(((rows.size + 255) // 256) * 256)
        pad[:rows.size] = rows
        acc = np.zeros(256)
        for row in pad.reshape(-1, 256):          # a lane past the end adds nothing: x + 0.0 keeps the bits of x (the accumulators start at +0.0)
            acc = acc + row
        half = 128
        while half > 0:
            acc = acc[:half] + acc[half:2 * half]
            half //= 2
        part[g] = acc[0]
    pad = np.zeros(((groups + 63) // 64) * 64)
    pad[:groups] = part
    v = np.zeros(64)
    for row in pad.reshape(-1, 64):
        v = v + row
    half = 32
    while half > 0:
        v = v[:half] + v[half:2 * half]
        half //= 2
    return float(v[0])


# ---- the stepper with direct solves ----------------------------------------------------------------------------------------------------------
class PdNp:
    def __init__(self, V, F, pins=(), **params):
        p = dict(DEFAULTS)
        p.update(params)
        self.p = p
        self.V = np.ascontiguousarray(V, dtype=np.float64)
        self.F = np.ascontiguousarray(F, dtype=np.int32)
        self.nV, self.nF = self.V.shape[0], self.F.shape[0]
        self.pins = np.asarray(pins, dtype=np.int64).reshape(-1)
        self.r = rest_constants(self.V, self.F)
        self.m0 = M.massmatrix(self.V, self.F, "voronoi").diagonal()
        self.lists = corner_lists(self.F, self.nV)
        self.c_mass = p["density"] / (p["dt"] * p["dt"])
        self.L = M.cotmatrix(self.V, self.F).tocsr()
        self.A = (sp.diags(self.c_mass * self.m0) - p["stiffness"] * self.L).tocsr()
        mask = np.ones(self.nV, dtype=bool)
        mask[self.pins] = False
        self.unknown = np.nonzero(mask)[0]
        self.lu = spla.splu(self.A[self.unknown][:, self.unknown].tocsc())
        self.Auk = self.A[self.unknown][:, self.pins].tocsr()
        self.x, self.v = self.V.copy(), np.zeros_like(self.V)
        self.pin_pos = self.V[self.pins].copy()

    def area(self):
        return float(np.sum(self.r[:, 3]))

    def faces(self, Q):
        """(Fg, sigma, T, energy terms, corner shares, guard) of the pose Q"""
        p = self.p
        Fg = gradient(self.r, self.F, Q)
        sigma, T, guard = project(Fg, p["sigma_min"], p["sigma_max"])
        return Fg, sigma, T, face_energy(self.r, p["stiffness"], Fg, T), corner_shares(self.r, p["stiffness"], T), guard

    def local(self, S, Q):
        """(E, B, |B|_F) at the iterate Q"""
        _, _, _, et, share, _ = self.faces(Q)
        B, iterm, bsq = vertices(share, self.lists, self.m0, self.c_mass, S, Q)
        return float(np.sum(et) + np.sum(iterm)), B, float(np.sqrt(np.sum(bsq)))

    def solve(self, B, Q, pin_pos):
        Qn = Q.copy()
        Qn[self.unknown] = self.lu.solve(B[self.unknown] - (self.Auk @ pin_pos if self.pins.size else 0.0))
        Qn[self.pins] = pin_pos
        return Qn

    def prediction(self, pin_pos=None):
        p = self.p
        hp = self.pin_pos if pin_pos is None else np.asarray(pin_pos, dtype=np.float64).reshape(-1, 3)
        S = predict(self.x, self.v, pressure_fext(self.x, self.F, p["pressure"]), self.m0, p["dt"], p["density"], p["gravity"])
        S[self.pins] = hp
        return S, hp

    def step(self, pin_pos=None, n_iter=10, record=False):
        """One step with direct solves.  Returns (energy_his with n_iter + 1 entries, info); info holds S, the iterates and right-hand sides
        when record."""
        S, hp = self.prediction(pin_pos)
        Q = S.copy()
        E, info = [], dict(S=S, iterates=[Q.copy()], rhs=[])
        for _ in range(n_iter):
            e, B, _ = self.local(S, Q)
            E.append(e)
            Q = self.solve(B, Q, hp)
            if record:
                info["iterates"].append(Q.copy())
                info["rhs"].append(B)
        E.append(self.local(S, Q)[0])
        self.v = (Q - self.x) / self.p["dt"]
        self.x = Q
        self.pin_pos = hp
        return np.array(E), info


def load_mesh(name):
    V, F = M.read_smgm(name)
    return M.normalize_unit_area(V, F), F


def perturbed(V, F, amp, seed=0):
    """rest + amp sqrt(mean double area) N(0, 1)"""
    return V + amp * np.sqrt(np.mean(M.doublearea(V, F))) * np.random.default_rng(seed).standard_normal(V.shape)


@functools.lru_cache(maxsize=None)
def reference_run(name, band=(1.0, 1.0), pressure=5.0, n_steps=3, n_iter=10):
    """(PdNp after the steps, [energy_his per step], [(x, v) before step 0 and after every step]) of the issue's table run on a fixture: computed
    once per session and left unchanged by its users"""
    V, F = load_mesh(name)
    P = PdNp(V, F, sigma_min=band[0], sigma_max=band[1], pressure=pressure)
    Es, states = [], [(P.x.copy(), P.v.copy())]
    for _ in range(n_steps):
        E, _ = P.step(n_iter=n_iter)
        Es.append(E)
        states.append((P.x.copy(), P.v.copy()))
    for a in Es + [s for st in states for s in st]:
        a.setflags(write=False)
    return P, Es, states


# ---- the library's side, shared with tests/test_gpu_pd.py ---------------------------------------------------------------------------------------
def pd_params_c(smg, **params):
    p = dict(DEFAULTS)
    p.update(params)
    return smg.pd_params(**p)


def project_host(smg, V0, P, F, smin, smax):
    """smg_pd_project_host -> (rc, Fg nF x 6, sigma nF x 2, T nF x 6, guard hits)"""
    L = smg._lib.load()
    ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
    V0, P = np.ascontiguousarray(V0, dtype=np.float64), np.ascontiguousarray(P, dtype=np.float64)
    F = np.ascontiguousarray(F, dtype=np.int32)
    nF = F.shape[0]
    Fg, sg, T = np.full(6 * nF, np.nan), np.full(2 * nF, np.nan), np.full(6 * nF, np.nan)
    hits = C.c_int(-1)
    rc = L.smg_pd_project_host(V0.ctypes.data_as(dp), P.ctypes.data_as(dp), V0.shape[0], F.ctypes.data_as(ip), nF, smin, smax, Fg.ctypes.data_as(dp),
                               sg.ctypes.data_as(dp), T.ctypes.data_as(dp), C.byref(hits))
    return rc, Fg.reshape(6, nF).T, sg.reshape(2, nF).T, T.reshape(6, nF).T, hits.value


def pd_hook(smg, op, nV, F, V0=None, P=None, inp=None, n_out=0, **params):
    """one call of smg_debug_pd; returns (rc, guard hits, out)"""
    L = smg._lib.load()
    ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
    F = np.ascontiguousarray(F, dtype=np.int32)
    keep = [None if a is None else np.ascontiguousarray(a, dtype=np.float64) for a in (V0, P, inp)]
    arr = lambda a: None if a is None else a.ctypes.data_as(dp)   # noqa: E731
    out = np.full(max(n_out, 1), np.nan)
    bad = C.c_int(-1)
    par = pd_params_c(smg, **params)
    rc = L.smg_debug_pd(op, nV, F.shape[0], F.ctypes.data_as(ip), arr(keep[0]), arr(keep[1]), arr(keep[2]), C.byref(par),
                        out.ctypes.data_as(dp) if n_out else None, C.byref(bad))
    return rc, bad.value, out


# ---- hand-made single faces --------------------------------------------------------------------------------------------------------------------
REST_FACE = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.3, 0.8, 0.0]])
ROT = np.array([[0.36, 0.48, -0.8], [-0.8, 0.6, 0.0], [0.48, 0.64, 0.6]])    # a rotation with exact entries


def hand_faces(band=(0.9, 1.2)):
    """[(label, pose 3 x 3, guard expected)] of REST_FACE: one face in each clamp outcome of the band (lo < hi), one collapsed to a segment
    (f2 == 0 exactly: 0.6 - 0.3 * 2), one collapsed to a point"""
    lo, hi = band
    mid = 0.5 * (lo + hi)

    def stretched(sx, sy):
        return (REST_FACE * np.array([sx, sy, 1.0])) @ ROT.T + np.array([0.1, -0.2, 0.3])

    return [("inside", stretched(mid, 0.99 * mid), False), ("above", stretched(1.5 * hi, mid), False), ("below", stretched(mid, 0.5 * lo), False),
            ("segment", np.array([[0.0, 0.0, 0.0], [2.0, 0.0, 0.0], [0.6, 0.0, 0.0]]), True), ("point", np.tile([0.25, -1.0, 2.0], (3, 1)), True)]
