"""CPU: harmonic and as-rigid-as-possible flattening of disk meshes (include/smg.h: smg_param_*) -- the ABI and its refusals without a GPU,
and the numpy / scipy restatement of the method (direct solves) that tests/test_gpu_param.py checks the device against.  The restatement
follows csrc/smg_param_inl.hpp and the kernels of csrc/smg_param_device.hip operation by operation (three terms per face in corner order, the
right-hand side in the order of the vertex's corner list)."""
import ctypes as C
import functools
import json
import math
import os

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from oracle import mesh_np as M
from test_arap_host import _fake_hierarchy, roll_onto_cylinder
from test_geodesics_host import flat_square
from test_membrane_host import corner_lists

INVALID, NO_DEVICE = -1, -2
PARAM_REST, PARAM_COVARIANCE, PARAM_ROTATIONS, PARAM_RHS, PARAM_FACE_ENERGY, PARAM_ENERGY, PARAM_DISTORTION = range(7)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "param_refusals.json")
EPS = 2.0 ** -52

# the issue's table: fixture -> (nV, loop length, E_0, E_1, E_10, flipped faces at E_10), after normalize_unit_area, 10 iterations from the harmonic map
TABLE = {"ogre_sim.smgm": (2612, 150, 1.287e-1, 5.137e-2, 5.0801e-2, 0),
         "bunny.smgm": (9353, 149, 9.956e-1, 4.250e-1, 4.2295e-1, 707),
         "ogre.smgm": (19985, 112, 2.974e-1, 1.305e-1, 1.2970e-1, 0)}


# ---- the method in numpy (the expressions of smg_param_inl.hpp, in their order) -----------------------------------------------------------------
def rest_constants(V, F):
    """nF x 6: a, b, c (x1 = (a, 0), x2 = (b, c)) and c0, c1, c2 (param_rest)"""
    p0, p1, p2 = V[F[:, 0]], V[F[:, 1]], V[F[:, 2]]
    e1x, e1y, e1z = (p1 - p0).T
    e2x, e2y, e2z = (p2 - p0).T
    a = np.sqrt(e1x * e1x + e1y * e1y + e1z * e1z)
    dot = e1x * e2x + e1y * e2y + e1z * e2z
    wx, wy, wz = e1y * e2z - e1z * e2y, e1z * e2x - e1x * e2z, e1x * e2y - e1y * e2x
    b, c = dot / a, np.sqrt(wx * wx + wy * wy + wz * wz) / a
    dA = a * c
    return np.stack([a, b, c, (b * (b - a) + c * c) / dA, (a * b) / dA, (a * (a - b)) / dA], axis=1)


def rest_edges(r):
    """d_i = x_i - x_{i+1} as (dx, dy), nF x 3 each (param_edges)"""
    a, b, c = r[:, 0], r[:, 1], r[:, 2]
    z = np.zeros_like(a)
    return np.stack([0.0 - a, a - b, b], axis=1), np.stack([z, 0.0 - c, c], axis=1)


def map_edges(F, UV):
    """g_i = u_i - u_{i+1} as (gx, gy), nF x 3 each (param_map_edges)"""
    u = UV[F]                                                     # nF x 3 x 2
    return (np.stack([u[:, i, 0] - u[:, (i + 1) % 3, 0] for i in range(3)], axis=1),
            np.stack([u[:, i, 1] - u[:, (i + 1) % 3, 1] for i in range(3)], axis=1))


def covariance(r, F, UV):
    """nF x 4: S00, S01, S10, S11 of S_f = sum_i c_i g_i d_i^T (param_covariance)"""
    dx, dy = rest_edges(r)
    gx, gy = map_edges(F, UV)
    S = np.zeros((F.shape[0], 4))
    for i in range(3):
        wx, wy = r[:, 3 + i] * gx[:, i], r[:, 3 + i] * gy[:, i]
        S[:, 0] += wx * dx[:, i]
        S[:, 1] += wx * dy[:, i]
        S[:, 2] += wy * dx[:, i]
        S[:, 3] += wy * dy[:, i]
    return S


def rotations(S):
    """(cos, sin, h) of the closest rotation; the identity where h == 0 (param_rotation)"""
    a, b = S[:, 0] + S[:, 3], S[:, 2] - S[:, 1]
    h = np.sqrt(a * a + b * b)
    pos = h > 0.0
    safe = np.where(pos, h, 1.0)
    return np.where(pos, a / safe, 1.0), np.where(pos, b / safe, 0.0), h


def face_energy(r, F, UV, cs, sn):
    """(1/2) sum_i c_i |g_i - R d_i|^2 per face (param_face_energy)"""
    dx, dy = rest_edges(r)
    gx, gy = map_edges(F, UV)
    acc = np.zeros(F.shape[0])
    for i in range(3):
        ex = gx[:, i] - (cs * dx[:, i] - sn * dy[:, i])
        ey = gy[:, i] - (sn * dx[:, i] + cs * dy[:, i])
        acc += r[:, 3 + i] * (ex * ex + ey * ey)
    return 0.5 * acc


def rhs(r, F, nV, cs, sn):
    """nV x 2: per vertex the sum over its corners (faces ascending) of (1/2) R_f (c_i d_i - c_{i-1} d_{i-1}) (param_corner_rhs, k_param_rhs)"""
    dx, dy = rest_edges(r)
    share = np.zeros((3 * F.shape[0], 2))
    for i in range(3):
        m = (i + 2) % 3
        mx = r[:, 3 + i] * dx[:, i] - r[:, 3 + m] * dx[:, m]
        my = r[:, 3 + i] * dy[:, i] - r[:, 3 + m] * dy[:, m]
        share[i::3, 0] = 0.5 * (cs * mx - sn * my)
        share[i::3, 1] = 0.5 * (sn * mx + cs * my)
    b = np.zeros((nV, 2))
    for vs, ts in corner_lists(F, nV):
        b[vs] += share[ts]
    return b


def distortion(r, F, UV):
    """(J as nF x 2 x 2, det J, sigma1, sigma2) (param_distortion)"""
    u = UV[F]
    q1x, q1y = u[:, 1, 0] - u[:, 0, 0], u[:, 1, 1] - u[:, 0, 1]
    q2x, q2y = u[:, 2, 0] - u[:, 0, 0], u[:, 2, 1] - u[:, 0, 1]
    j00, j10 = q1x / r[:, 0], q1y / r[:, 0]
    j01, j11 = (q2x - j00 * r[:, 1]) / r[:, 2], (q2y - j10 * r[:, 1]) / r[:, 2]
    det = j00 * j11 - j01 * j10
    pa, pb, ma, mb = j00 + j11, j10 - j01, j00 - j11, j10 + j01
    Q, T = 0.5 * np.sqrt(pa * pa + pb * pb), 0.5 * np.sqrt(ma * ma + mb * mb)
    return np.stack([np.stack([j00, j01], axis=1), np.stack([j10, j11], axis=1)], axis=1), det, Q + T, np.abs(Q - T)


def dirichlet_matrix(r, F, nV):
    """-L from the rest triangles: (1/2) sum_f c_i on edge (i, i + 1), the row sums on the diagonal"""
    I, J, W = [], [], []
    for i in range(3):
        a, b, w = F[:, i], F[:, (i + 1) % 3], 0.5 * r[:, 3 + i]
        I += [a, b, a, b]
        J += [b, a, a, b]
        W += [-w, -w, w, w]
    K = sp.coo_matrix((np.concatenate(W), (np.concatenate(I), np.concatenate(J))), shape=(nV, nV)).tocsr()
    K.sum_duplicates()
    K.sort_indices()
    return K


def mesh_area(V, F):
    """half the sum of the faces' double areas, summed in face order (check_mesh)"""
    u, v = V[F[:, 1]] - V[F[:, 0]], V[F[:, 2]] - V[F[:, 0]]
    wx, wy, wz = u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1], u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2], u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]
    return 0.5 * float(np.cumsum(np.sqrt(wx * wx + wy * wy + wz * wz))[-1])


def circle(V, loop, area):
    """the loop on the circle of that area by cumulative 3D edge length from angle 0 (libm's cos / sin, as the library's host code)"""
    def d(a, b):
        x, y, z = (float(V[a, k]) - float(V[b, k]) for k in range(3))
        return math.sqrt(x * x + y * y + z * z)
    ln = [0.0]
    for i in range(1, len(loop)):
        ln.append(ln[-1] + d(loop[i - 1], loop[i]))
    total = ln[-1] + d(loop[-1], loop[0])
    pi = 3.141592653589793
    radius = math.sqrt(area / pi)
    return np.array([[radius * math.cos(x * (2.0 * pi) / total), radius * math.sin(x * (2.0 * pi) / total)] for x in ln])


class ParamNp:
    """the restatement with direct solves: -L with the loop known (harmonic) and with loop[0] known (global step), each factored once"""

    def __init__(self, V, F):
        self.V, self.F, self.nV = np.ascontiguousarray(V, dtype=np.float64), np.ascontiguousarray(F, dtype=np.int32), V.shape[0]
        self.r = rest_constants(self.V, self.F)
        self.K = (-M.cotmatrix(self.V, self.F)).tocsr()            # the system the library assembles
        self.loop = M.boundary_loop(self.F)
        self.area = float(np.sum(0.5 * (self.r[:, 0] * self.r[:, 2])))
        self._lu = {}

    def _solver(self, known):
        key = len(known)
        if key not in self._lu:
            mask = np.ones(self.nV, dtype=bool)
            mask[known] = False
            unk = np.nonzero(mask)[0]
            self._lu[key] = (unk, spla.splu(self.K[unk][:, unk].tocsc()), self.K[unk][:, known].tocsr())
        return self._lu[key]

    def scale(self):
        """s = sqrt(sum_v (sum over v's corners of (1/2) (|c_i| |d_i| + |c_{i-1}| |d_{i-1}|))^2)"""
        dx, dy = rest_edges(self.r)
        w = np.abs(self.r[:, 3:6]) * np.sqrt(dx * dx + dy * dy)
        bound = np.zeros(3 * self.F.shape[0])
        for i in range(3):
            bound[i::3] = 0.5 * (w[:, i] + w[:, (i + 2) % 3])
        row = np.zeros(self.nV)
        for vs, ts in corner_lists(self.F, self.nV):
            row[vs] += bound[ts]
        return float(np.sqrt(np.sum(row * row)))

    def harmonic(self):
        ub = circle(self.V, self.loop, mesh_area(self.V, self.F))
        unk, lu, Kuk = self._solver(self.loop)
        U = np.zeros((self.nV, 2))
        U[self.loop] = ub
        U[unk] = lu.solve(-(Kuk @ ub))
        return U

    def harmonic_scale(self):
        ub = circle(self.V, self.loop, mesh_area(self.V, self.F))
        return float(np.linalg.norm(self._solver(self.loop)[2] @ ub))

    def local(self, U):
        cs, sn, _ = rotations(covariance(self.r, self.F, U))
        return cs, sn, float(np.sum(face_energy(self.r, self.F, U, cs, sn)))

    def step(self, U):
        """one iteration: (U_{t+1}, E_t)"""
        cs, sn, E = self.local(U)
        b = rhs(self.r, self.F, self.nV, cs, sn)
        pin = self.loop[:1]
        unk, lu, Kuk = self._solver(pin)
        Un = U.copy()
        Un[unk] = lu.solve(b[unk] - Kuk @ U[pin])
        return Un, E

    def run(self, U0=None, n_iter=10):
        """returns (U, energy_his with n_iter + 1 entries, the iterates U_0 .. U_n_iter)"""
        U = self.harmonic() if U0 is None else np.array(U0, dtype=np.float64)
        E, its = [], [U.copy()]
        for _ in range(n_iter):
            U, e = self.step(U)
            E.append(e)
            its.append(U.copy())
        E.append(self.local(U)[2])
        return U, np.array(E), its

    def flipped(self, U):
        return int(np.sum(distortion(self.r, self.F, U)[1] <= 0.0))


def load_mesh(name):
    V, F = M.read_smgm(name)
    return M.normalize_unit_area(V, F), F


@functools.lru_cache(maxsize=None)
def reference_run(name, n_iter=10):
    """(ParamNp, U, energy_his, iterates) of the restatement on a fixture, computed once per session and left unchanged by its users"""
    V, F = load_mesh(name)
    P = ParamNp(V, F)
    U, E, its = P.run(n_iter=n_iter)
    for a in [U, E] + its:
        a.setflags(write=False)
    return P, U, E, its


def euler_characteristic(F, nV):
    e = np.sort(np.concatenate([F[:, [0, 1]], F[:, [1, 2]], F[:, [2, 0]]]), axis=1)
    return nV - np.unique(e, axis=0).shape[0] + F.shape[0]


# ---- the restatement itself -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(TABLE))
def test_energy_never_rises_and_reproduces_the_table(name):
    nV, n_loop, E0, E1, E10, flips = TABLE[name]
    P, U, E, _ = reference_run(name)
    h = rotations(covariance(P.r, P.F, U))[2]
    print(name, "E", np.array2string(E, precision=5), "flipped %d, fit radius min / max %.1e, negative cotangents %.1f %%"
          % (P.flipped(U), h.min() / h.max(), 100.0 * np.mean(P.r[:, 3:6] < 0)))
    assert P.nV == nV and len(P.loop) == n_loop and euler_characteristic(P.F, nV) == 1
    assert np.all(np.isfinite(E)) and np.all(E[1:] <= E[:-1])               # exact solves: the energy never rises
    for got, want in ((E[0], E0), (E[1], E1), (E[10], E10)):
        assert abs(got / want - 1.0) <= 5e-4                                # the table's figures, to 4 digits
    assert P.flipped(U) == flips


def test_the_refusal_fixtures_are_not_disks():
    for name, chi in (("bunny_15K_init.smgm", 2), ("hilbert_cube_known.smgm", 0)):
        V, F = M.read_smgm(name)
        assert euler_characteristic(F, V.shape[0]) == chi


def rigid_2d(P2, angle=0.7, shift=(0.3, -1.1)):
    c, s = math.cos(angle), math.sin(angle)
    return P2 @ np.array([[c, -s], [s, c]]).T + np.asarray(shift)


def test_isometry_is_a_fixed_point():
    V, F = flat_square()
    P = ParamNp(V, F)
    U0 = rigid_2d(V[:, :2])
    diag = float(np.linalg.norm(U0.max(axis=0) - U0.min(axis=0)))
    U1, E0 = P.step(U0)
    _, det, s1, s2 = distortion(P.r, P.F, U0)
    print("flat square: E_0 %.2e (area %.3f), step %.2e diagonals, |sigma - 1| %.2e"
          % (E0, P.area, np.abs(U1 - U0).max() / diag, max(np.abs(s1 - 1).max(), np.abs(s2 - 1).max())))
    assert E0 <= 1e-24 * P.area
    assert np.abs(U1 - U0).max() <= 1e-12 * diag
    assert np.abs(s1 - 1.0).max() <= 1e-13 and np.abs(s2 - 1.0).max() <= 1e-13 and np.all(det > 0.0)


def test_rolled_onto_a_cylinder_keeps_the_rest_triangles():
    """The rest triangle depends on the 3D triangle's shape alone.  Rolling the VERTICES onto a cylinder is an isometry of the plane but not
    of its triangulation -- an edge of length l across the axis becomes a chord, shorter by l theta^2 / 24 with theta = l / radius -- so the
    radius is chosen for the bound: l <= 0.08 on this mesh, and 0.08 (0.08 / radius)^2 / 24 <= 1e-14 from radius = 1e5 on (measured there:
    1.2e-15; at roll_onto_cylinder's default radius 0.5 the chords alone differ by 4.6e-5).  A rigid motion of the rolled mesh keeps the
    rest triangles too."""
    V, F = flat_square()
    r0 = rest_constants(V, F)
    W = roll_onto_cylinder(V, radius=1e5)
    r1 = rest_constants(W, F)
    print("rest constants, flat against rolled: %.2e" % np.abs(r1[:, :3] - r0[:, :3]).max())
    assert np.abs(r1[:, :3] - r0[:, :3]).max() <= 1e-13
    assert np.abs(r1[:, 3:] - r0[:, 3:]).max() <= 1e-13 * np.abs(r0[:, 3:]).max() / r0[:, 2].min()     # cotangents: divided by the smallest height
    from test_arap_host import rotation_matrix
    W2 = roll_onto_cylinder(V) @ rotation_matrix([1.0, 2.0, -0.5], 1.1).T + np.array([0.3, -0.2, 0.7])
    assert np.abs(rest_constants(W2, F)[:, :3] - rest_constants(roll_onto_cylinder(V), F)[:, :3]).max() <= 1e-13
    # and the rest triangle is isometric to the 3D triangle it came from
    r = rest_constants(W2, F)
    dx, dy = rest_edges(r)
    l3 = np.stack([np.linalg.norm(W2[F[:, i]] - W2[F[:, (i + 1) % 3]], axis=1) for i in range(3)], axis=1)
    assert np.abs(np.sqrt(dx * dx + dy * dy) - l3).max() <= 1e-13


def total_energy(r, F, UV, cs, sn):
    return float(np.sum(face_energy(r, F, UV, cs, sn)))


def test_rhs_is_the_energy_gradient():
    """rhs = -(1/2) dE/du + (-L) u at fixed R.  E is quadratic in u, so a central difference has no truncation error; its rounding error is
    about eps E / step = 2e-16 * 1 / 1e-3, far below the bound of 1e-8 |rhs|_max."""
    V, F = flat_square(6, seed=3)
    V = roll_onto_cylinder(V)
    rng = np.random.default_rng(5)
    P = ParamNp(V, F)
    U = V[:, :2] + 0.1 * rng.standard_normal((P.nV, 2))
    ang = rng.uniform(-np.pi, np.pi, F.shape[0])
    cs, sn = np.cos(ang), np.sin(ang)
    b = rhs(P.r, P.F, P.nV, cs, sn)
    K = dirichlet_matrix(P.r, P.F, P.nV)
    step, grad = 1e-3, np.zeros((P.nV, 2))
    for v in range(P.nV):
        for c in range(2):
            Up, Um = U.copy(), U.copy()
            Up[v, c] += step
            Um[v, c] -= step
            grad[v, c] = (total_energy(P.r, P.F, Up, cs, sn) - total_energy(P.r, P.F, Um, cs, sn)) / (2 * step)
    err = np.abs(b - (-0.5 * grad + K @ U)).max()
    print("rhs against the finite-difference gradient: %.2e of |rhs|_max" % (err / np.abs(b).max()))
    assert err <= 1e-8 * np.abs(b).max()


@pytest.mark.parametrize("name", sorted(TABLE))
def test_rest_triangle_weights_assemble_the_cotangent_matrix(name):
    V, F = load_mesh(name)
    K = dirichlet_matrix(rest_constants(V, F), F, V.shape[0])
    Kn = sp.csr_matrix(-M.cotmatrix(V, F))
    Kn.sort_indices()
    assert np.array_equal(K.indptr, Kn.indptr) and np.array_equal(K.indices, Kn.indices)
    # entry for entry.  An entry sums up to two cotangents per face pair; where two of opposite sign nearly cancel the entry itself is small
    # and the difference is measured against the magnitudes that meet in it (ogre.obj, 9.9 % negative cotangents: 2.4e-12 of the entry,
    # 1.3e-13 of the magnitudes); on the two meshes without such entries it is measured against the entry (6e-15 and 6e-13).
    mag = abs(dirichlet_matrix(np.abs(rest_constants(V, F)), F, V.shape[0]))
    rel = np.abs(K.data - Kn.data) / np.abs(Kn.data)
    rel_mag = np.abs(K.data - Kn.data) / mag.data
    print(name, "relative to the entry %.2e, to the magnitudes %.2e" % (rel.max(), rel_mag.max()))
    assert rel_mag.max() <= 1e-12
    if name != "ogre.smgm":
        assert rel.max() <= 1e-12


# ---- the ABI without a GPU ------------------------------------------------------------------------------------------------------------------
def _create(L, h, V, F, nV=None, null=None):
    out = C.c_void_p(1)
    V = np.ascontiguousarray(V, dtype=np.float64)
    F = np.ascontiguousarray(F, dtype=np.int32)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    rc = L.smg_param_create(None if null == "h" else h, None if null == "V" else V.ctypes.data_as(dp), V.shape[0] if nV is None else nV,
                            None if null == "F" else F.ctypes.data_as(ip), F.shape[0], None if null == "out" else C.byref(out))
    if rc == 0:
        L.smg_param_destroy(out)
        return rc, ""
    assert null == "out" or out.value is None, "a refused create must leave *out == NULL"
    return rc, L.smg_last_error().decode()


def refusal_cases(smg):
    """[(name, thunk -> (code, message), holds only without a device)]"""
    L = smg._lib.load()
    V, F = flat_square(8)
    V = roll_onto_cylinder(V)
    n = V.shape[0]
    keep = {"mg": smg.mg_precompute(V, F, 0.25, 20, 1), "blk": smg.mg_precompute_block(V, F, 0.25, 20, 1)}
    keep["un"] = smg.Hierarchy.union([keep["mg"], keep["mg"]])
    mg, fake = keep["mg"], _fake_hierarchy(smg, n)
    V2, F2 = np.concatenate([V, V + 3.0]), np.concatenate([F, F + n])
    cases = [("null %s" % a, (lambda a=a: _create(L, mg.h, V, F, null=a)), False) for a in ("h", "V", "F", "out")]
    cases.append(("block hierarchy", lambda: _create(L, keep["blk"].h, V, F), False))
    cases.append(("union", lambda: _create(L, keep["un"].h, V2, F2), False))
    cases.append(("rows", lambda: _create(L, mg.h, V[:-1], F, nV=n - 1), False))
    for name in ("bunny_15K_init.smgm", "hilbert_cube_known.smgm"):
        Vm, Fm = M.read_smgm(name)
        h = _fake_hierarchy(smg, Vm.shape[0])
        keep[name] = h
        cases.append(("closed mesh" if name.startswith("bunny") else "two loops", lambda Vm=Vm, Fm=Fm, h=h: _create(L, h.h, Vm, Fm), False))
    count = {}
    for a, b in np.concatenate([F[:, [0, 1]], F[:, [1, 2]], F[:, [2, 0]]]):
        count[(min(a, b), max(a, b))] = count.get((min(a, b), max(a, b)), 0) + 1
    inner = [f for f in range(F.shape[0]) if all(count[(min(F[f, i], F[f, (i + 1) % 3]), max(F[f, i], F[f, (i + 1) % 3]))] == 2 for i in range(3))][0]
    # a third face on an interior edge, with a new vertex
    Vx, Fx = np.concatenate([V, [V[F[inner, 0]] + [0.0, 0.0, 0.5]]]), np.concatenate([F, [[F[inner, 1], F[inner, 0], n]]])
    keep["nm"] = _fake_hierarchy(smg, n + 1)
    cases.append(("non-manifold edge", lambda: _create(L, keep["nm"].h, Vx, Fx), False))
    Ff = F.copy()
    Ff[inner] = Ff[inner, [1, 0, 2]]
    cases.append(("flipped face", lambda: _create(L, fake.h, V, Ff), False))
    Vz = V.copy()
    Vz[F[0, 1]] = Vz[F[0, 0]]
    cases.append(("zero area", lambda: _create(L, fake.h, Vz, F), False))
    Fo = F.copy()
    Fo[3, 2] = n
    cases.append(("face index", lambda: _create(L, fake.h, V, Fo), False))
    for tag, bad in (("nan", np.nan), ("inf", np.inf)):
        Vn = V.copy()
        Vn[F[F.shape[0] - 1, 0], 1] = bad
        cases.append(("%s coordinate" % tag, lambda Vn=Vn: _create(L, fake.h, Vn, F), False))
    keep["two"] = _fake_hierarchy(smg, 2 * n)
    cases.append(("two components", lambda: _create(L, keep["two"].h, V2, F2), False))
    Vt, Ft = np.array([[0.0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]]), np.array([[0, 1, 2], [0, 2, 3]], dtype=np.int32)
    keep["sq"] = _fake_hierarchy(smg, 4)
    cases.append(("all boundary", lambda: _create(L, keep["sq"].h, Vt, Ft), False))
    cases.append(("valid, real hierarchy", lambda: _create(L, mg.h, V, F), True))
    cases.append(("valid, fake hierarchy", lambda: _create(L, fake.h, V, F), True))
    return cases, keep


def test_abi_present(smg_mod):
    L = smg_mod._lib.load()
    for name in ("smg_param_create", "smg_param_destroy", "smg_param_set_solver", "smg_param_device_bytes", "smg_param_boundary",
                 "smg_param_harmonic", "smg_param_arap", "smg_param_distortion", "smg_debug_param"):
        assert hasattr(L, name)
    assert hasattr(smg_mod, "Parameterizer")
    assert L.smg_param_device_bytes(None) == 0
    assert L.smg_param_set_solver(None, 1) == INVALID
    n = C.c_int(0)
    assert L.smg_param_boundary(None, C.byref(n), None) == INVALID
    U, st = np.zeros(8), np.zeros(6)
    assert L.smg_param_harmonic(None, 0, None, U.ctypes.data, 4, None) == INVALID
    assert L.smg_param_arap(None, None, 0, 0, 1, 0.0, None, U.ctypes.data, 4, None, None, None) == INVALID
    assert L.smg_param_distortion(None, U.ctypes.data, 4, 0, None, st.ctypes.data_as(C.POINTER(C.c_double))) == INVALID


def test_create_refusals_keep_code_and_message(smg_mod):
    """every refusal of smg_param_create, with the code and the smg_last_error() text recorded in tests/golden/param_refusals.json"""
    L = smg_mod._lib.load()
    golden = json.load(open(GOLDEN))
    cases, keep = refusal_cases(smg_mod)
    no_device = L.smg_device_count() == 0
    seen = set()
    for name, thunk, device_only in cases:
        if device_only and not no_device:
            continue
        rc, msg = thunk()
        seen.add(name)
        assert [rc, msg] == golden[name], name
        assert rc == (NO_DEVICE if device_only else INVALID), name
    assert seen == set(golden) - (set() if no_device else {c[0] for c in cases if c[2]})
    assert len({golden[k][1] for k in ("closed mesh", "two loops", "non-manifold edge")}) == 3      # each has its own message
    del keep


def param_hook(L, op, nV, F, V0=None, UV=None, R_in=None, n_out=0):
    """one call of smg_debug_param; UV is nV x 2 (passed column-major), R_in (cos, sin) as two planes; returns (rc, guard hits, out)"""
    ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
    F = np.ascontiguousarray(F, dtype=np.int32)
    keep = [None if V0 is None else np.ascontiguousarray(V0, dtype=np.float64),
            None if UV is None else np.ascontiguousarray(np.asarray(UV, dtype=np.float64).T),
            None if R_in is None else np.ascontiguousarray(np.concatenate([R_in[0], R_in[1]]), dtype=np.float64)]
    arr = lambda a: None if a is None else a.ctypes.data_as(dp)   # noqa: E731
    out = np.full(max(n_out, 1), np.nan)
    bad = C.c_int(-1)
    rc = L.smg_debug_param(op, nV, F.shape[0], F.ctypes.data_as(ip), arr(keep[0]), arr(keep[1]), arr(keep[2]), out.ctypes.data_as(dp) if n_out else None,
                           C.byref(bad))
    return rc, bad.value, out


def test_hook_refusals(smg_mod):
    L = smg_mod._lib.load()
    V, F = flat_square(4)
    n, nF = V.shape[0], F.shape[0]
    UV, R = V[:, :2].copy(), (np.ones(nF), np.zeros(nF))
    assert param_hook(L, 7, n, F, V, UV, R, 6 * nF)[0] == INVALID                     # unknown op
    assert param_hook(L, -1, n, F, V, UV, R, 6 * nF)[0] == INVALID
    assert param_hook(L, PARAM_REST, n, F, None, UV, R, 6 * nF)[0] == INVALID          # V0 missing
    assert param_hook(L, PARAM_COVARIANCE, n, F, V, None, R, 4 * nF)[0] == INVALID     # UV missing
    assert param_hook(L, PARAM_DISTORTION, n, F, V, None, R, 3 * nF)[0] == INVALID
    assert param_hook(L, PARAM_RHS, n, F, V, UV, None, 2 * n)[0] == INVALID            # R_in missing
    assert param_hook(L, PARAM_ENERGY, n, F, V, UV, None, 1)[0] == INVALID
    assert param_hook(L, PARAM_ROTATIONS, n, F, V, UV, R, 0)[0] == INVALID             # out missing
    for bad in (n, -1):                                                                # a face index out of range
        Fo = F.copy()
        Fo[2, 1] = bad
        assert param_hook(L, PARAM_REST, n, Fo, V, UV, R, 6 * nF)[0] == INVALID
    if L.smg_device_count() == 0:
        assert param_hook(L, PARAM_REST, n, F, V, UV, R, 6 * nF)[0] == NO_DEVICE
        assert param_hook(L, PARAM_ENERGY, n, F, V, UV, R, 1)[0] == NO_DEVICE


def test_host_and_numpy_agree_on_the_default_scale(smg_mod):
    """the restatement's scale is the expression the library evaluates on the host (same text as the device's, smg_param_inl.hpp): both are
    sums of non-negative terms in the same order"""
    V, F = load_mesh("ogre_sim.smgm")
    P = ParamNp(V, F)
    assert P.scale() > 0 and np.isfinite(P.scale()) and P.harmonic_scale() > 0


def test_face_kernels_keep_everything_in_registers():
    """the ISA notes of k_param_local and k_param_distortion (the build's flags, device side only): no scratch, no spills"""
    import re
    import subprocess
    from surface_multigrid_code_amd import build as B
    src = os.path.join(B.CSRC, "smg_param_device.hip")
    asm = subprocess.check_output([B._hipcc()] + B.FLAGS + ["--cuda-device-only", "-S", src, "-o", "-"], text=True)
    for pattern in (r"k_param_localILi1E", r"k_param_distortionE"):
        notes = re.findall(r"\.name:\s+(\S*%s\S*)(.*?)\.wavefront_size" % pattern, asm, flags=re.S)
        assert len(notes) == 1
        body = notes[0][1]
        field = lambda k: int(re.search(r"\.%s:\s+(\d+)" % k, body).group(1))   # noqa: E731
        print("%s: vgpr_count %d, private_segment_fixed_size %d, vgpr_spill_count %d"
              % (pattern, field("vgpr_count"), field("private_segment_fixed_size"), field("vgpr_spill_count")))
        assert field("private_segment_fixed_size") == 0 and field("vgpr_spill_count") == 0
        assert field("vgpr_count") <= 64          # 512 / 64 = 8 waves per SIMD (56 and 35)
