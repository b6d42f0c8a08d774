"""CPU: as-rigid-as-possible deformation (include/smg.h: smg_arap_*) -- the ABI and its refusals without a GPU, and the numpy / scipy
restatement of the method (LAPACK SVDs, direct solves) that tests/test_gpu_arap.py checks the device against.  The restatement follows the
kernels of csrc/smg_arap_device.hip operation by operation (covariance, energy terms and right-hand side in the row's stored order)."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from oracle import mesh_np as M
from test_geodesics_host import flat_square, icosphere

INVALID, NO_DEVICE = -1, -2
ARAP_COVARIANCE, ARAP_ROTATIONS, ARAP_RHS, ARAP_VERTEX_ENERGY, ARAP_ENERGY = 0, 1, 2, 3, 4


# ---- the deformation every test uses --------------------------------------------------------------------------------------------------------
def twist(V, angle_deg=60.0, shift=0.15, share=0.05):
    """handles = the lowest and the highest 5 % of the vertices along the longest bounding-box axis (bottom first); the top set is rotated by
    60 degrees about that axis (through the box centre) and shifted along it by 15 % of the extent.  Returns (handles, handle_pos)."""
    lo, hi = V.min(axis=0), V.max(axis=0)
    ax = int(np.argmax(hi - lo))
    order = np.argsort(V[:, ax], kind="stable")
    m = max(1, int(round(share * V.shape[0])))
    bottom, top = order[:m], order[-m:]
    u, v = (ax + 1) % 3, (ax + 2) % 3
    c, s = np.cos(np.deg2rad(angle_deg)), np.sin(np.deg2rad(angle_deg))
    ctr = 0.5 * (lo + hi)
    T = V[top].copy()
    du, dv = V[top, u] - ctr[u], V[top, v] - ctr[v]
    T[:, u] = ctr[u] + c * du - s * dv
    T[:, v] = ctr[v] + s * du + c * dv
    T[:, ax] += shift * (hi - lo)[ax]
    return np.concatenate([bottom, top]).astype(np.int32), np.concatenate([V[bottom], T])


def rotation_matrix(axis, angle):
    """Rodrigues: the rotation by `angle` about `axis`"""
    a = np.asarray(axis, dtype=np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def bbox_diag(V):
    return float(np.linalg.norm(V.max(axis=0) - V.min(axis=0)))


# ---- the method in numpy (the kernels' expressions, in their order) ---------------------------------------------------------------------------
class ArapRest:
    """the CSR of L (rowptr, col, w; diagonal entries skipped) and the rest positions; slot p of every row that has one, for sequential sums"""

    def __init__(self, L, P0):
        L = sp.csr_matrix(L)
        L.sort_indices()
        self._set(L.indptr, L.indices, L.data, P0)
        self.L = L

    @classmethod
    def from_csr(cls, rowptr, col, w, P0):
        """the rest data of a hand-made CSR, entries in the order given (rows may be empty, unsorted, or hold their diagonal anywhere)"""
        A = cls.__new__(cls)
        A._set(rowptr, col, w, P0)
        A.L = None
        return A

    def _set(self, rowptr, col, w, P0):
        self.n = len(rowptr) - 1
        self.rowptr = np.ascontiguousarray(rowptr, dtype=np.int32)
        self.col = np.ascontiguousarray(col, dtype=np.int32)
        self.w = np.ascontiguousarray(w, dtype=np.float64)
        self.P0 = np.ascontiguousarray(P0, dtype=np.float64)
        row = np.repeat(np.arange(self.n), np.diff(self.rowptr))
        q = np.nonzero(self.col != row)[0]
        r = row[q]
        rank = np.arange(q.size) - np.searchsorted(r, np.arange(self.n))[r]
        self.slots = [(r[rank == p], q[rank == p]) for p in range(int(rank.max()) + 1)]
        self.deg = np.bincount(r, minlength=self.n)

    def scale(self):
        """s = sqrt(sum_i (sum_j |w_ij| |e_ij|)^2): |b|_F <= s for every set of rotations"""
        row = np.zeros(self.n)
        for rows, qs in self.slots:
            row[rows] += np.abs(self.w[qs]) * np.linalg.norm(self.P0[rows] - self.P0[self.col[qs]], axis=1)
        return float(np.sqrt(np.sum(row * row)))


def covariance(A, P):
    """S_i = sum_j (w_ij e_ij) e'_ij^T, entry (a, c) += (w e_a) e'_c in stored order (k_arap_rotations)"""
    S = np.zeros((A.n, 3, 3))
    for rows, qs in A.slots:
        j = A.col[qs]
        e, d = A.P0[rows] - A.P0[j], P[rows] - P[j]
        we = A.w[qs, None] * e
        S[rows] += we[:, :, None] * d[:, None, :]
    return S


def rotations_np(S):
    """R = V D U^T of S = U Sigma V^T (LAPACK), D = diag(1, 1, det(V U^T)); S == 0: the identity.  Returns (R, gap, d) with
    gap = (sigma_2 + d sigma_3) / sigma_1 (0 where S == 0)."""
    U, s, Vt = np.linalg.svd(S)
    d = np.where(np.linalg.det(np.einsum("nji,nkj->nik", Vt, U)) < 0, -1.0, 1.0)
    D = np.ones_like(s)
    D[:, 2] = d
    R = np.einsum("nji,nj,nkj->nik", Vt, D, U)
    zero = s[:, 0] == 0.0
    R[zero] = np.eye(3)
    gap = np.where(zero, 0.0, (s[:, 1] + d * s[:, 2]) / np.where(zero, 1.0, s[:, 0]))
    return R, gap, d


def vertex_energy(A, P, R):
    """sum_j w_ij |e'_ij - R_i e_ij|^2 in stored order (k_arap_rotations, second walk)"""
    out = np.zeros(A.n)
    for rows, qs in A.slots:
        j = A.col[qs]
        e, Ri = A.P0[rows] - A.P0[j], R[rows]
        ex, ey, ez = e[:, 0], e[:, 1], e[:, 2]
        dx = (P[rows, 0] - P[j, 0]) - (Ri[:, 0, 0] * ex + Ri[:, 0, 1] * ey + Ri[:, 0, 2] * ez)
        dy = (P[rows, 1] - P[j, 1]) - (Ri[:, 1, 0] * ex + Ri[:, 1, 1] * ey + Ri[:, 1, 2] * ez)
        dz = (P[rows, 2] - P[j, 2]) - (Ri[:, 2, 0] * ex + Ri[:, 2, 1] * ey + Ri[:, 2, 2] * ez)
        out[rows] += A.w[qs] * (dx * dx + dy * dy + dz * dz)
    return out


def rhs(A, R):
    """b_i = sum_j (w_ij / 2) (R_i + R_j) e_ij in stored order (k_arap_rhs); n x 3"""
    b = np.zeros((A.n, 3))
    for rows, qs in A.slots:
        j = A.col[qs]
        e, Mx = A.P0[rows] - A.P0[j], R[rows] + R[j]
        ex, ey, ez = e[:, 0], e[:, 1], e[:, 2]
        h = A.w[qs] * 0.5
        for c in range(3):
            b[rows, c] += h * (Mx[:, c, 0] * ex + Mx[:, c, 1] * ey + Mx[:, c, 2] * ez)
    return b


class ArapNp:
    """the restatement with direct solves: (-L)_uu factored once, one local / global step per iteration"""

    def __init__(self, L, P0, handles):
        self.A = ArapRest(L, P0)
        self.handles = np.asarray(handles, dtype=np.int64)
        mask = np.ones(self.A.n, dtype=bool)
        mask[self.handles] = False
        self.unknown = np.nonzero(mask)[0]
        K = (-self.A.L).tocsr()
        self.lu = spla.splu(K[self.unknown][:, self.unknown].tocsc())
        self.Kuk = K[self.unknown][:, self.handles].tocsr()

    def start(self, handle_pos, U0=None):
        U = (self.A.P0 if U0 is None else np.asarray(U0, dtype=np.float64)).copy()
        U[self.handles] = handle_pos
        return U

    def local(self, U):
        R, _, _ = rotations_np(covariance(self.A, U))
        return R, float(np.sum(vertex_energy(self.A, U, R)))

    def run(self, handle_pos, U0=None, n_iter=10):
        """returns (U, energy_his with n_iter + 1 entries, the iterates U_0 .. U_n_iter)"""
        U = self.start(handle_pos, U0)
        E, its = [], [U.copy()]
        for _ in range(n_iter):
            R, e = self.local(U)
            E.append(e)
            b = rhs(self.A, R)
            Un = U.copy()
            Un[self.unknown] = self.lu.solve(b[self.unknown] - self.Kuk @ handle_pos)
            U = Un
            its.append(U.copy())
        E.append(self.local(U)[1])
        return U, np.array(E), its


def load_mesh(name):
    if name == "icosphere5":
        return icosphere(5)
    if name == "torus":
        return M.torus(96, 48)
    V, F = M.read_smgm(name)
    return M.normalize_unit_area(V, F), F


# ---- the restatement itself -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["bunny.smgm", "icosphere5", "torus"])
def test_energy_does_not_increase(name):
    V, F = load_mesh(name)
    handles, hp = twist(V)
    _, E, _ = ArapNp(M.cotmatrix(V, F), V, handles).run(hp, n_iter=10)
    drops = (E[:-1] - E[1:]) / E[:-1]
    print(name, "E_0 %.4e, relative drops" % E[0], np.array2string(drops, precision=3))
    assert np.all(np.isfinite(E)) and E[0] > 0
    assert np.all(E[1:] <= E[:-1])          # exact solves: the energy never increases


@pytest.mark.parametrize("name", ["icosphere5", "torus", "bunny.smgm"])
def test_rigid_image_is_a_fixed_point(name):
    V, F = load_mesh(name)
    Q = rotation_matrix([1.0, 2.0, -0.5], 1.1)
    t = np.array([0.3, -0.2, 0.7])
    rigid = V @ Q.T + t
    handles, _ = twist(V)
    arap = ArapNp(M.cotmatrix(V, F), V, handles)
    R, E0 = arap.local(rigid)
    U, E, _ = arap.run(rigid[handles], U0=rigid, n_iter=2)
    diag = bbox_diag(V)
    E_twist = arap.local(arap.start(twist(V)[1]))[1]
    print(name, "|R - Q| %.2e, step %.2e diagonals, E %.2e (twist %.2e)" % (np.abs(R - Q).max(), np.abs(U - rigid).max() / diag, E.max(), E_twist))
    assert np.abs(R - Q).max() <= 1e-12        # measured 1.3e-14
    assert np.abs(U - rigid).max() <= 1e-12 * diag
    assert E.max() <= 1e-20 * E_twist


def test_reflection_branch_and_flat_patch():
    """the twist sends some covariances through D = diag(1, 1, -1); a flat rest pose has rank-2 covariances, sigma_3 == 0"""
    V, F = load_mesh("bunny.smgm")
    handles, hp = twist(V)
    arap = ArapNp(M.cotmatrix(V, F), V, handles)
    _, gap, d = rotations_np(covariance(arap.A, arap.start(hp)))
    assert 0 < np.mean(d < 0) < 0.05 and gap.min() > 1e-3
    V, F = flat_square()
    A = ArapRest(M.cotmatrix(V, F), V)
    S = covariance(A, roll_onto_cylinder(V))
    assert np.all(S[:, 2, :] == 0.0)                                  # every rest edge has a zero z component
    R, gap, d = rotations_np(S)
    print("flat square on a cylinder: min gap %.3f, reflection share %.2f" % (gap.min(), np.mean(d < 0)))
    assert np.all(np.linalg.svd(S, compute_uv=False)[:, 2] <= 1e-15 * np.abs(S).max()) and gap.min() > 1e-3 and np.all(np.isfinite(R))


def roll_onto_cylinder(V, radius=0.5):
    """the plane z = 0 rolled onto the cylinder of that radius about the y direction"""
    a = V[:, 0] / radius
    return np.stack([radius * np.sin(a), V[:, 1], radius * (1.0 - np.cos(a))], axis=1)


# ---- the ABI without a GPU ------------------------------------------------------------------------------------------------------------------
def _create(L, h, V, F, handles, nV=None, n_handles=None):
    out = C.c_void_p(1)
    V = np.ascontiguousarray(V, dtype=np.float64)
    F = np.ascontiguousarray(F, dtype=np.int32)
    handles = np.ascontiguousarray(handles, dtype=np.int32)
    rc = L.smg_arap_create(h, V.ctypes.data_as(C.POINTER(C.c_double)), V.shape[0] if nV is None else nV, F.ctypes.data_as(C.POINTER(C.c_int)),
                           F.shape[0], handles.ctypes.data_as(C.POINTER(C.c_int)), handles.shape[0] if n_handles is None else n_handles,
                           C.byref(out))
    if rc == 0:
        L.smg_arap_destroy(out)
    else:
        assert out.value is None, "a refused create must leave *out == NULL"
        assert len(L.smg_last_error()) > 0
    return rc


def _fake_hierarchy(smg, n):
    """a 2-level handle whose level 0 has n rows: the create checks read nothing else of it"""
    H = smg.Hierarchy(2)
    H.set_prolong(1, sp.csr_matrix(np.ones((n, 1))))
    return H


def test_abi_present(smg_mod):
    L = smg_mod._lib.load()
    for name in ("smg_arap_create", "smg_arap_destroy", "smg_arap_set_solver", "smg_arap_device_bytes", "smg_arap_solve", "smg_debug_arap"):
        assert hasattr(L, name)
    assert hasattr(smg_mod, "ArapDeformer")
    assert L.smg_arap_device_bytes(None) == 0
    assert L.smg_arap_set_solver(None, 1) == INVALID
    hp = np.zeros(3)
    U = np.zeros(12)
    assert L.smg_arap_solve(None, hp.ctypes.data, 1, None, 0, 0, 1, 0.0, None, U.ctypes.data, 4, None, None, None) == INVALID


def test_create_refusals(smg_mod):
    smg = smg_mod
    L = smg._lib.load()
    V, F = icosphere(3)
    n = V.shape[0]
    hd = np.array([0, 5, 9], dtype=np.int32)
    mg = smg.mg_precompute(V, F, 0.25, 50, 1)
    assert _create(L, None, V, F, hd) == INVALID                                     # null arguments
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    out = C.c_void_p()
    assert L.smg_arap_create(mg.h, None, n, F.ctypes.data_as(ip), F.shape[0], hd.ctypes.data_as(ip), 3, C.byref(out)) == INVALID
    assert L.smg_arap_create(mg.h, V.ctypes.data_as(dp), n, None, F.shape[0], hd.ctypes.data_as(ip), 3, C.byref(out)) == INVALID
    assert L.smg_arap_create(mg.h, V.ctypes.data_as(dp), n, F.ctypes.data_as(ip), F.shape[0], None, 3, C.byref(out)) == INVALID
    assert L.smg_arap_create(mg.h, V.ctypes.data_as(dp), n, F.ctypes.data_as(ip), F.shape[0], hd.ctypes.data_as(ip), 3, None) == INVALID
    assert _create(L, mg.h, V, F, hd, n_handles=0) == INVALID                        # n_handles < 1
    assert _create(L, mg.h, V, F, [0, n]) == INVALID                                 # a handle out of range
    assert _create(L, mg.h, V, F, [-1, 3]) == INVALID
    assert _create(L, mg.h, V, F, [4, 7, 4]) == INVALID                              # a repeated handle
    assert _create(L, mg.h, V[:-1], F, hd, nV=n - 1) == INVALID                      # nV != rows of level 0
    blk = smg.mg_precompute_block(V, F, 0.25, 50, 1)                                 # block (3-DOF) hierarchy, with and without the row match
    assert _create(L, blk.h, V, F, hd) == INVALID
    V3 = np.concatenate([V, V + 3.0, V + 6.0])
    F3 = np.concatenate([F, F + n, F + 2 * n])
    assert _create(L, blk.h, V3, F3, hd) == INVALID
    un = smg.Hierarchy.union([mg, mg])                                               # union handle
    V2, F2 = np.concatenate([V, V + 3.0]), np.concatenate([F, F + n])
    assert _create(L, un.h, V2, F2, hd) == INVALID
    two = _fake_hierarchy(smg, 2 * n)                                                # two connected components
    assert _create(L, two.h, V2, F2, hd) == INVALID
    iso = _fake_hierarchy(smg, n + 1)                                                # a vertex in no face
    assert _create(L, iso.h, np.concatenate([V, [[5.0, 5.0, 5.0]]]), F, hd) == INVALID
    fake = _fake_hierarchy(smg, n)
    Vz = V.copy()
    Vz[F[0, 1]] = Vz[F[0, 0]]                                                        # a face with zero double area
    assert _create(L, fake.h, Vz, F, hd) == INVALID
    Fo = F.copy()
    Fo[3, 2] = n                                                                     # a face index out of range
    assert _create(L, fake.h, V, Fo, hd) == INVALID
    for bad in (np.nan, np.inf):                                                     # a non-finite coordinate (of a vertex far from face 0)
        Vn = V.copy()
        Vn[n - 1, 1] = bad
        assert _create(L, fake.h, Vn, F, hd) == INVALID
    if L.smg_device_count() == 0:
        assert _create(L, mg.h, V, F, hd) == NO_DEVICE                               # valid arguments: the device is what is missing
        assert _create(L, fake.h, V, F, [n - 1]) == NO_DEVICE


def arap_hook(L, op, A, P=None, R_in=None, out=None, rowptr=None, col=None):
    """one call of smg_debug_arap on the rest data A (ArapRest); returns (rc, guard_hits)"""
    ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
    arr = lambda a, t: None if a is None else a.ctypes.data_as(t)   # noqa: E731
    bad = C.c_int(-1)
    rowptr = A.rowptr if rowptr is None else rowptr
    col = A.col if col is None else col
    rc = L.smg_debug_arap(op, A.n, arr(rowptr, ip), arr(col, ip), arr(A.w, dp), arr(A.P0, dp), arr(P, dp), arr(R_in, dp), arr(out, dp), C.byref(bad))
    return rc, bad.value


def test_hook_refusals(smg_mod):
    L = smg_mod._lib.load()
    V, F = icosphere(1)
    A = ArapRest(M.cotmatrix(V, F), V)
    n = A.n
    P, R, out = np.ascontiguousarray(V * 1.5), np.tile(np.eye(3).ravel(), n), np.zeros(9 * n)
    assert arap_hook(L, 5, A, P, R, out)[0] == INVALID                               # unknown op
    assert arap_hook(L, -1, A, P, R, out)[0] == INVALID
    assert arap_hook(L, ARAP_COVARIANCE, A, None, R, out)[0] == INVALID              # P missing
    assert arap_hook(L, ARAP_RHS, A, P, None, out)[0] == INVALID                     # R_in missing
    assert arap_hook(L, ARAP_ROTATIONS, A, P, R, None)[0] == INVALID                 # out missing
    cb = A.col.copy()
    cb[3] = n
    assert arap_hook(L, ARAP_COVARIANCE, A, P, R, out, col=cb)[0] == INVALID          # a column out of range
    pb = A.rowptr.copy()
    pb[2] = pb[1] - 1
    assert arap_hook(L, ARAP_COVARIANCE, A, P, R, out, rowptr=pb)[0] == INVALID       # row pointers not monotone
    if L.smg_device_count() == 0:
        assert arap_hook(L, ARAP_COVARIANCE, A, P, R, out)[0] == NO_DEVICE
        assert arap_hook(L, ARAP_ENERGY, A, P, R, out)[0] == NO_DEVICE


def test_library_weights_are_the_restatement_s(smg_mod):
    """smg_mesh_cotmatrix (== smg_assemble's L) has the pattern the restatement walks; values agree with the numpy cotangent matrix to rounding"""
    V, F = load_mesh("bunny.smgm")
    Ll = smg_mod.mesh.cotmatrix(V, F)
    Ln = sp.csr_matrix(M.cotmatrix(V, F))
    Ln.sort_indices()
    assert np.array_equal(Ll.indptr, Ln.indptr) and np.array_equal(Ll.indices, Ln.indices)
    assert np.abs(Ll.data - Ln.data).max() <= 1e-9 * np.abs(Ln.data).max()


def test_rotations_kernel_keeps_everything_in_registers():
    """the ISA notes of k_arap_rotations (the build's flags, device side only): no scratch, no spills, and a VGPR count that leaves 5 waves per SIMD"""
    import os
    import re
    import subprocess
    from surface_multigrid_code_amd import build as B
    src = os.path.join(B.CSRC, "smg_arap_device.hip")
    asm = subprocess.check_output([B._hipcc()] + B.FLAGS + ["--cuda-device-only", "-S", src, "-o", "-"], text=True)
    notes = re.findall(r"\.name:\s+(\S*k_arap_rotationsILi1E\S*)(.*?)\.wavefront_size", asm, flags=re.S)
    assert len(notes) == 1
    body = notes[0][1]
    field = lambda k: int(re.search(r"\.%s:\s+(\d+)" % k, body).group(1))   # noqa: E731
    print("k_arap_rotations: vgpr_count %d, private_segment_fixed_size %d, vgpr_spill_count %d"
          % (field("vgpr_count"), field("private_segment_fixed_size"), field("vgpr_spill_count")))
    assert field("private_segment_fixed_size") == 0 and field("vgpr_spill_count") == 0
    assert field("vgpr_count") <= 96          # 512 / 96 = 5 waves per SIMD (86)
