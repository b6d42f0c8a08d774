"""CPU: host-side C++ of libsmg (mesh numerics, Galerkin / constraint elimination, colour ordering, mg_precompute)
against the numpy restatement and the C oracle.  No GPU compute is called: smg_precompute runs its host half,
then reports SMG_ERR_NO_DEVICE, after which the host matrices can still be inspected."""
import os

import numpy as np
import pytest
import scipy.sparse as sp

from oracle import mesh_np as M
from problems import subdiv_problem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _host_precompute(smg, mg, A, known=None):
    try:
        mg.precompute(A, known)
    except smg.SmgError as e:
        assert e.code == -2      # expected on a box without GPU: host half done
    return mg


def test_mesh_numerics_match_numpy(smg_mod):
    mesh = smg_mod.mesh
    for name in ("ogre_sim.smgm", "bunny.smgm"):
        V, F = mesh.read_triangle_mesh(name)
        V2, F2 = M.read_smgm(name)
        assert np.array_equal(V, V2) and np.array_equal(F, F2)
        Vn, Vn2 = mesh.normalize_unit_area(V, F), M.normalize_unit_area(V2, F2)
        np.testing.assert_allclose(Vn, Vn2, atol=1e-14)
        assert abs(M.doublearea(Vn, F).sum() / 2 - 1.0) < 1e-12
        L, L2 = mesh.cotmatrix(Vn, F), M.cotmatrix(Vn2, F2)
        assert L.nnz == L2.nnz and abs(L - L2).max() < 1e-11 * abs(L2).max()
        assert abs(L - L.T).max() < 1e-12 * abs(L).max()                      # symmetric
        assert abs(np.asarray(L.sum(axis=1))).max() < 1e-9 * abs(L).max()     # rows sum to zero
        for kind in ("voronoi", "barycentric"):
            m, m2 = mesh.massmatrix(Vn, F, kind).diagonal(), M.massmatrix(Vn2, F2, kind).diagonal()
            np.testing.assert_allclose(m, m2, rtol=1e-12)
            assert abs(m.sum() - 1.0) < 1e-12                                   # sum M_ii = area = 1
        b, b2 = mesh.boundary_loop(F), M.boundary_loop(F2)
        assert len(b) == len(b2) and set(b) == set(b2)
        S, NF = mesh.midpoint_upsample(V.shape[0], F)
        S2, NF2 = M.midpoint_upsample(V2.shape[0], F2)
        assert abs(S - S2).max() == 0 and np.array_equal(NF, NF2)
    assert len(M.boundary_loop(M.read_smgm("bunny.smgm")[1])) == 149
    Vt, Ft = mesh.torus(12, 9)
    Vt2, Ft2 = M.torus(12, 9)
    assert np.array_equal(Ft, Ft2) and abs(Vt - Vt2).max() < 1e-15


@pytest.mark.parametrize("kind,k", [("mcf", 1), ("poisson", 1)])
def test_precompute_host_half_is_bit_identical_to_oracle(smg_mod, oracle_mod, kind, k):
    smg = smg_mod
    p = subdiv_problem(kind=kind, k=k, n_sub=2)
    mg = _host_precompute(smg, smg.Hierarchy.from_prolongs(p["Ps"]), p["A"], p["known"])
    orc = oracle_mod.OracleMG(p["Ps"])
    orc.precompute(p["A"], p["known"])
    for l in range(mg.n_levels):
        A, Ao = mg.matrix(l, "A"), orc.level_A(l).tocsr()
        Ao.sort_indices()
        assert A.shape == Ao.shape and np.array_equal(A.indptr, Ao.indptr) and np.array_equal(A.indices, Ao.indices)
        assert np.array_equal(A.data, Ao.data), "Galerkin operator differs bitwise on level %d" % l
        assert np.array_equal(mg.Adiag(l), orc.level_Adiag(l))
        if l >= 1:
            for which, ref in (("P", orc.level_P(l)), ("PT", orc.level_PT(l))):
                Mx, Rx = mg.matrix(l, which), ref.tocsr()
                Rx.sort_indices()
                assert np.array_equal(Mx.indptr, Rx.indptr) and np.array_equal(Mx.indices, Rx.indices)
                assert np.array_equal(Mx.data, Rx.data)
    if p["known"] is not None:
        assert np.array_equal(mg.unknown(), orc.unknown())
        Auk, Ao = mg.matrix(0, "Auk"), orc.data_Auk().tocsr()
        Ao.sort_indices()
        assert np.array_equal(Auk.indices, Ao.indices) and np.array_equal(Auk.data, Ao.data)
    # coarsest diagonal carries the +1e-12 shift (min_quad_with_fixed_mg.cpp:32-36)
    Lc = mg.n_levels - 1
    unshifted = (mg.matrix(Lc, "PT") @ mg.matrix(Lc - 1, "A") @ mg.matrix(Lc, "P")).diagonal()
    assert np.allclose(mg.Adiag(Lc) - unshifted, 1e-12, atol=1e-13)


def test_precompute_host_half_with_many_threads_on_a_bigger_system_is_bit_identical(smg_mod, oracle_mod):
    """The host half at a size where its multi-threaded paths are the ones that run -- SpGEMM by row chunks with per-row hash tables, the
    chunked transposition (>= 200 k entries), the parallel copies into arrays that were sized without initialisation, the hand-over to
    the device half (which ends with 'no device' here) -- against the single-threaded oracle, bit for bit: 163 k unknowns, with constraints."""
    smg = smg_mod
    p = subdiv_problem(kind="poisson", k=1, n_sub=3)
    assert p["A"].shape[0] > 150000 and p["Ps"][0].nnz >= 200000 and p["known"] is not None
    mg = _host_precompute(smg, smg.Hierarchy.from_prolongs(p["Ps"]), p["A"], p["known"])
    orc = oracle_mod.OracleMG(p["Ps"])
    orc.precompute(p["A"], p["known"])
    for l in range(mg.n_levels):
        A, Ao = mg.matrix(l, "A"), orc.level_A(l).tocsr()
        Ao.sort_indices()
        assert np.array_equal(A.indptr, Ao.indptr) and np.array_equal(A.indices, Ao.indices) and np.array_equal(A.data, Ao.data), l
        assert np.array_equal(mg.Adiag(l), orc.level_Adiag(l))
        if l >= 1:
            for which, ref in (("P", orc.level_P(l)), ("PT", orc.level_PT(l))):
                Mx, Rx = mg.matrix(l, which), ref.tocsr()
                Rx.sort_indices()
                assert np.array_equal(Mx.indptr, Rx.indptr) and np.array_equal(Mx.indices, Rx.indices) and np.array_equal(Mx.data, Rx.data), (l, which)
    assert np.array_equal(mg.unknown(), orc.unknown())
    # the numbering the host half hands over: a permutation, colour classes independent
    for l in range(mg.n_levels - 1):
        perm = mg.perm(l)
        assert np.array_equal(np.sort(perm), np.arange(len(perm)))


def test_constraint_cascade_drops_empty_columns(smg_mod, oracle_mod):
    """Pin whole coarse 1-rings so that coarse columns become empty and the drop cascade (.cpp:190-220) fires."""
    smg = smg_mod
    p = subdiv_problem(kind="poisson", k=1, n_sub=2)
    P1 = p["Ps"][0].tocsc()
    # all fine vertices that touch coarse vertices 0..39 => those columns of P_1(unknown,:) vanish
    rows = np.unique(np.concatenate([P1.indices[P1.indptr[c]:P1.indptr[c + 1]] for c in range(40)]))
    known = np.unique(np.concatenate([rows, p["known"]])).astype(np.int32)
    mg = _host_precompute(smg, smg.Hierarchy.from_prolongs(p["Ps"]), p["A"], known)
    orc = oracle_mod.OracleMG(p["Ps"])
    orc.precompute(p["A"], known)
    assert mg.rows(1) == orc.rows(1) < p["Ps"][0].shape[1]
    for l in range(mg.n_levels):
        assert mg.rows(l) == orc.rows(l)
        Ao = orc.level_A(l).tocsr()
        Ao.sort_indices()
        assert np.array_equal(mg.matrix(l, "A").data, Ao.data)


def test_colour_ordering_is_a_valid_colouring(smg_mod):
    """The device numbering is computed in the host half: colour-major, no two coupled rows in one colour, 4 colours on
    subdivision levels (inherited from the coarse 4-colouring), and the internal matrix is the permuted caller matrix."""
    smg = smg_mod
    for kind, known in (("mcf", False), ("poisson", True)):
        p = subdiv_problem(kind=kind, k=1, n_sub=2)
        mg = _host_precompute(smg, smg.Hierarchy.from_prolongs(p["Ps"]), p["A"], p["known"] if known else None)
        for lv in range(mg.n_levels - 1):
            A = mg.matrix(lv, "A", internal=True).tocoo()
            cp = mg.colors(lv)
            n = mg.rows(lv)
            assert cp[0] == 0 and cp[-1] == n and (np.diff(cp) > 0).all()
            col_of = np.searchsorted(cp, np.arange(n), side="right") - 1
            off = A.row != A.col
            assert (col_of[A.row[off]] != col_of[A.col[off]]).all()
            perm = mg.perm(lv)
            assert sorted(perm) == list(range(n))
            assert abs(mg.matrix(lv, "A").tocsr()[perm][:, perm] - A.tocsr()).max() == 0
            if not known:
                assert len(cp) - 1 == 4, "subdivision levels inherit a 4-colouring"
        # transfer operators in the device numbering
        for lv in range(1, mg.n_levels):
            P, Pi = mg.matrix(lv, "P"), mg.matrix(lv, "P", internal=True)
            assert abs(P.tocsr()[mg.perm(lv - 1)][:, mg.perm(lv)] - Pi).max() == 0
            assert abs(mg.matrix(lv, "PT", internal=True) - Pi.T).max() == 0


def test_mesh_level_of_a_decimated_hierarchy_gets_a_clean_four_colouring(smg_mod):
    """No colours to inherit on a mesh the library does not know to be subdivided (ogre.obj under mg_precompute): DSATUR + the class-dissolving
    passes used to leave ONE vertex in a fifth class (a launch per sweep, two more phases per one-launch relax); the random walk of Kempe
    interchanges settles it.  The colouring is valid, has four classes, and depends on the matrix alone (two builds, same numbering)."""
    smg = smg_mod
    mesh = smg.mesh
    V, F = mesh.read_triangle_mesh("ogre.smgm")
    V = mesh.normalize_unit_area(V, F)
    A = (mesh.massmatrix(V, F, "barycentric") - 0.01 * mesh.cotmatrix(V, F)).tocsr()
    A.sort_indices()
    perms = []
    for rep in range(2):
        mg = _host_precompute(smg, smg.mg_precompute(V, F, 0.25, 500, 1), A)
        cp = np.asarray(mg.colors(0))
        assert len(cp) - 1 == 4, "level 0 of ogre.obj: %d colour classes %s" % (len(cp) - 1, np.diff(cp).tolist())
        Ai = mg.matrix(0, "A", internal=True).tocoo()
        col_of = np.searchsorted(cp, np.arange(mg.rows(0)), side="right") - 1
        off = Ai.row != Ai.col
        assert (col_of[Ai.row[off]] != col_of[Ai.col[off]]).all()
        for lv in range(1, mg.n_levels - 1):      # Galerkin levels: valid, and no class of a handful of rows
            cl = np.asarray(mg.colors(lv)); Al = mg.matrix(lv, "A", internal=True).tocoo()
            c_of = np.searchsorted(cl, np.arange(mg.rows(lv)), side="right") - 1
            o = Al.row != Al.col
            assert (c_of[Al.row[o]] != c_of[Al.col[o]]).all()
            assert np.diff(cl).min() > 8, np.diff(cl).tolist()
        perms.append(np.asarray(mg.perm(0)).copy())
    assert np.array_equal(perms[0], perms[1])


def test_mg_precompute_invariants(smg_mod):
    smg, mesh = smg_mod, smg_mod.mesh
    V, F = mesh.read_triangle_mesh("bunny.smgm")
    V = mesh.normalize_unit_area(V, F)
    mg = smg.mg_precompute(V, F, 0.25, 500, 1)
    # level count by the float rule (src/mg_precompute.cpp:27-38): 9353 -> 2338.25 -> 584.6 -> 146 => 3 levels
    assert mg.n_levels == 3
    nprev = V.shape[0]
    for l in range(1, mg.n_levels):
        P = mg.matrix(l, "P_full")
        assert P.shape[0] == nprev
        assert np.all(np.diff(P.indptr) == 3)                     # exactly 3 stored entries per row
        assert P.data.min() >= 0.0
        np.testing.assert_allclose(np.asarray(P.sum(axis=1)).ravel(), 1.0, atol=1e-14)
        assert 0.2 < P.shape[1] / P.shape[0] < 0.3                # ~1/4 per level
        assert (np.asarray((P > 0).sum(axis=0)).ravel() > 0).all()  # every coarse vertex is used
        nprev = P.shape[1]
    # closed mesh, vertex-removal flavour
    V, F = mesh.read_triangle_mesh("ogre_sim.smgm")
    mg2 = smg.mg_precompute(mesh.normalize_unit_area(V, F), F, 0.25, 100, 2)
    assert mg2.n_levels == 3
    # vertex removal keeps the surviving end point where it is: the fine vertex sitting on a coarse vertex interpolates from it
    # alone (regression: the merged vertex used to be flattened apart from that end point, 8 levels of ogre.obj at ratio 0.5 then
    # had coarse vertices nobody interpolated from -- zero rows in the Galerkin operator)
    V, F = mesh.read_triangle_mesh("ogre.smgm")
    mg3 = smg.mg_precompute(mesh.normalize_unit_area(V, F), F, 0.5, 100, 2)
    assert mg3.n_levels == 8
    for l in range(1, mg3.n_levels):
        P = mg3.matrix(l, "P_full")
        assert (np.asarray((P > 1e-12).sum(axis=0)).ravel() > 0).all()
        assert (np.asarray((P > 1 - 1e-12).sum(axis=0)).ravel() > 0).all()   # ... by a one-hot row, even
    # dec_type 0 ("qslim": quadric error metric, merged vertex at the quadric's minimiser): same structure of P
    V, F = mesh.read_triangle_mesh("bunny.smgm")
    mg0 = smg.mg_precompute(mesh.normalize_unit_area(V, F), F, 0.25, 500, 0)
    assert mg0.n_levels == 3
    for l in range(1, mg0.n_levels):
        P = mg0.matrix(l, "P_full")
        assert np.all(np.diff(P.indptr) == 3) and P.data.min() >= 0.0
        np.testing.assert_allclose(np.asarray(P.sum(axis=1)).ravel(), 1.0, atol=1e-14)
        assert 0.2 < P.shape[1] / P.shape[0] < 0.3
        assert (np.asarray((P > 0).sum(axis=0)).ravel() > 0).all()
    with pytest.raises(smg.SmgError):
        smg.mg_precompute(V, F, 0.25, 500, 3)                     # no such decimation type


def test_mg_precompute_reproduces_linear_functions(smg_mod):
    """P built by the decimator interpolates: on a flat mesh P * (coarse positions) = fine positions."""
    smg, mesh = smg_mod, smg_mod.mesh
    n = 40
    xs, ys = np.meshgrid(np.linspace(0, 1, n), np.linspace(0, 1, n), indexing="ij")
    V = np.stack([xs.ravel(), ys.ravel(), 0 * xs.ravel()], axis=1)
    idx = lambda i, j: i * n + j
    F = np.array([(idx(i, j), idx(i + 1, j), idx(i + 1, j + 1)) for i in range(n - 1) for j in range(n - 1)] +
                 [(idx(i, j), idx(i + 1, j + 1), idx(i, j + 1)) for i in range(n - 1) for j in range(n - 1)], dtype=np.int32)
    mg = smg.mg_precompute(V, F, 0.25, 50, 1)
    P = mg.matrix(1, "P_full")
    # coarse positions are recovered from the vertices that survive with a one-hot row; interior fine points
    # must be reproduced by barycentric interpolation of SOME coarse positions: solve least squares and check fit
    Vc, *_ = np.linalg.lstsq(P.toarray(), V, rcond=None)
    assert abs(P @ Vc - V).max() < 2e-2


def test_hierarchy_save_load_roundtrip_and_block_variant(smg_mod, tmp_path):
    smg, mesh = smg_mod, smg_mod.mesh
    V, F = mesh.read_triangle_mesh("ogre_sim.smgm")
    V = mesh.normalize_unit_area(V, F)
    mg = smg.mg_precompute(V, F, 0.25, 100, 1)
    path = str(tmp_path / "ogre_sim.smgh")
    mg.save(path)
    mg2 = smg.Hierarchy.load(path)
    assert mg2.n_levels == mg.n_levels
    for l in range(1, mg.n_levels):
        a, b = mg.matrix(l, "P_full"), mg2.matrix(l, "P_full")
        assert a.shape == b.shape and np.array_equal(a.indptr, b.indptr) and np.array_equal(a.indices, b.indices)
        assert np.array_equal(a.data, b.data)
    with pytest.raises(smg.SmgError):
        smg.Hierarchy.load(str(tmp_path / "missing.smgh"))
    # truncated / corrupt files are refused with SMG_ERR_IO, not read out of bounds: cut the file, poison a column index, a row
    # pointer, a count
    raw = open(path, "rb").read()
    import struct
    bad_files = {"cut": raw[: len(raw) // 2], "short": raw[:11]}
    nV0, nF0 = struct.unpack_from("<ii", raw, 12)
    off1 = 12 + 8 + 24 * nV0 + 12 * nF0                       # level 1: i32 nV, nF, V, F, then the P header
    nV1, nF1 = struct.unpack_from("<ii", raw, off1)
    offP = off1 + 8 + 24 * nV1 + 12 * nF1
    nr, nc, nnz = struct.unpack_from("<iii", raw, offP)
    assert nr == V.shape[0] and nnz == 3 * nr
    col_at = offP + 12 + 4 * (nr + 1)
    b = bytearray(raw); struct.pack_into("<i", b, col_at + 40, nc + 5); bad_files["col"] = bytes(b)
    b = bytearray(raw); struct.pack_into("<i", b, offP + 12 + 4 * 7, 2 ** 30); bad_files["ptr"] = bytes(b)
    b = bytearray(raw); struct.pack_into("<i", b, offP + 8, 2 ** 31 - 1); bad_files["nnz"] = bytes(b)
    b = bytearray(raw); struct.pack_into("<i", b, 12, 2 ** 31 - 1); bad_files["nV"] = bytes(b)
    b = bytearray(raw); struct.pack_into("<i", b, 12 + 8 + 24 * nV0 + 4, nV0 + 3); bad_files["face"] = bytes(b)
    for name, data in bad_files.items():
        bp = str(tmp_path / ("bad_%s.smgh" % name))
        open(bp, "wb").write(data)
        with pytest.raises(smg.SmgError) as e:
            smg.Hierarchy.load(bp)
        assert e.value.code == -6, (name, e.value)
    # block variant: P (x) I_3 with DOF index 3*vertex + d (src/get_prolong.cpp:104-114)
    mb = smg.mg_precompute_block(V, F, 0.25, 100, 1)
    for l in range(1, mg.n_levels):
        P, Pb = mg.matrix(l, "P_full"), mb.matrix(l, "P_full")
        assert abs(Pb - sp.kron(P, sp.eye(3), format="csr")).max() == 0


def test_malformed_inputs_are_rejected(smg_mod):
    """Edge cases: out-of-range / duplicate indices, broken pointer arrays, inconsistent sizes, degenerate hierarchies."""
    import ctypes as C
    smg = smg_mod
    L = smg._lib.load()
    p = subdiv_problem(kind="mcf", k=1, n_sub=1)
    P = p["Ps"][0].tocsr()
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    h = L.smg_hierarchy_create(2)
    ptr, col, val = P.indptr.astype(np.int32), P.indices.astype(np.int32), P.data.copy()
    bad = col.copy(); bad[3] = P.shape[1] + 7
    assert L.smg_level_set_prolong(h, 1, P.shape[0], P.shape[1], ip(ptr), ip(bad), dp(val)) == -1
    badptr = ptr.copy(); badptr[5] = badptr[4] - 1
    assert L.smg_level_set_prolong(h, 1, P.shape[0], P.shape[1], ip(badptr), ip(col), dp(val)) == -1
    assert L.smg_level_set_prolong(h, 2, P.shape[0], P.shape[1], ip(ptr), ip(col), dp(val)) == -1       # no such level
    assert L.smg_level_set_prolong(h, 1, P.shape[0], P.shape[1], ip(ptr), ip(col), dp(val)) == 0
    A = p["A"].tocsr()
    ap, ac, av = A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data.copy()
    badc = ac.copy(); badc[0] = -1
    assert L.smg_precompute(h, A.shape[0], ip(ap), ip(badc), dp(av), None, 0) == -1
    kn = np.array([1, 5, 5], dtype=np.int32)
    assert L.smg_precompute(h, A.shape[0], ip(ap), ip(ac), dp(av), ip(kn), 3) == -1 and b"twice" in L.smg_last_error()
    kn = np.array([A.shape[0]], dtype=np.int32)
    assert L.smg_precompute(h, A.shape[0], ip(ap), ip(ac), dp(av), ip(kn), 1) == -1
    assert L.smg_precompute(h, 100, ip(ap), ip(ac), dp(av), None, 0) == -1                              # size mismatch with P_1
    L.smg_hierarchy_destroy(h)
    h1 = L.smg_hierarchy_create(1)
    # a single level is legal (mg_VCycle goes straight to coarseSolve, src/mg_VCycle.cpp:28-33): the host half accepts it and the
    # call only stops at the missing GPU on a CPU-only box
    assert L.smg_precompute(h1, A.shape[0], ip(ap), ip(ac), dp(av), None, 0) in (0, -2)
    L.smg_hierarchy_destroy(h1)
    assert not L.smg_hierarchy_create(0)
    # unsorted rows with duplicate entries are accepted and merged (Eigen setFromTriplets semantics)
    mgA = smg.Hierarchy.from_prolongs(p["Ps"])
    coo = A.tocoo()
    rows = np.concatenate([coo.row, coo.row[:10]]); cols = np.concatenate([coo.col, coo.col[:10]])
    vals = np.concatenate([coo.data * 1.0, coo.data[:10] * 0.0])
    order = np.lexsort((-cols, rows))                                       # descending columns inside a row
    ptr2 = np.zeros(A.shape[0] + 1, np.int32); np.add.at(ptr2, rows + 1, 1); ptr2 = np.cumsum(ptr2).astype(np.int32)
    rc = L.smg_precompute(mgA.h, A.shape[0], ip(ptr2), ip(cols[order].astype(np.int32)), dp(vals[order].copy()), None, 0)
    assert rc in (0, -2)                                                    # -2: host half done, no GPU here
    assert abs(mgA.matrix(0, "A") - A).max() == 0


def test_mg_precompute_rejects_meshes_the_reference_bails_out_on(smg_mod):
    """src/SSP_decimate.cpp:20-23 (the reference stops on non-manifold input): an edge with three faces, two faces running along an edge in
    the same direction, an out-of-range index and a degenerate face each fail smg_mg_precompute with a message saying which; a valid
    mesh with a boundary (open fan) goes through."""
    import ctypes as C
    smg = smg_mod
    L = smg._lib.load()
    V, F = smg.mesh.torus(12, 10)
    V = np.ascontiguousarray(V, dtype=np.float64)

    def run(Fx, Vx=V):
        Fx = np.ascontiguousarray(Fx, dtype=np.int32)
        out = C.c_void_p()
        rc = L.smg_mg_precompute(Vx.ctypes.data_as(C.POINTER(C.c_double)), Vx.shape[0], Fx.ctypes.data_as(C.POINTER(C.c_int)), Fx.shape[0],
                                 C.c_float(0.25), 10, 1, C.byref(out))
        msg = L.smg_last_error()
        if rc == 0: L.smg_hierarchy_destroy(out)
        return rc, msg

    assert run(F)[0] == 0
    a, b, c = (int(x) for x in F[0])
    far = [v for v in range(V.shape[0]) if v not in set(F[np.any(np.isin(F, [a, b]), axis=1)].ravel())][0]
    rc, msg = run(np.vstack([F, [[a, b, far]]]))                 # a third face on the edge (a, b)
    assert rc == -1 and b"edge-manifold" in msg
    Fo = F.copy(); Fo[0] = [a, c, b]                             # face 0 flipped: its three edges now run the way the neighbours' do
    rc, msg = run(Fo)
    assert rc == -1 and b"consistently oriented" in msg
    Fb = F.copy(); Fb[5, 1] = V.shape[0]
    rc, msg = run(Fb)
    assert rc == -1 and b"out of range" in msg
    Fd = F.copy(); Fd[7, 2] = Fd[7, 1]
    rc, msg = run(Fd)
    assert rc == -1 and b"degenerate" in msg
    keep = ~np.any(np.isin(F, [a]), axis=1)                     # the torus with the star of one vertex removed: a boundary loop
    Vh = np.delete(V, a, axis=0)
    Fh = F[keep].copy(); Fh[Fh > a] -= 1
    assert run(Fh, np.ascontiguousarray(Vh))[0] == 0


def test_kat_bunny_500_faces(smg_mod):
    """The only decimation output the reference checks in: 08_subdiv_remesh/output_s0.obj = bunny.obj decimated by
    mid-point collapse to tarF = 500 -> 261 V / 499 F.  With the reference's construction (boundary closed by a
    vertex at infinity, mid-point placement also on the boundary, libigl's refuse / re-cost queue discipline, the three flattening
    cases and their thresholds) the counts are reproduced exactly.  By Euler's formula V = 1 + (F + #boundary edges) / 2, so 261 fixes
    the number of boundary collapses as well: 21 boundary edges remain of 149."""
    import ctypes as C
    smg, mesh = smg_mod, smg_mod.mesh
    V, F = mesh.read_triangle_mesh("bunny.smgm")
    ratio = float(np.float32(500 / 18555))
    mg = smg.mg_precompute(V, F, ratio, 200, 1)
    assert mg.n_levels == 2
    nV, nF = C.c_int(), C.c_int()
    smg._lib.load().smg_level_get_mesh(mg.h, 1, C.byref(nV), C.byref(nF), None, None)
    assert nF.value == 499 and nV.value == 261
    assert mg.matrix(1, "P_full").shape == (9353, nV.value)
    Vc = np.zeros((nV.value, 3)); Fc = np.zeros((nF.value, 3), np.int32)
    smg._lib.load().smg_level_get_mesh(mg.h, 1, None, None, Vc.ctypes.data_as(C.POINTER(C.c_double)), Fc.ctypes.data_as(C.POINTER(C.c_int)))
    assert len(mesh.boundary_loop(Fc)) == 21
    # the opt-in absorption cap is a different collapse order: it is not what the known answer is about
    mgc = smg.mg_precompute(V, F, ratio, 200, 1, absorption_cap=2.0)
    smg._lib.load().smg_level_get_mesh(mgc.h, 1, C.byref(nV), C.byref(nF), None, None)
    assert nF.value in (499, 500)


from kat_remesh import _level_mesh, check_subdiv_remesh_kat  # noqa: E402


def test_kat_subdiv_remesh_outputs_of_the_reference(smg_mod):
    """REFERENCE-DERIVED golden vectors: libsmg's decimator + smg_query_coarse_to_fine land on the 261 / 1020 / 4035 points the reference
    checks in as 08_subdiv_remesh/output_s0/_s1/_s2.obj (body and docstring: tests/kat_remesh.py; GPU-lane twin: tests/test_gpu_reference_kat.py)."""
    check_subdiv_remesh_kat(smg_mod)


def test_subdiv_remesh_example_writes_the_reference_s_files(smg_mod, tmp_path):
    """examples/08_subdiv_remesh.cpp (the reference's 08_subdiv_remesh/main.cpp:113-166 on the C ABI, host only) writes output_s0/1/2.obj:
    all three are the reference's checked-in files vertex for vertex and face for face (same numbering of the coarse mesh: the smaller
    index survives a collapse on both sides; the example numbers the upsampled meshes the way libigl's upsample does)."""
    import subprocess
    lib = os.path.join(ROOT, "surface_multigrid_code_amd", "lib")
    src = os.path.join(ROOT, "examples", "08_subdiv_remesh.cpp")
    exe = str(tmp_path / "08_subdiv_remesh")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", src, "-I" + os.path.join(ROOT, "include"), "-L" + lib, "-lsmg",
                           "-Wl,-rpath," + lib, "-o", exe])
    env = dict(os.environ, LD_LIBRARY_PATH=lib + ":" + os.environ.get("LD_LIBRARY_PATH", ""))
    out = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "meshes", "bunny.smgm"), str(tmp_path)], env=env, capture_output=True, text=True)
    assert out.returncode == 0, (out.stdout[-1000:], out.stderr[-1000:])
    G = np.load(os.path.join(ROOT, "tests", "golden", "bunny_remesh_500.npz"))

    def read_obj(path):
        V, F = [], []
        for ln in open(path):
            t = ln.split()
            if t and t[0] == "v":
                V.append([float(x) for x in t[1:4]])
            elif t and t[0] == "f":
                F.append([int(x) - 1 for x in t[1:4]])
        return np.array(V), np.array(F, np.int32)
    for k, nF in ((0, 499), (1, 1996), (2, 7984)):
        Vk, Fk = read_obj(str(tmp_path / ("output_s%d.obj" % k)))
        ref = G["s%d_V" % k]
        assert Vk.shape == ref.shape and Fk.shape == (nF, 3)
        assert np.abs(Vk - ref).max() <= 1e-10          # vertex for vertex (15 digits printed of numbers up to 50)
        assert np.array_equal(Fk, G["s%d_F" % k])       # face for face, corner for corner


def test_query_fine_to_coarse_is_the_prolongation_and_the_inverse_of_the_walk_back(smg_mod):
    """smg_query_fine_to_coarse (the reference's query_fine_to_coarse, what get_prolong runs for the vertices, src/get_prolong.cpp:23-57):
    a fine vertex given as a one-hot point of one of its faces arrives where its row of P_full says; arbitrary points of the fine mesh
    return to themselves through query_coarse_to_fine (the map is a bijection: 2e-14 measured on a bounding box of 80)."""
    smg, mesh = smg_mod, smg_mod.mesh
    V, F = mesh.read_triangle_mesh("bunny.smgm")
    diag = float(np.linalg.norm(V.max(0) - V.min(0)))
    mg = smg.mg_precompute(V, F, float(np.float32(500 / 18555)), 200, 1, keep_log=True)
    Vc, Fc = _level_mesh(smg, mg, 1)
    face = np.full(V.shape[0], -1, np.int32); bary = np.zeros((V.shape[0], 3))
    for f in range(F.shape[0] - 1, -1, -1):
        for c in range(3):
            face[F[f, c]] = f; bary[F[f, c]] = 0.0; bary[F[f, c], c] = 1.0
    of, ob = smg.query_fine_to_coarse(mg, 1, face, bary)
    assert of.min() >= 0 and of.max() < Fc.shape[0] and ob.min() >= 0.0
    Q = sp.csr_matrix((ob.ravel(), (np.repeat(np.arange(V.shape[0]), 3), Fc[of].ravel())), shape=(V.shape[0], Vc.shape[0]))
    Q.sum_duplicates()
    assert abs(mg.matrix(1, "P_full").tocsr() - Q).max() <= 1e-13
    rng = np.random.default_rng(1)
    fq = rng.integers(0, F.shape[0], 2000).astype(np.int32); bq = rng.dirichlet(np.ones(3), 2000)
    cf, cb = smg.query_fine_to_coarse(mg, 1, fq, bq)
    ff, fb = smg.query_coarse_to_fine(mg, 1, cf, cb)
    p0 = (bq[:, :, None] * V[F[fq]]).sum(1); p1 = (fb[:, :, None] * V[F[ff]]).sum(1)
    assert np.linalg.norm(p0 - p1, axis=1).max() <= 1e-11 * diag
    with pytest.raises(smg.SmgError):
        smg.query_fine_to_coarse(mg, 1, np.array([F.shape[0]], np.int32), np.array([[1.0, 0.0, 0.0]]))
    with pytest.raises(smg.SmgError):
        smg.query_fine_to_coarse(smg.mg_precompute(V, F, 0.25, 500, 1), 1, np.zeros(1, np.int32), np.array([[1.0, 0.0, 0.0]]))


def test_query_coarse_to_fine_contract(smg_mod):
    """smg_query_coarse_to_fine: needs the log (SMG_ERR_INVALID without), checks its arguments, works level by level on a deeper hierarchy
    (every point lands on the finer level's surface with valid coordinates; coarse vertices of level 2 carried to level 0 stay close to
    where the coarse vertex is)."""
    import ctypes as C
    smg, mesh = smg_mod, smg_mod.mesh
    V, F = mesh.read_triangle_mesh("bunny.smgm")
    V = mesh.normalize_unit_area(V, F)
    mg0 = smg.mg_precompute(V, F, 0.25, 500, 1)
    with pytest.raises(smg.SmgError):
        smg.query_coarse_to_fine(mg0, 1, np.zeros(1, np.int32), np.array([[1.0, 0.0, 0.0]]))
    mg = smg.mg_precompute(V, F, 0.25, 500, 1, keep_log=True)
    assert mg.n_levels >= 3
    for bad_lv in (0, mg.n_levels):
        with pytest.raises(smg.SmgError):
            smg.query_coarse_to_fine(mg, bad_lv, np.zeros(1, np.int32), np.array([[1.0, 0.0, 0.0]]))
    V2, F2 = _level_mesh(smg, mg, 2)
    with pytest.raises(smg.SmgError):
        smg.query_coarse_to_fine(mg, 2, np.array([F2.shape[0]], np.int32), np.array([[1.0, 0.0, 0.0]]))
    with pytest.raises(smg.SmgError):
        smg.query_coarse_to_fine(mg, 2, np.zeros(1, np.int32), np.array([[np.nan, 0.0, 0.0]]))
    of, ob = smg.query_coarse_to_fine(mg, 2, np.zeros(0, np.int32), np.zeros((0, 3)))
    assert of.shape == (0,)
    rng = np.random.default_rng(0)
    face = rng.integers(0, F2.shape[0], 500).astype(np.int32)
    bary = rng.dirichlet(np.ones(3), 500)
    V1, F1 = _level_mesh(smg, mg, 1)
    f1, b1 = smg.query_coarse_to_fine(mg, 2, face, bary)
    assert f1.min() >= 0 and f1.max() < F1.shape[0] and b1.min() >= 0 and np.abs(b1.sum(1) - 1).max() < 1e-14
    f0, b0 = smg.query_coarse_to_fine(mg, 1, f1, b1)
    assert f0.min() >= 0 and f0.max() < F.shape[0] and b0.min() >= 0 and np.abs(b0.sum(1) - 1).max() < 1e-14
    p2 = (bary[:, :, None] * V2[F2[face]]).sum(1)
    p0 = (b0[:, :, None] * V[F[f0]]).sum(1)
    edge2 = np.linalg.norm(V2[F2[:, 0]] - V2[F2[:, 1]], axis=1).mean()
    assert np.median(np.linalg.norm(p2 - p0, axis=1)) < 0.25 * edge2      # the map is a parameterisation, not a projection: close, not equal


@pytest.mark.parametrize("mesh_name,bound,dec_type,cap", [("bunny.smgm", 0.12, 1, 0.0), ("bunny_15K_init.smgm", 0.2, 1, 0.0), ("ogre_sim.smgm", 0.2, 1, 0.0),
                                                          ("ogre.smgm", 0.75, 1, 0.0), ("ogre.smgm", 0.36, 1, 2.0), ("bunny_15K_init.smgm", 0.12, 1, 2.0),
                                                          ("bunny.smgm", 0.35, 0, 0.0), ("bunny.smgm", 0.3, 2, 0.0)])
def test_mg_precompute_hierarchies_converge(smg_mod, oracle_mod, mesh_name, bound, dec_type, cap):
    """the hierarchy builder is judged by what it is for -- the V-cycle convergence factor of the reference
    algorithm (CPU oracle) on its hierarchy, expected <~ 0.3.  The reference's plain greedy order (cap 0, the default) delivers that on
    evenly sampled meshes; on ogre.obj (strongly non-uniform sampling) shortest-edge-first coarsens the dense regions far beyond the
    ratio and the factor is 0.6-0.7 -- a property of the construction, which the opt-in absorption cap repairs (0.3)."""
    V, F = M.read_smgm(mesh_name)
    V = M.normalize_unit_area(V, F)
    mg = smg_mod.mg_precompute(V, F, ratio=0.25, nVCoarsest=500, dec_type=dec_type, absorption_cap=cap)
    Ps = [mg.matrix(l, "P_full") for l in range(1, mg.n_levels)]
    sizes = [Ps[0].shape[0]] + [P.shape[1] for P in Ps]
    assert all(0.2 < sizes[i + 1] / sizes[i] < 0.3 for i in range(len(sizes) - 1))
    A = (M.massmatrix(V, F, "barycentric") - 0.01 * M.cotmatrix(V, F)).tocsr()
    A.sort_indices()
    o = oracle_mod.OracleMG(Ps)
    o.precompute(A)
    rng = np.random.default_rng(0)
    e = rng.uniform(-1, 1, (V.shape[0], 1))
    zero = np.zeros_like(e)
    factor = 1.0
    for _ in range(25):   # power iteration on the error propagation of one V(2,2) cycle
        e2 = o.vcycle(zero, e)
        factor = np.linalg.norm(e2) / np.linalg.norm(e)
        e = e2 / np.linalg.norm(e2)
    assert factor < bound


# ----------------------------------------------------------------------------------------------- block (3-DOF) hierarchies
def _block_problem(seed=5, mesh="ogre_sim.smgm", coupled=True):
    V, F = M.read_smgm(mesh)
    V = M.normalize_unit_area(V, F)
    S = (M.massmatrix(V, F, "barycentric") - 0.01 * M.cotmatrix(V, F)).tocsr()
    rng = np.random.default_rng(seed)
    B3 = rng.uniform(-1, 1, (3, 3))
    C3 = B3 @ B3.T + 3.0 * np.eye(3) if coupled else np.eye(3)
    A = sp.kron(S, sp.csr_matrix(C3), format="csr")          # DOF index 3 v + d
    A.sort_indices()
    return V, F, A


def test_block_hierarchy_host_half(smg_mod):
    """SURVEY 8 f-4, host half (no GPU): a hierarchy whose prolongations are Pv (x) I_3 (mg_precompute_block,
    reference src/get_prolong.cpp:104-114) and a system with full 3 x 3 blocks switch the library to the block variant: VERTICES are
    coloured (as many Gauss-Seidel launches per sweep as the mesh has colours, not three times as many), the DOF numbering is 3 v + d on the
    colour-major vertex numbering, and the 3 x 3 block SELL image reproduces the scalar matrix in that numbering entry for entry."""
    smg = smg_mod
    V, F, A = _block_problem()
    n = V.shape[0]
    mg = _host_precompute(smg, smg.mg_precompute_block(V, F, 0.25, 100, 1), A)
    assert mg.block_size() == 3
    for lv in range(mg.n_levels - 1):
        perm = mg.perm(lv)
        nv = len(perm) // 3
        assert np.array_equal(perm.reshape(nv, 3) % 3, np.tile(np.arange(3), (nv, 1)))          # DOFs of a vertex stay together, in order
        assert np.array_equal(perm.reshape(nv, 3)[:, 0] // 3, perm.reshape(nv, 3)[:, 2] // 3)
        cp = mg.colors(lv)
        # (a mesh level: 4-6 classes; the Galerkin levels of a decimated hierarchy couple second neighbours: about 10)
        assert np.all(cp % 3 == 0) and len(cp) - 1 <= (6 if lv == 0 else 14), "vertex colours expected, got %d classes" % (len(cp) - 1)
        Ai = mg.matrix(lv, "A", internal=True)
        # a valid VERTEX colouring: inside a colour class only the 3 x 3 diagonal blocks are populated
        for c in range(len(cp) - 1):
            blk = sp.coo_matrix(Ai[cp[c]:cp[c + 1], cp[c]:cp[c + 1]])
            assert np.all(blk.row // 3 == blk.col // 3)
        # the block image is the scalar matrix: rebuild it from the panels
        img = mg.block_image(lv)
        rows, cols, vals = [], [], []
        for s in range(len(img["slice_w"])):
            r0, r1, off, w = img["slice_row"][s], img["slice_row"][s + 1], img["slice_off"][s], img["slice_w"][s]
            assert r1 - r0 <= 64
            for j in range(w):
                c = img["col"][off + j, :r1 - r0]
                ok = c >= 0
                if j > 0:   # block columns ascend inside a block row
                    prev = img["col"][off + j - 1, :r1 - r0]
                    assert np.all((c[ok] > prev[ok]))
                for e in range(9):
                    rows.append(3 * (r0 + np.nonzero(ok)[0]) + e // 3); cols.append(3 * c[ok] + e % 3); vals.append(img["val"][off + j, e, :r1 - r0][ok])
        R = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=Ai.shape)
        assert abs(R - Ai).max() == 0.0
        assert R.nnz >= Ai.nnz and (R != 0).sum() == (Ai != 0).sum()       # explicit zeros only where the scalar matrix stores nothing
    # the scalar path of the same problem needs at least three times the colours on level 0
    mg2 = smg.mg_precompute_block(V, F, 0.25, 100, 1)
    mg2.set_block_mode("scalar")
    _host_precompute(smg, mg2, A)
    assert mg2.block_size() == 1 and len(mg2.colors(0)) - 1 >= 3 * (len(mg.colors(0)) - 1)
    # kron(S, I_3): three scalar problems -- the automatic choice stays scalar, 'block' can be forced, constraints select the scalar path
    V, F, Ad = _block_problem(coupled=False)
    mg3 = _host_precompute(smg, smg.mg_precompute_block(V, F, 0.25, 100, 1), Ad)
    assert mg3.block_size() == 1
    mg3.set_block_mode("block")
    _host_precompute(smg, mg3, Ad)
    assert mg3.block_size() == 3
    mg4 = smg.mg_precompute_block(V, F, 0.25, 100, 1)
    _host_precompute(smg, mg4, A, known=np.array([0, 1, 2, 30], np.int32))
    assert mg4.block_size() == 1
    mg4.set_block_mode("block")
    with pytest.raises(smg.SmgError):
        mg4.precompute(A, np.array([0, 1, 2, 30], np.int32))


# ----------------------------------------------------------------------------------------------- round-3 host components
def test_tiling_plan_reproduces_the_colour_sweeps_bit_for_bit(smg_mod):
    """relax(sweeps) as ONE launch per level (csrc/smg_tiled.hpp): the plan -- compact tiles, halo rings, tile-local panels -- executed on
    the host exactly as the kernel executes it gives the bits of the plain colour-by-colour Gauss-Seidel sweeps (the reference's relax(),
    src/mg_VCycle.cpp:113-178, on the colour-major numbering), for several tile sizes and sweep counts, on mesh levels and Galerkin levels."""
    import ctypes as C
    smg = smg_mod
    p = subdiv_problem(kind="poisson", k=1, n_sub=2)
    mg = _host_precompute(smg, smg.Hierarchy.from_prolongs(p["Ps"]), p["A"], p["known"])
    L = smg._lib.load()
    for lv in range(mg.n_levels - 1):
        for sweeps, tile_rows in ((1, 64), (2, 256), (2, 100), (3, 512)):
            nt, me, red, diff = C.c_int(), C.c_int(), C.c_double(), C.c_double(-1.0)
            rc = L.smg_debug_check_tiling_plan(mg.h, lv, sweeps, tile_rows, C.byref(nt), C.byref(me), C.byref(red), C.byref(diff))
            assert rc == 0
            ncol = len(mg.colors(lv)) - 1
            if ncol * sweeps > 15 or ncol > 5:
                assert nt.value == 0           # too many phases: the level keeps one launch per colour
                continue
            assert nt.value >= mg.rows(lv) // tile_rows and red.value >= 1.0 and me.value >= min(tile_rows // 2, mg.rows(lv))
            assert diff.value == 0.0, "level %d, %d sweeps, tiles of %d rows: the tiled sweeps differ by %g" % (lv, sweeps, tile_rows, diff.value)


def test_block_gauss_seidel_plan_is_the_lexicographic_sweep_in_its_order(smg_mod):
    """Block Gauss-Seidel for many right-hand sides (csrc/smg_bgs.hpp, round 4): the plan -- compact blocks, block colours, per block an image of
    its rows and rim, units of <= 16 rows of one vertex colour with local indices -- executed on the host exactly as k_bgs executes it gives the
    bits of the reference's lexicographic sweep (src/mg_VCycle.cpp:146-160) on the numbering (block colour, block, vertex colour, row); invariants:
    every row in one block, blocks of one colour share no entry, few colours, a rim below one row per row.  Mesh levels with and without
    constraints, Galerkin levels, several block sizes."""
    import ctypes as C
    smg = smg_mod
    L = smg._lib.load()
    for kind, pins in (("poisson", 40), ("mcf", 0)):
        p = subdiv_problem(kind=kind, k=1, n_sub=2, n_pins=pins)
        mg = _host_precompute(smg, smg.Hierarchy.from_prolongs(p["Ps"]), p["A"], p["known"])
        for lv in range(mg.n_levels - 1):
            for block_rows in (64, 32, 16):
                nb, nc, rim, fill, diff = C.c_int(), C.c_int(), C.c_double(), C.c_double(), C.c_double(-1.0)
                rc = L.smg_debug_check_block_gs_plan(mg.h, lv, block_rows, C.byref(nb), C.byref(nc), C.byref(rim), C.byref(fill), C.byref(diff))
                assert rc == 0, L.smg_last_error()
                assert nb.value >= mg.rows(lv) // block_rows and 3 <= nc.value <= 9
                assert 0.0 < rim.value < 2.5 and (0.5 if block_rows == 64 else 0.1) < fill.value <= 1.0
                assert diff.value == 0.0, "level %d, blocks of %d rows: the block sweep differs by %g" % (lv, block_rows, diff.value)


def test_wave_gauss_seidel_plan_is_the_lexicographic_sweep_in_its_order(smg_mod):
    """Wave Gauss-Seidel on the Galerkin levels of the reference's own hierarchies (csrc/smg_wgs.hpp, round 5): the plan -- pieces of <= 64 rows (compact,
    or cut along breadth-first level sets), piece colours, per piece an image of its rows and rim, phases, packed byte offsets -- executed on the host
    exactly as k_wgs executes it gives the bits of the reference's lexicographic sweep (src/mg_VCycle.cpp:146-160) on the numbering (piece colour, piece,
    local colour, row); invariants: every row in one piece, pieces of one colour share no entry, few colours, few phases.  Hierarchies by mg_precompute
    (ogre.obj: 18 - 25 entries per row, restriction rows of up to 177 entries) and by subdivision."""
    import ctypes as C
    smg = smg_mod
    L = smg._lib.load()
    V, F = M.read_smgm("ogre.smgm")
    V = M.normalize_unit_area(V, F)
    mgd = smg.mg_precompute(V, F, 0.25, 200, 1)
    A = (M.massmatrix(V, F, "barycentric") - 0.01 * M.cotmatrix(V, F)).tocsr()
    A.sort_indices()
    _host_precompute(smg, mgd, A)
    p = subdiv_problem(kind="poisson", k=1, n_sub=2, n_pins=40)
    mgs = _host_precompute(smg, smg.Hierarchy.from_prolongs(p["Ps"]), p["A"], p["known"])
    for mg in (mgd, mgs):
        for lv in range(mg.n_levels - 1):
            for piece_rows, mode in ((64, 0), (32, 0), (64, 1), (16, 1)):
                nb, nc, diff = C.c_int(), C.c_int(), C.c_double(-1.0)
                st = np.zeros(3)
                rc = L.smg_debug_check_wave_gs_plan(mg.h, lv, piece_rows, mode, C.byref(nb), C.byref(nc), st.ctypes.data_as(C.POINTER(C.c_double)), C.byref(diff))
                assert rc == 0, L.smg_last_error()
                assert nb.value >= mg.rows(lv) // piece_rows and 3 <= nc.value <= 10
                assert 0.0 < st[0] < 6.0 and 1.0 <= st[1] <= st[2] <= 20
                assert diff.value == 0.0, "level %d, pieces of %d rows (mode %d): the piece sweep differs by %g" % (lv, piece_rows, mode, diff.value)


def test_wave_kernel_variant_hooks_state_the_launchers_choice(smg_mod):
    """smg_debug_wgs_launches and smg_debug_wgs_level_plan (read-only; the launcher's own functions; smg_debug_deep_launches and smg_debug_gs_colour_wpb refuse what they cannot answer): with the default knobs a level of at most 1 600
    pieces runs every column as KB = 1, one group per column; a larger one groups of 4 and one launch of k % 4 columns at the column offset; the
    row-width classes change at 3 / 5 batches, the rim slots per lane follow the pitch; a plan the kernel has no variant for is refused.  On the host
    the plan of a Galerkin level of the decimated bunny is the one the first sweep would build (tests/test_gpu_wgs_variants.py asserts the same
    numbers on the device), and a level no sweep has run on reports no plan in use."""
    import ctypes as C
    import kernel_hooks as H
    smg = smg_mod
    L = smg._lib.load()
    for k in (1, 2, 3, 4, 5, 7, 8, 11, 18, 64):
        for n_pieces in (1, 37, 1600):
            assert H.wgs_launches(L, n_pieces, 4, 256, k) == (5, 4, [(1, k)])
        tail = [(k % 4, 1)] if k % 4 else []
        assert H.wgs_launches(L, 1601, 4, 256, k) == (5, 4, ([(4, k // 4)] if k >= 4 else []) + tail)
    assert [H.wgs_launches(L, 10, nb, 128, 1)[0] for nb in range(1, 9)] == [3, 3, 3, 5, 5, 8, 8, 8]
    assert [H.wgs_launches(L, 10, 1, pitch, 1)[1] for pitch in (128, 256, 448)] == [2, 4, 7]
    n = C.c_int(-1)
    out = np.zeros(8, np.int32)
    ip = out.ctypes.data_as(C.POINTER(C.c_int))
    for bad in ((0, 4, 256, 1), (10, 0, 256, 1), (10, 9, 256, 1), (10, 4, 192, 1), (10, 4, 512, 1), (10, 4, 256, 0)):
        assert L.smg_debug_wgs_launches(*bad, None, None, ip, 4, C.byref(n)) == -1 and b"smg_debug_wgs_launches" in L.smg_last_error(), bad
    assert L.smg_debug_wgs_launches(10, 4, 256, 1, None, None, None, 4, C.byref(n)) == -1 and L.smg_debug_wgs_launches(10, 4, 256, 1, None, None, ip, 4, None) == -1
    assert L.smg_debug_wgs_launches(2000, 4, 256, 7, None, None, ip, 1, C.byref(n)) == 0 and n.value == 2 and out[:4].tolist() == [4, 1, 0, 0]      # cap: no write behind it
    V, F = M.read_smgm("bunny.smgm")
    V = M.normalize_unit_area(V, F)
    mg = smg.mg_precompute(V, F, 0.25, 60, 1)
    A = (M.massmatrix(V, F, "barycentric") - 0.01 * M.cotmatrix(V, F)).tocsr()
    A.sort_indices()
    _host_precompute(smg, mg, A)
    assert [H.wgs_level_plan(mg, lv, 1, from_host=True) for lv in (1, 2)] == [(62, 4, 256), (18, 6, 128)]
    if L.smg_device_count() == 0:
        assert H.wgs_level_plan(mg, 1, 1) is None
    a = C.c_int(-1)
    assert L.smg_debug_wgs_level_plan(None, 1, 1, 1, C.byref(a), C.byref(a), C.byref(a)) == -1
    assert L.smg_debug_wgs_level_plan(mg.h, mg.n_levels - 1, 1, 1, C.byref(a), C.byref(a), C.byref(a)) == -1
    assert L.smg_debug_wgs_level_plan(mg.h, 1, 0, 1, C.byref(a), C.byref(a), C.byref(a)) == -1
    assert L.smg_debug_deep_launches(None, 0, 0, 0, 1, None, None, 0, C.byref(a)) == -1
    assert L.smg_debug_deep_launches(mg.h, 0, 3, 0, 1, None, None, 0, C.byref(a)) == -1 and L.smg_debug_deep_launches(mg.h, 0, 0, 2, 1, None, None, 0, C.byref(a)) == -1
    assert L.smg_debug_deep_launches(mg.h, 0, 0, 0, 5, None, None, 0, C.byref(a)) == -1 and L.smg_debug_deep_launches(mg.h, 0, 0, 0, 0, None, None, 0, C.byref(a)) == -1      # one narrow group
    assert L.smg_debug_gs_colour_wpb(None, 0, 1, C.byref(a), None, None) == -1 and L.smg_debug_gs_colour_wpb(mg.h, 0, 0, C.byref(a), None, None) == -1
    assert L.smg_debug_gs_colour_wpb(mg.h, 0, 1, None, None, None) == -1 and L.smg_debug_gs_colour_wpb(mg.h, mg.n_levels - 1, 1, C.byref(a), None, None) == -1


def test_sweep_plans_copy_the_level_values_their_maps_name_and_pad_with_zero_and_one(smg_mod):
    """The three plan-based sweeps keep copies of the level's values and diagonals; a value-only re-precompute gathers them anew through the plans'
    maps and leaves every slot without a map untouched (csrc/smg_sweep_plans.cpp: refresh_plan_values).  So, for every plan as the solves build it:
    a mapped slot holds the bits of the level value its map names -- of A_lv^T where the level sweeps on the transpose --, an unmapped entry slot
    +0.0 and an unmapped diagonal slot 1.0.  Torus subdivision levels (tiled, wave and block plans) and the decimated bunny (level 0 tiled, its
    Galerkin levels wave), with A1 = M - 0.01 L (level 0 bit-symmetric: sweeps on A; Galerkin levels on A^T) and with value_step(A1, 1) (no level
    bit-symmetric: every level on A^T; without a GPU the hook applies the first precompute's rule from the bits, and reports its choice).  The comparison against the mirrored values -- what the map of the wrong one of A / A^T
    would pass -- must count mismatches wherever the level's matrix is not bit-symmetric, and none on the bit-symmetric level 0 of A1."""
    import ctypes as C
    from problems import value_step
    smg = smg_mod
    L = smg._lib.load()

    def check(mg, lv, which, sweeps, against_transpose=0):
        ns, npad, bad, on_t = C.c_int(-1), C.c_int(-1), C.c_int(-1), C.c_int(-1)
        rc = L.smg_debug_check_plan_value_maps(mg.h, lv, which, sweeps, against_transpose, C.byref(ns), C.byref(npad), C.byref(bad), C.byref(on_t))
        assert rc == 0, L.smg_last_error()
        assert on_t.value == int(stepped or lv > 0), "level %d: built from %s" % (lv, "A^T" if on_t.value else "A")
        return ns.value, npad.value, bad.value

    def torus():
        V, F = smg.mesh.torus(8, 8)
        mg, Vf, Ff = smg.mg_precompute_subdiv(V, F, 3, n_extra_levels=0)
        Vf = M.normalize_unit_area(Vf, Ff)
        return mg, (M.massmatrix(Vf, Ff, "barycentric") - 0.01 * M.cotmatrix(Vf, Ff)).tocsr(), {0: (0, 1, 2), 1: (0, 1, 2), 2: (0, 1, 2)}, 3

    def bunny():
        V, F = M.read_smgm("bunny.smgm")
        V = M.normalize_unit_area(V, F)
        return smg.mg_precompute(V, F, 0.25, 200, 1), (M.massmatrix(V, F, "barycentric") - 0.01 * M.cotmatrix(V, F)).tocsr(), {0: (0,), 1: (0, 1), 2: (0,)}, 2

    for make in (torus, bunny):
        for stepped in (False, True):
            mg, A1, must_have, n_smoothed = make()      # must_have: plan kind -> the levels that have such a plan
            A1.sort_indices()
            assert (A1 != A1.T).nnz == 0
            A = value_step(A1, 1) if stepped else A1
            _host_precompute(smg, mg, A)
            assert mg.n_levels - 1 == n_smoothed
            for lv in range(n_smoothed):
                Al = mg.matrix(lv, "A")
                unsym = (Al != Al.T).nnz
                assert (unsym > 0) == (stepped or lv > 0), "level %d: %d entries differ from their mirror image" % (lv, unsym)
                plans = [(1, 0), (2, 0)] + [(0, s) for s in (1, 2, 3)]
                for which, sweeps in plans:
                    ns, npad, bad = check(mg, lv, which, sweeps)
                    if ns == 0:      # the level does not qualify: more than 5 colours or 12 entries per row (tiling), too wide a rim (block)
                        assert lv not in must_have[which], "level %d has no plan of kind %d (%d sweeps)" % (lv, which, sweeps)
                        continue
                    assert bad == 0, "level %d, plan kind %d, %d sweeps: %d of %d slots do not hold the value their map names" % (lv, which, sweeps, bad, ns)
                    assert npad > 0 and ns > npad
                    # the same comparison fed the values of the other one of A / A^T
                    ns2, npad2, bad2 = check(mg, lv, which, sweeps, against_transpose=1)
                    assert (ns2, npad2) == (ns, npad)
                    if unsym:
                        assert bad2 > 0, "level %d, plan kind %d: the check passes with the map of A where A^T is due" % (lv, which)
                        assert bad2 >= unsym      # every entry that differs from its mirror image sits in at least one slot
                    else:
                        assert bad2 == 0
    # refusals: no handle, an unknown plan kind, a sweep count the tiling has no plan for, a level that is not smoothed
    z = C.c_int()
    assert L.smg_debug_check_plan_value_maps(None, 0, 0, 1, 0, C.byref(z), C.byref(z), C.byref(z), C.byref(z)) == -1
    for lv, which, sweeps in ((0, 3, 1), (0, -1, 1), (0, 0, 0), (0, 0, 4), (mg.n_levels - 1, 1, 1), (-1, 1, 1)):
        assert L.smg_debug_check_plan_value_maps(mg.h, lv, which, sweeps, 0, C.byref(z), C.byref(z), C.byref(z), C.byref(z)) == -1, (lv, which, sweeps)


def test_union_of_hierarchies_is_block_diagonal(smg_mod):
    """smg_hierarchy_create_union (independent meshes in one handle, csrc/smg_union.cpp): P_full of every level is diag(P_full of the members), member row
    ranges are reported, the Galerkin operators of the union are the members' (bit for bit: block-diagonal products add nothing), members of unequal depth
    are refused."""
    import scipy.sparse as sp
    smg = smg_mod
    ms, As = [], []
    for name, nvc in (("ogre_sim.smgm", 100), ("bunny.smgm", 200), ("ogre_sim.smgm", 100)):
        V, F = M.read_smgm(name)
        V = M.normalize_unit_area(V, F)
        ms.append(smg.mg_precompute(V, F, 0.25, nvc, 1))
        A = (M.massmatrix(V, F, "barycentric") - 0.01 * M.cotmatrix(V, F)).tocsr(); A.sort_indices()
        As.append(A)
    assert all(m.n_levels == 3 for m in ms)
    u = smg.Hierarchy.union(ms)
    assert u.union_members() == 3 and ms[0].union_members() == 0
    off = 0
    for i, m in enumerate(ms):
        first, cnt = u.union_member_rows(i)
        assert first == off and cnt == As[i].shape[0]
        off += cnt
    for lv in (1, 2):
        ref = sp.block_diag([m.matrix(lv, "P_full") for m in ms], format="csr")
        got = u.matrix(lv, "P_full")
        assert got.shape == ref.shape and abs(got - ref).max() == 0 and got.nnz == ref.nnz
    Au = sp.block_diag(As, format="csr"); Au.sort_indices()
    _host_precompute(smg, u, Au)
    for m, A in zip(ms, As):
        _host_precompute(smg, m, A)
    for lv in (1, 2):
        ref = sp.block_diag([m.matrix(lv, "A") for m in ms], format="csr")
        got = u.matrix(lv, "A")
        assert abs(got - ref).max() == 0
    with pytest.raises(smg.SmgError):
        V, F = M.read_smgm("bunny.smgm")
        smg.Hierarchy.union([ms[0], smg.mg_precompute(M.normalize_unit_area(V, F), F, 0.25, 1000, 1)])      # 2 levels against 3


def test_sparse_cholesky_of_the_coarse_solver(smg_mod):
    """csrc/smg_coarse.cpp (coarsest levels beyond the dense range; the reference: Eigen::SimplicialLDLT, src/min_quad_with_fixed_mg.cpp:47-48):
    nested dissection + up-looking Cholesky on mesh operators -- residual of a host solve with the factor at rounding level, fill O(n log n),
    dependency depth (= the length of the device's triangular-solve chain) O(sqrt n); an indefinite matrix is refused."""
    import ctypes as C
    smg = smg_mod
    L = smg._lib.load()
    for name in ("ogre_sim.smgm", "bunny.smgm", "bunny_15K_init.smgm"):
        V, F = M.read_smgm(name)
        V = M.normalize_unit_area(V, F)
        A = (M.massmatrix(V, F, "barycentric") - 0.01 * M.cotmatrix(V, F)).tocsr()
        A.sort_indices()
        n = A.shape[0]
        ne, dep, res = C.c_long(), C.c_int(), C.c_double()
        ptr, col, val = A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data.astype(np.float64)
        rc = L.smg_debug_check_sparse_cholesky(n, ptr.ctypes.data_as(C.POINTER(C.c_int)), col.ctypes.data_as(C.POINTER(C.c_int)),
                                               val.ctypes.data_as(C.POINTER(C.c_double)), C.byref(ne), C.byref(dep), C.byref(res))
        assert rc == 0 and res.value < 1e-11
        assert n < ne.value < 12 * n * np.log2(n) and dep.value < 12 * np.sqrt(n)
    bad = val.copy()
    bad[A.indptr[:-1][0] + list(A.indices[A.indptr[0]:A.indptr[1]]).index(0)] = -1.0      # a negative diagonal entry
    rc = L.smg_debug_check_sparse_cholesky(n, ptr.ctypes.data_as(C.POINTER(C.c_int)), col.ctypes.data_as(C.POINTER(C.c_int)),
                                           bad.ctypes.data_as(C.POINTER(C.c_double)), None, None, None)
    assert rc == -1


def test_schur_coarse_solver_plan_executed_on_the_host(smg_mod):
    """csrc/smg_schur.cpp (the coarse solver of the upper part of the dense range; the reference: solver.compute / solver.solve,
    src/min_quad_with_fixed_mg.cpp:47-48, src/mg_VCycle.cpp:181-201): the plan -- blocks of <= 64 rows, separator, scatter lists, sum lists of the
    Schur complement, the lists of the three solve steps -- executed on the host the way the kernels read it, against scipy's sparse LU: to
    rounding.  A Galerkin-like operator (two-ring stencil) and a one-ring one; a block-diagonal matrix (no separator) has no plan."""
    import ctypes as C
    import scipy.sparse.linalg as spla
    smg = smg_mod
    L = smg._lib.load()
    ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
    L.smg_debug_schur_solve_host.argtypes = [C.c_int, ip, ip, dp, dp, dp, ip, ip]
    rng = np.random.default_rng(3)

    def run(A):
        A = A.tocsr(); A.sort_indices()
        n = A.shape[0]
        ptr, col, val = A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data.astype(np.float64)
        b, x = rng.uniform(-1, 1, n), np.zeros(n)
        nb, ns = C.c_int(), C.c_int()
        rc = L.smg_debug_schur_solve_host(n, ptr.ctypes.data_as(ip), col.ctypes.data_as(ip), val.ctypes.data_as(dp), b.ctypes.data_as(dp), x.ctypes.data_as(dp),
                                          C.byref(nb), C.byref(ns))
        assert rc == 0
        return nb.value, ns.value, b, x

    V, F = M.read_smgm("ogre_sim.smgm")
    V = M.normalize_unit_area(V, F)
    A1 = (M.massmatrix(V, F, "barycentric") - 0.01 * M.cotmatrix(V, F)).tocsr()
    A2 = (A1 @ A1 + 1e-3 * sp.identity(A1.shape[0])).tocsr()            # SPD, two-ring pattern: what a Galerkin product looks like
    for A, sep_max in ((A1, 0.35), (A2, 0.6)):
        n = A.shape[0]
        nb, ns, b, x = run(A)
        assert nb >= n // 64 and 0 < ns <= sep_max * n, (n, nb, ns)
        ref = spla.spsolve(A.tocsc(), b)
        assert np.linalg.norm(x - ref) <= 1e-11 * np.linalg.norm(ref)
    # only the lower triangle (caller numbering) counts, as for SimplicialLDLT: garbage above the diagonal changes nothing
    Au = A1.tolil(copy=True)
    r, c = sp.triu(A1, 1).nonzero()
    Au[r[:50], c[:50]] = 7.0
    _, _, b, x = run(Au.tocsr())
    assert np.linalg.norm(x - spla.spsolve(A1.tocsc(), b)) <= 1e-11 * np.linalg.norm(x)
    nb, ns, _, _ = run(sp.identity(300, format="csr") * 2.0)
    assert nb == 0


def test_coarsest_smoothed_level_inherits_its_colouring_from_the_coarsest_level(smg_mod):
    """bunny_15K subdivided twice, three levels: the coarsest SMOOTHED level (63 210 rows) is a mid-point subdivision of the coarsest level (15 804).
    Coloured from scratch that level ends with five colours and no finer level can inherit (five launches per sweep, a from-scratch colouring of every
    finer level); the 4-colouring of the coarsest level's small graph is handed down instead (csrc/smg_precompute.cpp, colouring thread): four
    colours on every smoothed level, each a valid colouring."""
    smg = smg_mod
    V, F = M.read_smgm("bunny_15K_init.smgm")
    V = M.normalize_unit_area(V, F)
    Vf, Ff, Ps = M.subdivision_hierarchy(V, F, 2)
    A = (M.massmatrix(Vf, Ff, "barycentric") - 0.01 * M.cotmatrix(Vf, Ff)).tocsr(); A.sort_indices()
    mg = _host_precompute(smg, smg.Hierarchy.from_prolongs(Ps), A)
    assert mg.n_levels == 3 and mg.rows(1) == 63210 and mg.rows(2) == 15804
    for lv in (0, 1):
        cp = mg.colors(lv)
        assert len(cp) - 1 == 4, "level %d: %d colours" % (lv, len(cp) - 1)
        Ai = mg.matrix(lv, "A", internal=True).tocoo()
        col_of = np.searchsorted(cp, np.arange(mg.rows(lv)), side="right") - 1
        off = Ai.row != Ai.col
        assert (col_of[Ai.row[off]] != col_of[Ai.col[off]]).all()


def test_every_environment_knob_is_documented():
    """DESIGN.md section 11 lists every SMG_* variable the sources read (65 of them; round 5 documented 20), with its default -- and bench.py says which ones were
    set when it ran (`env_overrides` in its line), so that a number can be told from a number measured under a knob."""
    import glob
    import re
    names = set()
    for f in glob.glob(os.path.join(ROOT, "surface_multigrid_code_amd", "csrc", "*")):
        names |= set(re.findall(r'(?:env_int|getenv)\(\s*"(SMG_[A-Z0-9_]+)"', open(f).read()))
    for f in glob.glob(os.path.join(ROOT, "surface_multigrid_code_amd", "*.py")) + [os.path.join(ROOT, "bench.py")]:
        names |= set(re.findall(r'environ(?:\.get)?[\(\[]\s*"(SMG_[A-Z0-9_]+)"', open(f).read()))
    assert len(names) > 60
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = design[design.index("## 11. Environment knobs"):design.index("## 12.")]
    missing = sorted(n for n in names if "`%s`" % n not in sec)
    assert not missing, "knobs read by the sources but absent from DESIGN.md section 11: %s" % missing
    listed = set(re.findall(r"`(SMG_[A-Z0-9_]+)`", sec))
    stale = sorted(n for n in listed if n not in names)
    assert not stale, "knobs DESIGN.md section 11 lists that nothing reads any more: %s" % stale
