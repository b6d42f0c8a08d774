"""GPU (-m gpu): the LOBPCG eigensolver preconditioned by the V-cycle (include/smg.h: smg_eigs).

The checker is scipy.sparse.linalg.eigsh(A_uu, nev, M_uu, sigma=0) on the host.  X is checked by residuals computed on the host from the
returned vectors, by M-orthonormality and by principal angles against eigsh's span of each cluster -- never vector by vector.

Iteration bounds (history rows - 1) are the counts measured on an MI355X plus a margin of 50 % (rounded up): a degraded preconditioner (W = R,
a cycle on the wrong columns, a stale fp32 image) needs several times as many."""
import ctypes as C

import numpy as np
import pytest
import scipy.linalg as sl
import scipy.sparse as sp
import scipy.sparse.linalg as spla
import torch

from oracle import mesh_np as M
from test_gpu_parity import smg  # noqa: F401  (fixture)
from test_gpu_pcg import decimated

pytestmark = pytest.mark.gpu


def unknown_rows(mg, n):
    known = mg.known if mg.known is not None else np.zeros(0, np.int64)
    return np.setdiff1d(np.arange(n), np.asarray(known, dtype=np.int64))


def reference(A, mass, u, nev):
    Auu = A.tocsr()[u][:, u].tocsc()
    Muu = sp.diags(mass[u]).tocsc()
    w, V = spla.eigsh(Auu, nev + 4, Muu, sigma=0, which="LM")
    o = np.argsort(w)
    return Auu, w[o], V[:, o]


def check(A, mass, mg, evals, X, nev, tol, ev_rtol=1e-10):
    """host residuals, M-orthonormality, eigenvalues and cluster spans against eigsh; returns the reference eigenvalues"""
    n = A.shape[0]
    u = unknown_rows(mg, n)
    Auu, w, V = reference(A, mass, u, nev)
    assert np.all(np.diff(evals) >= 0)
    assert np.max(np.abs(evals - w[:nev]) / np.abs(w[:nev])) <= ev_rtol
    Xu = X[u]
    if len(u) < n:
        assert np.all(X[np.setdiff1d(np.arange(n), u)] == 0.0)
    mu = mass[u]
    assert np.abs(Xu.T @ (mu[:, None] * Xu) - np.eye(nev)).max() <= 1e-10
    R = Auu @ Xu - mu[:, None] * Xu * evals
    res = np.sqrt(np.sum(R * R / mu[:, None], axis=0)) / np.abs(evals)
    assert res.max() <= 10 * tol
    # principal angles of each cluster (relative gap 1e-6) against eigsh's span; a cluster cut by nev is compared inside the larger span
    i = 0
    while i < nev:
        j = i + 1
        while j < len(w) and abs(w[j] - w[i]) <= 1e-6 * abs(w[i]):
            j += 1
        ours = Xu[:, i:min(j, nev)] * np.sqrt(mu)[:, None]
        theirs = np.linalg.qr(V[:, i:j] * np.sqrt(mu)[:, None])[0]
        s = sl.subspace_angles(ours, theirs)
        assert np.max(s) <= 1e-4, (i, j, s)
        i = j
    return w[:nev]


def torus_mcf(smg, delta=0.01):
    V, F = M.torus(24, 16)
    V = M.normalize_unit_area(V, F)
    Vf, Ff, Ps = M.subdivision_hierarchy(V, F, 2)
    mass = np.asarray(M.massmatrix(Vf, Ff, "barycentric").diagonal())
    A = (sp.diags(mass) - delta * M.cotmatrix(Vf, Ff)).tocsr()
    A.sort_indices()
    mg = smg.Hierarchy.from_prolongs(Ps)
    mg.precompute(A, None)
    return mg, A, mass


def test_torus_mcf(smg):
    mg, A, mass = torus_mcf(smg)
    opts = smg.SolveOpts(tol=1e-8, max_iter=100)
    evals, X, his, nconv = mg.eigs(mass, 8, opts=opts)
    print("torus: rows", his.shape[0], "evals", evals)
    assert nconv == 8 and np.all(his[-1] <= 1e-8)
    assert his.shape[0] - 1 <= 24          # measured 16
    check(A, mass, mg, evals, X, 8, 1e-8)
    # the recipe of smg.h: Laplace-Beltrami eigenvalues (mu - 1) / delta; the first is the constant's 0
    lb = (evals - 1.0) / 0.01
    assert abs(lb[0]) <= 1e-6 * lb[1]


@pytest.mark.parametrize("block", [22, 64])
def test_torus_mcf_wide_blocks(smg, block):
    """block = 22: the 3 m = 66 basis columns cross a 64-column Gram tile edge; block = 64: 3 x 3 Gram tiles and four combine column chunks"""
    mg, A, mass = torus_mcf(smg)
    evals, X, his, nconv = mg.eigs(mass, 8, block=block, opts=smg.SolveOpts(tol=1e-8, max_iter=100))
    print("torus block %d: rows" % block, his.shape[0])
    assert nconv == 8 and np.all(his[-1] <= 1e-8)
    check(A, mass, mg, evals, X, 8, 1e-8)


def test_mixed_precision_same_eigenvalues(smg):
    mg, A, mass = torus_mcf(smg)
    e64, _, _, _ = mg.eigs(mass, 8, opts=smg.SolveOpts(tol=1e-8, max_iter=100))
    e32, X, his, nconv = mg.eigs(mass, 8, opts=smg.SolveOpts(tol=1e-8, max_iter=100, precision="mixed"))
    print("mixed: rows", his.shape[0])
    assert nconv == 8
    assert his.shape[0] - 1 <= 24          # measured 16
    assert np.max(np.abs(e32 - e64) / e64) <= 1e-10


def test_bunny_poisson_with_boundary(smg):
    mg, A, _, known = decimated(smg, "bunny.smgm", 1, kind="poisson")
    mg.precompute(A, known)
    V, F = M.read_smgm("bunny.smgm")
    V = M.normalize_unit_area(V, F)
    mass = np.asarray(M.massmatrix(V, F, "voronoi").diagonal())
    evals, X, his, nconv = mg.eigs(mass, 16, opts=smg.SolveOpts(tol=1e-8, max_iter=200))
    print("bunny: rows", his.shape[0])
    assert nconv == 16
    assert his.shape[0] - 1 <= 17          # measured 11
    check(A, mass, mg, evals, X, 16, 1e-8)


def test_closed_bunny_clustered(smg):
    mg, A, _, _ = decimated(smg, "bunny_15K_init.smgm", 1, kind="mcf")
    mg.precompute(A, None)
    V, F = M.read_smgm("bunny_15K_init.smgm")
    V = M.normalize_unit_area(V, F)
    mass = np.asarray(M.massmatrix(V, F, "barycentric").diagonal())
    evals, X, his, nconv = mg.eigs(mass, 24, opts=smg.SolveOpts(tol=1e-8, max_iter=300))
    print("bunny15K: rows", his.shape[0])
    assert nconv == 24
    assert his.shape[0] - 1 <= 24          # measured 16
    w = check(A, mass, mg, evals, X, 24, 1e-8)
    lb, lb_ref = (evals - 1.0) / 0.01, (w - 1.0) / 0.01
    assert abs(lb[0]) <= 1e-6 * lb[1]
    assert np.max(np.abs(lb[1:] - lb_ref[1:]) / lb_ref[1:]) <= 1e-8


def test_block_hierarchy_multiplicities(smg):
    V, F = M.read_smgm("ogre_sim.smgm")
    V = M.normalize_unit_area(V, F)
    mgb = smg.mg_precompute_block(V, F, 0.25, 200, 1)
    nv = V.shape[0]
    mb = np.asarray(M.massmatrix(V, F, "barycentric").diagonal())
    Ab = sp.kron(sp.diags(mb) - 0.01 * M.cotmatrix(V, F), sp.eye(3)).tocsr()
    Ab.sort_indices()
    mgb.set_block_mode("block")      # kron(S, I_3) would take the scalar path by default
    mgb.precompute(Ab, None)
    assert mgb.block_size() == 3
    mass = np.repeat(mb, 3)
    evals, X, his, nconv = mgb.eigs(mass, 6, block=12, opts=smg.SolveOpts(tol=1e-8, max_iter=200))   # whole triples in the block
    print("block: rows", his.shape[0], evals)
    assert nconv == 6
    assert his.shape[0] - 1 <= 32          # measured 21
    check(Ab, mass, mgb, evals, X, 6, 1e-8)
    assert nv * 3 == X.shape[0]
    # every eigenvalue of M - delta L appears three times (x, y, z)
    assert np.max(np.abs(evals[0:3] - evals[0])) <= 1e-10 * evals[0] and np.max(np.abs(evals[3:6] - evals[3])) <= 1e-10 * evals[3]


def test_deterministic_graphs_and_memspace(smg):
    mg, A, mass = torus_mcf(smg)
    o_on = smg.SolveOpts(tol=1e-8, max_iter=100, use_graph=1)
    o_off = smg.SolveOpts(tol=1e-8, max_iter=100, use_graph=0)
    a = mg.eigs(mass, 8, opts=o_on)
    b = mg.eigs(mass, 8, opts=o_on)
    c = mg.eigs(mass, 8, opts=o_off)
    n = A.shape[0]
    dm = torch.tensor(mass, device="cuda")
    dX = torch.zeros((8, n), dtype=torch.float64, device="cuda")     # column-major n x 8
    ev, his, _ = mg.eigs_device(dm.data_ptr(), dX.data_ptr(), n, 8, opts=o_on)
    torch.cuda.synchronize()
    Xd = dX.cpu().numpy().T
    for other in (b, c):
        assert a[0].tobytes() == other[0].tobytes() and a[1].tobytes() == other[1].tobytes() and a[2].tobytes() == other[2].tobytes()
    assert a[0].tobytes() == ev.tobytes() and np.asfortranarray(Xd).tobytes() == a[1].tobytes() and a[2].tobytes() == his.tobytes()


def test_warm_start_is_converged_at_row_0(smg):
    mg, A, mass = torus_mcf(smg)
    opts = smg.SolveOpts(tol=1e-8, max_iter=100)
    evals, X, his, _ = mg.eigs(mass, 8, block=8, opts=opts)
    e2, X2, his2, nconv = mg.eigs(mass, 8, block=8, X0=X, opts=opts)
    assert his2.shape[0] == 1 and nconv == 8 and np.all(his2[0] <= 1e-8)
    # block = 0 with a start block: the block is X0's column count (smg_eigs reads n x block doubles from X0)
    e3, X3, his3, nconv3 = mg.eigs(mass, 8, X0=X, opts=opts)
    assert his3.shape[0] == 1 and nconv3 == 8
    with pytest.raises(ValueError):
        mg.eigs(mass, 8, block=16, X0=X, opts=opts)
    with pytest.raises(ValueError):
        mg.eigs_device(0, 0, A.shape[0], 8, X0_ptr=1)


def test_full_size_c3_parent(smg):
    """the 252 834-vertex parent of C3 (bunny_15K_init x2, subdivision hierarchy): eig_groups at its cap, Gram partials of tens of MB"""
    from surface_multigrid_code_amd import mesh
    V, F = mesh.read_triangle_mesh("bunny_15K_init.smgm")
    V = mesh.normalize_unit_area(V, F)
    mg, Vf, Ff = smg.mg_precompute_subdiv(V, F, 2, ratio=0.25, nVCoarsest=1000, n_extra_levels=1)
    mass = np.asarray(mesh.massmatrix(Vf, Ff, "barycentric").diagonal())
    A = (sp.diags(mass) - 0.01 * mesh.cotmatrix(Vf, Ff)).tocsr()
    A.sort_indices()
    mg.precompute(A)
    assert A.shape[0] == 252834
    tol = 1e-6
    evals, X, his, nconv = mg.eigs(mass, 8, opts=smg.SolveOpts(tol=tol, max_iter=100))
    print("C3 parent: rows", his.shape[0], evals)
    assert nconv == 8
    assert his.shape[0] - 1 <= C3_PARENT_MAX_ITERS
    assert np.abs(X.T @ (mass[:, None] * X) - np.eye(8)).max() <= 1e-10
    R = A @ X - mass[:, None] * X * evals
    res = np.sqrt(np.sum(R * R / mass[:, None], axis=0)) / np.abs(evals)
    assert res.max() <= 10 * tol
    assert abs((evals[0] - 1.0) / 0.01) <= 1e-4 * (evals[1] - 1.0) / 0.01     # the closed mesh's constant mode


C3_PARENT_MAX_ITERS = 18          # measured 12


def test_refusals_and_isolation(smg):
    mg, A, mass = torus_mcf(smg)
    n = A.shape[0]
    rng = np.random.default_rng(1)
    RHS = np.asfortranarray(rng.uniform(-1, 1, (n, 2)))
    z0 = np.zeros((n, 2), order="F")
    o = smg.SolveOpts(tol=1e-10, max_iter=30)
    assert "eigs" not in mg.device_bytes() or mg.device_bytes()["eigs"] == 0
    before = (mg.solve(RHS, z0, opts=o), mg.solve_pcg(RHS, z0, opts=o))
    bytes_before = mg.device_bytes()
    for kw in (dict(nev=0), dict(nev=4, block=3), dict(nev=4, block=65)):
        with pytest.raises(smg.SmgError) as e:
            mg.eigs(mass, kw.pop("nev"), **kw)
        assert e.value.code == -1
    bad = mass.copy()
    bad[5] = 0.0
    with pytest.raises(smg.SmgError) as e:
        mg.eigs(bad, 4)
    assert e.value.code == -1
    # a call during a split-phase solve
    L = mg.L
    oc = smg.SolveOpts(tol=1e-10, max_iter=5)
    assert L.smg_solve_begin(mg.h, RHS.ctypes.data, n, None, 0, z0.ctypes.data, n, 2, 0, C.byref(oc.c)) == 0
    with pytest.raises(smg.SmgError) as e:
        mg.eigs(mass, 4)
    assert e.value.code == -1
    z = np.zeros((n, 2), order="F")
    his, nh, cv = np.zeros(5), C.c_int(0), C.c_int(0)
    assert L.smg_solve_end(mg.h, z.ctypes.data, n, 0, his.ctypes.data_as(C.POINTER(C.c_double)), C.byref(nh), C.byref(cv)) == 0
    # a refused call changes nothing of the handle
    assert mg.device_bytes() == bytes_before
    mg.eigs(mass, 8, opts=smg.SolveOpts(tol=1e-6, max_iter=50))
    assert mg.device_bytes()["eigs"] > 0
    after = (mg.solve(RHS, z0, opts=o), mg.solve_pcg(RHS, z0, opts=o))
    for x, y in zip(before, after):
        assert x[1].tobytes() == y[1].tobytes() and x[2].tobytes() == y[2].tobytes()


def test_refusals_union_and_small_systems(smg):
    from test_gpu_union import members
    ms, As, _ = members(smg, 1)
    u = smg.Hierarchy.union(ms)
    Au = sp.block_diag(As, format="csr")
    Au.sort_indices()
    u.precompute(Au)
    with pytest.raises(smg.SmgError) as e:
        u.eigs(np.ones(Au.shape[0]), 4)
    assert e.value.code == -1
    # fewer unknowns than the block: a 64-column block on a mesh whose boundary leaves few unknowns is refused, 8 columns are not
    V, F = M.torus(4, 3)
    V = M.normalize_unit_area(V, F)
    Vf, Ff, Ps = M.subdivision_hierarchy(V, F, 1)
    mass = np.asarray(M.massmatrix(Vf, Ff, "barycentric").diagonal())
    A = (sp.diags(mass) - 0.01 * M.cotmatrix(Vf, Ff)).tocsr()
    A.sort_indices()
    mg = smg.Hierarchy.from_prolongs(Ps)
    mg.precompute(A, None)
    assert A.shape[0] < 64
    with pytest.raises(smg.SmgError) as e:
        mg.eigs(mass, 4, block=64)
    assert e.value.code == -1
    evals, X, his, nconv = mg.eigs(mass, 4, block=8, opts=smg.SolveOpts(tol=1e-8, max_iter=100))
    assert nconv == 4
