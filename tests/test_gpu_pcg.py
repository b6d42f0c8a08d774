"""GPU (-m gpu): the conjugate gradient solve preconditioned by the V-cycle (include/smg.h: smg_solve_pcg).

The host reference is tests/test_pcg_host.py::flexible_pcg -- the same loop in numpy -- with the handle's own V-cycle (mg.vcycle(r, 0), which
tests/test_gpu_parity.py holds against the oracle) as the preconditioner and the unknown system A_uu as the matrix."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from oracle import mesh_np as M
from problems import subdiv_problem
from test_gpu_parity import smg  # noqa: F401  (fixture)
from test_pcg_host import flexible_pcg, unknown_system

pytestmark = pytest.mark.gpu


def decimated(smg, name, k, kind="mcf", nVCoarsest=200, n_pins=0, seed=0):
    """the reference's hierarchy of a mesh (03_mg_solver/main.cpp:35-39) + one of its callers' systems (as tests/test_gpu_wgs.py builds it)"""
    V, F = M.read_smgm(name)
    V = M.normalize_unit_area(V, F)
    mg = smg.mg_precompute(V, F, 0.25, nVCoarsest, 1)
    n = V.shape[0]
    L = M.cotmatrix(V, F)
    rng = np.random.default_rng(seed)
    known = None
    if kind == "mcf":
        Mb = M.massmatrix(V, F, "barycentric")
        A = (Mb - 0.01 * L).tocsr()
        RHS = Mb @ rng.uniform(-1, 1, (n, k))
    else:
        A = (-L).tocsr()
        known = M.boundary_loop(F)
        if n_pins or len(known) == 0:
            known = np.sort(rng.choice(n, max(n_pins, 8), replace=False)).astype(np.int32)
        RHS = np.repeat((M.massmatrix(V, F, "voronoi") @ np.ones(n))[:, None], k, axis=1) * rng.uniform(0.5, 1.5, (1, k))
    A.sort_indices()
    return mg, A, np.asfortranarray(RHS), known


def setup(smg, **kw):
    p = subdiv_problem(**kw)
    mg = smg.Hierarchy.from_prolongs(p["Ps"])
    mg.precompute(p["A"], p["known"])
    return p, mg


def host_reference(mg, p, tol, max_iter=200, pre=2, post=2):
    unknown = mg.unknown()
    Auu, b = unknown_system(p, unknown)
    x, his, conv = flexible_pcg(Auu, b, p["z0"][unknown], lambda r: mg.vcycle(r, np.zeros_like(r), pre=pre, post=post), tol, max_iter)
    return unknown, Auu, b, x, his


def rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def check_against_host(smg, mg, p, tol, opts=None, max_iter=200):
    o = opts or smg.SolveOpts(tol=tol, max_iter=max_iter)
    conv, z, his = mg.solve_pcg(p["RHS"], p["z0"], p["known_val"], o)
    unknown, Auu, b, x, hh = host_reference(mg, p, tol, max_iter)
    assert conv
    m = min(len(his), len(hh))
    if len(his) != len(hh):
        assert abs(len(his) - len(hh)) <= 1 and any(abs(v - tol) <= 0.01 * tol for v in hh[-2:]), (len(his), len(hh), hh[-3:])
    # 1e-8 relative, above the rounding floor of a residual formed by cancellation (the last entries: a true |b - A x| near tol)
    np.testing.assert_allclose(his[:m], hh[:m], rtol=1e-8, atol=1e-14 * hh[0])
    if len(his) == len(hh):
        assert rel(z[unknown], x) <= 1e-8
    return conv, z, his, unknown, Auu, b


CASES = [dict(mesh="ogre_sim.smgm", n_sub=1, kind="mcf", k=k) for k in (1, 3, 5, 64)] + \
        [dict(mesh="torus", n_sub=2, kind="poisson", n_pins=12, k=k) for k in (1, 2)]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s-%s-k%d" % (c["mesh"], c["kind"], c["k"]))
def test_pcg_matches_host_reference_and_direct_solve(smg, case):
    tol = 1e-10
    p, mg = setup(smg, **case)
    conv, z, his, unknown, Auu, b = check_against_host(smg, mg, p, tol)
    # against a direct solve of the unknown system: the true residual is below tol, known rows are the known values exactly
    assert np.linalg.norm(b - Auu @ z[unknown]) <= tol
    if p["known"] is not None:
        assert np.array_equal(z[p["known"]], p["known_val"])
    xd = spla.spsolve(Auu.tocsc(), b)
    xd = xd.reshape(b.shape)
    cm, zm, hm = mg.solve(p["RHS"], p["z0"], p["known_val"], smg.SolveOpts(tol=tol, max_iter=200))
    assert cm and rel(z[unknown], xd) <= max(10 * rel(zm[unknown], xd), 1e-9)
    assert len(his) <= len(hm) + 1, (len(his), len(hm))


@pytest.mark.parametrize("k", [65, 100, 1100])
def test_pcg_wide_blocks_match_host_reference(smg, k):
    """widths no other case reaches: the second 64-column group of the reduction launches, and past 1024 columns the other summation path of
    the |r|^2 finalize"""
    p, mg = setup(smg, mesh="torus", n_sub=1, kind="poisson", n_pins=12, k=k)
    conv, z, his, unknown, Auu, b = check_against_host(smg, mg, p, 1e-10)
    assert np.linalg.norm(b - Auu @ z[unknown]) <= 1e-10


def test_pcg_fewer_cycles_on_ogre(smg):
    tol = 1e-10
    p, mg = setup(smg, mesh="ogre.smgm", n_sub=1, kind="poisson")
    o = smg.SolveOpts(tol=tol, max_iter=200)
    cm, zm, hm = mg.solve(p["RHS"], p["z0"], p["known_val"], o)
    cp, zp, hp = mg.solve_pcg(p["RHS"], p["z0"], p["known_val"], o)
    assert cm and cp
    assert len(hp) <= 0.6 * len(hm), (len(hp), len(hm))
    unknown = mg.unknown()
    Auu, b = unknown_system(p, unknown)
    assert np.linalg.norm(b - Auu @ zp[unknown]) <= tol


def test_pcg_fewer_cycles_on_decimated_ogre(smg):
    """the reference's own hierarchy of ogre.obj (mg_precompute defaults as in 03_mg_solver), mean-curvature-flow system"""
    tol = 1e-10
    mg, A, RHS, known = decimated(smg, "ogre.smgm", 1, kind="mcf")
    mg.precompute(A, known)
    o = smg.SolveOpts(tol=tol, max_iter=200)
    z0 = np.zeros_like(RHS)
    cm, zm, hm = mg.solve(RHS, z0, None, o)
    cp, zp, hp = mg.solve_pcg(RHS, z0, None, o)
    print("decimated ogre.obj mcf, tol 1e-10: MG %d entries, PCG %d entries" % (len(hm), len(hp)))
    assert cm and cp and len(hp) < len(hm), (len(hp), len(hm))
    assert np.linalg.norm(RHS - A @ zp) <= tol


def test_pcg_mixed_precision_reaches_fp64_accuracy(smg):
    tol = 1e-10
    p, mg = setup(smg, mesh="ogre_sim.smgm", n_sub=1, kind="mcf", k=3)
    conv, z, his = mg.solve_pcg(p["RHS"], p["z0"], None, smg.SolveOpts(tol=tol, max_iter=200, precision="mixed"))
    assert conv and np.linalg.norm(p["RHS"] - p["A"] @ z) <= tol


def test_pcg_block_hierarchy_matches_host_reference(smg):
    from test_gpu_block import elastic_like_system
    V, F = M.read_smgm("ogre_sim.smgm")
    V = M.normalize_unit_area(V, F)
    A = elastic_like_system(V, F, np.random.default_rng(5), mass=50.0)
    mg = smg.mg_precompute_block(V, F, 0.25, 100, 1)
    mg.precompute(A)
    assert mg.block_size() == 3
    RHS = np.asfortranarray(np.random.default_rng(6).uniform(-1, 1, (A.shape[0], 2)))
    p = dict(A=A, RHS=RHS, z0=np.zeros_like(RHS), known=None, known_val=None)
    check_against_host(smg, mg, p, 1e-10)


@pytest.mark.parametrize("smoother", ["gs", "jacobi", "hybrid", "chebyshev", "hybrid_chebyshev"])
def test_pcg_every_smoother_converges(smg, smoother):
    tol = 1e-10
    p, mg = setup(smg, mesh="ogre_sim.smgm", n_sub=1, kind="mcf", k=2)
    conv, z, his = mg.solve_pcg(p["RHS"], p["z0"], None, smg.SolveOpts(tol=tol, max_iter=300, smoother=smoother))
    assert conv and np.linalg.norm(p["RHS"] - p["A"] @ z) <= tol


def test_pcg_deterministic_across_graphs_polling_and_memspace(smg):
    import torch
    tol = 1e-10
    p, mg = setup(smg, mesh="torus", n_sub=2, kind="poisson", n_pins=12, k=3)
    runs = []
    for use_graph in (1, 0):
        for check_every in (0, 1, 3):
            o = smg.SolveOpts(tol=tol, max_iter=200, use_graph=use_graph, check_every=check_every)
            runs.append(mg.solve_pcg(p["RHS"], p["z0"], p["known_val"], o))
    runs.append(mg.solve_pcg(p["RHS"], p["z0"], p["known_val"], smg.SolveOpts(tol=tol, max_iter=200)))
    c0, z0_, h0 = runs[0]
    assert c0
    for c, z, h in runs[1:]:
        assert c and np.array_equal(z, z0_) and np.array_equal(h, h0)
    # SMG_DEVICE: the same bits
    dev = torch.device("cuda", 0)
    n, k = p["RHS"].shape
    t = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a).T)).to(dev)   # column-major n x k = row-major k x n
    rhs, z0, kv = t(p["RHS"]), t(p["z0"]), t(p["known_val"])
    zd = torch.empty((k, n), dtype=torch.float64, device=dev)
    o = smg.SolveOpts(tol=tol, max_iter=200)
    r_his = np.zeros(200)
    nh, cv = C.c_int(0), C.c_int(0)
    torch.cuda.synchronize()
    rc = mg.L.smg_solve_pcg(mg.h, rhs.data_ptr(), n, kv.data_ptr(), len(p["known"]), z0.data_ptr(), n, k, 1, C.byref(o.c), zd.data_ptr(), n,
                            r_his.ctypes.data_as(C.POINTER(C.c_double)), C.byref(nh), C.byref(cv))
    assert rc == 0 and cv.value == 1
    assert np.array_equal(zd.cpu().numpy().T, z0_) and np.array_equal(r_his[: nh.value], h0)


def test_pcg_does_not_disturb_mg_solves(smg):
    tol = 1e-10
    p, mg = setup(smg, mesh="ogre_sim.smgm", n_sub=1, kind="mcf", k=3)
    o = smg.SolveOpts(tol=tol, max_iter=200)
    a = mg.solve(p["RHS"], p["z0"], None, o)
    cp, zp, hp = mg.solve_pcg(p["RHS"], p["z0"], None, o)
    b = mg.solve(p["RHS"], p["z0"], None, o)
    p2, fresh = setup(smg, mesh="ogre_sim.smgm", n_sub=1, kind="mcf", k=3)
    c = fresh.solve(p["RHS"], p["z0"], None, o)
    assert cp and a[0] and b[0] and c[0]
    for x in (b, c):
        assert np.array_equal(a[1], x[1]) and np.array_equal(a[2], x[2])
    # and PCG again on the handle that has since run MG: the same bits as the first time
    cp2, zp2, hp2 = mg.solve_pcg(p["RHS"], p["z0"], None, o)
    assert np.array_equal(zp, zp2) and np.array_equal(hp, hp2)
    # r_his[0] is smg_solve's r_his[0]
    assert hp[0] == a[2][0]
    assert mg.device_bytes().get("krylov", 0) > 0 and fresh.device_bytes().get("krylov", 0) == 0


def test_pcg_edges(smg):
    p, mg = setup(smg, mesh="torus", n_sub=2, kind="poisson", n_pins=12, k=2)
    # max_iter = 0: z = z0 (known rows: the known values), no history
    conv, z, his = mg.solve_pcg(p["RHS"], p["z0"], p["known_val"], smg.SolveOpts(tol=1e-10, max_iter=0))
    unknown = mg.unknown()
    assert len(his) == 0 and np.array_equal(z[unknown], p["z0"][unknown])
    # a zero right-hand side column with a zero guess stays exactly zero
    RHS = np.asfortranarray(p["RHS"].copy())
    RHS[:, 1] = 0.0
    z0 = np.asfortranarray(p["z0"].copy())
    z0[:, 1] = 0.0
    conv, z, his = mg.solve_pcg(RHS, z0, p["known_val"], smg.SolveOpts(tol=1e-10, max_iter=200))
    assert conv and np.all(z[:, 1] == 0.0) and np.isfinite(z).all()
    # NaN in the right-hand side
    RHS[3, 0] = np.nan
    with pytest.raises(smg.SmgError) as e:
        mg.solve_pcg(RHS, z0, p["known_val"], smg.SolveOpts(tol=1e-10, max_iter=20))
    assert e.value.code == -4


def test_pcg_refuses_union_handles(smg):
    ps = [subdiv_problem(mesh="torus", n_sub=1, kind="mcf", k=1, seed=s) for s in (0, 1)]
    ms = []
    for q in ps:
        m = smg.Hierarchy.from_prolongs(q["Ps"])
        m.precompute(q["A"])
        ms.append(m)
    u = smg.Hierarchy.union(ms)
    Au = sp.block_diag([q["A"] for q in ps], format="csr")
    Au.sort_indices()
    u.precompute(Au)
    B = np.asfortranarray(np.concatenate([q["RHS"] for q in ps], axis=0))
    o = smg.SolveOpts(tol=1e-9, max_iter=60)
    before = u.solve(B, np.zeros_like(B), None, o)
    with pytest.raises(smg.SmgError) as e:
        u.solve_pcg(B, np.zeros_like(B), None, o)
    assert e.value.code == -1
    after = u.solve(B, np.zeros_like(B), None, o)
    assert before[0] and np.array_equal(before[1], after[1]) and np.array_equal(before[2], after[2])
