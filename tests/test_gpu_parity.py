"""GPU (-m gpu): parity of the HIP path (through the C ABI) with the CPU oracle.

Parity contract:
  K-level  SpMV / restrict / prolong / GS sweep: BIT-EXACT against the oracle run on the level's matrix in the
           device numbering (same ascending-column accumulation, no FMA contraction), <= 1e-14 relative against the
           oracle in the caller's numbering (summation order only);
  norm / coarse solve: <= 1e-12 relative (tree reduction / explicit inverse instead of LDL^T);
  solve-level: both reach the tolerance; relative solution difference <= 1e-8 at tol 1e-10, iteration counts within
           +-2 of the lexicographic-GS reference run; golden r_his of the restatement reproduced by the oracle and
           bracketed by the GPU run.
"""
import os

import numpy as np
import pytest
import scipy.sparse as sp

from problems import _path_interp, _path_matrix, random_spd_hierarchy as _random_spd_hierarchy, subdiv_problem

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def smg(smg_mod):
    assert smg_mod._lib.load().smg_device_count() > 0, "GPU tests need a HIP device (no CPU fallback exists)"
    return smg_mod


def build(smg, oracle_mod, **kw):
    p = subdiv_problem(**kw)
    mg = smg.Hierarchy.from_prolongs(p["Ps"])
    mg.precompute(p["A"], p["known"])
    orc = oracle_mod.OracleMG(p["Ps"])
    orc.precompute(p["A"], p["known"])
    return p, mg, orc


def oracle_on_device_numbering(oracle_mod, mg, lv):
    """An oracle whose level 0 is level `lv` of the hierarchy IN THE DEVICE NUMBERING (so that the reference's
    lexicographic sweep on it is the multi-colour sweep the GPU runs)."""
    A = mg.matrix(lv, "A", internal=True)
    P = mg.matrix(lv + 1, "P", internal=True)
    o = oracle_mod.OracleMG([P])
    o.precompute(A)
    return o


def gs_bit_exact(oracle_mod, mg, lv, b, x, iters):
    """relax() against the oracle's lexicographic sweep on level lv IN THE ORDER THE DEVICE SWEEPS IT: the internal (colour-major) numbering, or --
    where the level sweeps piece-wise (csrc/smg_wgs.hpp) / block-wise (csrc/smg_bgs.hpp) -- that order, mg.gs_order()."""
    order = mg.gs_order(lv, b.shape[1])          # position -> internal row
    to = mg.perm(lv)[order]                      # position -> caller
    A = mg.matrix(lv, "A", internal=True).tocsr()
    P = mg.matrix(lv + 1, "P", internal=True).tocsr()
    o = oracle_mod.OracleMG([P[order]])
    o.precompute(A[order][:, order].tocsr())
    return np.array_equal(mg.relax(lv, b, x, iters)[to], o.relax(0, b[to], x[to], iters))


# ----------------------------------------------------------------------------------------------- K-level, bitwise
@pytest.mark.parametrize("kind,k", [("mcf", 1), ("mcf", 3), ("poisson", 2), ("mcf", 6), ("mcf", 8), ("poisson", 27), ("mcf", 64)])
def test_kernels_bit_exact_in_device_numbering(smg, oracle_mod, kind, k):
    p, mg, orc = build(smg, oracle_mod, kind=kind, k=k, n_sub=2)
    rng = np.random.default_rng(3)
    for lv in range(mg.n_levels - 1):
        n, nc = mg.rows(lv), mg.rows(lv + 1)
        perm, permc = mg.perm(lv), mg.perm(lv + 1)
        oi = oracle_on_device_numbering(oracle_mod, mg, lv)
        x, b, xc = rng.uniform(-1, 1, (n, k)), rng.uniform(-1, 1, (n, k)), rng.uniform(-1, 1, (nc, k))
        # y = A x
        assert np.array_equal(mg.A(lv, x)[perm], oi.A(0, x[perm])), "SpMV not bit-exact on level %d" % lv
        # Gauss-Seidel: 1 and 3 sweeps
        for iters in (1, 3):
            assert gs_bit_exact(oracle_mod, mg, lv, b, x, iters), "GS sweep not bit-exact on level %d" % lv
        # restriction / prolongation with the explicitly stored PT / P
        assert np.array_equal(mg.restrict(lv, x)[permc], oi.restrict(0, x[perm]))
        assert np.array_equal(mg.prolong(lv, xc)[perm], oi.prolong(0, xc[permc]))
        # same kernels against the oracle in the caller's numbering: summation order only
        for got, ref in ((mg.A(lv, x), orc.A(lv, x)), (mg.restrict(lv, x), orc.restrict(lv, x)),
                         (mg.prolong(lv, xc), orc.prolong(lv, xc))):
            assert abs(got - ref).max() <= 1e-14 * max(abs(ref).max(), 1e-300) * 8
        # residual norm (tree reduction)
        rn = mg.residual_norm(lv, b, x)
        ref = np.linalg.norm(b - orc.A(lv, x))
        assert abs(rn - ref) <= 1e-13 * ref


def test_colouring_is_valid_and_sell_matches_csr(smg, oracle_mod):
    p, mg, orc = build(smg, oracle_mod, kind="mcf", k=1, n_sub=2)
    for lv in range(mg.n_levels - 1):
        A = mg.matrix(lv, "A", internal=True).tocsr()
        cp = mg.colors(lv)
        assert cp[0] == 0 and cp[-1] == mg.rows(lv) and 3 <= len(cp) - 1 <= 12
        Ac = A.tocoo()
        color_of = np.searchsorted(cp, np.arange(mg.rows(lv)), side="right") - 1
        off = Ac.row != Ac.col
        assert (color_of[Ac.row[off]] != color_of[Ac.col[off]]).all(), "two coupled rows share a colour"
        # internal matrix is the caller matrix under the permutation
        perm = mg.perm(lv)
        Ac2 = mg.matrix(lv, "A").tocsr()[perm][:, perm]
        assert abs(Ac2 - A).max() == 0
        st = mg.sell_stats(lv, "A")
        assert st["stored"] == A.nnz and st["padded"] >= st["stored"]
        if mg.rows(lv) > 20000:
            assert st["padded"] / st["stored"] < 1.10, "SELL padding above 10%"


@pytest.mark.parametrize("k", [1, 2, 7, 8, 12, 16, 40, 64, 91])
def test_coarse_solve_matches_ldlt(smg, oracle_mod, k):
    """k = 1: lower triangle of the symmetric inverse; 2..7: one wave per row; >= 8: 16 x 16 tiles on the fp64 matrix cores (blocks of
    64 / 32 / 16 columns, a block of 8..15 columns as a 16-column tile with idle lanes: 12, 40 = 32 + 8, 91 = 64 + 16 + 11)."""
    p, mg, orc = build(smg, oracle_mod, kind="poisson", k=2, n_sub=2)
    rng = np.random.default_rng(5)
    nc = mg.rows(mg.n_levels - 1)
    B, u = rng.uniform(-1, 1, (nc, k)), rng.uniform(-1, 1, (nc, k))
    got, ref = mg.coarse_solve(B, u), orc.coarse_solve(B, u)
    assert abs(got - ref).max() <= 1e-11 * abs(ref).max()


# ----------------------------------------------------------------------------------------------- V-cycle
@pytest.mark.parametrize("kind,k", [("mcf", 1), ("poisson", 1), ("mcf", 3)])
def test_vcycle_matches_oracle_in_device_numbering(smg, oracle_mod, kind, k):
    """One V(2,2) cycle on the 2-level hierarchy (level L-2 -> coarsest): the oracle runs the reference algorithm on
    the renumbered system; everything but the coarse solve is bit-exact, the cycle agrees to 1e-11."""
    p, mg, orc = build(smg, oracle_mod, kind=kind, k=k, n_sub=2)
    lv = mg.n_levels - 2
    oi = oracle_on_device_numbering(oracle_mod, mg, lv)
    rng = np.random.default_rng(9)
    n = mg.rows(lv)
    perm = mg.perm(lv)
    B, u = rng.uniform(-1, 1, (n, k)), rng.uniform(-1, 1, (n, k))
    got = mg.vcycle(B, u, lv=lv)[perm]
    ref = oi.vcycle(B[perm], u[perm], lv=0)
    assert abs(got - ref).max() <= 1e-11 * abs(ref).max()
    # full-depth cycle against the oracle in the caller's numbering: same contraction to rounding of the smoother order
    B0, u0 = rng.uniform(-1, 1, (mg.rows(0), k)), np.zeros((mg.rows(0), k))
    r_gpu = np.linalg.norm(B0 - orc.A(0, mg.vcycle(B0, u0)))
    r_ref = np.linalg.norm(B0 - orc.A(0, orc.vcycle(B0, u0)))
    assert r_gpu < 2.0 * r_ref and r_gpu < 0.5 * np.linalg.norm(B0)


# ----------------------------------------------------------------------------------------------- solve level
@pytest.mark.parametrize("kind,k,tol", [("mcf", 3, 5e-7), ("poisson", 1, 1e-10), ("poisson", 2, 1e-3), ("mcf", 1, 1e-10)])
def test_solve_matches_reference_algorithm(smg, oracle_mod, kind, k, tol):
    p, mg, orc = build(smg, oracle_mod, kind=kind, k=k, n_sub=2)
    opts = smg.SolveOpts(tol=tol, max_iter=40)
    conv, z, rh = mg.solve(p["RHS"], p["z0"], p["known_val"], opts)
    conv2, z2, rh2 = orc.solve(p["RHS"], p["z0"], p["known_val"], tol=tol, max_iter=40)
    assert conv and conv2
    assert abs(len(rh) - len(rh2)) <= 2
    assert abs(rh[0] - rh2[0]) <= 1e-12 * rh2[0]            # same initial residual
    assert rh[-1] < tol and (np.diff(rh) < 0).all()
    # A SPD: ||z_gpu - z_ref|| <= (r_gpu + r_ref) / lambda_min; stated bound: 1e-8 rel at tol 1e-10
    rel = np.linalg.norm(z - z2) / np.linalg.norm(z2)
    assert rel <= (1e-8 if tol <= 1e-9 else 1e-3)
    if p["known"] is not None:
        assert np.array_equal(z[p["known"]], p["known_val"])
    # the residual the GPU reports is the true residual of what it returned
    A = p["A"]
    if p["known"] is None:
        true = np.linalg.norm(p["RHS"] - A @ z)
        assert true < tol * 1.5 + 1e-15


def test_golden_residual_histories(smg, oracle_mod):
    """The restatement-derived goldens: lexicographic GS history; the multi-colour GPU history starts from the same
    residual, needs the same number of cycles (+-2) and lands on the same solution."""
    g1 = np.load(os.path.join(G, "g1_mcf_k3.npz"))
    p, mg, orc = build(smg, oracle_mod, kind="mcf", k=3, n_sub=2)
    conv, z, rh = mg.solve(p["RHS"], p["z0"], None, smg.SolveOpts(tol=5e-7, max_iter=20))
    assert conv and abs(len(rh) - len(g1["r_his"])) <= 2 and abs(rh[0] - g1["r_his"][0]) < 1e-12 * rh[0]
    assert abs(np.linalg.norm(z) - g1["z_norm"]) < 1e-6 * g1["z_norm"]
    g2 = np.load(os.path.join(G, "g2_poisson_bd.npz"))
    p, mg, orc = build(smg, oracle_mod, kind="poisson", k=1, n_sub=2)
    conv, z, rh = mg.solve(p["RHS"], p["z0"], p["known_val"], smg.SolveOpts(tol=1e-10, max_iter=30))
    assert conv and abs(len(rh) - len(g2["r_his"])) <= 2 and abs(rh[0] - g2["r_his"][0]) < 1e-12 * rh[0]
    np.testing.assert_allclose(z[g2["idx"], 0], g2["z_samples"], rtol=0, atol=1e-8 * g2["z_norm"])


def test_outer_loop_bookkeeping_matches_reference(smg, oracle_mod):
    p, mg, orc = build(smg, oracle_mod, kind="mcf", k=1, n_sub=1)
    # exhausts max_iter: r_his has max_iter entries, converged False, last cycle's effect not measured
    conv, z, rh = mg.solve(p["RHS"], p["z0"], None, smg.SolveOpts(tol=1e-30, max_iter=3))
    assert not conv and len(rh) == 3
    # already converged: one entry, no cycle executed, z == z0 bitwise
    conv, z, rh = mg.solve(p["RHS"], p["z0"], None, smg.SolveOpts(tol=1e30, max_iter=5))
    assert conv and len(rh) == 1 and np.array_equal(z, p["z0"])
    # the device-side break is independent of how often the host polls, and of graph replay vs eager launches
    ref = None
    for check_every, use_graph in ((1, 1), (0, 1), (4, 1), (50, 1), (1, 0), (0, 0), (7, 0)):      # 0: adaptive polling (the default)
        conv, z, rh = mg.solve(p["RHS"], p["z0"], None,
                               smg.SolveOpts(tol=1e-9, max_iter=50, check_every=check_every, use_graph=use_graph))
        assert conv
        if ref is None:
            ref = (z, rh)
        else:
            assert np.array_equal(z, ref[0]) and np.array_equal(rh, ref[1]), "result depends on polling/graph mode"


def test_deterministic_and_reentrant(smg, oracle_mod):
    p, mg, orc = build(smg, oracle_mod, kind="poisson", k=2, n_sub=2)
    o = smg.SolveOpts(tol=1e-9, max_iter=30)
    a = mg.solve(p["RHS"], p["z0"], p["known_val"], o)
    b = mg.solve(p["RHS"], p["z0"], p["known_val"], o)
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    # re-precompute with another matrix on the same handle (time-stepping callers, 05_example.../main.cpp:74)
    A2 = (p["A"] + 0.5 * sp.eye(p["A"].shape[0])).tocsr()
    mg.precompute(A2, p["known"])
    orc.precompute(A2, p["known"])
    c = mg.solve(p["RHS"], p["z0"], p["known_val"], o)
    d = orc.solve(p["RHS"], p["z0"], p["known_val"], tol=1e-9, max_iter=30)
    assert c[0] and np.linalg.norm(c[1] - d[1]) <= 1e-7 * np.linalg.norm(d[1])
    # and back without constraints on the same handle: restarts from P_full
    pm = subdiv_problem(kind="mcf", k=2, n_sub=2)
    mg.precompute(pm["A"], None)
    e = mg.solve(pm["RHS"], pm["z0"], None, o)
    assert e[0] and mg.rows(0) == pm["A"].shape[0]


def test_profc_scopes(smg, oracle_mod):
    p, mg, orc = build(smg, oracle_mod, kind="mcf", k=1, n_sub=2)
    mg.prof_enable(True)
    mg.solve(p["RHS"], p["z0"], None, smg.SolveOpts(tol=0.0, max_iter=3))
    t = mg.prof_table()
    mg.prof_enable(False)
    # reference scope names (src/mg_VCycle.cpp:121, src/min_quad_with_fixed_mg.cpp:123)
    assert t["MG: total VCycle"][0] == 3
    assert t["MG: relaxation"][0] == 3 * 2 * (mg.n_levels - 1)
    assert t["MG: relaxation"][1] > 0 and t["MG: total VCycle"][1] >= t["MG: relaxation"][1]


def test_decimated_hierarchy_bunny_poisson(smg, oracle_mod):
    """BASELINE config C1: bunny.obj Poisson with the boundary loop pinned (03_mg_solver), hierarchy from
    smg_mg_precompute (libsmg's own decimator), tol 1e-3 / maxIter 20 defaults."""
    from oracle import mesh_np as M
    mesh = smg.mesh
    V, F = mesh.read_triangle_mesh("bunny.smgm")
    V = mesh.normalize_unit_area(V, F)
    mg = smg.mg_precompute(V, F, 0.25, 500, 1)
    A = (-M.cotmatrix(V, F)).tocsr()
    b = M.boundary_loop(F)
    n = V.shape[0]
    B = M.massmatrix(V, F, "voronoi") @ np.ones(n)
    B[b] = 0.0
    data = smg.min_quad_with_fixed_mg_precompute(A, b, mg)
    assert data.n == n and len(data.unknown) == n - 149
    conv, z, rh = smg.min_quad_with_fixed_mg_solve(data, B, np.zeros(len(b)), np.zeros(n), mg)
    Ps = [mg.matrix(l, "P_full") for l in range(1, mg.n_levels)]
    orc = oracle_mod.OracleMG(Ps)
    orc.precompute(A, b)
    conv2, z2, rh2 = orc.solve(B, np.zeros(n), np.zeros(len(b)), tol=1e-3, max_iter=20)
    assert conv and conv2 and abs(len(rh) - len(rh2)) <= 2
    assert np.linalg.norm(z - z2) <= 1e-3 * np.linalg.norm(z2)
    # tight solve: same solution to 1e-8
    conv, z, rh = mg.solve(B, np.zeros(n), np.zeros(len(b)), smg.SolveOpts(tol=1e-10, max_iter=40))
    conv2, z2, rh2 = orc.solve(B, np.zeros(n), np.zeros(len(b)), tol=1e-10, max_iter=40)
    assert conv and conv2 and np.linalg.norm(z - z2) <= 1e-8 * np.linalg.norm(z2)


def test_many_columns(smg, oracle_mod):
    """BASELINE config C4 flavour at test size: k = 16 right-hand sides (5 column chunks), one Frobenius residual."""
    p, mg, orc = build(smg, oracle_mod, kind="mcf", k=16, n_sub=1)
    conv, z, rh = mg.solve(p["RHS"], p["z0"], None, smg.SolveOpts(tol=5e-7, max_iter=30))
    conv2, z2, rh2 = orc.solve(p["RHS"], p["z0"], tol=5e-7, max_iter=30)
    assert conv and conv2 and abs(len(rh) - len(rh2)) <= 2
    assert np.linalg.norm(z - z2) <= 1e-5 * np.linalg.norm(z2)
    # columns are independent: solving a subset alone gives the same per-column V-cycle iterates
    u_all = mg.vcycle(p["RHS"], p["z0"])
    u_one = mg.vcycle(p["RHS"][:, 5], p["z0"][:, 5])
    assert abs(u_all[:, 5] - u_one[:, 0]).max() <= 1e-12 * abs(u_one).max()
    assert np.array_equal(mg.relax(0, p["RHS"], p["z0"], 2)[:, 5], mg.relax(0, p["RHS"][:, 5], p["z0"][:, 5], 2)[:, 0])


def test_split_phase_api_equals_fused_solve(smg, oracle_mod):
    """The multi-GPU form of the loop (residual | all-reduce | decide + cycle) with a no-op reduction must reproduce
    smg_solve bit for bit; device-resident column-major inputs through torch tensors."""
    import torch
    from surface_multigrid_code_amd.dist import GpuEngine, sharded_solve
    p, mg, orc = build(smg, oracle_mod, kind="poisson", k=3, n_sub=2)
    opts = smg.SolveOpts(tol=1e-9, max_iter=30)
    conv, z, rh = mg.solve(p["RHS"], p["z0"], p["known_val"], opts)
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(st):
        mg.set_stream(st.cuda_stream)
        # (k, n) contiguous == column-major n x k with ld = n
        rhs = torch.from_numpy(np.ascontiguousarray(p["RHS"].T)).to(dev)
        z0 = torch.from_numpy(np.ascontiguousarray(p["z0"].T)).to(dev)
        kv = torch.from_numpy(np.ascontiguousarray(p["known_val"].T)).to(dev)
        eng = GpuEngine(mg, rhs, z0, kv, opts)
        conv2, z2, rh2 = sharded_solve(eng, 30, lambda t: None, check_every=3)
        torch.cuda.synchronize()
    assert conv2 == conv and np.array_equal(rh2, rh)
    assert np.array_equal(z2.cpu().numpy().T, z)
    mg.set_stream(None)


def test_error_paths(smg, oracle_mod):
    p = subdiv_problem(kind="mcf", k=1, n_sub=1)
    mg = smg.Hierarchy.from_prolongs(p["Ps"])
    with pytest.raises(smg.SmgError):            # solve before precompute
        mg.solve(p["RHS"], p["z0"])
    mg.precompute(p["A"])
    with pytest.raises(smg.SmgError):            # negative max_iter (any non-negative count is legal, tests/test_gpu_smoothers.py)
        mg.solve(p["RHS"], p["z0"], None, smg.SolveOpts(max_iter=-1))
    with pytest.raises(smg.SmgError):            # unknown smoother / damping out of range
        mg.set_smoother(2, 2.5)
    with pytest.raises(smg.SmgError):            # matrix size does not match P_1
        mg.precompute(p["A"][:100, :100].tocsr())
    mg.precompute(p["A"])
    # NaN in the right-hand side: reported, not looped on
    bad = p["RHS"].copy()
    bad[5, 0] = np.nan
    with pytest.raises(smg.SmgError) as e:
        mg.solve(bad, p["z0"])
    assert e.value.code == -4
    # a handle stays usable after an error
    conv, z, rh = mg.solve(p["RHS"], p["z0"], None, smg.SolveOpts(tol=1e-8, max_iter=30))
    assert conv
    # max_iter = 0: nothing measured, nothing executed (the reference would read an uninitialised residual)
    conv, z, rh = mg.solve(p["RHS"], p["z0"], None, smg.SolveOpts(tol=1e-8, max_iter=0))
    assert len(rh) == 0 and np.array_equal(z, p["z0"])


def test_c2_closed_mesh_with_pins(smg, oracle_mod):
    """BASELINE config C2 (04_mg_solver_nobd): closed surface, 346 pinned vertices (the size of hilbert_cube_known.obj;
    hilbert_cube.obj itself is missing from the reference checkout), z0 uniform(-1,1), tol 1e-10."""
    from oracle import mesh_np as M
    mesh = smg.mesh
    V, F = mesh.read_triangle_mesh("bunny_15K_init.smgm")
    V = mesh.normalize_unit_area(V, F)
    n = V.shape[0]
    assert len(M.boundary_loop(F)) == 0
    rng = np.random.default_rng(0)
    b = rng.choice(n, size=346, replace=False).astype(np.int32)
    mg = smg.mg_precompute(V, F, 0.25, 500, 1)
    A = (-M.cotmatrix(V, F)).tocsr()
    B = M.massmatrix(V, F, "voronoi") @ np.ones(n)
    B[b] = 0.0
    z0 = np.random.default_rng(1).uniform(-1, 1, n)
    mg.precompute(A, b)
    conv, z, rh = mg.solve(B, z0, np.zeros(346), smg.SolveOpts(tol=1e-10, max_iter=60))
    Ps = [mg.matrix(l, "P_full") for l in range(1, mg.n_levels)]
    orc = oracle_mod.OracleMG(Ps)
    orc.precompute(A, b)
    conv2, z2, rh2 = orc.solve(B, z0, np.zeros(346), tol=1e-10, max_iter=60)
    assert conv and conv2 and abs(len(rh) - len(rh2)) <= 3
    assert np.linalg.norm(z - z2) <= 1e-8 * np.linalg.norm(z2)
    assert np.array_equal(z[b, 0], np.zeros(346))


def test_c4_mean_curvature_flow_k64(smg, oracle_mod):
    """BASELINE config C4: ogre.obj (beard_man.obj is missing), LHS = M_bary - 0.01 L, 64 right-hand sides
    (3 coordinate columns + 61 random ones), tol 5e-7; column blocks solved separately give the same per-column result."""
    from oracle import mesh_np as M
    mesh = smg.mesh
    V, F = mesh.read_triangle_mesh("ogre.smgm")
    V = mesh.normalize_unit_area(V, F)
    n = V.shape[0]
    mg = smg.mg_precompute(V, F, 0.25, 500, 1)
    L = M.cotmatrix(V, F)
    Mb = M.massmatrix(V, F, "barycentric")
    A = (Mb - 0.01 * L).tocsr()
    X = np.concatenate([V] + [np.random.default_rng(100 + j).uniform(-1, 1, (n, 1)) for j in range(61)], axis=1)
    RHS = np.asfortranarray(Mb @ X)
    z0 = np.zeros((n, 64), order="F")
    z0[:, :3] = V
    mg.precompute(A)
    conv, z, rh = mg.solve(RHS, z0, None, smg.SolveOpts(tol=5e-7, max_iter=40))
    assert conv and (np.diff(rh) < 0).all()
    assert np.linalg.norm(RHS - A @ z) < 5e-7
    Ps = [mg.matrix(l, "P_full") for l in range(1, mg.n_levels)]
    orc = oracle_mod.OracleMG(Ps)
    orc.precompute(A)
    conv2, z2, rh2 = orc.solve(RHS[:, :8], z0[:, :8], tol=1e-12, max_iter=60)      # tight reference on 8 columns
    convt, zt, rht = mg.solve(RHS, z0, None, smg.SolveOpts(tol=1e-11, max_iter=60))
    assert convt and np.linalg.norm(zt[:, :8] - z2) <= 1e-8 * np.linalg.norm(z2)
    # an 8-way column shard reproduces its columns' V-cycle iterates (columns are independent); sparse
    # kernels are bit-identical for any k, the dense coarse solve sums in a k-dependent order => rounding-level slack
    u_all = mg.vcycle(RHS, z0)
    u_blk = mg.vcycle(RHS[:, 16:24], z0[:, 16:24])
    assert abs(u_all[:, 16:24] - u_blk).max() <= 1e-12 * abs(u_blk).max()
    assert np.array_equal(mg.relax(0, RHS, z0, 2)[:, 16:24], mg.relax(0, RHS[:, 16:24], z0[:, 16:24], 2))
    assert np.array_equal(mg.A(0, z0)[:, 16:24], mg.A(0, z0[:, 16:24]))


@pytest.mark.parametrize("kind,coarse", [("mcf", "never"), ("poisson", "never"), ("mcf", "always"), ("poisson", "refactor")])
def test_value_only_reprecompute_on_device_is_bit_exact(smg, oracle_mod, kind, coarse):
    """a second smg_precompute with the same sparsity runs the Galerkin products, the SELL refresh
    and the coarse factorisation on the GPU.  Every level's matrix must equal the host path (and hence the oracle) bit for bit,
    and solves on the refreshed handle must equal solves on a freshly built one -- bit for bit when both factor the coarsest matrix the
    same way (dense inverse: 'never', Schur complement: 'always'); under the default policy ('refactor') the refreshed handle has moved to the
    Schur complement while a fresh one starts on the dense inverse: same cycles, solutions equal to rounding."""
    p = subdiv_problem(kind=kind, k=2, n_sub=2)
    bits = coarse != "refactor"

    def same(r1, r2):
        if bits: return np.array_equal(r1[2], r2[2]) and np.array_equal(r1[1], r2[1])
        return len(r1[2]) == len(r2[2]) and np.allclose(r1[2][:-2], r2[2][:-2], rtol=1e-6, atol=0) and np.linalg.norm(r1[1] - r2[1]) <= 1e-9 * np.linalg.norm(r2[1])
    A1 = p["A"]
    rng = np.random.default_rng(42)
    D = sp.diags(1.0 + 0.01 * rng.uniform(size=A1.shape[0]))
    A2 = (D @ A1 @ D + sp.diags(rng.uniform(0, 0.5, A1.shape[0]) * A1.diagonal())).tocsr()   # same pattern, new values, SPD,
    A2.sort_indices()                               # and NOT bit-symmetric: the sweep must read columns (A^T)
    assert abs(A2 - A2.T).max() > 0
    assert np.array_equal(A2.indices, A1.indices)
    mg = smg.Hierarchy.from_prolongs(p["Ps"])
    mg.set_coarse_schur(coarse, 1)
    mg.precompute(A1, p["known"])                    # full (host + device) path
    mg.precompute(A2, p["known"])                    # value-only path on the device
    fresh = smg.Hierarchy.from_prolongs(p["Ps"])
    fresh.set_coarse_schur(coarse, 1)
    fresh.precompute(A2, p["known"])
    assert mg.coarse_solver()["kind"] == ("dense_inverse" if coarse == "never" else "schur_complement")
    assert fresh.coarse_solver()["kind"] == ("schur_complement" if coarse == "always" else "dense_inverse")
    orc = oracle_mod.OracleMG(p["Ps"])
    orc.precompute(A2, p["known"])
    for l in range(mg.n_levels):
        a, b = mg.matrix(l, "A"), fresh.matrix(l, "A")
        assert np.array_equal(a.indices, b.indices) and np.array_equal(a.data, b.data), "level %d differs" % l
        Ao = orc.level_A(l).tocsr()
        Ao.sort_indices()
        assert np.array_equal(a.data, Ao.data)
        assert np.array_equal(mg.Adiag(l), fresh.Adiag(l))
    o = smg.SolveOpts(tol=1e-9, max_iter=40)
    r1 = mg.solve(p["RHS"], p["z0"], p["known_val"], o)
    r2 = fresh.solve(p["RHS"], p["z0"], p["known_val"], o)
    assert same(r1, r2) and (np.diff(r1[2]) < 0).all()
    # and a third matrix on the same handle, back to back
    A3 = (A1 + 0.25 * sp.diags(A1.diagonal())).tocsr()
    A3.sort_indices()
    mg.precompute(A3, p["known"])
    fresh.precompute(A3, p["known"])
    r1 = mg.solve(p["RHS"], p["z0"], p["known_val"], o)
    r2 = fresh.solve(p["RHS"], p["z0"], p["known_val"], o)
    assert r1[0] and (same(r1, r2) if coarse != "refactor" else np.array_equal(r1[1], r2[1]))   # ('refactor': both handles have been refreshed by now)
    # a different pattern falls back to the full path
    pm = subdiv_problem(kind="mcf", k=2, n_sub=2)
    mg.precompute(pm["A"], None)
    assert mg.solve(pm["RHS"], pm["z0"], None, o)[0]


def _decimated_bunny_poisson(smg, k):
    """bunny.obj Poisson with the boundary loop pinned on the library's own decimated hierarchy (Galerkin levels, long restriction rows), k columns"""
    from oracle import mesh_np as M
    V, F = M.read_smgm("bunny.smgm")
    V = M.normalize_unit_area(V, F)
    mg = smg.mg_precompute(V, F, 0.25, 500, 1)
    b = M.boundary_loop(F)
    n = V.shape[0]
    rng = np.random.default_rng(0)
    B = np.repeat((M.massmatrix(V, F, "voronoi") @ np.ones(n))[:, None], k, axis=1) * rng.uniform(0.5, 1.5, (1, k))
    B[b, :] = 0.0
    mg.precompute((-M.cotmatrix(V, F)).tocsr(), b)
    return dict(RHS=np.asfortranarray(B), z0=np.asfortranarray(rng.uniform(-1, 1, (n, k))), known=b, known_val=np.zeros((len(b), k))), mg


@pytest.mark.parametrize("kind,k,tol", [("mcf", 3, 1e-10), ("poisson", 1, 1e-10), ("mcf", 16, 5e-7), ("mcf", 7, 5e-7), ("mcf", 13, 5e-7), ("mcf", 64, 5e-7),
                                        ("decimated", 2, 5e-7)])
def test_mixed_precision_reaches_fp64_accuracy(smg, oracle_mod, kind, k, tol):
    """BASELINE config 5 (fp32 vs fp64): fp32 V-cycle inside an fp64 outer loop.  r_his is measured in fp64, so the same
    tolerance is reached; the solution agrees with the all-fp64 run (and the oracle) at solver precision."""
    if kind == "decimated":
        p, mg = _decimated_bunny_poisson(smg, k)
    else:
        p, mg, orc = build(smg, oracle_mod, kind=kind, k=k, n_sub=2)
    c64, z64, r64 = mg.solve(p["RHS"], p["z0"], p["known_val"], smg.SolveOpts(tol=tol, max_iter=40))
    cmx, zmx, rmx = mg.solve(p["RHS"], p["z0"], p["known_val"], smg.SolveOpts(tol=tol, max_iter=40, precision="mixed"))
    assert c64 and cmx and rmx[-1] < tol
    assert abs(rmx[0] - r64[0]) <= 1e-14 * r64[0]             # same fp64 residual of the initial guess (the squares are summed in another order)
    assert abs(len(rmx) - len(r64)) <= 2 and (np.diff(rmx) < 0).all()
    assert np.linalg.norm(zmx - z64) <= (1e-8 if tol <= 1e-9 else 1e-4) * np.linalg.norm(z64)
    if p["known"] is not None:
        assert np.array_equal(zmx[p["known"]], p["known_val"])
    # the first cycle's contraction is the fp64 one to fp32 rounding
    assert abs(rmx[1] / rmx[0] - r64[1] / r64[0]) < 1e-4
    # mixed and fp64 solves can alternate on one handle; results are reproducible
    again = mg.solve(p["RHS"], p["z0"], p["known_val"], smg.SolveOpts(tol=tol, max_iter=40, precision="mixed"))
    assert np.array_equal(again[1], zmx) and np.array_equal(again[2], rmx)
    back = mg.solve(p["RHS"], p["z0"], p["known_val"], smg.SolveOpts(tol=tol, max_iter=40))
    assert np.array_equal(back[1], z64)


def test_speculative_split_phase_is_bit_identical(smg, oracle_mod):
    """The latency-hiding multi-GPU loop (V-cycle enqueued before the reduced residual is known, iterate restored when
    the loop had ended) must return exactly what the plain loop returns -- including the iteration that breaks."""
    import torch
    from surface_multigrid_code_amd.dist import GpuEngine, sharded_solve, sharded_solve_overlapped
    p, mg, orc = build(smg, oracle_mod, kind="mcf", k=2, n_sub=2)
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(st):
        mg.set_stream(st.cuda_stream)
        rhs = torch.from_numpy(np.ascontiguousarray(p["RHS"].T)).to(dev)
        z0 = torch.from_numpy(np.ascontiguousarray(p["z0"].T)).to(dev)
        for tol, max_iter in ((1e-9, 30), (1e-30, 5), (1e30, 5)):
            opts = smg.SolveOpts(tol=tol, max_iter=max_iter)
            a = sharded_solve(GpuEngine(mg, rhs, z0, None, opts), max_iter, lambda t: None, check_every=2)
            za = a[1].cpu().numpy().copy()
            b = sharded_solve_overlapped(GpuEngine(mg, rhs, z0, None, opts), max_iter, lambda t: None, check_every=2)
            zb = b[1].cpu().numpy()
            assert a[0] == b[0] and np.array_equal(a[2], b[2]) and np.array_equal(za, zb), (tol, max_iter)
        torch.cuda.synchronize()
    mg.set_stream(None)


def test_loop_forms_alternating_on_one_handle_replay_what_eager_launches_give(smg, oracle_mod):
    """Every loop form and several option sets in sequence on ONE handle and one user stream -- what makes the graph cache re-capture, keep
    and drop -- against the same calls with eager launches on a second, fresh handle: every z, r_his and converged bit for bit."""
    import torch
    from surface_multigrid_code_amd.dist import GpuEngine, sharded_solve, sharded_solve_overlapped
    p = subdiv_problem(kind="poisson", k=3, n_sub=2)
    dev = torch.device("cuda", 0)

    def sequence(use_graph):
        mg = smg.Hierarchy.from_prolongs(p["Ps"])
        mg.precompute(p["A"], p["known"])
        st = torch.cuda.Stream(device=dev)
        out, engines = [], []      # (the engines stay alive: each owns the reduction buffer its split-phase graphs were captured with)

        def opts(**kw):
            return smg.SolveOpts(tol=1e-9, max_iter=30, use_graph=use_graph, **kw)

        def host(fn, k, o):
            conv, z, rh = fn(p["RHS"][:, :k], p["z0"][:, :k], p["known_val"][:, :k], o)
            out.append((conv, z.copy(), rh.copy()))

        def split(loop):
            to = lambda a: torch.from_numpy(np.ascontiguousarray(a[:, :1].T)).to(dev)
            eng = GpuEngine(mg, to(p["RHS"]), to(p["z0"]), to(p["known_val"]), opts())
            engines.append(eng)
            conv, z, rh = loop(eng, 30, lambda t: None, check_every=2)
            out.append((conv, z.cpu().numpy().T.copy(), rh.copy()))

        with torch.cuda.stream(st):
            mg.set_stream(st.cuda_stream)
            host(mg.solve, 1, opts())
            host(mg.solve_pcg, 1, opts())
            host(mg.solve, 1, opts())
            split(sharded_solve)
            split(sharded_solve)                         # another reduction buffer
            split(sharded_solve_overlapped)
            host(mg.solve, 3, opts())                    # a key change
            host(mg.solve, 3, opts(precision="mixed"))
            host(mg.solve, 3, opts(pre=1))               # no head fusion for Gauss-Seidel
            host(mg.solve_pcg, 1, opts())
            torch.cuda.synchronize()
        assert engines[0].sumsq.data_ptr() != engines[1].sumsq.data_ptr()
        mg.set_stream(None)
        return out

    replayed, eager = sequence(1), sequence(0)
    assert len(replayed) == len(eager) == 10
    for i, (a, b) in enumerate(zip(replayed, eager)):
        assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]), "step %d differs between graph replay and eager launches" % i
    assert all(len(r[2]) > 2 for r in replayed)      # (every call iterated: tol 1e-9 from a random start)


# ----------------------------------------------------------------------------------------------- SELL panel layouts
@pytest.mark.parametrize("kind,k", [("mcf", 1), ("poisson", 3), ("mcf", 8)])
def test_compact_and_fixed_pitch_panels_give_the_same_bits(smg, oracle_mod, kind, k, monkeypatch):
    """Mesh operators are stored with a fixed panel pitch (panel address from the slice number alone, first columns requested
    ahead of the slice table); matrices with a few very wide slices fall back to compact panels addressed through slice_off.
    SMG_SELL_STRIDE=0 forces the fallback: kernels, cycles and solves must not change by a bit."""
    p = subdiv_problem(kind=kind, k=k, n_sub=2)
    out = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("SMG_SELL_STRIDE", mode)
        mg = smg.Hierarchy.from_prolongs(p["Ps"])
        mg.precompute(p["A"], p["known"])
        res = []
        for lv in range(mg.n_levels - 1):
            n = mg.rows(lv)
            r2 = np.random.default_rng(200 + lv)
            B, u = r2.uniform(-1, 1, (n, k)), r2.uniform(-1, 1, (n, k))
            res += [mg.A(lv, u), mg.relax(lv, B, u, 2), mg.vcycle(B, u, lv=lv)]
            if lv + 1 < mg.n_levels:
                res += [mg.restrict(lv, B), mg.prolong(lv, r2.uniform(-1, 1, (mg.rows(lv + 1), k)))]
        conv, z, rh = mg.solve(p["RHS"], p["z0"], p["known_val"], smg.SolveOpts(tol=1e-11, max_iter=30))
        assert conv
        out[mode] = res + [z, rh]
    for a, b in zip(out["1"], out["0"]):
        assert np.array_equal(a, b)


# ----------------------------------------------------------------------------------------------- tiny and ragged systems
@pytest.mark.parametrize("n,levels,k,known", [(3, 2, 1, None), (10, 2, 1, None), (63, 2, 1, None), (64, 2, 2, None), (65, 2, 1, None),
                                              (129, 2, 3, None), (37, 3, 5, None), (50, 2, 2, [0, 7, 49]), (30, 2, 1, "all but 3")])
def test_tiny_and_ragged_systems(smg, oracle_mod, n, levels, k, known):
    """Systems smaller than one slice, sizes around the 64-row slice boundary, a 19-row coarsest level, and constraint sets that
    leave three unknowns: same answers as the reference algorithm (iteration counts within 2: multi-colour vs lexicographic)."""
    Ps, m = [], n
    for _ in range(levels - 1):
        Ps.append(_path_interp(m)); m = (m + 1) // 2
    A = _path_matrix(n)
    if known == "all but 3":
        known = np.setdiff1d(np.arange(n), [3, 4, 20])
    kn = None if known is None else np.asarray(known, np.int32)
    rng = np.random.default_rng(1)
    mg = smg.Hierarchy.from_prolongs(Ps); mg.precompute(A, kn)
    o = oracle_mod.OracleMG(Ps); o.precompute(A, kn)
    rhs, z0 = rng.uniform(-1, 1, (n, k)), rng.uniform(-1, 1, (n, k))
    kv = rng.uniform(-1, 1, (len(kn), k)) if kn is not None else None
    a = mg.solve(rhs, z0, kv, smg.SolveOpts(tol=1e-10, max_iter=60))
    b = o.solve(rhs, z0, kv, tol=1e-10, max_iter=60)
    assert a[0] and b[0] and abs(len(a[2]) - len(b[2])) <= 2
    assert np.linalg.norm(a[1] - b[1]) <= 1e-8 * max(np.linalg.norm(b[1]), 1e-300)
    if kn is not None:
        assert np.array_equal(a[1][kn], kv)


# ----------------------------------------------------------------------------------------------- random non-mesh systems
@pytest.mark.parametrize("seed,n,levels,k,hub", [(1, 200, 2, 1, False), (2, 777, 3, 2, False), (3, 1500, 3, 1, True), (4, 4000, 4, 3, True),
                                                (5, 65, 2, 9, False), (6, 2600, 3, 1, False)])
def test_random_non_mesh_systems_match_the_oracle(smg, oracle_mod, seed, n, levels, k, hub):
    """Nothing in the library may depend on the operators coming from a triangle mesh: irregular random graphs (many colours,
    hub rows => very wide SELL slices => compact panels), random prolongations.  Kernels stay bit-exact against the oracle on the
    level matrices in the device numbering; solves agree with the reference algorithm."""
    rng = np.random.default_rng(seed)
    A, Ps = _random_spd_hierarchy(rng, n, levels, hub)
    mg = smg.Hierarchy.from_prolongs(Ps); mg.precompute(A)
    o = oracle_mod.OracleMG(Ps); o.precompute(A)
    for lv in range(mg.n_levels - 1):
        m = mg.rows(lv)
        cp = mg.colors(lv)
        Ai = mg.matrix(lv, "A", internal=True)
        # a valid colouring: no entry inside a diagonal colour block except the diagonal
        for c in range(len(cp) - 1):
            blk = sp.csr_matrix(Ai[cp[c]:cp[c + 1], cp[c]:cp[c + 1]]); blk.setdiag(0); blk.eliminate_zeros()
            assert blk.nnz == 0
        x = rng.uniform(-1, 1, (m, k)); b = rng.uniform(-1, 1, (m, k))
        perm = mg.perm(lv)
        oi = oracle_on_device_numbering(oracle_mod, mg, lv)
        assert np.array_equal(mg.A(lv, x)[perm], oi.A(0, x[perm]))
        assert gs_bit_exact(oracle_mod, mg, lv, b, x, 2)
        permc = mg.perm(lv + 1)
        assert np.array_equal(mg.restrict(lv, x)[permc], oi.restrict(0, x[perm]))
        xc = rng.uniform(-1, 1, (mg.rows(lv + 1), k))
        assert np.array_equal(mg.prolong(lv, xc)[perm], oi.prolong(0, xc[permc]))
    rhs, z0 = rng.uniform(-1, 1, (n, k)), rng.uniform(-1, 1, (n, k))
    a = mg.solve(rhs, z0, None, smg.SolveOpts(tol=1e-10, max_iter=200))
    bb = o.solve(rhs, z0, tol=1e-10, max_iter=200)
    assert a[0] and bb[0]
    assert np.linalg.norm(a[1] - bb[1]) <= 1e-7 * np.linalg.norm(bb[1])
    assert abs(len(a[2]) - len(bb[2])) <= max(3, len(bb[2]) // 4)


def test_unsorted_duplicate_input_and_explicit_zeros(smg, oracle_mod):
    """Eigen's setFromTriplets semantics at the boundary: the caller's CSR rows may be unsorted and hold duplicate (row, col)
    pairs (summed), prolongation rows may carry explicit zeros (the [1, 0, 0] rows of get_prolong.cpp:48-54); k = 100 columns
    go through one wide launch of 64, one of 32 and a narrow remainder."""
    p = subdiv_problem(kind="mcf", k=1, n_sub=2)
    A = sp.csr_matrix(p["A"])
    n = A.shape[0]
    rng = np.random.default_rng(11)
    # split every entry into two halves and shuffle each row
    ptr, col, val = [0], [], []
    for i in range(n):
        c = A.indices[A.indptr[i]:A.indptr[i + 1]]; v = A.data[A.indptr[i]:A.indptr[i + 1]]
        cc = np.concatenate([c, c]); vv = np.concatenate([0.25 * v, 0.75 * v])
        o = rng.permutation(len(cc))
        col.append(cc[o]); val.append(vv[o]); ptr.append(ptr[-1] + len(cc))
    ptr, col, val = np.asarray(ptr, np.int32), np.concatenate(col).astype(np.int32), np.concatenate(val)
    # explicit zeros in P: add a zero entry to every row of every P
    Ps = []
    for P in p["Ps"]:
        P = sp.csr_matrix(P)
        extra = sp.csr_matrix((np.zeros(P.shape[0]), (np.arange(P.shape[0]), rng.integers(0, P.shape[1], P.shape[0]))), shape=P.shape)
        Q = sp.csr_matrix(P + extra)       # scipy drops nothing here: the zeros land on new positions or on existing ones
        Ps.append(Q)
    mg = smg.Hierarchy.from_prolongs(Ps)
    rc = mg.L.smg_precompute(mg.h, n, ptr.ctypes.data_as(mg.L.smg_precompute.argtypes[2]), col.ctypes.data_as(mg.L.smg_precompute.argtypes[3]),
                             val.ctypes.data_as(mg.L.smg_precompute.argtypes[4]), None, 0)
    assert rc == 0
    # 0.25 v + 0.75 v is not bit-exactly v: compare with the oracle fed the same summed matrix
    Asum = sp.csr_matrix((val, col, ptr), shape=(n, n)); Asum.sum_duplicates(); Asum.sort_indices()
    o = oracle_mod.OracleMG(Ps); o.precompute(Asum)
    k = 100
    rhs, z0 = rng.uniform(-1, 1, (n, k)), rng.uniform(-1, 1, (n, k))
    a = mg.solve(rhs, z0, None, smg.SolveOpts(tol=1e-9, max_iter=40))
    b = o.solve(rhs, z0, tol=1e-9, max_iter=40)
    assert a[0] and b[0] and abs(len(a[2]) - len(b[2])) <= 2
    assert np.linalg.norm(a[1] - b[1]) <= 1e-7 * np.linalg.norm(b[1])
    x = rng.uniform(-1, 1, (n, 3))
    assert np.allclose(mg.A(0, x), Asum @ x, rtol=0, atol=1e-13 * abs(Asum).sum(axis=1).max())


def test_block_hierarchy_solves_a_3dof_system(smg, oracle_mod):
    """mg_precompute_block (P (x) I_3, DOF = 3 vertex + d; 06_example_balloon_sim's hierarchy): a vector-valued SPD system with
    coupling between the three components of a vertex, solved on the GPU and by the reference algorithm on the same hierarchy."""
    from oracle import mesh_np as M
    V, F = M.read_smgm("ogre_sim.smgm")
    V = M.normalize_unit_area(V, F)
    n = V.shape[0]
    mg = smg.mg_precompute_block(V, F, 0.25, 100, 1)
    Ps = [mg.matrix(l, "P_full") for l in range(1, mg.n_levels)]
    assert Ps[0].shape[0] == 3 * n
    S = (M.massmatrix(V, F, "barycentric") - 0.01 * M.cotmatrix(V, F)).tocsr()
    rng = np.random.default_rng(5)
    B3 = rng.uniform(-1, 1, (3, 3)); C3 = B3 @ B3.T + 3.0 * np.eye(3)            # SPD 3 x 3 coupling
    A = sp.kron(S, sp.csr_matrix(C3), format="csr")                              # DOF index 3 v + d
    A.sort_indices()
    rhs, z0 = rng.uniform(-1, 1, (3 * n, 2)), np.zeros((3 * n, 2))
    mg.precompute(A)
    o = oracle_mod.OracleMG(Ps); o.precompute(A)
    a = mg.solve(rhs, z0, None, smg.SolveOpts(tol=1e-10, max_iter=60))
    b = o.solve(rhs, z0, tol=1e-10, max_iter=60)
    assert a[0] and b[0] and abs(len(a[2]) - len(b[2])) <= 2
    assert np.linalg.norm(a[1] - b[1]) <= 1e-8 * np.linalg.norm(b[1])
    assert np.linalg.norm(rhs - A @ a[1]) < 1.5e-10


def test_relax_bit_exact_at_the_ends_of_the_one_launch_range(smg, oracle_mod):
    """relax() as one launch (overlapped tiling, csrc/smg_tiled.hpp) now also serves levels of 512 - 2 047 rows and, with parts of up to 512 rows, levels
    of 65 537 - 122 880 rows (tools/size_sweep.py: a 768-row level 37.5 -> 18.1 us per visit, a 69 120-row level 45.8 -> 33.9): Gauss-Seidel stays the
    oracle's lexicographic sweep on the level's numbering, bit for bit, on a 768-row and a 69 120-row level, one and three columns, 1 - 3 sweeps."""
    mesh = smg.mesh
    for (nu, nv), levels in (((16, 12), (0, 2)), ((36, 30), (0,))):
        V, F = mesh.torus(nu, nv)
        mg, Vf, Ff = smg.mg_precompute_subdiv(V, F, 3, n_extra_levels=0)
        Vf = mesh.normalize_unit_area(Vf, Ff)
        A = (mesh.massmatrix(Vf, Ff, "barycentric") - 0.01 * mesh.cotmatrix(Vf, Ff)).tocsr()
        A.sort_indices()
        mg.precompute(A)
        rng = np.random.default_rng(11)
        for lv in levels:
            n = mg.rows(lv)
            assert n in (12288, 768, 69120)
            for k in (1, 3):
                b, x = rng.uniform(-1, 1, (n, k)), rng.uniform(-1, 1, (n, k))
                for iters in (1, 2, 3):
                    assert gs_bit_exact(oracle_mod, mg, lv, b, x, iters), "relax(%d) not bit-exact on the %d-row level, %d columns" % (iters, n, k)
        # ... and a solve on the hierarchy agrees with the oracle's
        rhs = np.asfortranarray((mesh.massmatrix(Vf, Ff, "barycentric") @ rng.uniform(-1, 1, A.shape[0]))[:, None])
        z0 = np.zeros_like(rhs)
        a = mg.solve(rhs, z0, None, smg.SolveOpts(tol=1e-10, max_iter=40))
        o = oracle_mod.OracleMG([mg.matrix(l, "P_full") for l in range(1, mg.n_levels)])
        o.precompute(A)
        bref = o.solve(rhs, z0, tol=1e-10, max_iter=40)
        assert a[0] and bref[0] and abs(len(a[2]) - len(bref[2])) <= 2
        assert np.linalg.norm(a[1] - bref[1]) <= 1e-8 * np.linalg.norm(bref[1])


# ----------------------------------------------------------------------------------------------- launch shortcuts
_SHORTCUT_CHILD = r"""
import hashlib, os, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import numpy as np
import surface_multigrid_code_amd as smg
from problems import subdiv_problem
for kind, k in (("mcf", 1), ("mcf", 3), ("poisson", 2), ("poisson", 5), ("mcf", 7), ("poisson", 13)):     # the tiles take columns in groups of up to 3: 1, 3, 2, 3 + 2; 5, 7, 13: padded solves
    p = subdiv_problem(kind=kind, k=k, n_sub=3)
    mg = smg.Hierarchy.from_prolongs(p["Ps"])
    mg.precompute(p["A"], p["known"])
    rng = np.random.default_rng(3)
    n = mg.rows(0)
    B, u = rng.uniform(-1, 1, (n, k)), rng.uniform(-1, 1, (n, k))
    v = mg.vcycle(B, u)
    conv, z, rh = mg.solve(p["RHS"], p["z0"], p["known_val"], smg.SolveOpts(tol=1e-9, max_iter=30))
    print(kind, k, mg.n_levels, hashlib.sha256(np.ascontiguousarray(v).tobytes()).hexdigest(),
          hashlib.sha256(np.ascontiguousarray(z).tobytes()).hexdigest(), len(rh),
          "first_colour_rows=" + ",".join(str(mg.first_colour_rows(l)) for l in range(1, mg.n_levels - 1)))
"""


def test_launch_shortcuts_do_not_change_a_bit(smg):
    """The launch-count / latency shortcuts of the cycle -- the restriction launch producing the first colour of the coarse level's
    first sweep (SMG_FUSE_FIRST), small colour sweeps confined to one XCD (SMG_ONE_XCD_MAX), the whole panel pitch requested
    ahead on tiny launches (SMG_PITCH_SPEC_MAX), relax() of the latency-bound levels as ONE launch by overlapped tiling (SMG_TILED,
    csrc/smg_tiled.hpp: levels 1 and 2 of this hierarchy), four outer iterations in one graph (SMG_GRAPH_ITERS), the solve's internal blocks padded to
    kernel-friendly column counts (SMG_PAD_COLS: 5 -> 8, 7 -> 8, 13 -> 16 columns) -- are re-orderings of WHERE and WHEN the same arithmetic runs: a full-depth
    V-cycle and a solve on a 4-level hierarchy give identical bits with all of them off.  (The knobs are read once per process,
    hence the two child processes.)"""
    import subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    outs = []
    for off in (False, True):
        env = dict(os.environ)
        env["SMG_DEVICE_FILL_MIN"] = "1000"     # the panels of every big enough A filled on the device from the caller's arrays + the permutation ...
        if off:
            env.update(SMG_FUSE_FIRST="0", SMG_ONE_XCD_MAX="0", SMG_PITCH_SPEC_MAX="0", SMG_TILED="0", SMG_DEVICE_FILL="0", SMG_GRAPH_ITERS="1", SMG_PAD_COLS="0")   # ... or built on the host; one outer iteration per graph instead of four; no column padding
        r = subprocess.run([sys.executable, "-c", _SHORTCUT_CHILD, root], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith(("mcf", "poisson"))]
        assert len(lines) == 6, r.stdout
        outs.append(lines)
    assert all(int(ln.split()[2]) >= 4 for ln in outs[0])   # deep enough for the fused restriction to be in play
    # ... and it IS in play on every coarse smoothed level, whether the host or the device filled its image (the device works the diagonal
    # slots out itself, k_sell_diag_slots): same numbers of first-colour rows both ways, none of them zero
    assert all(all(int(x) > 0 for x in ln.split("first_colour_rows=")[1].split(",")) for ln in outs[0])
    assert outs[0] == outs[1]


_RCCL_CHILD = r"""
import os, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
os.environ.setdefault("MASTER_ADDR", "127.0.0.1"); os.environ.setdefault("MASTER_PORT", "29533")
import numpy as np, torch, torch.distributed as dist
import surface_multigrid_code_amd as smg
from surface_multigrid_code_amd.dist import StreamAllReduce
from problems import subdiv_problem
dist.init_process_group("nccl", rank=0, world_size=1)
torch.cuda.set_device(0)
dev = torch.device("cuda", 0)
stream = torch.cuda.Stream()
t = torch.tensor([1.5, -2.0, 4.25], dtype=torch.float64, device=dev)
with torch.cuda.stream(stream):
    sar = StreamAllReduce(0, 1, stream.cuda_stream, device=dev)
    assert sar.ready and sar.connect(), sar.err
    sar(t.data_ptr(), 3)
    stream.synchronize()
    assert t.tolist() == [1.5, -2.0, 4.25]
    # the split-phase loop with the reduction on the solve stream == the fused solve, bit for bit
    p = subdiv_problem(kind="mcf", k=1, n_sub=2)
    mg = smg.Hierarchy.from_prolongs(p["Ps"]); mg.precompute(p["A"], p["known"])
    mg.set_stream(stream.cuda_stream)
    n = mg.rows(0)
    conv, z_ref, rh_ref = mg.solve(p["RHS"], p["z0"], None, smg.SolveOpts(tol=1e-9, max_iter=30))
    rhs = torch.from_numpy(np.ascontiguousarray(p["RHS"][:, 0])).to(dev); z0 = torch.from_numpy(np.ascontiguousarray(p["z0"][:, 0])).to(dev)
    z = torch.empty(n, dtype=torch.float64, device=dev); ss = torch.zeros(1, dtype=torch.float64, device=dev)
    mg.solve_begin(rhs.data_ptr(), n, z0.data_ptr(), n, 1, opts=smg.SolveOpts(tol=1e-9, max_iter=30))
    for _ in range(30):
        mg.iter_residual(ss.data_ptr()); sar(ss.data_ptr()); mg.iter_cycle(ss.data_ptr())
    conv2, rh = mg.solve_end(z.data_ptr(), n, max_iter=30)
    assert conv2 and len(rh) == len(rh_ref) and np.array_equal(np.asarray(rh), np.asarray(rh_ref))
    assert np.array_equal(z.cpu().numpy(), z_ref[:, 0])
    sar.close()
dist.destroy_process_group()
print("RCCL_STREAM_OK")
"""


def test_allreduce_on_the_solve_stream(smg):
    """dist.StreamAllReduce (ncclAllReduce through ctypes on the solve's own stream, world size 1 here): values pass through
    unchanged, and the split-phase loop driven with it reproduces the fused solve bit for bit."""
    import subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", _RCCL_CHILD, root], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "RCCL_STREAM_OK" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])


_NONSYM_CHILD = r"""
import os, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import numpy as np, scipy.sparse as sp
import surface_multigrid_code_amd as smg
from problems import subdiv_problem
from oracle import oracle as oracle_mod
oracle_mod.build()
p = subdiv_problem(kind="mcf", k=1, n_sub=2)
A = p["A"].tocsr().copy(); A.sort_indices()
n = A.shape[0]
# (1) values that differ from their mirror images in the last bits, pattern symmetric: the sweep must stream A^T (reference relax() walks
#     COLUMN i, src/mg_VCycle.cpp:149-155), on level 0 too -- whose A^T image the device now fills itself
rng = np.random.default_rng(5)
A1 = A.copy(); A1.data = A1.data * (1.0 + 1e-13 * rng.integers(-3, 4, A1.nnz))
mg = smg.Hierarchy.from_prolongs(p["Ps"]); mg.precompute(A1)
for lv in range(mg.n_levels - 1):
    Ai = mg.matrix(lv, "A", internal=True); Pi = mg.matrix(lv + 1, "P", internal=True)
    oi = oracle_mod.OracleMG([Pi]); oi.precompute(Ai)
    perm = mg.perm(lv)
    x = rng.uniform(-1, 1, (mg.rows(lv), 2)); b = rng.uniform(-1, 1, (mg.rows(lv), 2))
    assert np.array_equal(mg.A(lv, x)[perm], oi.A(0, x[perm])), lv
    assert np.array_equal(mg.relax(lv, b, x, 2)[perm], oi.relax(0, b[perm], x[perm], 2)), lv
o = oracle_mod.OracleMG(p["Ps"]); o.precompute(A1)
a = mg.solve(p["RHS"], p["z0"], None, smg.SolveOpts(tol=1e-9, max_iter=40)); r = o.solve(p["RHS"], p["z0"], None, tol=1e-9, max_iter=40)
assert a[0] and r[0] and abs(len(a[2]) - len(r[2])) <= 2 and np.linalg.norm(a[1] - r[1]) <= 1e-7 * np.linalg.norm(r[1])
print("VALUES_OK")
# (2) an entry without a mirror image: refused, with the level named
A2 = A.tolil(); i = 10; j = [c for c in A.indices[A.indptr[i]:A.indptr[i + 1]] if c != i][0]; A2[j, i] = 0.0
A2 = A2.tocsr(); A2.eliminate_zeros(); A2.sort_indices()
assert A2.nnz == A.nnz - 1
try:
    smg.Hierarchy.from_prolongs(p["Ps"]).precompute(A2)
    print("ACCEPTED")
except smg.SmgError as e:
    print("REFUSED", e.code, str(e))
"""


def test_a_level_0_matrix_that_is_not_bit_symmetric_on_the_device_fill_path(smg):
    """Level 0 filled on the device (SMG_DEVICE_FILL_MIN lowered to reach it on a test-sized mesh; the default path with the host-built
    images as the control): a matrix whose values differ from their mirror images in the last bits gets its A^T image (k_sell_fill,
    transposed) and the sweeps are the oracle's bit for bit; one whose pattern is not symmetric is refused."""
    import subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for fill_min in ("100", "100000000"):
        env = dict(os.environ, SMG_DEVICE_FILL_MIN=fill_min)
        r = subprocess.run([sys.executable, "-c", _NONSYM_CHILD, root], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
        assert "VALUES_OK" in r.stdout
        refused = [ln for ln in r.stdout.splitlines() if ln.startswith("REFUSED")]
        assert refused and "-1" in refused[0].split()[1] and "symmetric" in refused[0], r.stdout


_LONGROW_CHILD = r"""
import hashlib, os, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import numpy as np
import surface_multigrid_code_amd as smg
from surface_multigrid_code_amd import mesh
V, F = mesh.read_triangle_mesh("ogre.smgm"); V = mesh.normalize_unit_area(V, F)
mg = smg.mg_precompute(V, F, 0.25, 500, 1)
A = (mesh.massmatrix(V, F, "barycentric") - 0.01 * mesh.cotmatrix(V, F)).tocsr(); A.sort_indices()
mg.precompute(A)
rng = np.random.default_rng(3)
for k in (1, 3, 8, 64):
    for sm in ("gs", "hybrid_chebyshev"):
        B, u = rng.uniform(-1, 1, (V.shape[0], k)), rng.uniform(-1, 1, (V.shape[0], k))
        mg.set_smoother(sm)
        v = mg.vcycle(B, u)
        conv, z, rh = mg.solve(B, u, None, smg.SolveOpts(tol=1e-9, max_iter=60, smoother=sm, precision="mixed" if k == 3 else "f64"))
        print("case", k, sm, hashlib.sha256(np.ascontiguousarray(v).tobytes()).hexdigest(), hashlib.sha256(np.ascontiguousarray(z).tobytes()).hexdigest(), len(rh))
"""


def test_long_rows_of_decimated_restrictions_are_bit_exact(smg, oracle_mod):
    """A coarse vertex of the reference's decimation may gather from > 100 fine ones (ogre.obj: a row of PT with 177 entries).  Such rows
    leave the SELL panels and are served by k_long_ax (one wave per row and column: products in parallel, additions in the panel
    kernel's order): restriction bit-exact against the oracle in the device numbering for k = 1..64, and whole cycles / solves
    bit-identical to the build that keeps them in the panels (SMG_LONG_ROW_MIN=0)."""
    import subprocess, sys
    mesh = smg.mesh
    V, F = mesh.read_triangle_mesh("ogre.smgm")
    V = mesh.normalize_unit_area(V, F)
    mg = smg.mg_precompute(V, F, 0.25, 500, 1)
    A = (mesh.massmatrix(V, F, "barycentric") - 0.01 * mesh.cotmatrix(V, F)).tocsr()
    A.sort_indices()
    mg.precompute(A)
    PT = mg.matrix(1, "PT", internal=True).tocsr()
    assert np.diff(PT.indptr).max() >= 100                       # the situation this is about
    rng = np.random.default_rng(4)
    for lv in range(mg.n_levels - 1):
        oi = oracle_on_device_numbering(oracle_mod, mg, lv)
        perm, permc = mg.perm(lv), mg.perm(lv + 1)
        for k in (1, 2, 3, 5, 8, 27, 64):
            x = rng.uniform(-1, 1, (mg.rows(lv), k))
            assert np.array_equal(mg.restrict(lv, x)[permc], oi.restrict(0, x[perm])), "restriction with long rows not bit-exact: level %d, k %d" % (lv, k)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    outs = []
    for off in (False, True):
        env = dict(os.environ)
        if off:
            env.update(SMG_LONG_ROW_MIN="0")
        r = subprocess.run([sys.executable, "-c", _LONGROW_CHILD, root], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("case")]
        assert len(lines) == 8, r.stdout
        outs.append(lines)
    assert outs[0] == outs[1]


def test_wide_kernel_with_the_whole_row_in_flight_is_bit_exact_on_decimated_levels(smg, oracle_mod):
    """k_sell_wide<..., R = 1, U = 8 / 16 / 32> (8 <= k < 64 on launches of few waves): the Galerkin levels of a decimated hierarchy have
    15 - 30 entries per row, so these are the launches that take the 16- and 32-column batches.  Every kernel of the cycle, bit for bit
    against the oracle on the level's matrix in the device numbering: SpMV, Gauss-Seidel, damped Jacobi, Chebyshev, restriction,
    prolongation; k = 8 (one group of 8), 20 (16 + 4 narrow), 40 (32 + 8)."""
    mesh = smg.mesh
    V, F = mesh.read_triangle_mesh("bunny.smgm")
    V = mesh.normalize_unit_area(V, F)
    mg = smg.mg_precompute(V, F, 0.25, 500, 1)
    A = (mesh.massmatrix(V, F, "barycentric") - 0.01 * mesh.cotmatrix(V, F)).tocsr()
    A.sort_indices()
    mg.precompute(A)
    assert mg.n_levels >= 3
    widths = [int(np.diff(mg.matrix(lv, "A", internal=True).tocsr().indptr).max()) for lv in range(mg.n_levels - 1)]
    assert max(widths) > 16                                           # a level that needs the 32-column batch
    rng = np.random.default_rng(11)
    for lv in range(mg.n_levels - 1):
        oi = oracle_on_device_numbering(oracle_mod, mg, lv)
        perm, permc = mg.perm(lv), mg.perm(lv + 1)
        for k in (8, 20, 40):
            x = rng.uniform(-1, 1, (mg.rows(lv), k)); b = rng.uniform(-1, 1, (mg.rows(lv), k))
            xc = rng.uniform(-1, 1, (mg.rows(lv + 1), k))
            tag = "level %d (widest row %d), k %d" % (lv, widths[lv], k)
            assert np.array_equal(mg.A(lv, x)[perm], oi.A(0, x[perm])), "A: " + tag
            mg.set_smoother("gs"); oi.set_smoother(0, "gs", 1.0)
            assert gs_bit_exact(oracle_mod, mg, lv, b, x, 2), "Gauss-Seidel: " + tag
            mg.set_smoother("jacobi", 0.7); oi.set_smoother(0, "jacobi", 0.7)
            assert np.array_equal(mg.relax(lv, b, x, 3)[perm], oi.relax(0, b[perm], x[perm], 3)), "Jacobi: " + tag
            mg.set_smoother("chebyshev"); oi.set_smoother(0, "chebyshev", 0.1)
            assert np.array_equal(mg.relax(lv, b, x, 2)[perm], oi.relax(0, b[perm], x[perm], 2)), "Chebyshev: " + tag
            mg.set_smoother("gs")
            assert np.array_equal(mg.restrict(lv, x)[permc], oi.restrict(0, x[perm])), "restrict: " + tag
            assert np.array_equal(mg.prolong(lv, xc)[perm], oi.prolong(0, xc[permc])), "prolong: " + tag


def test_solve_sharded_with_one_rank_is_smg_solve_and_reports_a_failing_reduction(smg, oracle_mod):
    """smg_solve_sharded at world size 1 with a reduction that does nothing is smg_solve's loop (same bits: iterate and history); a reduction
    that reports failure aborts the solve with SMG_ERR_REDUCE and leaves the handle usable; k_local = 0 alone converges on its zero residual."""
    import torch
    p, mg, orc = build(smg, oracle_mod, kind="mcf", k=3, n_sub=2)
    dev = torch.device("cuda", 0)
    n = mg.rows(0)
    rhs = torch.from_numpy(np.ascontiguousarray(p["RHS"].T)).to(dev)
    z0 = torch.from_numpy(np.ascontiguousarray(p["z0"].T)).to(dev)
    z = torch.empty_like(z0)
    o = smg.SolveOpts(tol=1e-9, max_iter=40)
    calls = []
    conv, rh = mg.solve_sharded(rhs.data_ptr(), z0.data_ptr(), z.data_ptr(), n, 3, lambda ptr, cnt, st: calls.append(cnt), opts=o)
    torch.cuda.synchronize()
    ref = mg.solve(p["RHS"], p["z0"], None, o)
    assert conv == ref[0] and np.array_equal(rh, ref[2]) and np.array_equal(z.cpu().numpy().T, ref[1])
    assert len(calls) >= len(rh) and set(calls) == {1}

    def broken(ptr, cnt, st):
        raise RuntimeError("link down")
    with pytest.raises(RuntimeError, match="link down"):
        mg.solve_sharded(rhs.data_ptr(), z0.data_ptr(), z.data_ptr(), n, 3, broken, opts=o)
    again = mg.solve(p["RHS"], p["z0"], None, o)
    assert np.array_equal(again[1], ref[1])
    conv0, rh0 = mg.solve_sharded(None, None, None, 0, 0, lambda ptr, cnt, st: None, opts=o)
    assert conv0 and len(rh0) == 1 and rh0[0] == 0.0
