"""CPU: the restatement of the union kernels and of the union loop (tests/union_reference.py) against plain references.

member_sumsq against the correctly rounded sum of squares, decide on a table of hand-written cases (union_reference.DECIDE_CASES, which the GPU
lane runs through the device as well), and UnionLoop driven by the CPU oracle on the block-diagonal system of three small members against the
stand-alone oracle solve of every member."""
import numpy as np
import pytest
import scipy.sparse as sp

import union_reference as UR
from kernel_hooks import exact_dot, gamma
from oracle import mesh_np as M
from problems import _path_interp, _path_matrix


# ---------------------------------------------------------------------------------------------------- member_sumsq
@pytest.mark.parametrize("k", [1, 3, 5])
@pytest.mark.parametrize("rows", [1, 1023, 1024, 1025, 2049])
def test_member_sumsq_is_the_sum_of_squares(rows, k):
    """Bound (derived): N = rows k products, one rounding each, and at most N - 1 additions on the way of any term to the root, against the
    correctly rounded sum (one more rounding): gamma(N + 1) relative, whatever the order."""
    rng = np.random.default_rng(rows * 8 + k)
    n = rows + 37
    r = rng.uniform(-1, 1, (n, k)) * 10.0 ** rng.integers(-3, 4, (n, 1))
    rows_i = rng.permutation(n)[:rows]
    ss = UR.member_sumsq(r, rows_i, k)
    exact = exact_dot(r[rows_i], r[rows_i])
    assert abs(ss - exact) <= gamma(rows * k + 1) * exact, (ss, exact)
    # rows outside the list do not enter
    r2 = r.copy()
    r2[np.setdiff1d(np.arange(n), rows_i)] = np.nan
    assert UR.member_sumsq(r2, rows_i, k) == ss


def test_member_sumsq_orders_its_terms_like_the_kernel():
    """A sum whose value tells the order.  2^54 has ulp 4.  Thread 0 holds positions 0 (2^54) and 1024 (1): its own sum stays 2^54.  Threads 1, 3
    and 5 hold 1 each; the tree adds red[5] to red[1] at o = 4, red[3] to red[1] at o = 2, and red[1] = 3 to red[0] at o = 1: 2^54 + 3 rounds
    to 2^54 + 4.  One by one the four ones would all be lost (2^54), and two at a time would tie to even (2^54)."""
    r = np.zeros((2048, 1))
    r[0] = 2.0 ** 27
    r[[1024, 1, 3, 5]] = 1.0
    rows_i = np.arange(2048)
    assert UR.member_sumsq(r, rows_i, 1) == 2.0 ** 54 + 4.0
    assert UR.member_sumsq(r[:, [0, 0]], rows_i, 2) == 2.0 ** 55 + 8.0               # two columns: every thread adds its row's columns first
    # overflow: a residual of 1e200 gives ss = inf, which decide() takes as a failure of that member
    r[5] = 1e200
    assert UR.member_sumsq(r, rows_i, 1) == np.inf
    st = UR.decide(UR.UnionState(1, 4), [np.inf], 1e-3)
    assert st.mdone[0] == 2 and st.done == 1 and st.sumsq == 0.0 and st.his[0, 0] == np.inf


# ---------------------------------------------------------------------------------------------------- decide
@pytest.mark.parametrize("case", UR.DECIDE_CASES, ids=[c["name"] for c in UR.DECIDE_CASES])
def test_decide_on_hand_written_cases(case):
    st = UR.decide(UR.state_of_case(case), case["ss"], case["tol"])
    e = case["expect"]
    assert list(st.mdone) == list(e["mdone"]) and list(st.nhis) == list(e["nhis"])
    assert (st.done, st.n_his) == (e["done"], e["n_his"])
    if "sumsq" in e:
        assert st.sumsq == e["sumsq"] and st.r_last == np.sqrt(e["sumsq"])
    for (i, j), v in e.get("his", {}).items():
        assert st.his[i, j] == v or (v != v and st.his[i, j] != st.his[i, j]), (i, j, st.his[i, j], v)
    # every history entry the case does not name still holds what it held
    before = UR.state_of_case(case)
    named = set(e.get("his", {}))
    for i in range(st.m):
        for j in range(st.cap):
            if (i, j) not in named:
                assert st.his[i, j] == before.his[i, j], (i, j)
    if "r_prev" in e:
        assert st.r_prev == e["r_prev"]
    # the handle's own history: the entry is written below its cap only
    j = case.get("n_his", 0)
    for q in range(st.his_cap):
        assert st.r_his[q] == (st.r_last if q == j and not case.get("done", 0) else before.r_his[q]), q


def test_restore_and_blockdiag_exact():
    rng = np.random.default_rng(4)
    n, k = 30, 3
    rows = rng.permutation(n)[:24]
    rptr = np.array([0, 5, 5, 17, 24])
    u, zs = rng.uniform(-1, 1, (n, k)), rng.uniform(-1, 1, (n, k))
    out = UR.restore(u, zs, rows, rptr, [1, 1, 0, 2], k)
    ended = np.concatenate([rows[0:5], rows[17:24]])
    assert np.array_equal(out[ended], zs[ended])
    rest = np.setdiff1d(np.arange(n), ended)
    assert np.array_equal(out[rest], u[rest])
    # the block-diagonal product: against the dense product in long double
    sizes, ldas = [3, 70], [64, 128]
    blocks = []
    for ni, lda in zip(sizes, ldas):
        B = np.zeros((lda, lda))
        S = rng.uniform(-1, 1, (ni, ni))
        B[:ni, :ni] = S + S.T
        blocks.append(B)
    mrow0 = [0, 3, 73]
    b, u = rng.uniform(-1, 1, (73, 2)), rng.uniform(-1, 1, (73, 2))
    out, mag = UR.blockdiag_exact(blocks, mrow0, b, u)
    full = sp.block_diag([blocks[0][:3, :3], blocks[1][:70, :70]]).toarray().astype(np.longdouble)
    ref = u.astype(np.longdouble) + full @ b.astype(np.longdouble)
    # the dot product rounded once (<= u mag), one addition (<= u |out|), and the long-double reference's own 71 roundings of 2^-64
    assert np.all(np.abs(out - ref) <= 2.0 ** -53 * (mag + np.abs(out)) + gamma(72) * 2.0 ** -11 * (np.abs(u) + mag))
    # the residual as a sum of two doubles against math.fsum of the exactly split products, entry by entry
    A = sp.random(40, 40, 0.2, random_state=3, format="csr") + sp.eye(40, format="csr")
    z, B = rng.uniform(-1, 1, (40, 2)) * 1e3, rng.uniform(-1, 1, (40, 2))
    hi, lo, mag, W = UR.residual_twofold(A, B, z)
    assert W == np.diff(A.indptr).max()
    for i in range(40):
        for c in range(2):
            ai = A[i].toarray().ravel()
            exact = exact_dot(np.concatenate([[1.0], -ai]), np.concatenate([[B[i, c]], z[:, c]]))
            assert hi[i, c] == exact and abs(lo[i, c]) <= 2.0 ** -53 * abs(exact), (i, c)
            assert abs(mag[i, c] - (abs(B[i, c]) + np.abs(ai) @ np.abs(z[:, c]))) <= gamma(W + 2) * mag[i, c]
    assert UR.norm_twofold(hi, 0 * lo) == np.sqrt(exact_dot(hi, hi))


# ---------------------------------------------------------------------------------------------------- UnionLoop on the CPU oracle
TOL, MAX_ITER = 1e-9, 60
# max over members and history entries of |rhi[j] - rh1[j]| / rh1[j] between the union loop's history and the stand-alone oracle's, measured here:
# 1.48e-15 (1.41e-15, 1.14e-15, 1.48e-15 for the three members: the sum of squares of up to 5 224 terms is formed in another order; the iterates
# themselves come out bit for bit, the LDL^T of the block-diagonal coarse matrix eliminating every member's block as it does alone).  The bound
# is 100 x that, rounded up to a power of ten.
HIS_MEASURED, HIS_BOUND = 1.48e-15, 1e-12


def _mesh_member(smg_mod, ratio, nvc, k, rng):
    V, F = M.read_smgm("ogre_sim.smgm")
    V = M.normalize_unit_area(V, F)
    mg = smg_mod.mg_precompute(V, F, ratio, nvc, 1)                      # the library's decimator runs on the host
    Ps = [mg.matrix(l, "P_full") for l in range(1, mg.n_levels)]
    Mb = M.massmatrix(V, F, "barycentric")
    A = (Mb - 0.01 * M.cotmatrix(V, F)).tocsr(); A.sort_indices()
    return A, Ps, np.asfortranarray(Mb @ rng.uniform(-1, 1, (V.shape[0], k)))


def _path_member(n, levels, k, rng):
    Ps, m = [], n
    for _ in range(levels - 1):
        Ps.append(_path_interp(m)); m = (m + 1) // 2
    return _path_matrix(n), Ps, np.asfortranarray(rng.uniform(-1, 1, (n, k)))


@pytest.fixture(scope="module")
def three_members(smg_mod, oracle_mod):
    """ogre_sim with coarsest levels of 176 and of 667 rows (a union's members need the same number of levels, so the second size comes from
    the decimation ratio) and a three-level path system of 257 rows; k = 2.  The stand-alone oracle solves are computed once."""
    rng = np.random.default_rng(11)
    k = 2
    mem = [_mesh_member(smg_mod, 0.25, 100, k, rng), _mesh_member(smg_mod, 0.5, 400, k, rng), _path_member(257, 3, k, rng)]
    assert {len(Ps) for _, Ps, _ in mem} == {2}
    assert mem[0][1][-1].shape[1] != mem[1][1][-1].shape[1]
    alone = []
    for A, Ps, B in mem:
        o = oracle_mod.OracleMG(Ps)
        o.precompute(A)
        alone.append(o.solve(B, np.zeros_like(B), tol=TOL, max_iter=MAX_ITER))
    return mem, alone


def test_union_loop_on_the_oracle_is_every_members_own_loop(three_members, oracle_mod):
    mem, alone = three_members
    assert all(cv for cv, _, _ in alone)
    assert len({len(rh) for _, _, rh in alone}) > 1, "the members need different numbers of cycles: that is the point"
    assert UR.tol_is_clear_of_the_histories([rh for _, _, rh in alone], TOL)
    Au = sp.block_diag([A for A, _, _ in mem], format="csr"); Au.sort_indices()
    Pu = [sp.block_diag([Ps[l] for _, Ps, _ in mem], format="csr") for l in range(2)]
    Bu = np.asfortranarray(np.concatenate([B for _, _, B in mem], axis=0))
    orc = oracle_mod.OracleMG(Pu)
    orc.precompute(Au)
    off = np.concatenate([[0], np.cumsum([A.shape[0] for A, _, _ in mem])])
    rows_of = [np.arange(off[i], off[i + 1]) for i in range(len(mem))]
    loop = UR.UnionLoop(lambda z: Bu - orc.A(0, z), lambda z: orc.vcycle(Bu, z), rows_of, TOL, MAX_ITER)
    out = loop.run(np.zeros_like(Bu))
    st, zs = out["st"], out["zs"]
    assert st.done == 1 and list(st.mdone) == [1, 1, 1]
    worst = 0.0
    for i, (cv1, z1, rh1) in enumerate(alone):
        rhi = st.his[i, :st.nhis[i]]
        assert out["stop"][i] == len(rh1) - 1 == len(rhi) - 1, (i, out["stop"][i], len(rh1))          # stops where its stand-alone solve stops
        for j in range(out["stop"][i], len(zs)):                                                    # ... and its rows do not change afterwards
            assert np.array_equal(zs[j][rows_of[i]], zs[out["stop"][i]][rows_of[i]]), (i, j)
        worst = max(worst, np.max(np.abs(rhi - rh1) / rh1))
        assert np.all(np.abs(rhi - rh1) <= HIS_BOUND * rh1), (i, np.max(np.abs(rhi - rh1) / rh1))
        assert rhi[-1] < TOL and np.all(rhi[:-1] >= TOL)
        assert np.array_equal(out["z"][rows_of[i]], z1), i                                            # the iterate itself: the same cycles, the same bits
    print("union loop vs stand-alone oracle: max relative difference of a history entry %.2e (bound %.0e)" % (worst, HIS_BOUND))
    assert worst <= HIS_BOUND and HIS_MEASURED * 100 <= HIS_BOUND <= HIS_MEASURED * 1000
    # the handle's history: the root of the sum over the members (none failed), entry by entry while members run or stand frozen.  Bound
    # (derived): N = n k squares and their sum in any order, the m member sums added, one root, against the correctly rounded norm.
    assert st.n_his == max(len(rh) for _, _, rh in alone)
    for j in range(st.n_his):
        r = Bu - orc.A(0, zs[j])
        exact = np.sqrt(exact_dot(r, r))
        assert abs(st.r_his[j] - exact) <= gamma(r.size + len(mem) + 2) * exact, j
    # the same run with the stops handed in (what the GPU lane does with the device's own histories) gives the same iterates
    again = loop.run(np.zeros_like(Bu), stops=[(s, 1) for s in out["stop"]])
    assert len(again["zs"]) == len(zs) and all(np.array_equal(a, b) for a, b in zip(again["zs"], zs))


def test_union_loop_cap_and_failed_member(three_members, oracle_mod):
    """max_iter = 3 at a tolerance nobody reaches: three entries each, nobody ended; a NaN in one member ends that member alone"""
    mem, _ = three_members
    A, Ps, B = mem[2]
    Au = sp.block_diag([A, A], format="csr")
    Pu = [sp.block_diag([P, P], format="csr") for P in Ps]
    Bu = np.asfortranarray(np.concatenate([B, 2.0 * B], axis=0))
    orc = oracle_mod.OracleMG(Pu); orc.precompute(Au)
    n = A.shape[0]
    rows_of = [np.arange(n), np.arange(n, 2 * n)]
    out = UR.UnionLoop(lambda z: Bu - orc.A(0, z), lambda z: orc.vcycle(Bu, z), rows_of, 1e-300, 3).run(np.zeros_like(Bu))
    assert list(out["st"].nhis) == [3, 3] and list(out["st"].mdone) == [0, 0] and out["st"].n_his == 3 and len(out["zs"]) == 4 and not out["st"].done
    Bn = Bu.copy(); Bn[n + 7, 1] = np.nan
    bad = UR.UnionLoop(lambda z: Bn - orc.A(0, z), lambda z: orc.vcycle(Bn, z), rows_of, 1e-9, 60).run(np.zeros_like(Bu))
    ok = UR.UnionLoop(lambda z: Bu - orc.A(0, z), lambda z: orc.vcycle(Bu, z), rows_of, 1e-9, 60).run(np.zeros_like(Bu))
    assert list(bad["st"].mdone) == [1, 2] and bad["st"].nhis[1] == 1 and bad["stop"] == [ok["stop"][0], 0]
    assert np.array_equal(bad["z"][rows_of[0]], ok["z"][rows_of[0]])                               # the block-diagonal oracle does not read across members
    assert np.array_equal(bad["st"].his[0, :bad["st"].nhis[0]], ok["st"].his[0, :ok["st"].nhis[0]])
    assert np.array_equal(bad["z"][rows_of[1]], np.zeros((n, 2)))                                  # frozen at the iterate it failed on
    assert np.all(np.isfinite(bad["st"].r_his[:bad["st"].n_his]))
