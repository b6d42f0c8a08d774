"""GPU (-m gpu): the kernels only a union handle runs (csrc/smg_union_device.hip), launcher by launcher through the handle-free hook
smg_debug_union (guarded buffers, selectable done flag), and the loop they form on real union handles, against the restatement in
tests/union_reference.py.

Every bound here is one of three kinds, named where it is used: bit equality; a bound derived from gamma(.) (kernel_hooks.gamma: Higham's
gamma_N = N u / (1 - N u)); the one measured bound lives in the CPU lane (tests/test_union_host.py).  NaN compares equal to NaN: the payload of
a NaN that a square root or a sum hands on is not part of any contract."""
import numpy as np
import pytest
import scipy.sparse as sp

import kernel_hooks as KH
import union_reference as UR
from kernel_hooks import gamma, sentinel
from problems import _path_interp, _path_matrix
from test_gpu_parity import gs_bit_exact, oracle_on_device_numbering, smg  # noqa: F401  (fixture)
from test_gpu_union import members as mesh_members

pytestmark = pytest.mark.gpu

SIZES = (1, 3, 255, 256, 257, 1023, 1024, 1025, 2049)         # rows of the members of the launcher tests
COARSE_SIZES = (1, 2, 63, 64, 65, 127, 128, 129, 200)         # ... of the coarse product: ni == lda, < 32 active lanes, a partial second trip
COARSE_KS = (1, 2, 3, 4, 5, 6, 7, 8, 9, 13, 16)
I_SENT = 0x5B5B5B5B


def same(a, b):
    """bit for bit, NaN equal to NaN"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    nan = np.isnan(a) & np.isnan(b)
    return bool(np.all(nan | (a.view(np.int64) == b.view(np.int64))))


@pytest.fixture(scope="module")
def L(smg):
    return smg._lib.load()


@pytest.fixture(scope="module")
def lists():
    """the members' row lists, interleaved by a fixed random permutation of [0, n) as the colour-major numbering interleaves them; 40 rows
    belong to no member"""
    n = sum(SIZES) + 40
    perm = np.random.default_rng(2024).permutation(n).astype(np.int32)
    rptr = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int32)
    rows = perm[:rptr[-1]].copy()
    return n, rptr, rows, perm[rptr[-1]:]


def member_rows(rptr, rows):
    return [rows[rptr[i]:rptr[i + 1]] for i in range(len(rptr) - 1)]


def check_sumsq_decide(L, n, rptr, rows, outside, r, u, tol, st0, k):
    """one launch_union_sumsq_decide against member_sumsq + decide: everything bit for bit, sentinels where nothing may be written"""
    m = len(rptr) - 1
    got = KH.union_sumsq_decide(L, rptr, rows, r, u, sentinel((n, k)), sentinel(m), st0.mdone, st0.nhis, st0.his, tol, done=st0.done, status=st0.status,
                                n_his=st0.n_his, his_cap=st0.his_cap, r_last=st0.r_last, r_his=st0.r_his)
    ss = [UR.member_sumsq(r, ri, k) for ri in member_rows(rptr, rows)]
    st = UR.decide(UR.UnionState(m, st0.cap, his_cap=st0.his_cap, done=st0.done, status=st0.status, n_his=st0.n_his, r_last=st0.r_last, mdone=st0.mdone,
                                 nhis=st0.nhis, his=st0.his, r_his=st0.r_his), ss, tol)
    assert same(got["r"], r) and same(got["u"], u), "an input changed"
    if st0.done:
        assert same(got["ss"], sentinel(m)) and same(got["zsave"], sentinel((n, k))), "done = 1: the launch wrote"
    else:
        assert same(got["ss"], ss), (got["ss"], ss)
        assert same(got["zsave"][rows], u[rows]), "zsave is not u on the listed rows"
        assert same(got["zsave"][outside], sentinel((len(outside), k))), "zsave was written outside every list"
    assert np.array_equal(got["mdone"], st.mdone), (got["mdone"], st.mdone)
    assert np.array_equal(got["nhis"], st.nhis), (got["nhis"], st.nhis)
    assert same(got["his"], st.his), "a member's history (an entry written, or a sentinel beyond what may be written)"
    assert same(got["r_his"][:st0.his_cap], st.r_his), "the handle's history"
    assert (got["done"], got["status"], got["n_his"]) == (st.done, st.status, st.n_his)
    if not st0.done:
        assert same([got["r_last"], got["r_prev"], got["sumsq"]], [st.r_last, st.r_prev, st.sumsq]), (got, st.r_last, st.r_prev, st.sumsq)
    else:
        assert got["r_last"] == st0.r_last
    return got, st


# ---------------------------------------------------------------------------------------------------- SUMSQ_DECIDE
@pytest.mark.parametrize("variant", ["fresh", "running"])
@pytest.mark.parametrize("k", [1, 3, 5, 8])
def test_sumsq_decide_is_member_sumsq_and_decide(L, lists, k, variant):
    """bit equality throughout.  fresh: nobody ended, a tolerance that some members pass.  running: members already at 1 and 2, histories at
    cap - 1 / cap / cap + 1, a NaN inside one running member, a handle history at its cap."""
    n, rptr, rows, outside = lists
    m, cap = len(SIZES), 4
    rng = np.random.default_rng(100 + k)
    r = rng.uniform(-1, 1, (n, k)) * 10.0 ** rng.integers(-2, 3, (n, 1))
    u = rng.uniform(-1, 1, (n, k))
    r[outside] = np.nan                                                   # rows of no member must not enter any sum
    norms = np.sqrt([UR.member_sumsq(r, ri, k) for ri in member_rows(rptr, rows)])
    tol = float(np.sort(norms)[m // 2])                                   # r == tol for one member: it does not stop; those below do
    st0 = UR.UnionState(m, cap, his=sentinel((m, cap)), r_his=sentinel(cap))
    if variant == "running":
        st0 = UR.UnionState(m, cap, his_cap=2, n_his=2, r_last=0.75, mdone=[0, 1, 2, 0, 0, 1, 0, 2, 0], nhis=[3, 2, 1, 4, 5, 0, 0, 3, 1],
                            his=sentinel((m, cap)), r_his=sentinel(2))
        r[rows[rptr[4] + 100], k - 1] = np.nan                            # member 4 (257 rows) fails now
    got, st = check_sumsq_decide(L, n, rptr, rows, outside, r, u, tol, st0, k)
    if variant == "fresh":
        assert 0 < int(np.sum(st.mdone == 1)) < m and st.done == 0 and st.nhis.tolist() == [1] * m
    else:
        assert st.mdone[4] == 2 and st.nhis.tolist() == [4, 2, 1, 5, 6, 0, 1, 3, 2] and got["n_his"] == 3


@pytest.mark.parametrize("case", UR.DECIDE_CASES, ids=[c["name"] for c in UR.DECIDE_CASES])
def test_decide_table_runs_through_the_device(L, case):
    """the hand-written cases of the CPU lane (tests/test_union_host.py holds decide() to their expected values): one-row members whose residual
    is the exact root of the case's ss -- 1e200 where ss is to overflow to inf -- so that k_union_sumsq hands k_union_decide the very ss of
    the case.  Bit equality."""
    ss = np.array(case["ss"])
    m = len(ss)
    with np.errstate(invalid="ignore", over="ignore"):
        r = np.where(np.isinf(ss), 1e200, np.sqrt(ss)).reshape(m, 1)
        assert same((r * r).ravel(), ss)
    rptr, rows = np.arange(m + 1, dtype=np.int32), np.arange(m, dtype=np.int32)[::-1].copy()
    r = r[::-1].copy()                                                    # member i owns row m - 1 - i
    st0 = UR.state_of_case(case, fill=sentinel)
    got, st = check_sumsq_decide(L, m, rptr, rows, np.zeros(0, np.int64), r, np.ones((m, 1)), case["tol"], st0, 1)
    if not st0.done:
        assert same(got["ss"], ss)
    e = case["expect"]
    assert got["mdone"].tolist() == list(e["mdone"]) and got["nhis"].tolist() == list(e["nhis"]) and (got["done"], got["n_his"]) == (e["done"], e["n_his"])


# ---------------------------------------------------------------------------------------------------- RESTORE
@pytest.mark.parametrize("pattern", ["none", "all", "mixed", "mixed2"])
@pytest.mark.parametrize("k", [1, 3, 5, 8])
def test_restore_gives_ended_members_their_rows_back(L, lists, k, pattern):
    """bit equality: rows of the ended members (mdone 1 or 2) equal zsave, every other row -- running members, rows of no member -- is untouched"""
    n, rptr, rows, outside = lists
    m = len(SIZES)
    mdone = dict(none=[0] * m, all=[1, 2] * 4 + [1], mixed=[0, 1, 2, 0, 1, 0, 2, 1, 0], mixed2=[1, 0, 0, 2, 0, 1, 0, 0, 2])[pattern]
    rng = np.random.default_rng(200 + k)
    u, zsave = rng.uniform(-1, 1, (n, k)), rng.uniform(-1, 1, (n, k))
    got_u, got_z, got_d = KH.union_restore(L, rptr, rows, u, zsave, mdone)
    assert same(got_z, zsave) and got_d.tolist() == mdone
    assert same(got_u, UR.restore(u, zsave, rows, rptr, mdone, k))
    for i, ri in enumerate(member_rows(rptr, rows)):
        assert same(got_u[ri], zsave[ri] if mdone[i] else u[ri]), i
    assert same(got_u[outside], u[outside])


# ---------------------------------------------------------------------------------------------------- COARSE
@pytest.fixture(scope="module")
def coarse(L):
    """random symmetric blocks with zero padding (lda = the next multiple of 64), 16 columns of b and u, the exact reference of every column
    and the one-column call of every column -- computed once"""
    rng = np.random.default_rng(7)
    ldas = [(s + 63) // 64 * 64 for s in COARSE_SIZES]
    blocks = []
    for ni, lda in zip(COARSE_SIZES, ldas):
        S = rng.uniform(-1, 1, (ni, ni))
        B = np.zeros((lda, lda))
        B[:ni, :ni] = S + S.T
        blocks.append(B)
    n = sum(COARSE_SIZES)
    b = rng.uniform(-1, 1, (n, 16)) * 10.0 ** rng.integers(-2, 3, (n, 1))
    u = rng.uniform(-1, 1, (n, 16))
    mrow0 = np.concatenate([[0], np.cumsum(COARSE_SIZES)])
    exact, mag = UR.blockdiag_exact(blocks, mrow0, b, u)
    lda_of_row = np.repeat(ldas, COARSE_SIZES)
    one = np.concatenate([KH.union_coarse(L, blocks, COARSE_SIZES, b[:, [c]], u[:, [c]])[0] for c in range(16)], axis=1)
    return dict(blocks=blocks, b=b, u=u, mrow0=mrow0, exact=exact, mag=mag, lda_of_row=lda_of_row, one=one)


@pytest.mark.parametrize("k", COARSE_KS)
def test_blockdiag_product_every_column_chunk(L, coarse, k):
    """k = 1 .. 9, 13, 16: every KB and a second, third and fourth chunk of four columns.
    Bound (derived): gamma(lda + 2) (|u| + sum |a||b|) per entry.  On the device a term is rounded as a product, in at most lda / 32 additions
    of its lane's running sum, in the six steps of the shuffle tree and in the addition to u; the reference rounds its dot product and its
    addition: lda / 32 + 10 roundings in all, no more than lda + 2 from lda = 64 on.  Column c of a k-column call is the one-column call of
    that column bit for bit: the kernel forms every column with the same additions."""
    C = coarse
    b, u = C["b"][:, :k], C["u"][:, :k]
    got, got_b = KH.union_coarse(L, C["blocks"], COARSE_SIZES, b, u)
    assert same(got_b, b), "b changed"
    bound = gamma(C["lda_of_row"] + 2)[:, None] * (np.abs(u) + C["mag"][:, :k])
    err = np.abs(got - C["exact"][:, :k])
    assert np.all(err <= bound), (k, float((err / bound).max()))
    assert np.any(got != u)
    for c in range(k):
        assert same(got[:, c], C["one"][:, c]), "column %d of the %d-column call is not the one-column call" % (c, k)
    # b = 0 returns u bit for bit
    assert same(KH.union_coarse(L, C["blocks"], COARSE_SIZES, np.zeros_like(b), u)[0], u)


@pytest.mark.parametrize("k", [1, 5, 13])
def test_blockdiag_product_does_not_read_across_members(L, coarse, k):
    """with the b rows of member j NaN every other member's rows keep the bits of the clean call (0 x NaN of a padding column would be NaN)"""
    C = coarse
    b, u = C["b"][:, :k], C["u"][:, :k]
    clean = KH.union_coarse(L, C["blocks"], COARSE_SIZES, b, u)[0]
    for j in range(len(COARSE_SIZES)):
        bn = b.copy()
        bn[C["mrow0"][j]:C["mrow0"][j + 1]] = np.nan
        got = KH.union_coarse(L, C["blocks"], COARSE_SIZES, bn, u)[0]
        others = np.r_[0:C["mrow0"][j], C["mrow0"][j + 1]:len(b)]
        assert same(got[others], clean[others]), j
        assert np.all(np.isnan(got[C["mrow0"][j]:C["mrow0"][j + 1]])), j


# ---------------------------------------------------------------------------------------------------- done = 1
@pytest.mark.parametrize("k", [1, 5])
def test_done_flag_stops_every_union_launch(L, lists, coarse, k):
    """done = 1: every output buffer is uploaded as sentinels and comes back unchanged"""
    n, rptr, rows, outside = lists
    m = len(SIZES)
    rng = np.random.default_rng(300 + k)
    r, u = rng.uniform(-1, 1, (n, k)), rng.uniform(-1, 1, (n, k))
    isent = np.full(m, I_SENT, np.int32)
    got = KH.union_sumsq_decide(L, rptr, rows, r, u, sentinel((n, k)), sentinel(m), isent, isent, sentinel((m, 3)), 1e-3, done=1, n_his=1, his_cap=3)
    assert same(got["zsave"], sentinel((n, k))) and same(got["ss"], sentinel(m)) and same(got["his"], sentinel((m, 3))) and same(got["r_his"], sentinel(3))
    assert got["mdone"].tolist() == isent.tolist() == got["nhis"].tolist()
    assert (got["done"], got["n_his"], got["status"], got["r_last"], got["r_prev"], got["sumsq"]) == (1, 1, 0, -1.0, -1.0, -1.0)
    assert same(got["r"], r) and same(got["u"], u)
    got_u, got_z, _ = KH.union_restore(L, rptr, rows, sentinel((n, k)), u, [1] * m, done=1)
    assert same(got_u, sentinel((n, k))) and same(got_z, u)
    nc = sum(COARSE_SIZES)
    got_u, got_b = KH.union_coarse(L, coarse["blocks"], COARSE_SIZES, coarse["b"][:, :k], sentinel((nc, k)), done=1)
    assert same(got_u, sentinel((nc, k))) and same(got_b, coarse["b"][:, :k])


# ====================================================================================================== on handles
TOL, MAX_ITER = 1e-9, 60
RAGGED = (3, 65, 129, 257, 1025, 2049)


class Union:
    """a precomputed union handle with what the tests need of it: the block-diagonal system, right-hand sides, the members' rows"""

    def __init__(self, name, h, A, B, known=None, keep=None):
        self.name, self.h, self.A, self.B, self.keep = name, h, A.tocsr(), B, keep
        self.m = h.union_members()
        self.known = None if known is None else np.asarray(known, np.int32)
        self.unk = np.arange(A.shape[0]) if known is None else np.setdiff1d(np.arange(A.shape[0]), known)
        self.Auu = self.A[self.unk][:, self.unk].tocsr()
        self.first = [h.union_member_rows(i) for i in range(self.m)]
        # member i's rows among the unknowns (the numbering of the handle's level 0 pieces)
        self.rows_of = [np.nonzero((self.unk >= f) & (self.unk < f + c))[0] for f, c in self.first]

    def rhs(self, k):
        return np.asfortranarray(self.B[:, :k])


def _ragged(smg, sizes, name, scale=True):
    ms = [smg.Hierarchy.from_prolongs([_path_interp(n)]) for n in sizes]
    h = smg.Hierarchy.union(ms)
    A = sp.block_diag([_path_matrix(n) for n in sizes], format="csr"); A.sort_indices()
    h.precompute(A)
    rng = np.random.default_rng(len(sizes))
    # the members' right-hand sides differ in size, so that their loops end at different iterations under the one absolute tolerance
    B = np.concatenate([rng.uniform(-1, 1, (n, 16)) * (10.0 ** (i % 7 - 3) if scale else 1.0) for i, n in enumerate(sizes)], axis=0)
    return Union(name, h, A, B, keep=ms)


@pytest.fixture(scope="module")
def unions(smg):
    """the mesh union (the four members of test_gpu_union.py), the same with five pins per member, and the ragged unions of two-level path
    systems: 3 .. 2049 rows in one handle, a union of one, and 70 three-row members"""
    ms, As, Bs = mesh_members(smg, 16)
    Au = sp.block_diag(As, format="csr"); Au.sort_indices()
    Bu = np.concatenate(Bs, axis=0)
    h = smg.Hierarchy.union(ms)
    h.precompute(Au)
    out = dict(mesh=Union("mesh", h, Au, Bu, keep=ms))
    hp = smg.Hierarchy.union(ms)
    rng = np.random.default_rng(9)
    known = np.sort(np.concatenate([hp.union_member_rows(i)[0] + rng.choice(hp.union_member_rows(i)[1], 5, replace=False) for i in range(len(ms))]))
    hp.precompute(Au, known.astype(np.int32))
    out["pinned"] = Union("pinned", hp, Au, Bu, known=known, keep=ms)
    out["ragged"] = _ragged(smg, RAGGED, "ragged")
    out["one"] = _ragged(smg, (257,), "one")
    out["seventy"] = _ragged(smg, (3,) * 70, "seventy")
    return out


def sweep_plan_name(h, lv, k):
    """which Gauss-Seidel plan relax() takes on level lv with k columns, by the selection of csrc/smg_sweep_plans.cpp: the piece- and block-wise
    orders as the handle reports them, else the overlapped tiling (k <= 7, 512 .. 122 880 rows, at most 5 colours) or one launch per colour"""
    if h.wave_gs_order(lv, k) is not None:
        return "piece-wise"
    if h.block_gs_order(lv, k) is not None:
        return "block-wise"
    n, nc = h.rows(lv), len(h.colors(lv)) - 1
    return "overlapped tiling, one launch" if k <= 7 and 512 <= n <= 122880 and nc <= 5 else "one launch per colour"


@pytest.mark.parametrize("k", [1, 3, 5, 7, 13])
@pytest.mark.parametrize("which", ["mesh", "ragged", "one", "seventy"])
def test_union_levels_bit_exact_in_device_numbering(smg, oracle_mod, unions, which, k):
    """the sparse pieces of every union level -- one disconnected graph per member -- against the oracle on the level's matrix in the device
    numbering, at the raw widths a union runs (its columns are not padded).  Bit equality."""
    h = unions[which].h
    rng = np.random.default_rng(3)
    for lv in range(h.n_levels - 1):
        n, nc = h.rows(lv), h.rows(lv + 1)
        print("%s union, k = %d, level %d: %d rows, %d colours, relax by %s" % (which, k, lv, n, len(h.colors(lv)) - 1, sweep_plan_name(h, lv, k)))
        perm, permc = h.perm(lv), h.perm(lv + 1)
        oi = oracle_on_device_numbering(oracle_mod, h, lv)
        x, b, xc = rng.uniform(-1, 1, (n, k)), rng.uniform(-1, 1, (n, k)), rng.uniform(-1, 1, (nc, k))
        assert np.array_equal(h.A(lv, x)[perm], oi.A(0, x[perm])), "SpMV not bit-exact on level %d" % lv
        for iters in (1, 2):
            assert gs_bit_exact(oracle_mod, h, lv, b, x, iters), "GS sweep (%d) not bit-exact on level %d" % (iters, lv)
        assert np.array_equal(h.restrict(lv, x)[permc], oi.restrict(0, x[perm])), "restriction not bit-exact on level %d" % lv
        assert np.array_equal(h.prolong(lv, xc)[perm], oi.prolong(0, xc[permc])), "prolongation not bit-exact on level %d" % lv


@pytest.mark.parametrize("k", [1, 5])
@pytest.mark.parametrize("which", ["mesh", "ragged"])
def test_a_whole_cycle_is_isolated_member_by_member(unions, which, k):
    """vcycle(B, z) gives member i's rows the same bits whatever the other members' rows of B and z hold -- other random values, or NaN: the
    check on the tiling's rim and on pieces across member boundaries.  Bit equality."""
    U = unions[which]
    rng = np.random.default_rng(40 + k)
    n = U.A.shape[0]
    B, z = U.rhs(k), np.asfortranarray(rng.uniform(-1, 1, (n, k)))
    base = U.h.vcycle(B, z)
    assert np.all(np.isfinite(base)) and not np.array_equal(base, z)
    for i, ri in enumerate(U.rows_of):
        others = np.setdiff1d(np.arange(n), ri)
        for fill in ("random", "nan"):
            B2, z2 = B.copy(order="F"), z.copy(order="F")
            B2[others] = rng.uniform(-9, 9, (len(others), k)) if fill == "random" else np.nan
            z2[others] = rng.uniform(-9, 9, (len(others), k)) if fill == "random" else np.nan
            got = U.h.vcycle(B2, z2)
            assert np.array_equal(got[ri], base[ri]), "member %d's rows depend on the other members' (%s)" % (i, fill)


def run_loop_case(smg, U, k, tol=TOL, max_iter=MAX_ITER, z0_seed=None):
    """one full solve and its restatement: returns everything the assertions below need"""
    n = U.A.shape[0]
    B = U.rhs(k)
    z0 = np.zeros((n, k), order="F") if z0_seed is None else np.asfortranarray(np.random.default_rng(z0_seed).uniform(-1, 1, (n, k)))
    kv = None if U.known is None else np.zeros((len(U.known), k))
    if U.known is not None:
        z0[U.known] = 0.0
    o = smg.SolveOpts(tol=tol, max_iter=max_iter)
    conv, z, rh = U.h.solve(B, z0, kv, o)
    his = [U.h.union_history(i) for i in range(U.m)]
    return dict(B=B, z0=z0, kv=kv, conv=conv, z=z, rh=rh, his=his)


LOOP_CASES = [("mesh", k, None) for k in (1, 3, 4, 5, 7, 8, 13, 16)] + [("ragged", 1, None), ("ragged", 5, None), ("pinned", 3, 77), ("one", 1, None),
                                                                       ("seventy", 1, None)]


@pytest.mark.parametrize("which,k,z0_seed", LOOP_CASES, ids=["%s-k%d" % (w, k) for w, k, _ in LOOP_CASES])
def test_the_loop_is_its_restatement(smg, unions, which, k, z0_seed):
    """One full solve gives the histories; UnionLoop with cycle = the device's own vcycle() and the members' stop iterations read from
    union_history reproduces the iterate of every solve with max_iter = 1 .. N bit for bit: frozen rows stay frozen, running rows are the
    cycle's.  Every history entry is held to the correctly rounded norm of that member's residual of that iterate.
    Bounds: bit equality for the iterates; for history entry j of member i (derived)
        || gamma(L + 1) (|B| + |A| |z_j|) ||_2 + gamma(n_i k + 2) rhi[j],
    L the longest row: the residual's entries (L products, L additions), the n_i k squares and their sum, one root, and the reference's rounding;
    for the handle's history gamma(m + 4): the roots and squares of the members' entries, their sum, one root, the reference's rounding."""
    U = unions[which]
    S = run_loop_case(smg, U, k, z0_seed=z0_seed)
    rh, his, B = S["rh"], S["his"], S["B"]
    N = len(rh)
    assert S["conv"] and all(cv for cv, _ in his) and N == max(len(r) for _, r in his) < MAX_ITER
    assert UR.tol_is_clear_of_the_histories([r for _, r in his], TOL), "choose another tolerance: a residual lies within 1e-3 of it"
    for i, (cv, rhi) in enumerate(his):                                   # a stop happens exactly at the first entry below tol
        assert rhi[-1] < TOL and np.all(rhi[:-1] >= TOL), (i, rhi)
    # the restatement, in the numbering of the handle's level-0 pieces (the unknown rows)
    Bu = np.asfortranarray(B[U.unk])                                      # (the pins' values are zero: the reduced right-hand side is B's rows)
    loop = UR.UnionLoop(None, lambda z: U.h.vcycle(Bu, z), U.rows_of, TOL, MAX_ITER)
    out = loop.run(S["z0"][U.unk], stops=[(len(rhi) - 1, 1) for _, rhi in his])
    zs = out["zs"]
    assert len(zs) == N and out["st"].n_his == N
    o_of = lambda J: smg.SolveOpts(tol=TOL, max_iter=J)
    for J in range(1, N + 1):
        conv, z, rhJ = U.h.solve(B, S["z0"], S["kv"], o_of(J))
        want = zs[min(J, N - 1)]
        assert np.array_equal(z[U.unk], want), "the iterate after max_iter = %d is not the restated one" % J
        assert np.array_equal(rhJ, rh[:J]) and conv == (J == N)
        if U.known is not None:
            assert np.array_equal(z[U.known], S["kv"])
    assert np.array_equal(S["z"][U.unk], zs[-1])
    for i, (cv, rhi) in enumerate(his):                                   # frozen rows stay frozen
        for j in range(len(rhi) - 1, N):
            assert np.array_equal(zs[j][U.rows_of[i]], zs[len(rhi) - 1][U.rows_of[i]]), (i, j)
    # the histories against the correctly rounded norms
    worst = 0.0
    for j in range(N):
        running = [i for i in range(U.m) if j < len(his[i][1])]
        rows = np.concatenate([U.rows_of[i] for i in running])
        hi, lo, mag, Lmax = UR.residual_twofold(U.Auu[rows], Bu[rows], zs[j])
        at = 0
        for i in running:
            ni = len(U.rows_of[i])
            sl = slice(at, at + ni)
            at += ni
            exact = UR.norm_twofold(hi[sl], lo[sl])
            rhij = his[i][1][j]
            bound = gamma(Lmax + 1) * float(np.linalg.norm(mag[sl])) + gamma(ni * k + 2) * rhij
            worst = max(worst, abs(rhij - exact) / bound)
            assert abs(rhij - exact) <= bound, (i, j, rhij, exact, bound)
    print("%s union, k = %d: %d entries of the handle's history, members' %s; worst history error / bound %.3f" % (which, k, N, [len(r) for _, r in his], worst))
    # the handle's own history: the root of the sum over the members (none failed); an ended member's sum is the one of its last entry
    for j in range(N):
        ent = np.array([his[i][1][min(j, len(his[i][1]) - 1)] for i in range(U.m)])
        ref = np.sqrt(KH.exact_dot(ent, ent))
        assert abs(rh[j] - ref) <= gamma(U.m + 4) * ref, (j, rh[j], ref)
    # a solve after the piece calls returns the bits of the one before them
    conv2, z2, rh2 = U.h.solve(B, S["z0"], S["kv"], smg.SolveOpts(tol=TOL, max_iter=MAX_ITER))
    assert conv2 and np.array_equal(z2, S["z"]) and np.array_equal(rh2, rh)
    assert [U.h.union_history(i)[1].tolist() for i in range(U.m)] == [r.tolist() for _, r in his]


@pytest.mark.parametrize("which,k", [("mesh", 3), ("mesh", 5), ("ragged", 5)])
def test_the_cap(smg, unions, which, k):
    """max_iter = 3 at a tolerance nobody reaches: three entries per member, nobody converged, three entries of the handle's history, and z is
    the restated z_3 (bit equality)"""
    U = unions[which]
    S = run_loop_case(smg, U, k, tol=1e-300, max_iter=3)
    assert not S["conv"] and len(S["rh"]) == 3
    for cv, rhi in S["his"]:
        assert not cv and len(rhi) == 3
    Bu = np.asfortranarray(S["B"][U.unk])
    out = UR.UnionLoop(None, lambda z: U.h.vcycle(Bu, z), U.rows_of, 1e-300, 3).run(S["z0"][U.unk], stops=[None] * U.m)
    assert len(out["zs"]) == 4 and np.array_equal(S["z"][U.unk], out["zs"][3])


def test_same_bits_eager_replayed_and_after_other_shapes(smg, unions):
    """use_graph = 0 and 1 give the same bits; two calls in a row give the same bits; and after a solve of another width and another history
    capacity (k = 5, max_iter = 7: a larger zsave, a new his_cap, the graphs dropped) and a value-only re-precompute of the same values, the
    first solve's bits come back.  Bit equality."""
    U = unions["mesh"]
    n = U.A.shape[0]
    B3, B5 = U.rhs(3), U.rhs(5)
    z3, z5 = np.zeros((n, 3), order="F"), np.zeros((n, 5), order="F")
    state = lambda: [U.h.union_history(i) for i in range(U.m)]
    first = U.h.solve(B3, z3, None, smg.SolveOpts(tol=TOL, max_iter=60))
    his1 = state()
    again = U.h.solve(B3, z3, None, smg.SolveOpts(tol=TOL, max_iter=60))
    assert first[0] and again[0] and np.array_equal(first[1], again[1]) and np.array_equal(first[2], again[2])
    eager = U.h.solve(B3, z3, None, smg.SolveOpts(tol=TOL, max_iter=60, use_graph=0))
    his_e = state()
    assert eager[0] and np.array_equal(first[1], eager[1]) and np.array_equal(first[2], eager[2])
    assert all(a[0] == b[0] and np.array_equal(a[1], b[1]) for a, b in zip(his1, his_e))
    mid = U.h.solve(B5, z5, None, smg.SolveOpts(tol=TOL, max_iter=7))
    assert 1 < len(mid[2]) <= 7 and all(len(r) <= 7 for _, r in state())
    mid_eager = U.h.solve(B5, z5, None, smg.SolveOpts(tol=TOL, max_iter=7, use_graph=0))
    assert np.array_equal(mid[1], mid_eager[1]) and np.array_equal(mid[2], mid_eager[2])
    U.h.precompute(U.A)                                                   # the same values on the same pattern: the members' inverses are re-made
    third = U.h.solve(B3, z3, None, smg.SolveOpts(tol=TOL, max_iter=60))
    his3 = state()
    assert third[0] and np.array_equal(first[1], third[1]) and np.array_equal(first[2], third[2])
    assert all(a[0] == b[0] and np.array_equal(a[1], b[1]) for a, b in zip(his1, his3))
