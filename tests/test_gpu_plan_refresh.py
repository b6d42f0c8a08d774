"""GPU (-m gpu): the three plan-based Gauss-Seidel sweeps -- overlapped tiling (k_tiled_gs), wave (k_wgs) and block (k_bgs) -- across value-only
re-precomputes, against the oracle built from the CALLER's matrices.

A time-stepping caller runs smg_precompute again and again on one pattern.  From the second call on the numeric work stays on the device, and the
plans, which hold private copies of the level's values and diagonals, are kept current in two places (csrc/smg_sweep_plans.cpp):
  refresh_plan_values   a plan that is live when the new values arrive gathers them through its maps; slots without a map keep their padding;
  set_plan_values       a plan built while the host copies are stale is built from old values and gathers the new ones at once.
Both read the level's values through the transpose map: after the first value-only call every level sweeps on the image of A^T.

One handle takes A1 (fresh) -> step(A1, 1) -> step(A1, 2) -> step(A1, 3) -> A1, A1 = the caller's bit-symmetric system and step = value_step
(tests/problems.py: same pattern, not bit-symmetric).  The first transition builds the recipes and drops every plan; the later ones refresh live
plans; the last returns to bit-symmetric values on a handle that stays on the A^T images.  After each, relax() is compared BITWISE with the
oracle's lexicographic sweep (the reference's loop: it walks column i) on OracleMG(Ps).precompute(A_i).level_A(lv), permuted into the order the
device sweeps.  Nothing of the reference comes from the handle's own matrix(): that call brings the host copies up to date and would turn the
stale state under test into the fresh one -- relax() runs before any such call (one case calls it on purpose).  Which plan ran is asserted through
device_bytes() and the order queries, so that a level that fell back to colour launches cannot pass for a plan."""
import numpy as np
import pytest
import scipy.sparse as sp

from oracle import mesh_np as M
from problems import subdiv_problem, value_step
from test_gpu_parity import smg  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

N_MATRICES = 5
_CACHE = {}


# ----------------------------------------------------------------------------------------------- the callers' systems and their references
def _csr(A):
    A = sp.csr_matrix(A)
    A.sort_indices()
    return A


def _mesh(smg, name):
    """(A1, known) of the three meshes, built once"""
    if ("mesh", name) not in _CACHE:
        if name == "torus":          # 4096 / 1024 / 256 / 64 rows, 4 colours: levels 0 and 1 tile, level 2 keeps one launch per colour
            mg, Vf, Ff = smg.mg_precompute_subdiv(*M.torus(8, 8), 3, n_extra_levels=0)
            Vf = M.normalize_unit_area(Vf, Ff)
            A1, known = _csr(M.massmatrix(Vf, Ff, "barycentric") - 0.01 * M.cotmatrix(Vf, Ff)), None
        elif name == "bunny":        # 9353 rows (tiled) / 2353 rows, 10 colours (wave Gauss-Seidel) / coarsest
            V, F = M.read_smgm("bunny.smgm")
            V = M.normalize_unit_area(V, F)
            A1, known = _csr(M.massmatrix(V, F, "barycentric") - 0.01 * M.cotmatrix(V, F)), None
            _CACHE[("VF", name)] = (V, F)
        else:                        # ogre_sim, two subdivisions, the boundary loop pinned: 40 277 / 10 295 rows, rows of up to 12 entries
            p = subdiv_problem("ogre_sim.smgm", n_sub=2, kind="poisson")
            A1, known = _csr(p["A"]), p["known"]
            _CACHE[("Ps", name)] = p["Ps"]
        _CACHE[("mesh", name)] = (A1, known)
    return _CACHE[("mesh", name)]


def _hierarchy(smg, name):
    """the mesh's hierarchy, before any smg_precompute"""
    _mesh(smg, name)
    if name == "torus":
        mg, Vf, Ff = smg.mg_precompute_subdiv(*M.torus(8, 8), 3, n_extra_levels=0)
        return mg
    if name == "bunny":
        V, F = _CACHE[("VF", name)]
        return smg.mg_precompute(V, F, 0.25, 200, 1)
    return smg.Hierarchy.from_prolongs(_CACHE[("Ps", name)])


def _matrix(name, i):
    """matrix i of the sequence A1, step(A1, 1), step(A1, 2), step(A1, 3), A1 (and step(A1, i) beyond)"""
    A1, known = _CACHE[("mesh", name)]
    if i in (0, N_MATRICES - 1):
        return A1
    if ("A", name, i) not in _CACHE:
        _CACHE[("A", name, i)] = value_step(A1, i)
    return _CACHE[("A", name, i)]


def _level_matrices(oracle_mod, name, i, Ps):
    """the oracle's level matrices of the caller's matrix i, CSR in the caller's numbering: computed once per mesh and matrix, never modified"""
    i = 0 if i == N_MATRICES - 1 else i
    if ("levels", name, i) not in _CACHE:
        A1, known = _CACHE[("mesh", name)]
        orc = oracle_mod.OracleMG(Ps)
        orc.precompute(_matrix(name, i), known)
        out = [_csr(orc.level_A(lv)) for lv in range(orc.n_levels - 1)]
        for a in out:
            a.data.setflags(write=False)
        _CACHE[("levels", name, i)] = out
    return _CACHE[("levels", name, i)]


def _oracle_sweeps(oracle_mod, A, to, b, x, iters):
    """the reference's relax() -- rows one after the other, row t's update from COLUMN t of the matrix it is given -- on A in the order `to`
    (position -> row); the result back in A's numbering.  (The oracle needs a hierarchy: one aggregate of all rows, its 1 x 1 Galerkin matrix.)"""
    n = A.shape[0]
    o = oracle_mod.OracleMG([sp.csr_matrix(np.ones((n, 1)))])
    o.precompute(_csr(A[to][:, to]))
    out = np.empty((n, b.shape[1]))
    out[to] = o.relax(0, b[to], x[to], iters)
    return out


def _vectors(n, k, lv):
    """b and x: uniform(-1, 1) from fixed seeds, k columns taken as a contiguous copy of a wider block"""
    wide_b = np.random.default_rng(100 + lv).uniform(-1, 1, (n, k + 3))
    wide_x = np.random.default_rng(200 + lv).uniform(-1, 1, (n, k + 3))
    return np.ascontiguousarray(wide_b[:, 1:k + 1]), np.ascontiguousarray(wide_x[:, 1:k + 1])


class Handle:
    """one hierarchy on the sequence of one mesh's matrices: what was fetched while the host copies were current, and the checks"""

    def __init__(self, smg, oracle_mod, name, before_precompute=None):
        self.oracle_mod, self.name = oracle_mod, name
        self.A1, self.known = _mesh(smg, name)
        self.mg = _hierarchy(smg, name)
        if before_precompute:
            before_precompute(self.mg)
        self.mg.precompute(self.A1, self.known)
        self.i = 0
        self.Ps = [self.mg.matrix(l, "P_full") for l in range(1, self.mg.n_levels)]
        self.perm = [self.mg.perm(lv) for lv in range(self.mg.n_levels - 1)]      # internal -> caller

    def precompute(self, i):
        self.mg.precompute(_matrix(self.name, i), self.known)
        self.i = i

    def bytes(self, lv, what):
        return self.mg.device_bytes().get("level%d.%s" % (lv, what), 0)

    def relax(self, lv, k, iters):
        b, x = _vectors(self.mg.rows(lv), k, lv)
        got = self.mg.relax(lv, b, x, iters)
        assert got.shape == b.shape and not np.isnan(got).any()
        return got

    def reference(self, lv, k, iters, order=None):
        """order: position -> internal row of the sweep (None: the internal numbering itself -- colour launches and overlapped tiling)"""
        A = _level_matrices(self.oracle_mod, self.name, self.i, self.Ps)[lv]
        to = self.perm[lv] if order is None else self.perm[lv][order]
        b, x = _vectors(A.shape[0], k, lv)
        return _oracle_sweeps(self.oracle_mod, A, to, b, x, iters)

    def check(self, lv, k, iters, order=None, got=None, what="relax"):
        got = self.relax(lv, k, iters) if got is None else got
        ref = self.reference(lv, k, iters, order)
        wrong = int((got != ref).any(axis=1).sum())
        assert wrong == 0, "%s: matrix %d, level %d, %d columns, %d sweeps: %d of %d rows differ from the oracle on the caller's matrix" % (
            what, self.i, lv, k, iters, wrong, got.shape[0])
        return got


# ----------------------------------------------------------------------------------------------- the references can tell
@pytest.mark.parametrize("name,levels", [("torus", (0, 1, 2)), ("bunny", (0, 1)), ("ogre", (0, 1))])
def test_the_references_tell_the_matrices_and_their_transposes_apart(smg, oracle_mod, name, levels):
    """What keeps the comparisons below from passing for a wrong reason, asserted on the oracle alone (caller's numbering, one sweep, one column):
    for every matrix that is not bit-symmetric and every checked level, the sweep on A_lv and the sweep on A_lv^T differ in EVERY row (a plan that
    gathered A where A^T is due would be seen everywhere); for A1, whose level 0 is bit-symmetric, the Galerkin levels still differ in some row;
    and the reference of matrix i differs from that of matrix i - 1 in every row (a plan left on stale values cannot pass)."""
    mg = _hierarchy(smg, name)
    Ps = [mg.matrix(l, "P_full") for l in range(1, mg.n_levels)]
    del mg
    prev = None
    for i in range(N_MATRICES):
        As = _level_matrices(oracle_mod, name, i, Ps)
        now = []
        for lv in levels:
            A = As[lv]
            n = A.shape[0]
            b, x = _vectors(n, 1, lv)
            on_A = _oracle_sweeps(oracle_mod, _csr(A.T), np.arange(n), b, x, 1)      # (the oracle walks the columns of what it is given)
            on_AT = _oracle_sweeps(oracle_mod, A, np.arange(n), b, x, 1)
            differ = int((on_A != on_AT).any(axis=1).sum())
            if i in (0, N_MATRICES - 1):
                assert (A != A.T).nnz == 0 if lv == 0 else differ >= 1, "A1, level %d: %d rows tell A from A^T" % (lv, differ)
            else:
                assert differ == n, "matrix %d, level %d: only %d of %d rows tell A from A^T" % (i, lv, differ, n)
            now.append(on_AT)
        if prev is not None:
            for lv, a, b_ in zip(levels, prev, now):
                assert (a != b_).all(), "matrices %d and %d give the same sweep in some row of level %d" % (i - 1, i, lv)
        prev = now


# ----------------------------------------------------------------------------------------------- overlapped tiling (and the colour launches next to it)
def _fresh_results(smg, oracle_mod, name, k, levels, sweeps, key, setup=None, order=None):
    """relax() of a freshly built handle on A1 (the A images, plans built from current host values), checked against the oracle; shared by the cases"""
    if key not in _CACHE:
        h = Handle(smg, oracle_mod, name, setup)
        out = {}
        for lv in levels:
            for s in sweeps:
                out[lv, s] = h.relax(lv, k, s)
            o = None if order is None else order(h.mg, lv)
            for s in sweeps:
                h.check(lv, k, s, o, got=out[lv, s], what="fresh handle")
        _CACHE[key] = out
    return _CACHE[key]


@pytest.mark.parametrize("k,mode", [(1, "stale"), (1, "unsolved"), (3, "stale"), (3, "peek"), (5, "stale"), (7, "stale"), (8, "stale")])
def test_tiled_relax_follows_the_callers_matrix(smg, oracle_mod, k, mode):
    """torus, levels 0 and 1 (4096 and 1024 rows: one-launch relax for k <= 7 in column groups 1, 3, 3 + 2, 3 + 3 + 1; k = 8: the wide colour kernels on
    the refreshed A^T image) and level 2 (256 rows: below the tiling range, one launch per colour on the SELL image refreshed through its own map).
    Plan states: after the first value-only call relax(2) and relax(1) only -- plans built while the host copies are stale (peek: after matrix(0)
    has brought them up to date, the not-stale build after a value-only call; unsolved: nothing ran on the handle before the first value-only call,
    so that a level whose internal matrix the host never needed builds it now, which brings the host copies up to date as well); after the
    second, relax(1) and relax(2) were refreshed live and relax(3) is used for the first time -- built stale while the others are live; after
    the third and after the return to A1 all three are live."""
    levels, tiled = (0, 1, 2), k <= 7
    h = Handle(smg, oracle_mod, "torus")
    mg = h.mg
    assert [mg.rows(lv) for lv in range(mg.n_levels)] == [4096, 1024, 256, 64]
    assert all(len(mg.colors(lv)) - 1 <= 5 for lv in levels)
    if mode != "unsolved":
        h.relax(0, k, 2)                               # a caller that has solved: plans exist, the first value-only call drops them

    def plans_live():
        for lv in (0, 1):
            assert (h.bytes(lv, "tiled_plans") > 0) == tiled, "level %d: tiled plans hold %d bytes" % (lv, h.bytes(lv, "tiled_plans"))
        assert h.bytes(2, "tiled_plans") == 0 and all(h.bytes(lv, "wgs_plan") == 0 and h.bytes(lv, "bgs_plan") == 0 for lv in levels)

    h.precompute(1)                                    # the first value-only call: recipes built, every level moves to A^T, all plans dropped
    assert h.bytes(0, "tiled_plans") == 0 and h.bytes(1, "tiled_plans") == 0 and h.bytes(0, "AT_sell") > 0
    if mode == "peek":
        assert (mg.matrix(0) != mg.matrix(0).T).nnz > 0
    for s in (2, 1):
        for lv in levels:
            h.check(lv, k, s)
            plans_live()
    h.precompute(2)                                    # relax(1), relax(2): refreshed live
    for s in (1, 2):
        for lv in levels:
            plans_live()
            h.check(lv, k, s)
    before = [h.bytes(lv, "tiled_plans") for lv in (0, 1)]
    got3 = {lv: h.relax(lv, k, 3) for lv in levels}    # relax(3): first use, built from stale host values next to live plans
    after = [h.bytes(lv, "tiled_plans") for lv in (0, 1)]
    assert all(a > b_ for a, b_ in zip(after, before)) if tiled else after == before == [0, 0]
    for lv in levels:
        h.check(lv, k, 3, got=got3[lv])
    fresh = _fresh_results(smg, oracle_mod, "torus", k, levels, (1, 2, 3), ("fresh", "torus", k))
    for i in (3, 4):                                   # all three live; 4: back to bit-symmetric values on the A^T images
        h.precompute(i)
        for s in (1, 2, 3):
            for lv in levels:
                plans_live()
                got = h.check(lv, k, s)
                if i == 4:
                    assert np.array_equal(got, fresh[lv, s]), "back on A1, level %d, %d sweeps: not the bits of a fresh handle" % (lv, s)
    assert after == [h.bytes(lv, "tiled_plans") for lv in (0, 1)]      # (nothing was rebuilt on the way)
    # which plan ran: no level sweeps piece- or block-wise (these queries build plans: after everything that was compared)
    assert all(mg.wave_gs_order(lv, k) is None and mg.block_gs_order(lv, k) is None for lv in levels)


def test_tiled_relax_with_rows_of_twelve_entries_and_constraints(smg, oracle_mod):
    """the W = 12 variant of the one-launch relax: ogre_sim subdivided twice, -L with the boundary loop pinned (the value-only call slices the unknown
    block out of the caller's values), levels 0 and 1 (40 277 and 10 295 rows), 3 columns, relax(2) across the five matrices"""
    k, s, levels = 3, 2, (0, 1)
    h = Handle(smg, oracle_mod, "ogre")
    mg = h.mg
    assert h.known is not None and [mg.rows(lv) for lv in levels] == [40277, 10295]
    h.relax(0, k, s)
    fresh = {lv: h.check(lv, k, s, what="fresh handle") for lv in levels}
    for i in range(1, N_MATRICES):
        h.precompute(i)
        for lv in levels:
            if i > 1:
                assert h.bytes(lv, "tiled_plans") > 0
            got = h.check(lv, k, s)
            assert h.bytes(lv, "tiled_plans") > 0
            if i == N_MATRICES - 1:
                assert np.array_equal(got, fresh[lv]), "back on A1, level %d: not the bits of the handle when it was fresh" % lv
    assert all(mg.wave_gs_order(lv, k) is None and mg.block_gs_order(lv, k) is None for lv in levels)


# ----------------------------------------------------------------------------------------------- wave Gauss-Seidel
@pytest.mark.parametrize("k", [1, 3, 8])
def test_wave_gauss_seidel_follows_the_callers_matrix(smg, oracle_mod, k):
    """the decimated bunny: level 0 (9353 rows) tiles for k <= 7, level 1 (2353 rows, 10 colours) sweeps piece-wise whatever k; relax(1) and relax(2)
    on both after every matrix -- built stale after the first value-only call, refreshed live from then on"""
    h = Handle(smg, oracle_mod, "bunny")
    mg = h.mg
    assert [mg.rows(lv) for lv in (0, 1)] == [9353, 2353] and len(mg.colors(1)) - 1 > 5
    order0 = mg.wave_gs_order(1, k)
    assert order0 is not None and mg.wave_gs_order(0, k) is None
    fresh = {}
    for lv in (0, 1):
        for s in (1, 2):
            fresh[lv, s] = h.check(lv, k, s, order0["rows"] if lv == 1 else None, what="fresh handle")
    for i in range(1, N_MATRICES):
        h.precompute(i)
        got = {}
        for s in (1, 2):
            for lv in (0, 1):
                if i > 1:
                    assert h.bytes(1, "wgs_plan") > 0 and (h.bytes(0, "tiled_plans") > 0) == (k <= 7)
                got[lv, s] = h.relax(lv, k, s)
        assert h.bytes(1, "wgs_plan") > 0 and (h.bytes(0, "tiled_plans") > 0) == (k <= 7) and h.bytes(0, "wgs_plan") == 0
        order = mg.wave_gs_order(1, k)
        assert order is not None and mg.wave_gs_order(0, k) is None
        assert np.array_equal(order["rows"], order0["rows"])       # (the pieces depend on the pattern alone)
        for (lv, s), g in got.items():
            h.check(lv, k, s, order["rows"] if lv == 1 else None, got=g)
            if i == N_MATRICES - 1:
                assert np.array_equal(g, fresh[lv, s]), "back on A1, level %d, %d sweeps: not the bits of the handle when it was fresh" % (lv, s)


def test_wave_gauss_seidel_on_every_level_next_to_unused_tiled_plans(smg, oracle_mod):
    """torus, 3 columns: after the first value-only call the tiled plans of relax(1) and relax(2) are built, then wave Gauss-Seidel is switched on for
    every level in range -- the tiled plans stay allocated, unused, and every later re-precompute refreshes both kinds.  Levels 0 and 1 sweep
    piece-wise and follow the matrices; back on automatic after one more matrix, the tiled plans that were refreshed unused are still right."""
    k, levels = 3, (0, 1)
    h = Handle(smg, oracle_mod, "torus")
    mg = h.mg
    h.relax(0, k, 2)                                   # (a caller that has solved)
    h.precompute(1)
    for s in (1, 2):
        for lv in levels:
            h.check(lv, k, s)
    tiled_bytes = [h.bytes(lv, "tiled_plans") for lv in levels]
    assert min(tiled_bytes) > 0 and all(h.bytes(lv, "wgs_plan") == 0 for lv in levels)
    mg.set_wave_gs("all")
    orders = None
    for i in range(1, N_MATRICES):
        if i > 1:
            h.precompute(i)
        got = {(lv, s): h.relax(lv, k, s) for s in (1, 2) for lv in levels}      # (i = 1: the wave plans are built stale next to live tiled plans)
        assert all(h.bytes(lv, "wgs_plan") > 0 and h.bytes(lv, "tiled_plans") >= tiled_bytes[lv] for lv in levels)
        now = [mg.wave_gs_order(lv, k) for lv in levels]
        assert all(o is not None for o in now) and mg.wave_gs_order(2, k) is None      # (256 rows: below the range)
        if orders is not None:
            assert all(np.array_equal(a["rows"], b_["rows"]) for a, b_ in zip(orders, now))
        orders = now
        for (lv, s), g in got.items():
            h.check(lv, k, s, orders[lv]["rows"], got=g, what="wave relax on every level")
    fresh = _fresh_results(smg, oracle_mod, "torus", k, levels, (1, 2), ("fresh-wave", "torus", k), setup=lambda m: m.set_wave_gs("all"),
                           order=lambda m, lv: m.wave_gs_order(lv, k)["rows"])
    for (lv, s), g in got.items():
        assert np.array_equal(g, fresh[lv, s]), "back on A1, level %d, %d sweeps: not the bits of a fresh handle" % (lv, s)
    mg.set_wave_gs("auto")
    h.precompute(N_MATRICES)                           # step(A1, 5): one more matrix, the tiled plans in use again
    for s in (1, 2):
        for lv in levels:
            assert h.bytes(lv, "tiled_plans") > 0
            h.check(lv, k, s, what="tiled relax after unused refreshes")
    assert all(mg.wave_gs_order(lv, k) is None for lv in levels)


# ----------------------------------------------------------------------------------------------- block Gauss-Seidel
def test_block_gauss_seidel_follows_the_callers_matrix(smg, oracle_mod):
    """torus with block Gauss-Seidel on every smoothed level (4096 / 1024 / 256 rows), 16 and 32 columns: 16 columns are first used after the first
    value-only call (the plan is built stale), relax(1) and relax(2) after every matrix; every later matrix reaches the plan through a live refresh"""
    levels = (0, 1, 2)
    h = Handle(smg, oracle_mod, "torus", lambda m: m.set_block_gs(0))
    mg = h.mg
    h.relax(0, 32, 2)                                  # (the plans exist; the first value-only call drops them)
    assert h.bytes(0, "bgs_plan") > 0
    h.precompute(1)
    assert all(h.bytes(lv, "bgs_plan") == 0 for lv in levels)
    orders = None
    for i in range(1, N_MATRICES):
        if i > 1:
            h.precompute(i)
            assert all(h.bytes(lv, "bgs_plan") > 0 for lv in levels)
        got = {(lv, k, s): h.relax(lv, k, s) for k in (16, 32) for s in (1, 2) for lv in levels}
        assert all(h.bytes(lv, "bgs_plan") > 0 and h.bytes(lv, "tiled_plans") == 0 and h.bytes(lv, "wgs_plan") == 0 for lv in levels)
        now = {(lv, k): mg.block_gs_order(lv, k) for k in (16, 32) for lv in levels}
        assert all(o is not None for o in now.values()) and all(mg.wave_gs_order(lv, 16) is None for lv in levels)
        assert all(np.array_equal(now[lv, 16]["rows"], now[lv, 32]["rows"]) for lv in levels)
        if orders is not None:
            assert all(np.array_equal(orders[key]["rows"], now[key]["rows"]) for key in now)
        orders = now
        for (lv, k, s), g in got.items():
            h.check(lv, k, s, orders[lv, k]["rows"], got=g, what="block relax")
    for k in (16, 32):
        fresh = _fresh_results(smg, oracle_mod, "torus", k, levels, (1, 2), ("fresh-block", "torus", k), setup=lambda m: m.set_block_gs(0),
                               order=lambda m, lv, k=k: m.block_gs_order(lv, k)["rows"])
        for lv in levels:
            for s in (1, 2):
                assert np.array_equal(got[lv, k, s], fresh[lv, s]), "back on A1, level %d, %d columns, %d sweeps: not the bits of a fresh handle" % (lv, k, s)
