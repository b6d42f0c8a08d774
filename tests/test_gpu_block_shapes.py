"""GPU (-m gpu): the 3 x 3 block kernels (csrc/smg_bsr3_device.hip: k_bsr3<MODE, LD1, T>, k_bsr3_fill, k_bsr3_gershgorin) and the transfers on
3 k columns, off the one mesh tests/test_gpu_block.py knows.

The systems come from problems.random_block_system on random graphs with hub rows and on path graphs (problems.BLOCK_SHAPES): block rows wider
than the 8 panel columns the Gauss-Seidel mode keeps in registers (its tail loop, with the diagonal block on either side of the seam), slices
of fewer than 64 vertices, systems of 1 - 3 vertices, dozens of tiny colours, blocks that are only partly stored, diagonal blocks that hold
their three diagonal entries and nothing else.  Every case proves from the host twin of its panels (block_image) that it reaches the edge
it is here for, so that another seed or size fails on its own input instead of passing without testing anything.

The checker and the bars are those of test_gpu_block.py / test_gpu_parity.py: the oracle on the scalar 3n x 3n matrix in the device numbering,
bit for bit per kernel (fp64, no FMA contraction); 1e-12 relative for the norm; the scalar tests' bars for the solves."""
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp

from problems import BLOCK_SHAPES, block_shape_system, random_spd_hierarchy, value_step
from test_gpu_parity import oracle_on_device_numbering, smg  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

K_OF = {"random": 1, "random-sparse-blocks": 2, "hub": 1, "under-half-fill": 4, "hub-wide-k": 8}
PATHS = ["path-1", "path-2", "path-3", "path-21", "path-22", "path-63", "path-64", "path-65", "path-129", "path-37-3lv"]
HUBS = ("hub", "hub-wide-k")
SPARSE = ("random-sparse-blocks", "hub", "under-half-fill") + tuple(PATHS[2:])      # keep < 1 and vertices without a coupling (path-1, -2: too few to say)
WR = 8                       # panel columns of a block row the Gauss-Seidel mode of k_bsr3 holds in registers; the rest is its tail loop
_HANDLES = {}


def block_handle(smg, name, A=None):
    """a hierarchy of the named system with the block kernels required; A: another matrix for the same prolongations"""
    A0, Ps = block_shape_system(name)
    mg = smg.Hierarchy.from_prolongs(Ps)
    mg.set_block_mode("block")                        # (under-half-fill: the automatic choice would be the scalar kernels)
    mg.precompute(A0 if A is None else A)
    assert mg.block_size() == 3
    return mg


def shared_handle(smg, name):
    if name not in _HANDLES:
        _HANDLES[name] = block_handle(smg, name)
    return _HANDLES[name]


def image_facts(mg, lv):
    """what the panels of level lv look like, from their host twin: vertices per slice, panel columns per slice, the panel column of every
    vertex's diagonal block (device numbering), and how many diagonal blocks store their three diagonal entries only"""
    mg.matrix(lv, "A", internal=True)                # (a level whose panels the device filled builds its host copy on demand)
    img = mg.block_image(lv)
    sr, so, sw = img["slice_row"], img["slice_off"], img["slice_w"]
    nrow = np.diff(sr)
    assert nrow.min() >= 1 and nrow.max() <= 64 and sr[-1] * 3 == mg.rows(lv)
    pos, diag_only = [], 0
    only = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1], bool)
    for s in range(len(sw)):
        lanes = np.arange(nrow[s])
        cols = img["col"][so[s]:so[s] + sw[s], :nrow[s]]
        own = cols == (sr[s] + lanes)[None, :]
        assert (own.sum(axis=0) == 1).all(), "a vertex without exactly one diagonal block in slice %d" % s
        assert (img["col"][so[s]:so[s] + sw[s], nrow[s]:] == -1).all(), "a lane behind the slice's vertices holds a block"
        j = own.argmax(axis=0)
        pos.append(j)
        v = img["val"][so[s] + j, :, lanes]          # (vertices, 9): the planes of the diagonal blocks
        diag_only += int(((v != 0) == only[None, :]).all(axis=1).sum())
    return dict(nrow=nrow, slice_w=sw, diag_pos=np.concatenate(pos), diag_only=diag_only)


def check_reaches_its_edge(mg, name):
    """the self-checks: this input runs the code it is here for"""
    facts = [image_facts(mg, lv) for lv in range(mg.n_levels - 1)]
    A0 = block_shape_system(name)[0]
    for lv, f in enumerate(facts):
        w, st = f["slice_w"], mg.block_stats(lv)
        print("%s lv%d: %d vertices in %d slices of %d .. %d (last %d), %d colours, slice_w %d .. %d, %d slices wider than %d (%d of them with w %% 4 != 0), diagonal block at panel "
              "column >= %d for %d vertices (largest %d), %d diagonal blocks with the diagonal only, %d entries in %d blocks (fill %.2f), %d block slots"
              % (name, lv, mg.rows(lv) // 3, len(w), f["nrow"].min(), f["nrow"].max(), f["nrow"][-1], st["vertex_colors"], w.min(), w.max(), (w > WR).sum(),
                 WR, ((w > WR) & (w % 4 != 0)).sum(), WR, (f["diag_pos"] >= WR).sum(), f["diag_pos"].max(), f["diag_only"], mg.matrix(lv, "A").nnz, st["blocks"],
                 mg.matrix(lv, "A").nnz / (9.0 * st["blocks"]), st["block_slots"]))
    if name in HUBS:
        wide = np.concatenate([f["slice_w"][f["slice_w"] > WR] for f in facts])
        assert len(wide) and (wide % 4 != 0).any(), "%s: no slice wider than %d panel columns with a ragged tail (widths %s)" % (name, WR, sorted(set(wide.tolist())))
        pos = np.concatenate([f["diag_pos"] for f in facts])
        assert (pos >= WR).any() and (pos < WR).any(), "%s: the diagonal blocks lie on one side of panel column %d only" % (name, WR)
    if name.startswith("path-"):
        nrow = facts[0]["nrow"]
        # a slice never straddles a colour: 129 vertices are 65 + 64, i.e. slices of 64, 1 and 64 -- the ragged one closes the first colour
        assert nrow.min() < 64 and (nrow[-1] < 64 or name == "path-129"), "%s: no ragged slice (vertices per slice %s)" % (name, nrow.tolist())
    if name in SPARSE:
        st = mg.block_stats(0)
        assert st["block_slots"] * 9 > A0.nnz and st["blocks"] * 9 > A0.nnz, "%s: every stored block is full" % name
        assert facts[0]["diag_only"] >= 1, "%s: no diagonal block with its three diagonal entries only" % name
    if name == "under-half-fill":
        assert A0.nnz < 0.5 * 9 * mg.block_stats(0)["blocks"]          # (what makes the automatic choice scalar)
    return facts


def check_kernels(oracle_mod, mg, k, seed=3):
    """every smoothed level: y = A x, 1 and 2 Gauss-Seidel sweeps, Jacobi and Chebyshev with 1 - 3 iterations, the Gershgorin bound, restriction
    and prolongation bit for bit the oracle on the scalar matrices in the device numbering; the residual norm within 1e-12"""
    rng = np.random.default_rng(seed)
    try:
        for lv in range(mg.n_levels - 1):
            n, nc = mg.rows(lv), mg.rows(lv + 1)
            perm, permc = mg.perm(lv), mg.perm(lv + 1)
            oi = oracle_on_device_numbering(oracle_mod, mg, lv)
            x, b, xc = rng.uniform(-1, 1, (n, k)), rng.uniform(-1, 1, (n, k)), rng.uniform(-1, 1, (nc, k))
            where = "level %d of %d (%d rows), k = %d" % (lv, mg.n_levels, n, k)
            mg.set_smoother("gs")
            oi.set_smoother(0, "gs")
            ref = oi.A(0, x[perm])
            assert np.array_equal(mg.A(lv, x)[perm], ref), "block SpMV not bit-exact on " + where
            for sweeps in (1, 2):
                assert np.array_equal(mg.relax(lv, b, x, sweeps)[perm], oi.relax(0, b[perm], x[perm], sweeps)), "%d block GS sweep(s) not bit-exact on %s" % (sweeps, where)
            mg.set_smoother("jacobi", 0.8)
            oi.set_smoother(0, "jacobi", 0.8)
            for iters in (1, 2, 3):
                assert np.array_equal(mg.relax(lv, b, x, iters)[perm], oi.relax(0, b[perm], x[perm], iters)), "%d block Jacobi sweep(s) not bit-exact on %s" % (iters, where)
            mg.set_smoother("chebyshev", cheby_fraction=0.1)
            oi.set_smoother(0, "chebyshev", 0.1)
            assert mg.spectral_bound(lv) == oi.spectral_bound(0), "Gershgorin bound on " + where
            for iters in (1, 2, 3):
                assert np.array_equal(mg.relax(lv, b, x, iters)[perm], oi.relax(0, b[perm], x[perm], iters)), "block Chebyshev of degree %d not bit-exact on %s" % (iters + 1, where)
            assert np.array_equal(mg.restrict(lv, x)[permc], oi.restrict(0, x[perm])), "restriction through Pv not bit-exact on " + where
            assert np.array_equal(mg.prolong(lv, xc)[perm], oi.prolong(0, xc[permc])), "prolongation through Pv not bit-exact on " + where
            nr = mg.residual_norm(lv, b, x)
            assert abs(nr - np.linalg.norm(b[perm] - ref)) <= 1e-12 * nr, "residual norm on " + where
    finally:
        mg.set_smoother("gs")


# ----------------------------------------------------------------------------------------------- kernels, per shape
@pytest.mark.parametrize("name", list(BLOCK_SHAPES) + PATHS)
def test_block_shape_kernels_bit_exact_in_device_numbering(smg, oracle_mod, name):
    """every shape at the column count of its row in problems.BLOCK_SHAPES' table (K_OF; the path systems at k = 2), after the proof that it
    reaches its edge; 21 / 22 vertices: 63 / 66 rows, the seam of the coarse solvers' tiles; 1 - 3 vertices: less than a slice, 3 coarse rows"""
    mg = shared_handle(smg, name)
    check_reaches_its_edge(mg, name)
    check_kernels(oracle_mod, mg, K_OF.get(name, 2))


@pytest.mark.parametrize("k", [4, 5, 8, 11, 16, 22])
@pytest.mark.parametrize("name", ["random-sparse-blocks", "hub-wide-k"])
def test_block_shape_kernels_at_every_column_seam(smg, oracle_mod, name, k):
    """The transfers of a block handle run on 3 k columns: 12, 15, 24, 33 (32 + 1), 48 and 66 (one wide launch of 64 and a remainder) -- the
    4-column blocks and the wide launches of launch_sell that k = 1 .. 3 never reach; launch_bsr3 runs one launch per column on a leading
    dimension of k.  k = 16: a scalar handle changes its sweep plan there, a block handle must keep the oracle's lexicographic sweep."""
    check_kernels(oracle_mod, shared_handle(smg, name), k, seed=100 + k)


@pytest.mark.parametrize("name", ["random-sparse-blocks", "hub"])
def test_block_shape_kernels_after_a_value_step(smg, oracle_mod, name):
    """A value-only re-precompute with a matrix that is not bit-symmetric (problems.value_step): the smoothers move to the image of A^T, built
    for partly filled blocks and irregular rows.  The level matrices are those of a fresh handle, the kernels the oracle's on them."""
    A1, Ps = block_shape_system(name)
    A2 = value_step(A1, 42)
    assert np.array_equal(A2.indices, A1.indices) and abs(A2 - A2.T).max() > 0
    mg = block_handle(smg, name)
    mg.precompute(A2)                                     # value-only
    assert mg.block_size() == 3
    fresh = block_handle(smg, name, A2)
    for l in range(mg.n_levels):
        a, b = mg.matrix(l, "A"), fresh.matrix(l, "A")
        assert np.array_equal(a.indptr, b.indptr) and np.array_equal(a.indices, b.indices) and np.array_equal(a.data, b.data), "level %d differs from a fresh handle's" % l
    Ai = mg.matrix(0, "A", internal=True)
    assert abs(Ai - Ai.T).max() > 0                       # (the sweep on A instead of A^T would give other bits)
    check_kernels(oracle_mod, mg, K_OF[name], seed=9)
    check_kernels(oracle_mod, fresh, K_OF[name], seed=9)


# ----------------------------------------------------------------------------------------------- solves
@pytest.mark.parametrize("name", list(BLOCK_SHAPES))
def test_block_shape_solves_match_the_oracle(smg, oracle_mod, name):
    """the bars of test_random_non_mesh_systems_match_the_oracle"""
    A, Ps = block_shape_system(name)
    mg = shared_handle(smg, name)
    o = oracle_mod.OracleMG(Ps); o.precompute(A)
    n, k = A.shape[0], K_OF[name]
    rng = np.random.default_rng(6)
    rhs, z0 = rng.uniform(-1, 1, (n, k)), rng.uniform(-1, 1, (n, k))
    a = mg.solve(rhs, z0, None, smg.SolveOpts(tol=1e-10, max_iter=200))
    b = o.solve(rhs, z0, tol=1e-10, max_iter=200)
    assert a[0] and b[0]
    assert np.linalg.norm(a[1] - b[1]) <= 1e-7 * np.linalg.norm(b[1])
    assert abs(len(a[2]) - len(b[2])) <= max(3, len(b[2]) // 4)


@pytest.mark.parametrize("name", PATHS)
def test_block_shape_solves_of_tiny_and_ragged_systems(smg, oracle_mod, name):
    """the bars of test_tiny_and_ragged_systems"""
    A, Ps = block_shape_system(name)
    mg = shared_handle(smg, name)
    o = oracle_mod.OracleMG(Ps); o.precompute(A)
    n, k = A.shape[0], 2
    rng = np.random.default_rng(1)
    rhs, z0 = rng.uniform(-1, 1, (n, k)), rng.uniform(-1, 1, (n, k))
    a = mg.solve(rhs, z0, None, smg.SolveOpts(tol=1e-10, max_iter=60))
    b = o.solve(rhs, z0, tol=1e-10, max_iter=60)
    assert a[0] and b[0] and abs(len(a[2]) - len(b[2])) <= 2
    assert np.linalg.norm(a[1] - b[1]) <= 1e-8 * max(np.linalg.norm(b[1]), 1e-300)


# ----------------------------------------------------------------------------------------------- the refusal
def _without_entry(A, p):
    """A without its p-th stored entry (explicit zeros stay)"""
    A = sp.csr_matrix(A)
    row = int(np.searchsorted(A.indptr, p, side="right")) - 1
    ptr = A.indptr.copy()
    ptr[row + 1:] -= 1
    return sp.csr_matrix((np.delete(A.data, p), np.delete(A.indices, p), ptr), shape=A.shape)


def _entry(A, r, c):
    p = A.indptr[r] + int(np.searchsorted(A.indices[A.indptr[r]:A.indptr[r + 1]], c))
    assert A.indices[p] == c
    return p


def broken_pattern(A, bs):
    """(Z, B): Z is A with one mirrored pair of off-diagonal entries stored as explicit 0.0 -- still structurally symmetric --, B is Z without
    one other off-diagonal entry whose mirror image stays.  bs = 3: both pairs lie in blocks that store further entries, so that the pattern
    of the blocks stays symmetric and only the scalar pattern breaks."""
    A = sp.csr_matrix(A).copy()
    A.sort_indices()
    n = A.shape[0]
    r = np.repeat(np.arange(n), np.diff(A.indptr))
    c = A.indices
    blk = (r // bs).astype(np.int64) * (n // bs) + c // bs
    uniq, inv, cnt = np.unique(blk, return_inverse=True, return_counts=True)
    cand = np.flatnonzero((r // bs != c // bs) & (cnt[inv] >= (2 if bs == 3 else 1)) & (r < c))
    z, d = cand[len(cand) // 3], cand[len(cand) // 2]
    assert r[z] // bs != r[d] // bs
    Z = A.copy()
    Z.data[z] = 0.0
    Z.data[_entry(A, c[z], r[z])] = 0.0
    B = _without_entry(Z, d)
    assert B.nnz == A.nnz - 1 and (B.data == 0).sum() == 2 and B[c[d], r[d]] != 0 and B[r[d], c[d]] == 0
    return Z, B


def test_block_shape_refusal_of_a_pattern_that_is_not_symmetric(smg, oracle_mod):
    """A scalar entry A(3i+d, 3j+e) whose mirror image is not stored: precompute refuses with "level %d matrix is not structurally symmetric",
    on a block handle and on a scalar one (with SMG_DEVICE_FILL_MIN=1 the device decides: the child of
    test_block_shape_kernels_with_device_filled_images runs this test too).  The images are made from the coarsest smoothed level upwards and
    a Galerkin product inherits the hole (many coarse entries have one path only), so random-sparse-blocks, three levels, is refused at level
    1; the two-level systems are refused at level 0, the matrix that was handed in.  An explicitly stored 0.0 is an entry like any other: no
    refusal, and the kernel on it is the oracle's.  A handle that holds a good matrix refuses the broken one as well and takes the good one
    again.
    (The same message in the value-only re-precompute, build_recipes, cannot be reached through the C ABI: that path is entered only with the
    pattern of the last full precompute, byte for byte -- the pattern key -- which was found symmetric then; a broken pattern of the same
    size is a new pattern and goes through the full precompute, as here.  That half of the check is left out.)"""
    rng = np.random.default_rng(2)
    for name, msg in (("random-sparse-blocks", "not structurally symmetric"), ("under-half-fill", "level 0 matrix is not structurally symmetric")):
        A, Ps = block_shape_system(name)
        Z, B = broken_pattern(A, 3)
        mg = block_handle(smg, name, Z)
        x = rng.uniform(-1, 1, (mg.rows(0), 1))
        perm = mg.perm(0)
        y = mg.A(0, x)
        assert np.array_equal(y[perm], oracle_on_device_numbering(oracle_mod, mg, 0).A(0, x[perm]))
        fresh = smg.Hierarchy.from_prolongs(Ps)
        fresh.set_block_mode("block")
        with pytest.raises(smg.SmgError, match=msg) as refused:
            fresh.precompute(B)
        print("%s without one scalar entry: %s" % (name, refused.value))
        with pytest.raises(smg.SmgError, match=msg):
            mg.precompute(B)
        mg.precompute(Z)
        assert mg.block_size() == 3 and np.array_equal(mg.A(0, x), y)
    # a scalar system, once
    As, Pss = random_spd_hierarchy(np.random.default_rng(5), 65, 2, False)
    Zs, Bs = broken_pattern(As, 1)
    sc = smg.Hierarchy.from_prolongs(Pss)
    sc.precompute(Zs)
    assert sc.block_size() == 1
    sc2 = smg.Hierarchy.from_prolongs(Pss)
    with pytest.raises(smg.SmgError, match="level 0 matrix is not structurally symmetric"):
        sc2.precompute(Bs)


# ----------------------------------------------------------------------------------------------- images filled on the device
def test_block_shape_kernels_with_device_filled_images():
    """SMG_DEVICE_FILL_MIN=1 (read once per process: a child): every smoothed level of the kernel tests above -- irregular rows, hub rows, partly
    filled blocks, slices of one vertex -- gets its panels from k_bsr3_fill (the rank by counting; the transposed bisection after the value
    step) instead of build_bsr3, and the device decides the refusal.  The solves stay out (-k)."""
    import time
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, SMG_DEVICE_FILL_MIN="1")
    t0 = time.time()
    # the child: 30 tests, 7.3 s on an MI355X, start of the interpreter and of the device included (8 s, doubled)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-p", "no:cacheprovider", "-k", "(kernels or refusal) and not device_filled"],
                       cwd=root, env=env, capture_output=True, text=True, timeout=16)
    print("the child with SMG_DEVICE_FILL_MIN=1: %.1f s, %s" % (time.time() - t0, r.stdout.strip().splitlines()[-1] if r.stdout.strip() else "no output"))
    assert r.returncode == 0 and " passed" in r.stdout and " failed" not in r.stdout and "deselected" in r.stdout, (r.stdout[-3000:], r.stderr[-2000:])
