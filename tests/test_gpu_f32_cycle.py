"""GPU (-m gpu): the fp32 V-cycle of the mixed-precision mode (precision = 1: enqueue_vcycle_t<float>, csrc/smg_cycle.cpp), piece by piece.

Parity contract (the fp32 row):
  sparse pieces   y = A x, r = b - A x, bc = PT r (+ the zeroed coarse iterate), u += P uc and relax() of every smoother: BIT-EXACT against the
                  float32 restatement tests/f32_reference.py on the level's matrices in the device numbering -- the same ascending-column sums,
                  separate multiply and add, as test_f32_reference_host.py proves against the oracle at float64 -- and, for the product-sums,
                  within gamma_32(w_i) sum_j |a_ij| |x_j| of the float64 sum, so that a failure can tell "wrong" from "another order";
  coarse solve    a bound derived from the roundings of the operation (below, at the tests);
  the cycle       bit for bit the composition of its pieces, fused first launches and buffer ping-pong included, SMG_FUSE_FIRST on and off;
  mixed solve     one outer iteration = z0 + double(V32((float)(b - A z0), 0)) bit for bit;
  done            a launch after convergence writes nothing.
All GPU work runs through smg_debug_cycle_f32 / smg_debug_convert_f32 (tests/kernel_hooks.py) and the library's public calls."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp

import f32_reference as R
import kernel_hooks as H
from oracle import mesh_np as M
from problems import block_shape_system, random_spd_hierarchy, subdiv_problem
from test_gpu_parity import _path_interp, _path_matrix, smg  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu
F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OMEGA, FRAC = 0.8, 0.1


# ----------------------------------------------------------------------------------------------- hierarchies
def _csr(M_):
    M_ = sp.csr_matrix(M_)
    M_.sort_indices()
    return M_


def _subdiv(smg, kind):
    p = subdiv_problem(kind=kind, k=1, n_sub=2)
    mg = smg.Hierarchy.from_prolongs(p["Ps"])
    mg.precompute(p["A"], p["known"])
    return mg


def _decimated(smg, name, with_system=False):
    V, F = M.read_smgm(name)
    V = M.normalize_unit_area(V, F)
    mg = smg.mg_precompute(V, F, 0.25, 500, 1)
    b = M.boundary_loop(F)
    if len(b):
        A, known = (-M.cotmatrix(V, F)).tocsr(), b
    else:
        A, known = (M.massmatrix(V, F, "barycentric") - 0.01 * M.cotmatrix(V, F)).tocsr(), None
    mg.precompute(A, known)
    return (mg, A, known) if with_system else mg


def _random(smg, seed, n, levels, hub):
    A, Ps = random_spd_hierarchy(np.random.default_rng(seed), n, levels, hub)
    mg = smg.Hierarchy.from_prolongs(Ps)
    mg.precompute(A)
    return mg


def _path(smg, n, levels, known=None):
    Ps, m = [], n
    for _ in range(levels - 1):
        Ps.append(_path_interp(m)); m = (m + 1) // 2
    mg = smg.Hierarchy.from_prolongs(Ps)
    mg.precompute(_path_matrix(n), None if known is None else np.asarray(known, np.int32))
    return mg


def _unsymmetric_values(A, seed=5):
    """A with every entry moved by up to 3e-5 relative, independently of its mirror image: far more than an fp32 ulp (6e-8), so that the
    fp32 image of A differs from the fp32 image of A^T and a smoother streaming the wrong one gives other bits"""
    A = A.tocsr().copy()
    A.sort_indices()
    A.data = A.data * (1.0 + 1e-5 * np.random.default_rng(seed).integers(-3, 4, A.nnz))
    return A


def _nonsym(smg):
    """a matrix that is not symmetric, neither in fp64 nor after rounding to fp32: the smoothers stream A^T (the reference walks column i),
    through its own fp32 image"""
    p = subdiv_problem(kind="mcf", k=1, n_sub=2)
    mg = smg.Hierarchy.from_prolongs(p["Ps"])
    mg.precompute(_unsymmetric_values(p["A"]))
    return mg


def _block(smg, kron=False, pinned=False, schur=False, nVCoarsest=100, nonsym=False, with_system=False):
    from test_gpu_block import elastic_like_system
    V, F = M.read_smgm("ogre_sim.smgm")
    V = M.normalize_unit_area(V, F)
    rng = np.random.default_rng(21 if pinned else 5)
    known = None
    if kron:
        S = (M.massmatrix(V, F, "barycentric") - 0.01 * M.cotmatrix(V, F)).tocsr()
        B3 = rng.uniform(-1, 1, (3, 3))
        A = _csr(sp.kron(S, sp.csr_matrix(B3 @ B3.T + 3.0 * np.eye(3)), format="csr"))
    elif pinned:
        A = elastic_like_system(V, F, rng, mass=0.0)
        pins = np.sort(rng.choice(V.shape[0], 37, replace=False))
        known = (3 * pins[:, None] + np.arange(3)[None, :]).ravel().astype(np.int32)
    else:
        A = elastic_like_system(V, F, rng, mass=50.0)
    if nonsym:
        A = _unsymmetric_values(A)
    mg = smg.mg_precompute_block(V, F, 0.25, nVCoarsest, 1)
    mg.set_block_mode("block")
    if schur:
        mg.set_coarse_schur("always", 1)
    mg.precompute(A, known)
    assert mg.block_size() == 3
    return (mg, A, known) if with_system else mg


def _block_shape(smg, name):
    """a block system off the mesh (problems.BLOCK_SHAPES; the fp64 checks and the proofs that these inputs reach the tail loop, ragged slices
    and partly filled blocks: test_gpu_block_shapes.py)"""
    A, Ps = block_shape_system(name)
    mg = smg.Hierarchy.from_prolongs(Ps)
    mg.set_block_mode("block")
    mg.precompute(A)
    assert mg.block_size() == 3
    return mg


BUILDERS = {
    "subdiv-mcf": lambda s: _subdiv(s, "mcf"),
    "subdiv-poisson": lambda s: _subdiv(s, "poisson"),
    "bunny-dec": lambda s: _decimated(s, "bunny.smgm"),
    "ogre-dec": lambda s: _decimated(s, "ogre.smgm"),
    "random-1500-hub": lambda s: _random(s, 3, 1500, 3, True),
    "random-4000-hub": lambda s: _random(s, 4, 4000, 4, True),
    "random-65": lambda s: _random(s, 5, 65, 2, False),
    "path-3": lambda s: _path(s, 3, 2), "path-10": lambda s: _path(s, 10, 2), "path-63": lambda s: _path(s, 63, 2),
    "path-64": lambda s: _path(s, 64, 2), "path-65": lambda s: _path(s, 65, 2), "path-129": lambda s: _path(s, 129, 2),
    "path-37-3lv": lambda s: _path(s, 37, 3), "path-50-pinned": lambda s: _path(s, 50, 2, [0, 7, 49]),
    "nonsym": _nonsym,
    "block-nonsym": lambda s: _block(s, nonsym=True),
    "block": lambda s: _block(s), "block-kron": lambda s: _block(s, kron=True), "block-pinned": lambda s: _block(s, pinned=True),
    "block-random-sparse": lambda s: _block_shape(s, "random-sparse-blocks"), "block-hub": lambda s: _block_shape(s, "hub"),
    "block-path-3": lambda s: _block_shape(s, "path-3"), "block-path-65": lambda s: _block_shape(s, "path-65"), "block-path-22": lambda s: _block_shape(s, "path-22"),
}
_CACHE = {}


class Case:
    """a precomputed hierarchy and, per smoothed level, the float32 restatement's images of its matrices in the device numbering"""

    def __init__(self, mg):
        self.mg = mg
        self.lv = []
        for lv in range(mg.n_levels - 1):
            A = _csr(mg.matrix(lv, "A", internal=True))
            G = _csr(A.T)                           # what the smoother streams (A itself where A is symmetric bit for bit)
            d = dict(perm=mg.perm(lv), permc=mg.perm(lv + 1), A=R.Ell(A, F32), G=R.Ell(G, F32), Gcsr=G,
                     P=R.Ell(_csr(mg.matrix(lv + 1, "P", internal=True)), F32), PT=R.Ell(_csr(mg.matrix(lv + 1, "PT", internal=True)), F32),
                     S=R.GsSchedule(G, F32, mg.colors(lv)), Acsr=A)
            d["unsym32"] = int((A.astype(F32) != G.astype(F32)).nnz)      # entries whose fp32 image differs from their mirror image's
            self.lv.append(d)


def case(smg, name):
    if name not in _CACHE:
        _CACHE[name] = Case(BUILDERS[name](smg))
    c = _CACHE[name]
    c.mg.set_smoother("gs", OMEGA, -1, FRAC)
    return c


def to_caller(perm, x):
    out = np.empty_like(x)
    out[perm] = x
    return out


def rnd(rng, shape):
    return rng.uniform(-1, 1, shape).astype(F32)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint32 if a.dtype == F32 else np.uint64),
                                                                          b.view(np.uint32 if b.dtype == F32 else np.uint64))


def worst(err, bound):
    return float((err / np.maximum(bound, 1e-300)).max())


# ----------------------------------------------------------------------------------------------- sparse pieces, bitwise
def check_sparse_pieces(c, k, smoothers=("gs",), seed=3):
    mg = c.mg
    rng = np.random.default_rng(seed)
    for lv, d in enumerate(c.lv):
        n, nc = mg.rows(lv), mg.rows(lv + 1)
        perm, permc = d["perm"], d["permc"]
        x, b, xc = rnd(rng, (n, k)), rnd(rng, (n, k)), rnd(rng, (nc, k))          # device numbering
        xC, bC, xcC = to_caller(perm, x), to_caller(perm, b), to_caller(permc, xc)
        x64, b64 = x.astype(np.float64), b.astype(np.float64)
        where = "level %d of %d, k = %d" % (lv, mg.n_levels, k)
        # y = A x
        got, ref = H.cycle_f32(mg, "A", lv, xC, out=H.sentinel((n, k), F32))[perm], R.spmv(d["A"], x)
        exact = d["A"].sums64(x)
        bound = R.product_sum_bound(d["A"], x)
        assert (np.abs(got - exact) <= bound).all(), "A x is WRONG (not an order effect) on %s: %.3g x the bound" % (where, worst(np.abs(got - exact), bound))
        assert same_bits(got, ref), "A x differs from the restatement in %d entries on %s (within the bound: another order?)" % ((got != ref).sum(), where)
        # r = b - A x
        got, ref = H.cycle_f32(mg, "RESID", lv, bC, xC, out=H.sentinel((n, k), F32))[perm], R.resid(d["A"], b, x)
        bound = R.product_sum_bound(d["A"], x, b64 - exact)
        assert (np.abs(got - (b64 - exact)) <= bound).all(), "b - A x is WRONG on %s: %.3g x the bound" % (where, worst(np.abs(got - (b64 - exact)), bound))
        assert same_bits(got, ref), "b - A x differs from the restatement in %d entries on %s" % ((got != ref).sum(), where)
        # bc = PT r, uc = 0
        gb, gu = H.cycle_f32(mg, "RESTRICT", lv, xC, out=(H.sentinel((nc, k), F32),) * 2)
        gb, ref = gb[permc], R.restrict(d["PT"], x)
        exact_r = d["PT"].sums64(x)
        bound = R.product_sum_bound(d["PT"], x)
        assert (np.abs(gb - exact_r) <= bound).all(), "PT r is WRONG on %s: %.3g x the bound" % (where, worst(np.abs(gb - exact_r), bound))
        assert same_bits(gb, ref), "PT r differs from the restatement in %d entries on %s" % ((gb != ref).sum(), where)
        assert same_bits(gu, np.zeros((nc, k), F32)), "the restriction launch did not leave +0 in the coarse iterate on %s" % where
        # u += P uc
        got, ref = H.cycle_f32(mg, "PROLONG_ADD", lv, xcC, out=xC)[perm], R.prolong_add(d["P"], x, xc)
        exact_p = x64 + d["P"].sums64(xc)
        bound = R.product_sum_bound(d["P"], xc, exact_p)
        assert (np.abs(got - exact_p) <= bound).all(), "u + P uc is WRONG on %s: %.3g x the bound" % (where, worst(np.abs(got - exact_p), bound))
        assert same_bits(got, ref), "u + P uc differs from the restatement in %d entries on %s" % ((got != ref).sum(), where)
        # relax(): 1 and 3 sweeps of every smoother asked for
        for sm in smoothers:
            mg.set_smoother(sm, OMEGA, -1, FRAC)
            if sm == "chebyshev":
                H.cycle_f32(mg, "RELAX", lv, bC, out=xC, pre=1)          # (the bound is computed with the first Chebyshev launch)
                lam = R.spectral_bound(d["Gcsr"])
                assert lam == mg.spectral_bound(lv), "the Gershgorin bound of %s: %r on the device, %r restated" % (where, mg.spectral_bound(lv), lam)
            for iters in (1, 3):
                got = H.cycle_f32(mg, "RELAX", lv, bC, out=xC, pre=iters)[perm]
                ref = (R.gauss_seidel(d["S"], b, x, iters) if sm == "gs" else R.jacobi(d["G"], b, x, iters, OMEGA) if sm == "jacobi"
                       else R.chebyshev(d["G"], b, x, iters, lam, FRAC))
                assert same_bits(got, ref), "%d %s sweep(s) differ from the restatement in %d entries on %s (largest difference %.3g)" % (
                    iters, sm, (got != ref).sum(), where, np.abs(got.astype(np.float64) - ref).max())
        mg.set_smoother("gs", OMEGA, -1, FRAC)


ALL3 = ("gs", "jacobi", "chebyshev")


@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 7, 8, 13, 16, 27, 64])
@pytest.mark.parametrize("name", ["subdiv-mcf", "subdiv-poisson"])
def test_sparse_pieces_on_subdivision_hierarchies_are_the_restatement_bit_for_bit(smg, name, k):
    """coded transfer operators, fixed-pitch panels, pinned vertices; every column-block seam of k_sell / k_sell_wide (4-column blocks, 8 / 16 /
    32 / 64 wide blocks and their remainders: 13 = 8 + 4 + 1, 27 = 16 + 8 + 3).  All three smoothers at k = 1, 3 and 16."""
    check_sparse_pieces(case(smg, name), k, ALL3 if (name == "subdiv-mcf" and k in (1, 3, 16)) else ("gs",))


@pytest.mark.parametrize("k", [1, 3, 8])
@pytest.mark.parametrize("name", ["bunny-dec", "ogre-dec"])
def test_sparse_pieces_on_decimated_hierarchies_are_the_restatement_bit_for_bit(smg, name, k):
    """Galerkin levels, value-carrying transfers, the long rows of the restrictions (long_valf): the levels whose fp64 sweeps run through the
    wave / tiled plans, so that only the fp32 cycle sweeps them colour by colour"""
    check_sparse_pieces(case(smg, name), k, ALL3 if k == 3 else ("gs",))


@pytest.mark.parametrize("name,k", [("random-1500-hub", 1), ("random-4000-hub", 3), ("random-65", 9), ("path-3", 1), ("path-10", 1), ("path-63", 1),
                                    ("path-64", 2), ("path-65", 1), ("path-129", 3), ("path-37-3lv", 5), ("path-50-pinned", 2)])
def test_sparse_pieces_on_irregular_tiny_and_unsymmetric_systems_are_the_restatement_bit_for_bit(smg, name, k):
    """hub rows (very wide slices, compact panels, many colours), systems smaller than one slice and around the 64-row boundary"""
    check_sparse_pieces(case(smg, name), k, ALL3 if name in ("random-1500-hub", "path-65") else ("gs",))


def unsymmetric_checks(smg_mod):
    """The smoothers must stream the fp32 image of A^T (dAT / bAT), everything else that of A.  On matrices whose fp32 images differ from
    their mirror images in most entries of every smoothed level -- asserted -- and for which the restatement itself gives other bits when it
    smooths with A instead of A^T -- asserted, for all three smoothers -- the sparse pieces are the restatement bit for bit, and the cycle
    (whose fused first launches take the coarse diagonal from the smoother's image) is the composition of its pieces.  Scalar and block."""
    rng = np.random.default_rng(7)
    for name in ("nonsym", "block-nonsym"):
        c = case(smg_mod, name)
        for lv, d in enumerate(c.lv):
            A = d["Acsr"]
            n = A.shape[0]
            assert d["unsym32"] >= 0.5 * (A.nnz - n), "level %d of %s: only %d of %d entries differ from their mirror image in fp32" % (lv, name, d["unsym32"], A.nnz)
            b, x = rnd(rng, (n, 2)), rnd(rng, (n, 2))
            EA = R.Ell(A, F32)
            assert not same_bits(R.gauss_seidel(d["S"], b, x, 1), R.gauss_seidel(R.GsSchedule(A, F32, c.mg.colors(lv)), b, x, 1)), (name, lv)
            assert not same_bits(R.jacobi(d["G"], b, x, 1, OMEGA), R.jacobi(EA, b, x, 1, OMEGA)), (name, lv)
            lam = R.spectral_bound(d["Gcsr"])
            assert not same_bits(R.chebyshev(d["G"], b, x, 1, lam, FRAC), R.chebyshev(EA, b, x, 1, lam, FRAC)), (name, lv)
        for k in (1, 3):
            check_sparse_pieces(c, k, ALL3)
        mg = c.mg
        for sm in SMOOTHERS5:
            set_smoother(mg, sm)
            for lv in sorted({0, min(1, mg.n_levels - 2)}):
                b, u = rnd(rng, (mg.rows(lv), 2)), rnd(rng, (mg.rows(lv), 2))
                for pre, post in ((2, 2), (1, 2)):
                    assert same_bits(H.cycle_f32(mg, "VCYCLE", lv, b, out=u, pre=pre, post=post), composed_vcycle(mg, lv, b, u, pre, post)), (name, sm, lv, pre, post)
        mg.set_smoother("gs", OMEGA, -1, FRAC)
    return "UNSYM_OK"


_UNSYM_CHILD = r"""
import os, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import surface_multigrid_code_amd as smg
import test_gpu_f32_cycle as T
print(T.unsymmetric_checks(smg))
"""


@pytest.mark.parametrize("fill_min", ["100", "100000000"])
def test_the_smoothers_stream_the_fp32_image_of_the_transpose(smg, fill_min):
    """unsymmetric_checks in a fresh child, with level 0's images filled on the device (SMG_DEVICE_FILL_MIN lowered to reach it on a test-sized
    mesh: A^T by k_sell_fill, transposed, then its fp32 image) and with the host-built images"""
    r = subprocess.run([sys.executable, "-c", _UNSYM_CHILD, ROOT], env=dict(os.environ, SMG_DEVICE_FILL_MIN=fill_min), capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0 and "UNSYM_OK" in r.stdout, (r.stdout[-1500:], r.stderr[-4000:])


@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("name", ["block", "block-kron", "block-pinned"])
def test_sparse_pieces_on_block_hierarchies_are_the_restatement_bit_for_bit(smg, name, k):
    """launch_bsr3 on the fp32 image (3 x 3 blocks; the restatement runs on the scalar 3n x 3n matrix: a block's structural zeros add +-0 to a sum that is
    never -0) and the transfers on 3 k columns"""
    check_sparse_pieces(case(smg, name), k, ALL3 if name == "block" else ("gs",))


@pytest.mark.parametrize("name,k", [("block-hub", 1)] + [(n, k) for n in ("block-random-sparse", "block-path-3", "block-path-65", "block-path-22") for k in (1, 2)]
                         + [("block-random-sparse", k) for k in (5, 11, 22)])
def test_sparse_pieces_on_block_systems_off_the_mesh_are_the_restatement_bit_for_bit(smg, name, k):
    """k_bsr3<.., float> on block rows wider than its 8 register columns (the Gauss-Seidel tail loop), slices of one to 33 vertices, dozens of tiny
    colours, partly stored blocks and diagonal blocks without a coupling; the transfers on 3 k = 15, 33 and 66 columns (a wide launch and its remainder)"""
    check_sparse_pieces(case(smg, name), k, ALL3 if name == "block-hub" else ("gs",))


def _more_diagonal(A):
    """A + diag(0.5 diag A): the same pattern, as symmetric as A, other values"""
    A2 = (A + 0.5 * sp.diags(A.diagonal())).tocsr()
    A2.sort_indices()
    return A2


@pytest.mark.parametrize("name", ["subdiv-mcf", "bunny-dec", "block"])
def test_the_fp32_images_follow_the_matrix(smg, name):
    """The fp32 images are made on demand from the matrices' current values.  A handle that has run the fp32 pieces -- its images exist -- is
    given new values for the same pattern (the value-only re-precompute, on the device), values that are not bit-symmetric (the smoothers move to
    the image of A^T, which did not exist before), and a new pattern (a full precompute on the same handle): after each, the sparse pieces are
    the restatement on the handle's current matrices, bit for bit.  bunny-dec: long rows and value-carrying transfers; block: 3 x 3 blocks.
    On the scalar handle's last state a mixed-precision solve returns the bits of a freshly built handle.
    (The unsymmetric step: D A1 D + diag differs from its transpose in the last bits of a double only -- its fp32 image is symmetric, 0 entries
    of 284 933 differ -- so every entry is moved by a further 1e-5 relative, _unsymmetric_values: the image of A and that of A^T then differ in
    most entries, asserted, and a smoother on the wrong one gives other bits.)"""
    if name == "bunny-dec":
        mg, A, known = _decimated(smg, "bunny.smgm", with_system=True)
        steps = [(1, ("gs",)), (3, ALL3)]
    elif name == "block":
        mg, A, known = _block(smg, with_system=True)
        steps = [(1, ("gs",)), (2, ("gs",))]
    else:
        p = subdiv_problem(kind="mcf", k=2, n_sub=2)
        A, known = _csr(p["A"]), p["known"]
        mg = smg.Hierarchy.from_prolongs(p["Ps"])
        mg.precompute(A, known)
        steps = [(1, ("gs",)), (3, ALL3)]
    mg.set_smoother("gs", OMEGA, -1, FRAC)
    check_sparse_pieces(Case(mg), steps[0][0], steps[0][1])          # the images now exist
    A2s = _more_diagonal(A)
    assert np.array_equal(A2s.indices, _csr(A).indices)
    mg.precompute(A2s, known)                                        # value-only
    check_sparse_pieces(Case(mg), steps[1][0], steps[1][1])
    if name != "subdiv-mcf":
        return
    assert (A2s != A2s.T).nnz == 0                                   # (bit-symmetric: the smoothers stayed on the image of A)
    rng = np.random.default_rng(42)
    D = sp.diags(1.0 + 0.01 * rng.uniform(size=A.shape[0]))
    A2 = _unsymmetric_values(_csr(D @ A @ D + sp.diags(rng.uniform(0, 0.5, A.shape[0]) * A.diagonal())))
    assert np.array_equal(A2.indices, A.indices)
    mg.precompute(A2, known)                                         # value-only, and no longer symmetric
    c = Case(mg)
    assert c.lv[0]["unsym32"] > 0, "the fp32 image of level 0 equals its mirror image: the wrong image would pass"
    assert c.lv[0]["unsym32"] >= 0.5 * (A2.nnz - A2.shape[0])
    check_sparse_pieces(c, 2)
    known2 = np.array([3, 500, 20000], np.int32)                     # another set of unknowns: a new pattern, a full precompute
    mg.precompute(A, known2)
    check_sparse_pieces(Case(mg), 1)
    fresh = smg.Hierarchy.from_prolongs(p["Ps"])
    fresh.precompute(A, known2)
    kv = np.zeros((len(known2), 2))
    o = smg.SolveOpts(tol=1e-9, max_iter=30, precision="mixed")
    r1, r2 = mg.solve(p["RHS"], p["z0"], kv, o), fresh.solve(p["RHS"], p["z0"], kv, o)
    assert r1[0] and np.array_equal(r1[1], r2[1]) and np.array_equal(r1[2], r2[2])


# ----------------------------------------------------------------------------------------------- coarse solve, derived bounds
COARSE_KS = [1, 2, 7, 8, 12, 16, 40, 64, 91]


def _coarse_handles(smg):
    if "coarse" not in _CACHE:
        p = subdiv_problem(kind="poisson", k=2, n_sub=2)
        dense = smg.Hierarchy.from_prolongs(p["Ps"]); dense.precompute(p["A"], p["known"])
        sch = smg.Hierarchy.from_prolongs(p["Ps"]); sch.set_coarse_schur("always", 1); sch.precompute(p["A"], p["known"])
        blk = _block(smg, kron=True, schur=True, nVCoarsest=600)
        assert dense.coarse_solver()["kind"] == "dense_inverse"
        assert sch.coarse_solver()["kind"] == "schur_complement" and blk.coarse_solver()["kind"] == "schur_complement"
        out = {}
        for name, mg in (("dense", dense), ("schur", sch), ("block-schur", blk)):
            Ac = mg.matrix(mg.n_levels - 1, "A").toarray()
            ev = np.linalg.eigvalsh(Ac)
            out[name] = dict(mg=mg, Ainv=np.linalg.inv(Ac), lmin=float(ev[0]), lmax=float(ev[-1]))
        _CACHE["coarse"] = out
    return _CACHE["coarse"]


@pytest.mark.parametrize("k", COARSE_KS)
def test_dense_coarse_product_within_the_bound_of_its_roundings(smg, k):
    """u += Ainv32 b with Ainv32 = fl32(A^-1), all three code paths of the fp32 launch_dense_gemv_add (k = 1: the symmetric tiles; 2 - 7: a wave
    per row; from 16 on 16-column tiles, 8 - 15 as narrow blocks in fp32).  Componentwise
        |got - (u + A^-1 b)| <= (gamma_32(n) + 2 u32) (|A^-1| |b|) + u32 |u + A^-1 b|
      gamma_32(n) |A^-1||b|   n rounded products and up to n rounded additions of a row's sum, in ANY order (tiles, partial sums, trees)
      u32 |A^-1||b|           the fp32 image: every entry of A^-1 rounded to nearest once
      u32 |A^-1||b|           the second-order terms of the two above ((1 + u)(1 + gamma) - 1 - u - gamma) and the fp64 inverse itself,
                              which the device forms by Gauss-Jordan to ~cond(A) 2^-53 -- both far below one u32
      u32 |u + A^-1 b|        the final rounded addition to the iterate.
    Largest observed multiple of the bound on an MI355X (n = 2 612; reported here and in DESIGN.md section 5, never fitted to): 0.004 - 0.007 for
    k = 1 .. 12, 0.019 - 0.023 for k = 16 .. 91."""
    h = _coarse_handles(smg)["dense"]
    mg, Ainv = h["mg"], h["Ainv"]
    nc = Ainv.shape[0]
    rng = np.random.default_rng(5)
    B, u = rnd(rng, (nc, k)), rnd(rng, (nc, k))
    got = H.cycle_f32(mg, "COARSE", 0, B, out=u)
    exact = u.astype(np.float64) + Ainv @ B.astype(np.float64)
    bound = (R.gamma32(nc) + 2 * R.U32) * (np.abs(Ainv) @ np.abs(B.astype(np.float64))) + R.U32 * np.abs(exact)
    err = np.abs(got - exact)
    print("dense coarse product, n = %d, k = %d: largest error / bound = %.4f" % (nc, k, worst(err, bound)))
    assert (err <= bound).all(), "k = %d: %.3g x the bound in column %d" % (k, worst(err, bound), int(np.argmax((err / np.maximum(bound, 1e-300)).max(axis=0))))
    assert err.max() > 0.0                      # (an fp32 product, not a widened fp64 one)


def _schur_factors(h):
    """the three factors of the handle's Schur-complement solver in float64, from its own partition of the rows (smg_debug_schur_partition)"""
    if "fac" not in h:
        mg = h["mg"]
        A = mg.matrix(mg.n_levels - 1, "A").toarray()
        blk = H.schur_partition(mg)
        I, S = np.flatnonzero(blk >= 0), np.flatnonzero(blk < 0)
        Dinv = np.zeros((len(I), len(I)))
        for b_ in range(blk.max() + 1):                      # D = diag(A_11 .. A_pp): interiors couple through the separator only
            q = np.flatnonzero(blk[I] == b_)
            Dinv[np.ix_(q, q)] = np.linalg.inv(A[np.ix_(I[q], I[q])])
        off = A[np.ix_(I, I)].copy()
        off[blk[I][:, None] == blk[I][None, :]] = 0.0
        assert not off.any(), "two interior blocks are coupled: not the partition of a Schur complement"
        P = A[np.ix_(I, S)]
        W = Dinv @ P
        Sinv = np.linalg.inv(A[np.ix_(S, S)] - P.T @ W)
        h["fac"] = dict(I=I, S=S, Dinv=Dinv, W=W, Sinv=Sinv)
    return h["fac"]


@pytest.mark.parametrize("k", COARSE_KS)
@pytest.mark.parametrize("name", ["schur", "block-schur"])
def test_schur_coarse_solve_within_the_bound_of_its_three_factors(smg, name, k):
    """the fp32 launch_schur_solve is not one product but three stages (csrc/smg_schur.hpp, csrc/smg_schur_device.hip: k_schur_g, the product with
    S^-1, k_schur_x), each a sum of products with an fp32 image -- of W = D^-1 P, of S^-1, of D^-1 and W:
        g = b_S - W^T b_I,      x_S = S^-1 g,      x_I = D^-1 b_I - W x_S,      u += x
    so its error carries the size of the intermediates g and x_S, and |A^-1||b| alone does not bound it.  The same reasoning as for the dense
    product, stage by stage, componentwise, with the factors formed in float64 from the solver's own partition of the rows and
    e = gamma_32(n + 66) + 2 u32   (a stage's sum has at most n + 64 rounded products -- the separator is padded to a multiple of 64 -- and one
                                    rounded addition of b; any order; the image of a factor rounds every entry once; the second u32 covers the
                                    second-order terms and the fp64 factorisation as in the dense case):
        dg   <= e (|b_S| + |W|^T |b_I|)                                 the computed g against the exact one
        dx_S <= |S^-1| dg + e |S^-1| (|g| + dg)                         an exact product with the computed g, plus this stage's own roundings
        dx_I <= |W| dx_S + e (|D^-1| |b_I| + |W| (|x_S| + dx_S))        likewise with the computed x_S
        |got - (u + A^-1 b)| <= dx (1 + u32) + u32 |u + A^-1 b|         the final rounded addition to the iterate
    The componentwise form of the dense product is printed beside it for comparison, not asserted.  Largest observed multiples on an MI355X
    (reported here and in DESIGN.md section 5, never fitted to): 0.0083 (scalar system, n = 2 612, 778 separator rows), 0.0046 (block system,
    n = 2 001, 1 138 separator rows); against the dense product's form 0.014 / 0.008."""
    h = _coarse_handles(smg)[name]
    mg, Ainv = h["mg"], h["Ainv"]
    f = _schur_factors(h)
    I, S, Dinv, W, Sinv = f["I"], f["S"], f["Dinv"], f["W"], f["Sinv"]
    nc = Ainv.shape[0]
    rng = np.random.default_rng(5)
    B, u = rnd(rng, (nc, k)), rnd(rng, (nc, k))
    got = H.cycle_f32(mg, "COARSE", 0, B, out=u)
    B64 = B.astype(np.float64)
    g = B64[S] - W.T @ B64[I]
    xS = Sinv @ g
    xI = Dinv @ B64[I] - W @ xS
    x = np.zeros((nc, k)); x[S] = xS; x[I] = xI
    assert np.abs(x - Ainv @ B64).max() <= 1e-9 * np.abs(x).max()          # (the factors are those of A: block elimination is exact)
    exact = u.astype(np.float64) + x
    e = float(R.gamma32(nc + 66)) + 2 * R.U32
    dg = e * (np.abs(B64[S]) + np.abs(W).T @ np.abs(B64[I]))
    dxS = np.abs(Sinv) @ dg + e * (np.abs(Sinv) @ (np.abs(g) + dg))
    dxI = np.abs(W) @ dxS + e * (np.abs(Dinv) @ np.abs(B64[I]) + np.abs(W) @ (np.abs(xS) + dxS))
    dx = np.zeros((nc, k)); dx[S] = dxS; dx[I] = dxI
    bound = dx * (1 + R.U32) + R.U32 * np.abs(exact)
    err = np.abs(got - exact)
    plain = (R.gamma32(nc) + 2 * R.U32) * (np.abs(Ainv) @ np.abs(B64)) + R.U32 * np.abs(exact)
    print("%s coarse solve, n = %d (%d separator rows), k = %d: largest error / derived bound = %.4f; error / the dense product's bound = %.4f"
          % (name, nc, len(S), k, worst(err, bound), worst(err, plain)))
    assert (err <= bound).all(), "k = %d: %.3g x the bound in column %d" % (k, worst(err, bound), int(np.argmax((err / np.maximum(bound, 1e-300)).max(axis=0))))
    assert err.max() > 0.0


# ----------------------------------------------------------------------------------------------- the cycle = its pieces
def composed_vcycle(mg, lv, b, u, pre, post):
    """the pieces in the order of enqueue_vcycle_t: relax, residual, restrict, the coarser cycle, prolong-add, relax (caller numbering)"""
    if lv == mg.n_levels - 1:
        return H.cycle_f32(mg, "COARSE", lv, b, out=u)
    u = H.cycle_f32(mg, "RELAX", lv, b, out=u, pre=pre)
    r = H.cycle_f32(mg, "RESID", lv, b, u)
    bc, uc = H.cycle_f32(mg, "RESTRICT", lv, r)
    uc = composed_vcycle(mg, lv + 1, bc, uc, pre, post)
    u = H.cycle_f32(mg, "PROLONG_ADD", lv, uc, out=u)
    return H.cycle_f32(mg, "RELAX", lv, b, out=u, pre=post)


SWEEPS = [(2, 2), (1, 2), (0, 3), (3, 1)]
SMOOTHERS5 = ["gs", "jacobi", "chebyshev", "hybrid", "hybrid_chebyshev"]


def set_smoother(mg, sm):
    mg.set_smoother(sm, OMEGA, mg.rows(1) if sm.startswith("hybrid") else -1, FRAC)      # hybrids: Gauss-Seidel on level 0 only


@pytest.mark.parametrize("sm", SMOOTHERS5)
@pytest.mark.parametrize("name,k", [("subdiv-mcf", 3), ("subdiv-poisson", 8), ("bunny-dec", 1), ("ogre-dec", 3), ("block", 2), ("block-pinned", 1)])
def test_the_cycle_is_the_composition_of_its_pieces(smg, name, k, sm):
    """SMG_F32_VCYCLE -- the launch sequence of the solve: the first colour / first Jacobi sweep / Chebyshev step 0 of a coarse level fused into
    the restriction launch, the Jacobi-type levels' ping-pong with the out-of-place prolongation for odd sweep counts -- returns bit for bit
    what the unfused pieces return one after the other, from level 0 and from an inner level."""
    c = case(smg, name)
    mg = c.mg
    set_smoother(mg, sm)
    rng = np.random.default_rng(17)
    try:
        for lv in sorted({0, min(1, mg.n_levels - 2)}):
            n = mg.rows(lv)
            b, u = rnd(rng, (n, k)), rnd(rng, (n, k))
            for pre, post in SWEEPS:
                got = H.cycle_f32(mg, "VCYCLE", lv, b, out=u, pre=pre, post=post)
                ref = composed_vcycle(mg, lv, b, u, pre, post)
                assert same_bits(got, ref), "%s, %s, V(%d,%d) from level %d, k = %d: %d entries differ, largest difference %.3g" % (
                    name, sm, pre, post, lv, k, (got != ref).sum(), np.abs(got.astype(np.float64) - ref).max())
                assert np.isfinite(got).all()
    finally:
        mg.set_smoother("gs", OMEGA, -1, FRAC)


def fuse_digest(smg_mod):
    """sha256 of V(2,2) and V(1,2) from level 0 on the subdivision and the decimated hierarchy with every smoother (parent and child process)"""
    hsh = hashlib.sha256()
    rng = np.random.default_rng(23)
    for name, k in (("subdiv-mcf", 3), ("bunny-dec", 2)):
        mg = case(smg_mod, name).mg
        b, u = rnd(rng, (mg.rows(0), k)), rnd(rng, (mg.rows(0), k))
        for sm in SMOOTHERS5:
            set_smoother(mg, sm)
            for pre, post in ((2, 2), (1, 2)):
                hsh.update(np.ascontiguousarray(H.cycle_f32(mg, "VCYCLE", 0, b, out=u, pre=pre, post=post)).tobytes())
        mg.set_smoother("gs", OMEGA, -1, FRAC)
    return hsh.hexdigest()


_FUSE_CHILD = r"""
import os, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import surface_multigrid_code_amd as smg
import test_gpu_f32_cycle as T
print("DIGEST", T.fuse_digest(smg))
"""


def test_the_fused_first_launches_do_not_change_a_bit(smg):
    """SMG_FUSE_FIRST=0 (read once per process: a fresh child) runs every first launch on its own; the cycle's bits are the same"""
    here = fuse_digest(smg)
    r = subprocess.run([sys.executable, "-c", _FUSE_CHILD, ROOT], env=dict(os.environ, SMG_FUSE_FIRST="0"), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    there = [ln.split()[1] for ln in r.stdout.splitlines() if ln.startswith("DIGEST")]
    assert there == [here], (here, r.stdout[-500:])


# ----------------------------------------------------------------------------------------------- one mixed outer iteration, converters
@pytest.mark.parametrize("kind,k", [("mcf", 3), ("mcf", 7), ("poisson", 2)])
def test_one_mixed_outer_iteration_is_the_fp32_cycle_between_the_two_converters(smg, kind, k):
    """solve(max_iter = 1, precision = "mixed") returns z0 + double(V32((float)(b - A z0), 0)) bit for bit: the residual by the fp64 piece,
    the conversion, the cycle and the addition by the fp32 hooks (k = 7: the solve pads to 8 columns, the hooks do not)"""
    p = subdiv_problem(kind=kind, k=k, n_sub=2)
    mg = smg.Hierarchy.from_prolongs(p["Ps"])
    mg.precompute(p["A"], p["known"])
    conv, z, rh = mg.solve(p["RHS"], p["z0"], p["known_val"], smg.SolveOpts(tol=1e-300, max_iter=1, precision="mixed"))
    assert len(rh) == 1 and not conv
    unk = mg.unknown()
    z0u = np.asarray(p["z0"])[unk]
    bu = np.asarray(p["RHS"])[unk]
    if p["known"] is not None:
        bu = bu - mg.matrix(0, "Auk") @ np.asarray(p["known_val"])
        assert not np.asarray(p["known_val"]).any()          # (zeros: the product's own rounding plays no part here)
    r = bu - mg.A(0, z0u)                                    # one rounded subtraction per entry, as the residual launch does
    assert abs(np.linalg.norm(r) - rh[0]) <= 1e-13 * rh[0]
    b32, u32 = H.residual_to_f32(mg, r)
    assert same_bits(b32, r.astype(F32)) and same_bits(u32, np.zeros_like(b32))
    e = H.cycle_f32(mg, "VCYCLE", 0, b32, out=u32, pre=2, post=2)
    zu = H.add_correction(mg, z0u, e)
    assert same_bits(zu, z0u + e.astype(np.float64))
    assert same_bits(np.ascontiguousarray(z[unk]), np.ascontiguousarray(zu)), "%d entries differ, largest %.3g" % ((z[unk] != zu).sum(), np.abs(z[unk] - zu).max())


def test_converters_round_as_ieee_says_and_stay_inside_their_block(smg):
    """(float) r: beyond the fp32 range -> +-inf, below it -> subnormals and +-0, ties to even; z + (double) e exact widening, one rounded
    addition; NaN-free in, NaN-free out; a handle that has served 5 columns keeps room behind a 2-column block: it is not written
    (the hook fills it with sentinel bytes and the wrapper asserts they survive)."""
    mg = case(smg, "subdiv-mcf").mg
    n = mg.rows(0)
    rng = np.random.default_rng(31)
    H.cycle_f32(mg, "A", 0, rnd(rng, (n, 5)))                # the fp32 vectors now hold 5 columns per row
    r = rng.uniform(-1, 1, (n, 2))
    special = np.array([1e39, -1e39, 3.5e38, -3.5e38, 3.4028235677973366e38, 1e-40, -1e-40, 1e-46, -1e-46, 2.0 ** -150, 1.5 * 2.0 ** -149,
                        2.0 ** -149, 2.0 ** -126, 1.0 + 2.0 ** -24, 1.0 + 2.0 ** -24 + 2.0 ** -50, 1.0 + 3 * 2.0 ** -24, 0.0, -0.0,
                        np.finfo(np.float64).max, np.finfo(np.float64).tiny])
    r[:len(special), 0] = special
    r[-len(special):, 1] = -special
    with np.errstate(over="ignore", under="ignore"):
        want = r.astype(F32)
    b32, u32 = H.residual_to_f32(mg, r)
    assert same_bits(b32, want) and same_bits(u32, np.zeros_like(want))
    assert np.isinf(b32).sum() == 12 and not np.isnan(b32).any()
    e = rnd(rng, (n, 2))
    e[:6, 0] = np.array([np.inf, -np.inf, 1e-40, -1e-45, 3.4e38, 0.0], F32)
    z = rng.uniform(-1, 1, (n, 2))
    z[3, 0] = 1e-300
    got = H.add_correction(mg, z, e)
    assert same_bits(got, z + e.astype(np.float64)) and not np.isnan(got).any()


# ----------------------------------------------------------------------------------------------- done, side effects
def _every_op(mg, k, rng, done, out_of):
    """every op once; out_of(shape): the block uploaded as the output.  Returns name -> (uploaded, returned)."""
    L = mg.n_levels
    n, nc, nl = mg.rows(0), mg.rows(1), mg.rows(L - 1)
    res = {}
    for op, rows_in, rows_out, kw in (("A", n, n, {}), ("RESID", n, n, dict(in1=rnd(rng, (n, k)))), ("RESTRICT", n, nc, {}), ("PROLONG_ADD", nc, n, {}),
                                      ("RELAX", n, n, dict(pre=2)), ("COARSE", nl, nl, {}), ("VCYCLE", n, n, dict(pre=2, post=2))):
        up = out_of((rows_out, k))
        got = H.cycle_f32(mg, op, 0, rnd(rng, (rows_in, k)), out=(up, up) if op == "RESTRICT" else up, done=done, **kw)
        res[op] = (up, got)
    return res


@pytest.mark.parametrize("k", [1, 8, 27])
@pytest.mark.parametrize("name", ["subdiv-mcf", "block"])
def test_a_launch_after_convergence_writes_nothing(smg, name, k):
    """every op with the control block's done flag set -- how the launches of a captured graph are replayed after the break test has fired:
    all outputs come back as the 0x5B sentinels they were uploaded as, with every smoother, and the hook finds every fp32 vector of every
    level (second iterates, update vectors, the coarser levels of the cycle) as it was after the uploads (kernel_hooks.cycle_f32 asserts
    it); the same calls with the flag clear do write"""
    mg = case(smg, name).mg
    rng = np.random.default_rng(41)
    try:
        for sm in ALL3:
            mg.set_smoother(sm, OMEGA, -1, FRAC)
            for op, (up, got) in _every_op(mg, k, rng, 1, lambda s: H.sentinel(s, F32)).items():
                for g in (got if isinstance(got, tuple) else (got,)):
                    assert same_bits(g, up), "%s with done = 1 wrote %d entries (%s, %s, k = %d)" % (op, (g.view(np.uint32) != up.view(np.uint32)).sum(), name, sm, k)
        for op, (up, got) in _every_op(mg, k, rng, 0, lambda s: H.sentinel(s, F32)).items():
            if op in ("PROLONG_ADD", "COARSE"):          # (a correction of size 1 added to the sentinel 6.2e16 is absorbed: no evidence either way)
                continue
            for g in (got if isinstance(got, tuple) else (got,)):
                assert not same_bits(g, up), "%s with done = 0 wrote nothing: the control of this test is broken" % op
        b32, u32 = H.residual_to_f32(mg, rng.uniform(-1, 1, (mg.rows(0), k)), done=1)
        assert same_bits(b32, H.sentinel(b32.shape, F32)) and same_bits(u32, H.sentinel(u32.shape, F32))
        z = rng.uniform(-1, 1, (mg.rows(0), k))
        assert same_bits(H.add_correction(mg, z, rnd(rng, z.shape), done=1), np.asfortranarray(z))
    finally:
        mg.set_smoother("gs", OMEGA, -1, FRAC)


def test_the_hooks_leave_the_handle_as_they_found_it(smg):
    """an fp64 solve and a mixed one return the same bits before and after the fp32 hooks ran (also with the done flag set), and the hooks at
    64, then 3, then 64 columns -- kcap32 grows once, the Jacobi-type levels' second iterate and update vector are re-allocated with it --
    return the same bits each time"""
    p = subdiv_problem(kind="mcf", k=3, n_sub=2)
    mg = smg.Hierarchy.from_prolongs(p["Ps"])
    mg.precompute(p["A"])
    o64, omx = smg.SolveOpts(tol=1e-9, max_iter=30), smg.SolveOpts(tol=1e-9, max_iter=30, precision="mixed")
    before = mg.solve(p["RHS"], p["z0"], None, o64), mg.solve(p["RHS"], p["z0"], None, omx)
    rng = np.random.default_rng(43)
    n = mg.rows(0)
    b64c, u64c, b3, u3 = rnd(rng, (n, 64)), rnd(rng, (n, 64)), rnd(rng, (n, 3)), rnd(rng, (n, 3))
    for sm in ("jacobi", "chebyshev"):           # the second iterate and the update vector exist at 3 columns: the 64-column calls re-allocate them
        mg.set_smoother(sm, OMEGA, -1, FRAC)
        H.cycle_f32(mg, "VCYCLE", 0, b3, out=u3, pre=1, post=1)
    runs = {}
    for sm in ("gs", "jacobi", "chebyshev"):
        mg.set_smoother(sm, OMEGA, -1, FRAC)
        for tag, (b, u) in (("64a", (b64c, u64c)), ("3", (b3, u3)), ("64b", (b64c, u64c))):
            runs[sm, tag] = H.cycle_f32(mg, "VCYCLE", 0, b, out=u, pre=2, post=1)
            H.cycle_f32(mg, "RELAX", 0, b, out=u, pre=1, done=1)
        assert same_bits(runs[sm, "64a"], runs[sm, "64b"]), sm
        assert same_bits(runs[sm, "3"], H.cycle_f32(mg, "VCYCLE", 0, b3, out=u3, pre=2, post=1)), sm
    mg.set_smoother("gs", OMEGA, -1, FRAC)
    after = mg.solve(p["RHS"], p["z0"], None, o64), mg.solve(p["RHS"], p["z0"], None, omx)
    for x, y in zip(before, after):
        assert x[0] and y[0] and np.array_equal(x[1], y[1]) and np.array_equal(x[2], y[2])


def test_the_hooks_refuse_what_the_fp32_cycle_refuses(smg):
    """a split-phase solve in progress, a union handle and a sparse coarse factorisation surface as SMG_ERR_INVALID with their message"""
    import ctypes as C
    p = subdiv_problem(kind="mcf", k=1, n_sub=1)
    mg = smg.Hierarchy.from_prolongs(p["Ps"]); mg.precompute(p["A"])
    L = mg.L
    n = mg.rows(0)
    x = np.zeros(n, F32); y = np.zeros(n, F32)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    call = lambda h: L.smg_debug_cycle_f32(h.h, 0, 0, 1, 0, 0, 0, fp(x), None, fp(y), None)
    assert call(mg) == 0
    assert L.smg_debug_cycle_f32(mg.h, 0, mg.n_levels - 1, 1, 0, 0, 0, fp(x), None, fp(y), None) == -1 and b"bad level" in L.smg_last_error()
    sparse = smg.Hierarchy.from_prolongs(p["Ps"]); sparse.set_coarse_dense_max(0); sparse.precompute(p["A"])
    assert sparse.coarse_solver()["kind"] == "sparse_cholesky"
    assert call(sparse) == -1 and b"sparse coarse" in L.smg_last_error()
    m2 = smg.Hierarchy.from_prolongs(p["Ps"])
    un = smg.Hierarchy.union([mg, m2])
    un.precompute(sp.block_diag([p["A"], p["A"]], format="csr"))
    xx = np.zeros(un.rows(0), F32); yy = np.zeros(un.rows(0), F32)
    assert L.smg_debug_cycle_f32(un.h, 0, 0, 1, 0, 0, 0, fp(xx), None, fp(yy), None) == -1 and b"union" in L.smg_last_error()
    import torch
    rhs = torch.tensor(np.asfortranarray(p["RHS"]).T.copy(), device="cuda").contiguous()
    z0 = torch.tensor(np.asfortranarray(p["z0"]).T.copy(), device="cuda").contiguous()
    mg.solve_begin(rhs.data_ptr(), mg.rows(0), z0.data_ptr(), mg.rows(0), 1)
    try:
        assert call(mg) == -1 and b"split-phase" in L.smg_last_error()
    finally:
        z = torch.zeros_like(z0)
        mg.solve_end(z.data_ptr(), mg.rows(0))
    assert call(mg) == 0
