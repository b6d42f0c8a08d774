"""GPU (-m gpu): the dense coarse solver -- launch_spd_inverse and launch_dense_gemv_add, csrc/smg_device.hip -- at the sizes where its kernels
change path, and the kernels that only an A/B knob selects.

One-level handles: Hierarchy(1), set_coarse_schur("never"), precompute(A); the coarse solve u += A^-1 b is then the whole call.  Sizes:
  2, 63, 64, 65            one tile (no look-ahead workgroup, no k_mirror_lower), one row past it
  127, 128, 129, 191       two and three tiles; row guards with n % 64 = 63, 0, 1
  257, 289                 five tiles; 289: n % 16 = 1
  448 | 449, 512           lda = 448: the last size where one column takes k_dense_gemv_add<1> | lda = 512: the first with the symmetric tiles
  513, 1 025               an odd tile count past the switch; n % 64 = 1
  8 129 ... 8 321          nt = 128, 129, 130, 131: the first sizes of the four-row update k_gj_update2<4> and its three remainders nt % 4
per = lda / 16 MFMA steps per wave is 4 at lda = 64 and 8 at 128: below DEPTH (12; 6 in the two-tile kernel), the prologue's and the tail's guards.

The matrix: a ring with three random chords per vertex, A = 1.05 diag(W 1) - W.  A mesh operator's inverse decays with distance, so a far tile of
the Gauss-Jordan iterate could miss an update and still pass under any tolerance; this family's inverse does not decay: the smallest per-tile
maximum of |A^-1| over the 64 x 64 tiles, relative to the largest, is asserted >= 1e-3 for every n <= 1 025 (a condition on the test's own
sensitivity, not a tolerance on the kernel; numpy on the host, seed 0: 0.21 at n = 65, 0.16 at 129, 0.034 at 257, 0.020 at 513, 0.013 at 1 025;
cond(A) 38 - 50 from n = 63 on) and was computed once for the large sizes, which the test does not invert on the host: 1.0e-3 at n = 8 129, 9.8e-4
at 8 193, 9.1e-4 at 8 257, 8.2e-4 at 8 321 (the smallest is the ragged last tile) -- a tile that missed an update would be wrong by eight orders
of magnitude more than the tolerance.

Reference: u + X with X from scipy's sparse LU (splu in its symmetric mode with the minimum-degree ordering of A + A^T: the default column
ordering fills this expander-like pattern almost completely, 40 s on the host at the large sizes instead of 7); |got - ref| <= 1e-11 max|ref|
(the tolerance of test_coarse_solve_matches_ldlt, at a condition number below its mesh matrices'), max|B - A X_got| <= 1e-11 max|B|, and a
second call returns the same bits."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import f32_reference as R
import kernel_hooks as H
from problems import _path_matrix
from test_gpu_parity import smg  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = [2, 63, 64, 65, 127, 128, 129, 191, 257, 289, 448, 449, 512, 513, 1025]
LARGE = [8129, 8193, 8257, 8321]
KS, KS_LARGE = (1, 2, 7, 8, 12, 16, 40, 64, 91), (1, 3, 16)
F32_SIZES = [63, 65, 289, 448, 512, 1025]
KNOB_SIZES = (65, 289, 512, 1025)
KNOBS = ["SMG_COARSE_MFMA=0", "SMG_COARSE_CPW=1", "SMG_GJ_2X2=0", "SMG_SYM_COARSE=0"]
TOL = 1e-11
CHILD_TIMEOUT = 300


def ring_with_chords(n, seed=0):
    """a ring with three random chords per vertex: weights U(0.5, 1.5), chords rng.integers(0, n, n) per round with the self-loops dropped,
    W + W.T, A = 1.05 diag(W 1) - W (strictly diagonally dominant, so SPD), sorted CSR.  n = 2: the path matrix."""
    if n == 2:
        A = _path_matrix(2)
    else:
        rng = np.random.default_rng(seed)
        i = np.arange(n)
        rows, cols = [i], [(i + 1) % n]
        for _ in range(3):
            c = rng.integers(0, n, n)
            rows.append(i[c != i]); cols.append(c[c != i])
        rows, cols = np.concatenate(rows), np.concatenate(cols)
        W = sp.coo_matrix((rng.uniform(0.5, 1.5, rows.size), (rows, cols)), shape=(n, n)).tocsr()
        W = W + W.T
        A = sp.diags(1.05 * np.asarray(W.sum(axis=1)).ravel()) - W
    A = sp.csr_matrix(A)
    A.sum_duplicates()
    A.sort_indices()
    return A


def tile_ratio(Ainv):
    """the smallest per-tile maximum of |A^-1| over the 64 x 64 tiles (the ragged last ones included) relative to the largest"""
    n = Ainv.shape[0]
    nt = -(-n // 64)
    m = np.array([[np.abs(Ainv[64 * I:64 * I + 64, 64 * J:64 * J + 64]).max() for J in range(nt)] for I in range(nt)])
    return float(m.min() / m.max())


_HANDLES = {}


def handle(smg_mod, n):
    """(mg, A, sparse LU of A, numpy inverse or None) of the one-level handle for size n, built once per process"""
    if n not in _HANDLES:
        A = ring_with_chords(n)
        mg = smg_mod.Hierarchy(1)
        mg.set_coarse_schur("never")
        mg.precompute(A)
        assert mg.n_levels == 1 and mg.rows(0) == n and mg.coarse_solver()["kind"] == "dense_inverse"
        Ainv = None
        if n <= 1025:
            Ainv = np.linalg.inv(A.toarray())
            ratio = tile_ratio(Ainv)
            print("n = %d: %d tiles, smallest / largest per-tile maximum of |A^-1| = %.3g" % (n, -(-n // 64), ratio))
            assert ratio >= 1e-3, "n = %d: the inverse decays to %.3g of its largest tile: a missed tile update could pass" % (n, ratio)
        lu = spla.splu(A.tocsc(), permc_spec="MMD_AT_PLUS_A", diag_pivot_thresh=0.0, options=dict(SymmetricMode=True))
        _HANDLES[n] = (mg, A, lu, Ainv)
    return _HANDLES[n]


def blocks(n, k, dtype=np.float64):
    """the right-hand side and the iterate of (n, k): the same in every process"""
    rng = np.random.default_rng(1000 * k + n)
    return rng.uniform(-1, 1, (n, k)).astype(dtype), rng.uniform(-1, 1, (n, k)).astype(dtype)


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def check_size(smg_mod, n, ks):
    """coarse_solve for every k against the sparse LU; returns {k: sha of the result}"""
    mg, A, lu, _ = handle(smg_mod, n)
    out = {}
    for k in ks:
        B, u = blocks(n, k)
        got = mg.coarse_solve(B, u)
        ref = u + lu.solve(B)
        err, res = np.abs(got - ref).max() / np.abs(ref).max(), np.abs(B - A @ (got - u)).max() / np.abs(B).max()
        print("n = %d, k = %d: |got - ref| / max|ref| = %.2e, max|B - A X| / max|B| = %.2e" % (n, k, err, res))
        assert err <= TOL, "n = %d, k = %d: %.3g max|ref| from the sparse LU, worst row %d, column %d" % (
            (n, k, err) + tuple(int(v) for v in np.unravel_index(np.argmax(np.abs(got - ref)), got.shape)))
        assert res <= TOL, "n = %d, k = %d: residual %.3g max|B|" % (n, k, res)
        assert np.array_equal(got, mg.coarse_solve(B, u)), "n = %d, k = %d: a second call returns other bits" % (n, k)
        out[k] = sha(got)
    return out


@pytest.mark.parametrize("n", SMALL)
def test_dense_coarse_solve_at_the_edges_of_its_tiles(smg, n):
    """k_gj_update2<2> with 1, 2, 3, 5, 7, 8, 9, 17 tiles, the row guards, the MFMA prologue and tail below DEPTH, the switch of one column to the
    symmetric tiles between lda = 448 and 512; every column path: 1 | 2 - 7 a wave per row | 8 - 15 a padded 16-column tile | 16, 32, 64 tiles
    (40 = 32 + 8, 91 = 64 + 16 + 11)"""
    check_size(smg, n, KS)


@pytest.mark.parametrize("n", LARGE)
def test_dense_coarse_solve_with_the_four_row_update(smg, n):
    """k_gj_update2<4> starts at nt = 128 tiles.  The kernel counts a block row's columns as (4 BY + 3) / 2 + 1 while gj_update2_blocks on the host
    clips that at the last tile: nt = 128, 129, 130, 131 are the four remainders nt % 4.  (The inverse of this family at these sizes: see the
    module's docstring -- every tile holds at least 8e-4 of the largest entry.)"""
    check_size(smg, n, KS_LARGE)


@pytest.mark.parametrize("n", F32_SIZES)
def test_fp32_coarse_product_at_the_edges_within_the_bound_of_its_roundings(smg, n):
    """u += fl32(A^-1) b through the fp32 launch_dense_gemv_add against the componentwise bound of
    test_dense_coarse_product_within_the_bound_of_its_roundings (test_gpu_f32_cycle.py, derived there):
        |got - (u + A^-1 b)| <= (gamma_32(n) + 2 u32) (|A^-1| |b|) + u32 |u + A^-1 b|,  A^-1 from numpy.
    Largest observed multiple of the bound on an MI355X (reported, never fitted to): 0.0010 - 0.020 below 16 columns, 0.0063 -
    0.061 from 16 columns on; it falls with n (gamma_32(n) grows faster than the error): 0.061 at n = 63, 0.048 at 65, 0.020 at 289, 0.018 at 448,
    0.012 at 512, 0.0083 at 1 025."""
    mg, A, lu, Ainv = handle(smg, n)
    for k in KS:
        B, u = blocks(n, k, np.float32)
        got = H.cycle_f32(mg, "COARSE", 0, B, out=u)
        exact = u.astype(np.float64) + Ainv @ B.astype(np.float64)
        bound = (R.gamma32(n) + 2 * R.U32) * (np.abs(Ainv) @ np.abs(B.astype(np.float64))) + R.U32 * np.abs(exact)
        err = np.abs(got - exact)
        worst = float((err / np.maximum(bound, 1e-300)).max())
        print("dense coarse product, n = %d, k = %d: largest error / bound = %.4f" % (n, k, worst))
        assert (err <= bound).all(), "n = %d, k = %d: %.3g x the bound in column %d" % (n, k, worst, int(np.argmax((err / np.maximum(bound, 1e-300)).max(axis=0))))


_CHILD = r"""
import os, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import surface_multigrid_code_amd as smg
import test_gpu_coarse_shapes as T
for n in T.KNOB_SIZES:
    for k, h in T.check_size(smg, n, T.KS).items():
        print("sha", n, k, h)
print("CHILD_OK")
"""


@pytest.mark.parametrize("knob", KNOBS)
def test_the_coarse_kernels_behind_a_knob(smg, knob):
    """The knobs are read once per process, so each runs in a fresh child: the same sizes' checks, the same reference, the same 1e-11.
      SMG_COARSE_MFMA=0   fp64 k_dense_gemm_tile<16 / 32 / 64, double>, 8 - 15 columns back on k_dense_gemv_add
      SMG_COARSE_CPW=1    k_dense_gemm_mfma<64> instead of the two-tile kernel, whose comment claims "the same bits": bit-equal at k = 64 and 91
      SMG_GJ_2X2=0        k_gj_update, one tile per workgroup
      SMG_SYM_COARSE=0    one column through k_dense_gemv_add<1> at every size"""
    name, value = knob.split("=")
    mine = {n: check_size(smg, n, KS) for n in KNOB_SIZES}
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT], env=dict(os.environ, **{name: value}), capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    assert r.returncode == 0 and "CHILD_OK" in r.stdout, "%s: exit status %s\n%s\n%s" % (knob, r.returncode, r.stdout[-3000:], r.stderr[-4000:])
    theirs = {(int(w[1]), int(w[2])): w[3] for w in (ln.split() for ln in r.stdout.splitlines() if ln.startswith("sha "))}
    assert sorted(theirs) == sorted((n, k) for n in KNOB_SIZES for k in KS), r.stdout[-3000:]
    other = sorted(nk for nk, h in theirs.items() if h != mine[nk[0]][nk[1]])
    print("%s: within %g of the sparse LU at every (n, k); other bits than the default kernels at %d of %d: %s" % (knob, TOL, len(other), len(theirs), other))
    if name == "SMG_COARSE_CPW":
        for n in KNOB_SIZES:
            for k in (64, 91):
                assert theirs[(n, k)] == mine[n][k], "k_dense_gemm_mfma<64> and the two-tile kernel give other bits at n = %d, k = %d" % (n, k)
