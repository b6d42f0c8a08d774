"""GPU (-m gpu): the multi-column variants of the wave Gauss-Seidel kernel, and three launch choices of the SELL kernels, at test size.

launch_wgs (csrc/smg_wgs_device.hip) serves one piece colour with k_wgs<NBMAX, KB, RIMI>: NBMAX = 3 / 5 / 8 by the batches of 8 entry slots the level's
widest row needs (nb_max <= 3, <= 5, <= 8), RIMI = 2 / 4 / 7 by the plan's rim pitch (128 / 256 / 448), KB columns per lane by the size of the level: a
level of at most SMG_WGS_KB2_MAX_PIECES (1600) pieces runs groups of SMG_WGS_KB_SMALL (1) columns, a larger one groups of SMG_WGS_KB_BIG (4), the
remaining k % KB columns in a launch of their own at a column offset.  Every test mesh is far below 1600 pieces, so every other test launches KB = 1
only.  Here every case runs four times -- in this process (default knobs) and in three fresh child processes, the knobs being read once per process:

  big      SMG_WGS_KB2_MAX_PIECES=0                               groups of 4 + a tail of k % 4
  small2   SMG_WGS_KB2_MAX_PIECES=1000000000 SMG_WGS_KB_SMALL=2   groups of 2 + a tail of 1
  small3   SMG_WGS_KB2_MAX_PIECES=1000000000 SMG_WGS_KB_SMALL=3   groups of 3 + a tail of 1 or 2

with k = 1, 2, 3, 4, 5, 6, 7, 8, 11, 18 columns (LAUNCHES below: the exact (KB, groups) list of every run, asserted through smg_debug_wgs_launches, which
answers through the functions launch_wgs itself calls; the plan it is asked about is the one relax() just used, smg_debug_wgs_level_plan: a level that
fell back to colour launches has none and fails).  The levels -- plans built on the host, smg_debug_wgs_level_plan(from_host = 1), before any GPU run:

  case          hierarchy                                                       level  rows  pieces  nb_max  rim pitch   NBMAX  RIMI
  torus         torus(8, 8) subdivided 3 times, set_wave_gs("all")                0    4096    103      1       256        3     4
                                                                                  1    1024     33      1       128        3     2
  bunny-dec     bunny.smgm, mg_precompute(V, F, 0.25, 60, 1), M - 0.01 L          1    2353     62      4       256        5     4
                                                                                  2     597     18      6       128        8     2
  bunny15k-pin  bunny_15K_init.smgm, mg_precompute(V, F, 0.25, 200, 1),           1    3952     87      4       256        5     4
                -L with 40 pinned vertices                                        2     989     29      6       256        8     4
  random-1500   random_spd_hierarchy(default_rng(1), 1500, 2, hub = False),       0    1500    174      3       448        3     7
                set_wave_gs("all"): no mesh, a rim of > 256 rows per piece
  random-700-a  random_wide(3, 700, 8, 14): 8 to 13 random links per row, rows of up   0     700     42      4       448        5     7
                to 31 entries, set_wave_gs("all")
  random-700-b  random_wide(3, 700, 12, 20): rows of up to 46 entries                  0     700     53      6       448        8     7
  band-600      band_matrix(600, 20): 20 links to either side, rows of up to 41             0     600     31      5       128        5     2
                entries, a rim of at most 40 rows per piece, set_wave_gs("all")
  (bunny-dec-stepped: bunny-dec after a value-only re-precompute with value_step(A, 1): the levels sweep on the A^T image, plans built from stale host values)

All nine (NBMAX, RIMI) pairs are reached (the mesh levels give five; wide rows with a rim above 256 rows need a matrix without locality, rows of 25 to 40
entries with a rim below 129 rows a band), and each level runs KB = 1 (this process), 2, 3 and 4 (k = 2, 3, 4 of the `big` child; k = 5, 6, 7, 11, 18
put a tail launch behind groups of 4; 8, 11 and 18 put several groups into the grid's second dimension).  A hub row of random_spd_hierarchy has 120
entries: more than 64 off-diagonal entries disqualify a level, so the widest class comes from the second Galerkin level of a decimated mesh.

Asserted, without a tolerance anywhere:
  relax() with 1 and 2 sweeps is, bit for bit, the oracle's lexicographic sweep on the level permuted into the piece order (order_oracle of
  test_gpu_wgs.py); b and x are columns 1 .. k of wider blocks from fixed seeds; every vector of every child has the SHA-256 of this process's: the
  sweep does not depend on KB.
  bunny-dec, k = 3 and 8: a solve of exactly 6 cycles (tol = 0) gives the same z and r_his bits in all four runs; with a tolerance the fourth residual
  meets, the history is the first four entries of that run and z is, bit for bit, the z of a solve of exactly 3 cycles: the launches behind the
  `done` flag -- the rest of the graph of four iterations and the next graph -- have written nothing, KB > 1 included.

The other launch choices DESIGN.md section 11 listed as held by no test, same pattern:
  SMG_DEEP=0          on bunny-dec and random-1500, k = 1, 2, 3, 4: A x, b - A x (smg_raw_spmv), the restriction against the oracle in the device numbering,
                      bit for bit, k_sell in the child and k_sell_deep here -- which launches are deep, in which row-width class (3 / 5 / 8: widest
                      slice <= 24, <= 40, <= 64 panel columns) and how four columns split (3 + 1, 2 + 2, 1 + 1 + 1 + 1) is asserted through
                      smg_debug_deep_launches; a full-depth V-cycle (the restriction with the zeroed coarse iterate and the fused first coarse colour,
                      the level residuals) and residual_norm (sums of squares: k_sell on both sides) have the same bits in both runs.
  SMG_DEEP_MIN_W=1    ogre_sim subdivided once, -L with the boundary pinned, rows of 4 to 11 entries: the deep kernel's per-lane width guards with one
                      and two live batches of 8, coded transfers included; the same pieces against the oracle, the same bits as k_sell here.
  SMG_GS_WPB=2 / 8    with SMG_ONE_XCD_MAX=0, SMG_PITCH_SPEC_MAX=0 and SMG_TILED=0, so that a colour launch of test size takes
                      k_sell<SELL_GS, 1, T, 7, 2 / 8> (asserted per colour through smg_debug_gs_colour_wpb): ogre_sim subdivided twice (fixed-pitch panels, lower width 7),
                      colours whose slices are no multiple of 2 and of 8; gs_bit_exact at k = 1 with 1 and 3 sweeps, the bits of this process.

No child replaces the program of a process that has opened the GPU: each is a fresh interpreter started with subprocess, with a time limit of its own;
at most three are alive at once and all of them are watched in turn; the first that fails, aborts or runs out of its time fails the test and the others
are stopped; nothing is retried."""
import hashlib
import os
import struct
import subprocess
import sys
import tempfile
import time

import numpy as np
import pytest
import scipy.sparse as sp

import kernel_hooks as H
from oracle import mesh_np as M
from problems import random_spd_hierarchy, subdiv_problem, value_step
from test_gpu_parity import gs_bit_exact, oracle_on_device_numbering, smg  # noqa: F401  (fixture)
from test_gpu_plan_refresh import _vectors
from test_gpu_wgs import decimated, order_oracle

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT = 300          # seconds, per child
MAX_ALIVE = 3
KS = (1, 2, 3, 4, 5, 6, 7, 8, 11, 18)
BIG = dict(SMG_WGS_KB2_MAX_PIECES="0")
SMALL2 = dict(SMG_WGS_KB2_MAX_PIECES="1000000000", SMG_WGS_KB_SMALL="2")
SMALL3 = dict(SMG_WGS_KB2_MAX_PIECES="1000000000", SMG_WGS_KB_SMALL="3")
WGS_CHILDREN = (("big", BIG), ("small2", SMALL2), ("small3", SMALL3))
# the (KB, groups) of the launches of one piece colour, in column order
LAUNCHES = {
    "default": {k: [(1, k)] for k in KS},
    "big": {1: [(1, 1)], 2: [(2, 1)], 3: [(3, 1)], 4: [(4, 1)], 5: [(4, 1), (1, 1)], 6: [(4, 1), (2, 1)], 7: [(4, 1), (3, 1)], 8: [(4, 2)],
            11: [(4, 2), (3, 1)], 18: [(4, 4), (2, 1)]},
    "small2": {1: [(1, 1)], 2: [(2, 1)], 3: [(2, 1), (1, 1)], 4: [(2, 2)], 5: [(2, 2), (1, 1)], 6: [(2, 3)], 7: [(2, 3), (1, 1)], 8: [(2, 4)],
               11: [(2, 5), (1, 1)], 18: [(2, 9)]},
    "small3": {1: [(1, 1)], 2: [(2, 1)], 3: [(3, 1)], 4: [(3, 1), (1, 1)], 5: [(3, 1), (2, 1)], 6: [(3, 2)], 7: [(3, 2), (1, 1)], 8: [(3, 2), (2, 1)],
               11: [(3, 3), (2, 1)], 18: [(3, 6)]},
}
# case -> level -> (rows, n_pieces, nb_max, rim_pitch, NBMAX, RIMI): the table of the docstring
TABLE = {
    "torus": {0: (4096, 103, 1, 256, 3, 4), 1: (1024, 33, 1, 128, 3, 2)},
    "bunny-dec": {1: (2353, 62, 4, 256, 5, 4), 2: (597, 18, 6, 128, 8, 2)},
    "bunny15k-pin": {1: (3952, 87, 4, 256, 5, 4), 2: (989, 29, 6, 256, 8, 4)},
    "random-1500": {0: (1500, 174, 3, 448, 3, 7)},
    "random-700-a": {0: (700, 42, 4, 448, 5, 7)},
    "random-700-b": {0: (700, 53, 6, 448, 8, 7)},
    "band-600": {0: (600, 31, 5, 128, 5, 2)},
}
# the deep variant's launches for a group of k <= 4 columns, by row-width class: (columns, class)
DEEP_LAUNCHES = {
    3: {1: [(1, 3)], 2: [(2, 3)], 3: [(3, 3)], 4: [(3, 3), (1, 3)]},
    5: {1: [(1, 5)], 2: [(2, 5)], 3: [(2, 5), (1, 5)], 4: [(2, 5), (2, 5)]},
    8: {k: [(1, 8)] * k for k in (1, 2, 3, 4)},
    0: {k: [(k, 0)] for k in (1, 2, 3, 4)},
}


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def bits(x):
    return struct.pack("<d", float(x)).hex()


# ----------------------------------------------------------------------------------------------- the hierarchies
def _mcf(V, F):
    A = (M.massmatrix(V, F, "barycentric") - 0.01 * M.cotmatrix(V, F)).tocsr()
    A.sort_indices()
    return A


def random_wide(seed, n, lo, hi):
    """random_spd_hierarchy's matrix with lo .. hi - 1 random links per row instead of 2 .. 8 (strictly diagonally dominant, symmetric) and one
    aggregation level of n // 3 rows: wide rows AND a rim of several hundred rows per piece"""
    rng = np.random.default_rng(seed)
    rows = np.repeat(np.arange(n), rng.integers(lo, hi, n))
    cols = rng.integers(0, n, rows.size)
    W = sp.coo_matrix((-rng.uniform(0.1, 1.0, rows.size), (rows, cols)), shape=(n, n)).tocsr()
    W.setdiag(0); W.eliminate_zeros()
    W = W + W.T
    A = (W + sp.diags(np.asarray(-W.sum(axis=1)).ravel() + rng.uniform(0.05, 0.5, n))).tocsr()
    A.sort_indices()
    mc = n // 3
    agg = rng.integers(0, mc, n); agg[:mc] = np.arange(mc)
    return A, [sp.coo_matrix((np.ones(n), (np.arange(n), agg)), shape=(n, mc)).tocsr()]


def band_matrix(n, hb):
    """a symmetric, strictly diagonally dominant band of half-bandwidth hb with random values and one aggregation level of n // 3 rows: wide rows AND
    small rims (a breadth-first level set has hb rows)"""
    rng = np.random.default_rng(5)
    W = sp.diags([-rng.uniform(0.1, 1.0, n - d) for d in range(1, hb + 1)], list(range(1, hb + 1)), shape=(n, n)).tocsr()
    W = W + W.T
    A = (W + sp.diags(np.asarray(-W.sum(axis=1)).ravel() + rng.uniform(0.05, 0.5, n))).tocsr()
    A.sort_indices()
    mc = n // 3
    return A, [sp.coo_matrix((np.ones(n), (np.arange(n), np.minimum(np.arange(n) // 3, mc - 1))), shape=(n, mc)).tocsr()]


def wave_case(smg, name):
    """(handle with its system precomputed, the levels that sweep piece-wise) of a case of TABLE"""
    base = name.replace("-stepped", "")
    if base == "torus":
        mg, Vf, Ff = smg.mg_precompute_subdiv(*M.torus(8, 8), 3, n_extra_levels=0)
        mg.set_wave_gs("all")
        A, known = _mcf(M.normalize_unit_area(Vf, Ff), Ff), None
    elif base == "bunny-dec":
        mg, A, RHS, known = decimated(smg, "bunny.smgm", 1, "mcf", nVCoarsest=60)
    elif base == "bunny15k-pin":
        mg, A, RHS, known = decimated(smg, "bunny_15K_init.smgm", 1, "poisson", n_pins=40)
    else:
        A, Ps = dict([("random-1500", lambda: random_spd_hierarchy(np.random.default_rng(1), 1500, 2, False)), ("random-700-a", lambda: random_wide(3, 700, 8, 14)),
                      ("random-700-b", lambda: random_wide(3, 700, 12, 20)), ("band-600", lambda: band_matrix(600, 20))])[base]()
        mg, known = smg.Hierarchy.from_prolongs(Ps), None
        mg.set_wave_gs("all")
    mg.precompute(A, known)
    if name.endswith("-stepped"):
        mg.precompute(value_step(A, 1), known)
    levels = sorted(TABLE[base])
    assert [mg.rows(lv) for lv in levels] == [TABLE[base][lv][0] for lv in levels], [mg.rows(lv) for lv in range(mg.n_levels)]
    return mg, levels


def launch_line(mg, name, lv, k, label):
    """the launches of one piece colour of the plan relax() has just swept level lv with, as the hooks state them; asserted against TABLE and LAUNCHES"""
    rows, n_pieces, nb_max, rim_pitch, nbmax, rimi = TABLE[name.replace("-stepped", "")][lv]
    plan = H.wgs_level_plan(mg, lv, k)
    assert plan is not None, "%s, level %d (%d rows), k = %d: relax() does not sweep piece-wise" % (name, lv, mg.rows(lv), k)
    assert plan == (n_pieces, nb_max, rim_pitch), "%s, level %d: the plan has (pieces, nb_max, rim pitch) = %s, the table says %s" % (name, lv, plan, (n_pieces, nb_max, rim_pitch))
    got_nbmax, got_rimi, la = H.wgs_launches(mg.L, *plan, k)
    assert (got_nbmax, got_rimi) == (nbmax, rimi), (name, lv, got_nbmax, got_rimi)
    assert la == LAUNCHES[label][k], "%s run, k = %d on %d pieces: launches %s, expected %s -- the gate is not where the knobs put it" % (label, k, n_pieces, la, LAUNCHES[label][k])
    return "wgs %s lv%d k%d NBMAX%d RIMI%d %s" % (name, lv, k, got_nbmax, got_rimi, "+".join("%dx%d" % (g, kb) for kb, g in la))


# ----------------------------------------------------------------------------------------------- what a run (this process or a child) does
def wave_lines(smg, oracle_mod, name, label):
    """relax(1) and relax(2) for every k of KS on every level of the case against the oracle in the piece order; "wgs" lines: the launches, "vec" lines: the hashes"""
    mg, levels = wave_case(smg, name)
    lines = []
    for lv in levels:
        n, rows, oi, to = mg.rows(lv), None, None, None
        for k in KS:
            b, x = _vectors(n, k, lv)
            got = {s: mg.relax(lv, b, x, s) for s in (1, 2)}
            lines.append(launch_line(mg, name, lv, k, label))
            info = mg.wave_gs_order(lv, k)
            assert info is not None
            if rows is None:           # (mg.matrix() brings the host copies up to date: after the first sweeps of the level, whose plan was built without)
                rows = info["rows"]
                oi, to = order_oracle(oracle_mod, mg, lv, rows), mg.perm(lv)[rows]
            assert np.array_equal(rows, info["rows"]), "the order of level %d depends on k" % lv
            for s in (1, 2):
                ref = oi.relax(0, b[to], x[to], s)
                bad = got[s][to] != ref
                assert not bad.any(), "%s run, %s level %d (%d rows), k = %d, %d sweep(s): %d entries in %d rows differ from the oracle, columns %s" % (
                    label, name, lv, n, k, s, bad.sum(), bad.any(axis=1).sum(), sorted(set(np.nonzero(bad)[1].tolist())))
                lines.append("vec %s lv%d k%d gs%d %s" % (name, lv, k, s, sha(got[s])))
    return lines


def solve_lines(smg, oracle_mod, name, label):
    """bunny-dec, k = 3 and 8: 6 cycles with a tolerance never reached, then with one the fourth residual meets"""
    assert name == "bunny-dec"
    lines = []
    for k in (3, 8):
        mg, A, RHS, known = decimated(smg, "bunny.smgm", k, "mcf", nVCoarsest=60)
        mg.precompute(A, known)
        z0 = np.zeros((A.shape[0], k), order="F")
        conv, z, rh = mg.solve(RHS, z0, None, smg.SolveOpts(tol=0.0, max_iter=6))
        rh = np.asarray(rh)
        assert not conv and len(rh) == 6 and np.isfinite(rh).all() and (np.diff(rh) < 0).all(), rh
        for lv in sorted(TABLE[name]):
            lines.append(launch_line(mg, name, lv, k, label))
        lines.append("vec %s k%d solve6-z %s" % (name, k, sha(z)))
        lines.append("vec %s k%d solve6-his %s" % (name, k, sha(rh)))
        tol = float(np.sqrt(rh[2] * rh[3]))                      # rh[3] < tol < rh[2]: met by the fourth residual, inside the first graph of four iterations
        assert rh[3] < tol < rh[2]
        conv, z_early, rh_early = mg.solve(RHS, z0, None, smg.SolveOpts(tol=tol, max_iter=6))
        assert conv and np.array_equal(np.asarray(rh_early), rh[:4]), (rh_early, rh)
        conv3, z3, rh3 = mg.solve(RHS, z0, None, smg.SolveOpts(tol=0.0, max_iter=3))
        assert not conv3 and np.array_equal(np.asarray(rh3), rh[:3])
        assert np.array_equal(z_early, z3), "%s run, k = %d: a launch behind the done flag wrote %d entries of the iterate" % (label, k, (z_early != z3).sum())
        lines.append("vec %s k%d early-z %s" % (name, k, sha(z_early)))
    return lines


_HIP = []


def _raw_resid(mg, lv, x_int, b_int):
    """b - A x of level lv through smg_raw_spmv: blocks in the device numbering, row-major, in one device buffer x | b | y of this module's own"""
    import ctypes as C
    if not _HIP:
        hip = C.CDLL("libamdhip64.so")
        hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        hip.hipFree.argtypes = [C.c_void_p]
        _HIP.append(hip)
    hip = _HIP[0]
    n, k = x_int.shape
    host = np.ascontiguousarray(np.stack([x_int, b_int, H.sentinel((n, k))]))
    size, d = n * k * 8, C.c_void_p()
    assert hip.hipMalloc(C.byref(d), 3 * size) == 0
    try:
        assert hip.hipMemcpy(d, host.ctypes.data, 3 * size, 1) == 0                      # host -> device, complete on return
        mg.raw_spmv(lv, 1, d.value, d.value + size, d.value + 2 * size, k)
        mg.synchronize()
        assert hip.hipMemcpy(host.ctypes.data, d, 3 * size, 2) == 0                      # device -> host
    finally:
        hip.hipFree(d)
    assert np.array_equal(host[0], x_int) and np.array_equal(host[1], b_int), "smg_raw_spmv wrote one of its inputs"
    return host[2]


def sell_pieces(oracle_mod, mg, name, label, ks, deep_expected):
    """A x, b - A x and the restriction of every smoothed level against the oracle in the device numbering; deep_expected(w_max) -> the class whose
    launches smg_debug_deep_launches must report (0: k_sell).  Returns (lines, the classes met on the A images)."""
    lines, classes = [], set()
    for lv in range(mg.n_levels - 1):
        n = mg.rows(lv)
        perm, permc = mg.perm(lv), mg.perm(lv + 1)
        oi = oracle_on_device_numbering(oracle_mod, mg, lv)
        for k in ks:
            b, x = _vectors(n, k, lv)
            tag = "%s lv%d k%d" % (name, lv, k)
            where = "%s run, %s level %d (%d rows), k = %d" % (label, name, lv, n, k)
            for which, at, modes in (("A", lv, ("A", "RESID")), ("PT", lv + 1, ("A",))):
                for mode in modes:
                    w_max, la = H.deep_launches(mg, at, which, mode, k)
                    cls = deep_expected(w_max)
                    assert la == DEEP_LAUNCHES[cls][k], "%s: %s on %s (widest slice %d): launches %s, expected %s" % (where, mode, which, w_max, la, DEEP_LAUNCHES[cls][k])
                    lines.append("deep %s %s-%s w%d %s" % (tag, which, mode, w_max, "+".join("%d@%d" % t for t in la)))
                    if which == "A":
                        classes.add(cls)
            ref_A = oi.A(0, x[perm])
            for what, got, ref, numbering in (("A", mg.A(lv, x), ref_A, perm), ("restrict", mg.restrict(lv, x), oi.restrict(0, x[perm]), permc),
                                              ("resid", _raw_resid(mg, lv, x[perm], b[perm]), b[perm] - ref_A, slice(None))):
                bad = got[numbering] != ref
                assert not bad.any(), "%s: %s differs from the oracle in %d entries of %d rows, columns %s" % (where, what, bad.sum(), bad.any(axis=1).sum(), sorted(set(np.nonzero(bad)[1].tolist())))
                lines.append("vec %s %s %s" % (tag, what, sha(got)))
            lines.append("vec %s residual_norm %s" % (tag, bits(mg.residual_norm(lv, b, x))))
    for k in ks:
        B, u = _vectors(mg.rows(0), k, 40)
        lines.append("vec %s k%d vcycle %s" % (name, k, sha(mg.vcycle(B, u))))
    return lines, classes


def _deep_class(w_max):
    return 0 if w_max < 13 or w_max > 64 else 3 if w_max <= 24 else 5 if w_max <= 40 else 8


def deep_lines(smg, oracle_mod, name, label):
    """label default: k_sell_deep wherever 13 <= widest slice <= 64; deep0 (SMG_DEEP=0): k_sell everywhere"""
    lines, classes = [], set()
    for case in ("bunny-dec", "random-1500"):
        mg, levels = wave_case(smg, case)
        li, cl = sell_pieces(oracle_mod, mg, case, label, (1, 2, 3, 4), _deep_class if label == "default" else (lambda w: 0))
        lines += li
        classes |= cl
    if label == "default":
        assert {3, 5, 8} <= classes, "the A images reach the deep kernel's classes %s only" % sorted(classes)
    else:
        assert classes == {0}
    return lines


def deepw1_lines(smg, oracle_mod, name, label):
    """label default: rows of 7 to 12 entries go through k_sell; deepw1 (SMG_DEEP_MIN_W=1): through k_sell_deep<.., 3> with one or two live batches"""
    p = subdiv_problem("ogre_sim.smgm", n_sub=1, kind="poisson")
    mg = smg.Hierarchy.from_prolongs(p["Ps"])
    mg.precompute(p["A"], p["known"])
    widths = np.diff(mg.matrix(0, "A", internal=True).tocsr().indptr)
    assert widths.min() <= 8 < widths.max() <= 12, (widths.min(), widths.max())       # slices of one live batch and of two
    lines, classes = sell_pieces(oracle_mod, mg, "ogre_sim-1", label, (1, 2, 3, 4), (lambda w: 0) if label == "default" else (lambda w: 3 if 1 <= w <= 24 else 0))
    assert classes == ({0} if label == "default" else {3}), classes
    return [ln for ln in lines if not ln.startswith("deep ")]         # (the launches differ between the two runs by design)


def wpb_lines(smg, oracle_mod, name, label):
    """Gauss-Seidel colour launches at k = 1 on the subdivision hierarchy; the children: SMG_GS_WPB = 2 / 8 with the shortcuts that would pre-empt the
    branch off.  "wpb" lines: the waves per workgroup of every colour's launch as smg_debug_gs_colour_wpb states them, asserted: 2 / 8 for every colour
    of every level in the children; 4 here (where levels this small take the one-launch relax in their place)."""
    p = subdiv_problem(kind="mcf", k=1, n_sub=2)
    mg = smg.Hierarchy.from_prolongs(p["Ps"])
    mg.precompute(p["A"], p["known"])
    expect = dict(default=4, wpb2=2, wpb8=8)[label]
    lines, odd, ragged = [], 0, 0
    for lv in range(mg.n_levels - 1):
        cp = mg.colors(lv)
        ns = [-(-int(cp[c + 1] - cp[c]) // 64) for c in range(len(cp) - 1)]
        odd += sum(s % 2 == 1 for s in ns)
        ragged += sum(s % 8 != 0 for s in ns)
        for c, s in enumerate(ns):
            wpb, stride, w_lo = H.gs_colour_wpb(mg, lv, s)
            assert stride > 0 and w_lo == 7, "level %d is no fixed-pitch image of lower width 7: pitch %d, lower width %d" % (lv, stride, w_lo)
            assert wpb == expect, "%s run, level %d, colour %d of %d slices: %d waves per workgroup, expected %d" % (label, lv, c, s, wpb, expect)
            lines.append("wpb subdiv-mcf lv%d colour%d slices%d pitch%d w_lo%d WPB%d" % (lv, c, s, stride, w_lo, wpb))
        b, x = _vectors(mg.rows(lv), 1, lv)
        for iters in (1, 3):
            assert gs_bit_exact(oracle_mod, mg, lv, b, x, iters), "%s run, level %d (%d rows, colours of %s slices): %d sweep(s) not the oracle's" % (label, lv, mg.rows(lv), ns, iters)
            lines.append("vec subdiv-mcf lv%d gs%d %s" % (lv, iters, sha(mg.relax(lv, b, x, iters))))
    assert odd >= 1 and ragged >= 1, "no colour whose slices are no multiple of 2 and of 8"
    return lines


TASKS = dict(wave=wave_lines, solve=solve_lines, deep=deep_lines, deepw1=deepw1_lines, wpb=wpb_lines)

_CHILD = r"""
import os, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import surface_multigrid_code_amd as smg
from oracle import oracle as oracle_mod
oracle_mod.build()
import test_gpu_wgs_variants as T
lines = T.TASKS[sys.argv[2]](smg, oracle_mod, sys.argv[3], sys.argv[4])
print("\n".join(lines))
print("CHILD_OK", len(lines))
"""
_PREFIXES = ("wgs ", "vec ", "deep ", "wpb ")


# ----------------------------------------------------------------------------------------------- the children
class _Child:
    def __init__(self, task, name, label, env):
        self.label, self.env = label, env
        self.out, self.err = tempfile.TemporaryFile("w+"), tempfile.TemporaryFile("w+")       # (files: a child cannot block on a full pipe)
        self.p = subprocess.Popen([sys.executable, "-c", _CHILD, ROOT, task, name, label], env=dict(os.environ, **env), stdout=self.out, stderr=self.err, text=True)
        self.deadline = time.monotonic() + CHILD_TIMEOUT

    def stop(self):
        if self.p.poll() is None:
            self.p.kill()
            self.p.wait()
        self.out.close(); self.err.close()


POLL = 0.05                  # seconds a wait on one live child may take before the next one is looked at


def run_with_children(mods, task, name, children, own_label="default"):
    """this process's run of the task (mods: the package and the oracle module) and one per child environment, at most MAX_ALIVE children alive at
    once, each with its own time limit; returns (this run's lines, {label: (lines, stderr)}).  All live children are watched in turn: the first one
    that fails, aborts or runs out of its time fails the test at once, and the rest are stopped."""
    pending, alive, done = list(children), [], {}

    def start_more():
        while pending and len(alive) < MAX_ALIVE:
            label, env = pending.pop(0)
            alive.append(_Child(task, name, label, env))

    def collect(ch):
        timed_out = ch.p.poll() is None
        if timed_out:
            ch.p.kill()
            ch.p.wait()
        ch.out.seek(0); ch.err.seek(0)
        stdout, stderr = ch.out.read(), ch.err.read()
        assert not timed_out and ch.p.returncode == 0 and "CHILD_OK" in stdout, "child %s (%s): %s, exit status %s\n%s\n%s" % (
            ch.label, " ".join("%s=%s" % kv for kv in ch.env.items()), "ran out of its %d s" % CHILD_TIMEOUT if timed_out else "failed", ch.p.returncode, stdout[-3000:], stderr[-4000:])
        lines = [ln for ln in stdout.splitlines() if ln.startswith(_PREFIXES)]
        assert "CHILD_OK %d" % len(lines) in stdout, stdout[-3000:]
        done[ch.label] = (lines, stderr)

    def reap(block):
        """every live child that has ended or is past its limit; block: wait (POLL per child and turn) until at least one has"""
        while alive:
            ready = []
            for ch in alive:
                if block and not ready:
                    try:
                        ch.p.wait(timeout=POLL)
                    except subprocess.TimeoutExpired:
                        pass
                if ch.p.poll() is not None or time.monotonic() > ch.deadline:
                    ready.append(ch)
            for ch in ready:
                collect(ch)              # (raises for a child that failed: the finally below stops the others)
                alive.remove(ch)
                ch.stop()
            if ready or not block:
                return

    try:
        start_more()
        mine = TASKS[task](*mods, name, own_label)
        while alive:
            reap(True)
            start_more()
    finally:
        for ch in alive:
            ch.stop()
    return mine, done


@pytest.fixture
def mods(smg, oracle_mod):
    return smg, oracle_mod


def vecs(lines):
    return [ln for ln in lines if ln.startswith("vec ")]


def same_bits(mine, done):
    assert vecs(mine)
    for label, (lines, _) in done.items():
        diff = [(a, b) for a, b in zip(vecs(mine), vecs(lines)) if a != b]
        assert len(vecs(lines)) == len(vecs(mine)) and not diff, "the %s run gives other bits than this process in %d of %d vectors, first: %s" % (label, len(diff), len(vecs(mine)), diff[:3])


def kernels(lines):
    """{(level, NBMAX, RIMI, KB)} of the "wgs" lines"""
    out = set()
    for ln in lines:
        if ln.startswith("wgs "):
            w = ln.split()
            out |= {(w[2], int(w[4][5:]), int(w[5][4:]), int(t.split("x")[1])) for t in w[6].split("+")}
    return out


# ----------------------------------------------------------------------------------------------- the tests
def test_the_levels_reach_every_row_width_class_and_every_rim_pitch():
    """TABLE (asserted against the plans in every run below) has a level for each of the nine pairs of NBMAX = 3, 5, 8 and RIMI = 2, 4, 7; every level runs KB = 1 .. 4"""
    rows = [t for levels in TABLE.values() for t in levels.values()]
    assert {t[4] for t in rows} == {3, 5, 8} and {t[5] for t in rows} == {2, 4, 7}
    assert {t[4:] for t in rows} == {(nbmax, rimi) for nbmax in (3, 5, 8) for rimi in (2, 4, 7)}            # all nine pairs
    for rows_, n_pieces, nb_max, rim_pitch, nbmax, rimi in rows:
        assert rows_ >= 512 and n_pieces <= 1600 and nbmax == (3 if nb_max <= 3 else 5 if nb_max <= 5 else 8) and rim_pitch == 64 * rimi
    assert {kb for la in LAUNCHES["big"].values() for kb, g in la} == {1, 2, 3, 4} and {kb for la in LAUNCHES["default"].values() for kb, g in la} == {1}
    for label, per_k in LAUNCHES.items():
        assert sorted(per_k) == list(KS) and all(sum(kb * g for kb, g in la) == k for k, la in per_k.items()), label


@pytest.mark.parametrize("name", ["torus", "bunny-dec", "bunny-dec-stepped", "bunny15k-pin", "random-1500", "random-700-a", "random-700-b", "band-600"])
def test_every_column_variant_of_the_wave_kernel_is_the_oracles_sweep(mods, name):
    mine, done = run_with_children(mods, "wave", name, WGS_CHILDREN)
    same_bits(mine, done)
    seen = kernels(mine) | {t for lines, _ in done.values() for t in kernels(lines)}
    for lv, (rows, n_pieces, nb_max, rim_pitch, nbmax, rimi) in TABLE[name.replace("-stepped", "")].items():
        assert {("lv%d" % lv, nbmax, rimi, kb) for kb in (1, 2, 3, 4)} <= seen, (lv, sorted(seen))
    assert kernels(mine) == {(lv, nbmax, rimi, 1) for lv, nbmax, rimi, kb in seen}            # (this process: KB = 1 on every level)
    for label, lines in [("default", mine)] + [(label, lines) for label, (lines, _) in done.items()]:
        print("\n".join("%-7s %s" % (label, ln) for ln in lines if ln.startswith("wgs ")))


def test_solves_do_not_depend_on_the_columns_per_lane_and_stop_writing_when_done(mods):
    mine, done = run_with_children(mods, "solve", "bunny-dec", WGS_CHILDREN)
    same_bits(mine, done)
    assert {kb for lv, nbmax, rimi, kb in kernels(done["big"][0])} == {3, 4} and {kb for lv, nbmax, rimi, kb in kernels(mine)} == {1}


def test_deep_and_plain_sell_kernels_give_the_oracles_bits_on_wide_rows(mods):
    mine, done = run_with_children(mods, "deep", "dec+random", (("deep0", dict(SMG_DEEP="0")),))
    same_bits(mine, done)
    print("\n".join(ln for ln in mine if ln.startswith("deep ")))


def test_deep_kernel_on_rows_of_one_and_two_batches(mods):
    mine, done = run_with_children(mods, "deepw1", "ogre_sim-1", (("deepw1", dict(SMG_DEEP_MIN_W="1")),))
    same_bits(mine, done)


def test_colour_launches_with_two_and_eight_waves_per_workgroup(mods):
    off = dict(SMG_ONE_XCD_MAX="0", SMG_PITCH_SPEC_MAX="0", SMG_TILED="0")
    mine, done = run_with_children(mods, "wpb", "subdiv-mcf", (("wpb2", dict(off, SMG_GS_WPB="2")), ("wpb8", dict(off, SMG_GS_WPB="8"))))
    same_bits(mine, done)
    for label, lines in [("default", mine)] + [(label, lines) for label, (lines, _) in done.items()]:
        print("\n".join("%-7s %s" % (label, ln) for ln in lines if ln.startswith("wpb ")))
    assert all({ln.split()[-1] for ln in done[label][0] if ln.startswith("wpb ")} == {want} for label, want in (("wpb2", "WPB2"), ("wpb8", "WPB8")))
