"""GPU (-m gpu): both variants of the multi-column SELL kernel at test size.

launch_wide_one (csrc/smg_device.hip) serves a block of KW in {8, 16, 32} columns with k_sell_wide<MODE, KW, T, 1, U> (one row per lane, the whole
row in flight) while n_slices * KW <= SMG_WIDE_LAT_MAX (16384) and with the streaming k_sell_wide<MODE, KW, T> (R = 2, U = 8: two rows per lane,
the batch's entries fetched by coalesced loads and redistributed by shuffles) above.  At the suite's sizes a colour sweep never crosses the gate,
a whole-matrix launch crosses it only at KW = 32 on the 40 877-row level.  So every case here runs three times: in this process with the default
gate, in a child with SMG_WIDE_LAT_MAX=0 (every wide launch streams, R = 2) and in a child with SMG_WIDE_LAT_MAX=1000000000 (every wide launch
one row per lane) -- the knob is read once per process.  Every run states through smg_debug_wide_latency_variant which side of the gate each of
its launches sits on (the slices of the whole matrix, sell_stats, and of every colour, colors) and holds

  fp64   A x, 1 and 3 Gauss-Seidel sweeps, 3 damped-Jacobi sweeps (0.7), 2 Chebyshev sweeps, restrict, prolong on every smoothed level: BIT FOR BIT
         the oracle on the level's matrices in the device numbering; residual_norm to 1e-13 relative (a sum over per-workgroup partials, whose
         number differs between the variants);
  fp32   check_sparse_pieces of test_gpu_f32_cycle.py, unchanged: the restatement's bits, and the product-sum bound that tells "wrong" from
         "another order";
  loops  a full-depth V-cycle and a solve of exactly 6 cycles (tol = 0), fp64 and mixed.

Across the three runs every vector has the same SHA-256, the norms and the histories agree to 1e-13 relative."""
import hashlib
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import kernel_hooks as H
import test_gpu_f32_cycle as F32C
from problems import subdiv_problem
from test_gpu_parity import gs_bit_exact, oracle_on_device_numbering, smg  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GATES = (("streaming", "0"), ("latency", "1000000000"))          # the children's SMG_WIDE_LAT_MAX: R = 2 everywhere / one row per lane everywhere
ALL_KS = (8, 12, 16, 24, 40, 56, 63)                             # 8 | 8 + 4 | 16 | 16 + 8 | 32 + 8 | 32 + 16 + 8 | 32 + 16 + 8 + 4 + 3
SOME_KS = (8, 24, 40)
CHILD_TIMEOUT = 300


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def wide_blocks(k):
    """the blocks of 64 / 32 / 16 / 8 columns launch_sell_mode cuts k columns into (the rest goes through the narrow kernels)"""
    out, c0 = [], 0
    while k - c0 >= 8:
        kw = 64
        while kw > k - c0:
            kw >>= 1
        out.append(kw)
        c0 += kw
    return out


def launches(mg, ks):
    """(what, level, n_slices, kw) of every gated launch the pieces below make for these column counts: whole-matrix launches on A, P and PT, and
    one colour of A at a time"""
    out = []
    for lv in range(mg.n_levels - 1):
        whole = mg.sell_stats(lv, "A")["n_slices"]
        cp = mg.colors(lv)
        colours = [-(-int(cp[c + 1] - cp[c]) // 64) for c in range(len(cp) - 1)]           # a colour's rows in slices of 64 (sell_layout)
        assert sum(colours) == whole, "level %d: the colours' slices do not add up to the matrix's" % lv
        sizes = [("A", whole), ("P", mg.sell_stats(lv + 1, "P")["n_slices"]), ("PT", mg.sell_stats(lv + 1, "PT")["n_slices"])]
        sizes += [("colour%d" % c, ns) for c, ns in enumerate(colours)]
        for kw in sorted({kw for k in ks for kw in wide_blocks(k) if kw < 64}):
            out += [(what, lv, ns, kw) for what, ns in sizes]
    return out


def gate_lines(mg, ks, expect=None):
    """one line per gated launch with the side smg_debug_wide_latency_variant reports; expect (0 / 1): asserted for the smallest and the largest
    launch first, then for all"""
    L = mg.L
    la = launches(mg, ks)
    assert la, "no wide launch at all"
    if expect is not None:
        for what, lv, ns, kw in (min(la, key=lambda t: t[2] * t[3]), max(la, key=lambda t: t[2] * t[3])):
            assert L.smg_debug_wide_latency_variant(ns, kw) == expect, "the gate is not where SMG_WIDE_LAT_MAX=%s puts it: %s of level %d, %d slices x %d columns" % (
                os.environ.get("SMG_WIDE_LAT_MAX"), what, lv, ns, kw)
    lines = []
    for what, lv, ns, kw in la:
        side = L.smg_debug_wide_latency_variant(ns, kw)
        assert side in (0, 1) and (expect is None or side == expect), (what, lv, ns, kw, side)
        lines.append("gate lv%d %s kw%d slices%d side%d" % (lv, what, kw, ns, side))
    return lines


def fp64_pieces(oracle_mod, mg, name, k):
    """every piece on every smoothed level against the oracle in the device numbering; returns the lines "vec <tag> <sha>" / "norm <tag> <value>" """
    lines = []
    rng = np.random.default_rng(100 + k)
    for lv in range(mg.n_levels - 1):
        n, nc = mg.rows(lv), mg.rows(lv + 1)
        perm, permc = mg.perm(lv), mg.perm(lv + 1)
        oi = oracle_on_device_numbering(oracle_mod, mg, lv)
        x, b, xc = rng.uniform(-1, 1, (n, k)), rng.uniform(-1, 1, (n, k)), rng.uniform(-1, 1, (nc, k))
        tag = "%s k%d lv%d" % (name, k, lv)
        where = "%s, level %d of %d (%d rows), k = %d, SMG_WIDE_LAT_MAX=%s" % (name, lv, mg.n_levels, n, k, os.environ.get("SMG_WIDE_LAT_MAX", "default"))

        def keep(what, got, ref, numbering):
            bad = got[numbering] != ref
            assert not bad.any(), "%s is not the oracle's bit for bit on %s: %d entries in %d rows and columns %s, largest difference %.3g" % (
                what, where, bad.sum(), bad.any(axis=1).sum(), sorted(set(np.nonzero(bad)[1].tolist()))[:16], np.abs(got[numbering] - ref).max())
            lines.append("vec %s %s %s" % (tag, what, sha(got)))

        keep("A", mg.A(lv, x), oi.A(0, x[perm]), perm)
        mg.set_smoother("gs"); oi.set_smoother(0, "gs", 1.0)
        for iters in (1, 3):
            assert gs_bit_exact(oracle_mod, mg, lv, b, x, iters), "%d Gauss-Seidel sweep(s) not the oracle's bit for bit on %s" % (iters, where)
            lines.append("vec %s gs%d %s" % (tag, iters, sha(mg.relax(lv, b, x, iters))))
        mg.set_smoother("jacobi", 0.7); oi.set_smoother(0, "jacobi", 0.7)
        keep("jacobi3", mg.relax(lv, b, x, 3), oi.relax(0, b[perm], x[perm], 3), perm)
        mg.set_smoother("chebyshev"); oi.set_smoother(0, "chebyshev", 0.1)
        keep("chebyshev2", mg.relax(lv, b, x, 2), oi.relax(0, b[perm], x[perm], 2), perm)
        mg.set_smoother("gs"); oi.set_smoother(0, "gs", 1.0)
        keep("restrict", mg.restrict(lv, x), oi.restrict(0, x[perm]), permc)
        keep("prolong", mg.prolong(lv, xc), oi.prolong(0, xc[permc]), perm)
        rn, ref = mg.residual_norm(lv, b, x), np.linalg.norm(b[perm] - oi.A(0, x[perm]))
        print("residual_norm on %s: %.17g, oracle %.17g, relative difference %.2e" % (where, rn, ref, abs(rn - ref) / ref))
        assert abs(rn - ref) <= 1e-13 * ref, "residual_norm on %s: %.17g, oracle %.17g" % (where, rn, ref)
        lines.append("norm %s residual_norm %.17g" % (tag, rn))
    return lines


def fp32_pieces(c, name, k):
    """check_sparse_pieces as it stands, then the hashes of two of its vectors per level (the product and a Gauss-Seidel sweep)"""
    F32C.check_sparse_pieces(c, k, F32C.ALL3)
    mg, lines = c.mg, []
    rng = np.random.default_rng(200 + k)
    for lv in range(mg.n_levels - 1):
        x, b = F32C.rnd(rng, (mg.rows(lv), k)), F32C.rnd(rng, (mg.rows(lv), k))
        lines.append("vec %s k%d lv%d f32-A %s" % (name, k, lv, sha(H.cycle_f32(mg, "A", lv, x))))
        lines.append("vec %s k%d lv%d f32-gs2 %s" % (name, k, lv, sha(H.cycle_f32(mg, "RELAX", lv, b, out=x, pre=2))))
    return lines


def pieces(smg_mod, oracle_mod, name, ks, expect=None):
    c = F32C.case(smg_mod, name)
    lines = gate_lines(c.mg, ks, expect)
    for k in ks:
        lines += fp64_pieces(oracle_mod, c.mg, name, k)
        c = F32C.case(smg_mod, name)                                # (the smoother back to what check_sparse_pieces starts from)
        lines += fp32_pieces(c, name, k)
    c.mg.set_smoother("gs", F32C.OMEGA, -1, F32C.FRAC)
    return lines


def loops(smg_mod, name, k, expect=None):
    """a full-depth V-cycle and a solve of exactly 6 cycles, fp64 and mixed: "vec" lines of the iterates, "his" lines of the histories"""
    assert name == "subdiv-mcf"
    c = F32C.case(smg_mod, name)
    mg = c.mg
    p = subdiv_problem(kind="mcf", k=k, n_sub=2)
    assert p["A"].shape[0] == mg.rows(0) and mg.n_levels == len(p["Ps"]) + 1
    lines = gate_lines(mg, (k,), expect)
    rng = np.random.default_rng(300 + k)
    B, u = rng.uniform(-1, 1, (mg.rows(0), k)), rng.uniform(-1, 1, (mg.rows(0), k))
    lines.append("vec %s k%d vcycle-f64 %s" % (name, k, sha(mg.vcycle(B, u))))
    lines.append("vec %s k%d vcycle-f32 %s" % (name, k, sha(H.cycle_f32(mg, "VCYCLE", 0, B.astype(np.float32), out=u.astype(np.float32), pre=2, post=2))))
    for prec in ("f64", "mixed"):
        conv, z, rh = mg.solve(p["RHS"], p["z0"], None, smg_mod.SolveOpts(tol=0.0, max_iter=6, precision=prec))
        assert len(rh) == 6 and np.isfinite(rh).all() and rh[-1] < rh[0], (prec, rh)
        lines.append("vec %s k%d solve-%s %s" % (name, k, prec, sha(z)))
        lines.append("his %s k%d solve-%s %s" % (name, k, prec, " ".join("%.17g" % r for r in rh)))
    return lines


_CHILD = r"""
import os, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import surface_multigrid_code_amd as smg
from oracle import oracle as oracle_mod
oracle_mod.build()
import test_gpu_wide_variants as T
what, name, ks, expect = sys.argv[2], sys.argv[3], tuple(int(k) for k in sys.argv[4].split(",")), int(sys.argv[5])
lines = T.pieces(smg, oracle_mod, name, ks, expect) if what == "pieces" else T.loops(smg, name, ks[0], expect)
print("\n".join(lines))
print("CHILD_OK", len(lines))
"""


def start_children(what, name, ks):
    """the same run in two fresh processes, one per gate (SMG_WIDE_LAT_MAX is read once per process); they work while this process does its own run
    and write into temporary files, so that none can block on a full pipe"""
    procs = []
    for _, gate in GATES:
        out, err = tempfile.TemporaryFile("w+"), tempfile.TemporaryFile("w+")
        p = subprocess.Popen([sys.executable, "-c", _CHILD, ROOT, what, name, ",".join(str(k) for k in ks), "0" if gate == "0" else "1"],
                             env=dict(os.environ, SMG_WIDE_LAT_MAX=gate), stdout=out, stderr=err, text=True)
        procs.append((p, out, err))
    return procs


def stop_children(procs):
    for p, out, err in procs:
        if p.poll() is None:
            p.kill()
            p.wait()
        out.close(); err.close()


def finish_children(procs):
    """each child's lines; a child that fails, aborts or runs out of its time fails the test with what it wrote.  Nothing is retried."""
    res = []
    try:
        for (label, gate), (p, out, err) in zip(GATES, procs):
            try:
                p.wait(timeout=CHILD_TIMEOUT)
            except subprocess.TimeoutExpired:
                p.kill()
                p.wait()
            out.seek(0); err.seek(0)
            stdout, stderr = out.read(), err.read()
            assert p.returncode == 0 and "CHILD_OK" in stdout, "SMG_WIDE_LAT_MAX=%s: exit status %s (limit %d s)\n%s\n%s" % (
                gate, p.returncode, CHILD_TIMEOUT, stdout[-3000:], stderr[-4000:])
            lines = [ln for ln in stdout.splitlines() if ln.startswith(("gate ", "vec ", "norm ", "his "))]
            assert "CHILD_OK %d" % len(lines) in stdout, stdout[-3000:]
            res.append(lines)
    finally:
        stop_children(procs)
    return res


def three_runs(what, name, ks, own_run):
    procs = start_children(what, name, ks)
    try:
        mine = own_run()
    except BaseException:
        stop_children(procs)
        raise
    compare(mine, finish_children(procs))


def split(lines):
    """(gate lines, exact lines, {tag: floats} of the norm and history lines)"""
    approx = {}
    for ln in lines:
        if ln.startswith(("norm ", "his ")):
            w = ln.split()
            nkey = 5 if w[0] == "norm" else 4
            approx[" ".join(w[:nkey])] = np.array([float(v) for v in w[nkey:]])
    return [ln for ln in lines if ln.startswith("gate ")], [ln for ln in lines if ln.startswith("vec ")], approx


def compare(mine, others):
    gates0, vec0, approx0 = split(mine)
    assert vec0 and gates0
    print("\n".join(gates0))
    sides = {}
    for (label, gate), lines in zip(GATES, others):
        gates, vec, approx = split(lines)
        assert [g.rsplit(" side", 1)[0] for g in gates] == [g.rsplit(" side", 1)[0] for g in gates0], "the %s run launched other sizes" % label
        sides[label] = {g.rsplit(" side", 1)[1] for g in gates}
        diff = [(a, b) for a, b in zip(vec0, vec) if a != b]
        assert len(vec) == len(vec0) and not diff, "SMG_WIDE_LAT_MAX=%s gives other bits than the default gate in %d of %d vectors, first: %s" % (gate, len(diff), len(vec0), diff[:3])
        assert approx.keys() == approx0.keys()
        for key, v0 in approx0.items():
            assert v0.shape == approx[key].shape and (np.abs(approx[key] - v0) <= 1e-13 * np.abs(v0)).all(), (key, gate, v0, approx[key])
    assert sides == {"streaming": {"0"}, "latency": {"1"}}, sides      # the two children really sat on the two sides, for every launch
    print("default gate: %d of %d launches one row per lane; all of them streamed in one child and ran one row per lane in the other" % (
        sum(g.endswith("side1") for g in gates0), len(gates0)))


# (one case per column count on the two 40 877-row hierarchies: the float32 restatement in numpy is what takes the time there)
CASES = ([("subdiv-mcf", (k,)) for k in ALL_KS] + [("subdiv-poisson", (k,)) for k in SOME_KS] +
         [(name, SOME_KS) for name in ("bunny-dec", "random-1500-hub", "path-65", "path-50-pinned")])


@pytest.mark.parametrize("name,ks", CASES, ids=["%s-k%s" % (n, "+".join(str(k) for k in ks)) for n, ks in CASES])
def test_both_wide_variants_give_the_oracles_and_the_restatements_bits(smg, oracle_mod, name, ks):
    """subdiv-mcf: fixed-pitch panels, coded transfers, every seam of the 8 / 16 / 32 blocks; subdiv-poisson: 600 pinned rows; bunny-dec: Galerkin
    rows wider than 16 (the 16- and 32-entry batches of the one-row variant against U = 8 of the streaming one), value-carrying transfers;
    random-1500-hub: compact panels, very wide slices, many colours; path-65: a slice of one row (nrow < RW, and sub * RW >= nrow for most waves of
    the slice); path-50-pinned.  With the default gate only the whole-matrix launches of 32 columns on the 40 877-row level stream."""
    three_runs("pieces", name, ks, lambda: pieces(smg, oracle_mod, name, ks))


@pytest.mark.parametrize("k", [8, 40])
def test_cycles_and_solves_do_not_depend_on_the_wide_variant(smg, k):
    """one full-depth V-cycle (fp64 and the fp32 cycle of the mixed mode) and one solve of exactly 6 cycles (tol = 0: the count does not depend on a
    norm) in fp64 and mixed precision on subdiv-mcf: the iterates of the three runs have equal SHA-256, the histories agree to 1e-13 relative"""
    three_runs("loops", "subdiv-mcf", (k,), lambda: loops(smg, "subdiv-mcf", k))
