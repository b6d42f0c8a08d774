"""The two quarter passes the V-cycle no longer makes on a level smoothed with one launch per colour, against the same cycle with them:

* SMG_RESID_BYPRODUCT: the last pre-smoothing launch also stores the residual of its rows (the last colour), and the residual launch
  walks the other colours only (csrc/smg_device.hpp: SELL_GS_RES / SELL_GS_OOP_RES);
* SMG_PROLONG_SKIP_FIRST: the prolongation leaves out the slices inside the first colour, whose rows the first post-smoothing launch
  overwrites without reading them.

Both are removals of work nobody reads: every output must keep every bit.  The knobs are read once per process, so each case runs two
child processes -- knobs on (the default) and off -- and compares sha256 sums of what they computed.  SMG_TILED=0 in both: on a mesh of
this size every level would otherwise run relax() as one launch and the new paths would never execute."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

_CHILD = r"""
import ctypes as C, hashlib, os, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
kind, k, what = sys.argv[2], int(sys.argv[3]), sys.argv[4]
import numpy as np
import surface_multigrid_code_amd as smg
from problems import subdiv_problem
sha = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
p = subdiv_problem(mesh="ogre_sim.smgm", n_sub=2, kind=kind, k=k, n_pins=20 if kind == "poisson" else 0)
mg = smg.Hierarchy.from_prolongs(p["Ps"])
mg.precompute(p["A"], p["known"])
n = mg.rows(0)
# the slices of level 0: 64 rows at a time inside each colour, as wide as their longest row
A0, cp = mg.matrix(0, "A", internal=True).tocsr(), mg.colors(0)
rl = np.diff(A0.indptr)
w = [int(rl[r0:min(r0 + 64, cp[c + 1])].max()) for c in range(len(cp) - 1) for r0 in range(cp[c], cp[c + 1], 64)]
print("shape", mg.n_levels, n, len(cp) - 1, sum(x > 8 for x in w), sum(x <= 8 for x in w), int(any((cp[c + 1] - cp[c]) % 64 for c in range(len(cp) - 1))))
if what == "cycles":
    rng = np.random.default_rng(3)
    B, u = rng.uniform(-1, 1, (n, k)), rng.uniform(-1, 1, (n, k))
    for pre, post in ((2, 2), (1, 1), (1, 0), (0, 1)):
        print("out vcycle_%d_%d" % (pre, post), sha(mg.vcycle(B, u, pre=pre, post=post)))
conv, z, rh = mg.solve(p["RHS"], p["z0"], p["known_val"], smg.SolveOpts(tol=1e-9, max_iter=30))
print("out solve", sha(z), sha(rh), len(rh), int(conv))
# a converged solve that keeps iterating: the tolerance is met after a few cycles, the launches that follow store nothing
tol = float(rh[min(3, len(rh) - 1)]) * 1.000001
kv = p["known_val"]
kvh = None if kv is None else np.asfortranarray(kv)
rhs, z0 = np.asfortranarray(p["RHS"]), np.asfortranarray(p["z0"])
zc = np.zeros_like(rhs, order="F")
mg.solve_begin(rhs.ctypes.data, rhs.shape[0], z0.ctypes.data, z0.shape[0], k, None if kvh is None else kvh.ctypes.data, 0 if kvh is None else kvh.shape[0],
               opts=smg.SolveOpts(tol=tol, max_iter=30), memspace=smg.api.SMG_HOST)
mg.outer_iterations(12)
conv2, rh2 = mg.solve_end(zc.ctypes.data, zc.shape[0], memspace=smg.api.SMG_HOST)
print("out converged", sha(zc), sha(rh2), len(rh2), int(conv2))
"""


def _child(kind, k, what, env):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", _CHILD, root, kind, str(k), what], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    shape = [ln.split()[1:] for ln in r.stdout.splitlines() if ln.startswith("shape ")]
    outs = [ln for ln in r.stdout.splitlines() if ln.startswith("out ")]
    assert len(shape) == 1, r.stdout
    return [int(x) for x in shape[0]], outs


@pytest.mark.parametrize("fuse_head", (1, 0))
@pytest.mark.parametrize("k", (1, 3))
@pytest.mark.parametrize("kind", ("mcf", "poisson"))
def test_dead_quarters_do_not_change_a_bit(kind, k, fuse_head):
    """V-cycles with (pre, post) = (2, 2), (1, 1) -- no out-of-place second sweep --, (1, 0) and (0, 1) -- one of the old paths stays in force --, a
    solve to 1e-9 (z and the residual history) and a solve that converges after a few cycles and is iterated on past that (the new store
    hangs on the same flag as the sweep's): identical bits with SMG_RESID_BYPRODUCT / SMG_PROLONG_SKIP_FIRST on and off, with the outer
    residual folded into the first sweep (the last pre-smoothing launch of level 0 is then the out-of-place one) and with SMG_FUSE_HEAD=0
    (solves only: the head is a solve's).  ogre_sim subdivided twice: 3 levels, irregular vertices (slices wider than the look-ahead batch,
    whose sums run over several batches, beside slices that are not), k = 3 takes the three-column kernels, the pins of the Poisson problem
    make the colour blocks end mid-slice."""
    res = []
    for on in ("1", "0"):
        env = dict(os.environ, SMG_TILED="0", SMG_RESID_BYPRODUCT=on, SMG_PROLONG_SKIP_FIRST=on, SMG_FUSE_HEAD=str(fuse_head))
        res.append(_child(kind, k, "cycles" if fuse_head else "solves", env))
    (shape, outs), (shape_off, outs_off) = res
    n_levels, n, n_colours, n_wide, n_narrow, ragged = shape
    print(kind, k, fuse_head, shape, outs)
    assert shape == shape_off
    assert n_levels >= 3 and n_colours >= 2          # two levels smoothed colour by colour
    assert n_wide >= 1 and n_narrow >= 1             # slices wider than 8 columns, and slices that are not
    assert ragged == 1                               # some colour block ends mid-slice
    assert len(outs) == (6 if fuse_head else 2)
    conv = [ln for ln in outs if ln.startswith("out converged")][0].split()
    assert conv[-1] == "1" and int(conv[-2]) <= 6    # the loop ended where the tolerance was met, not after the 12 iterations enqueued
    assert outs == outs_off
