"""Weight codes in the transfer images (SMG_TRANSFER_CODES, SellDev::codes in csrc/smg_device.hpp).

Mid-point subdivision builds P from two values (1.0 and 0.5), so its device image and that of P^T carry a 2-bit code in every column word
and no value array.  The kernels decode the value and run the same sums in the same order: every restriction, prolongation, V-cycle and
solve must give the same bits with the codes on and off.  Images with more than 4 distinct values (decimated hierarchies) keep the value
array.  The knob is read once per process, hence the child processes."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_CHILD = r"""
import hashlib, os, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import numpy as np
import scipy.sparse as sp
import surface_multigrid_code_amd as smg
from oracle import mesh_np as M
from problems import subdiv_problem

def h(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:16]

def sell_bytes(mg, what):
    d = mg.device_bytes()
    return sum(v for n, v in d.items() if n.endswith(what))

def pieces(tag, mg, k, rng):
    out = []
    for lv in range(mg.n_levels - 1):
        x = rng.uniform(-1, 1, (mg.rows(lv), k)); xc = rng.uniform(-1, 1, (mg.rows(lv + 1), k))
        out.append(h(mg.restrict(lv, x)) + "/" + h(mg.prolong(lv, xc)))
    B, u = rng.uniform(-1, 1, (mg.rows(0), k)), rng.uniform(-1, 1, (mg.rows(0), k))
    out.append(h(mg.vcycle(B, u)))
    print(tag, k, " ".join(out), "P_bytes=%d" % sell_bytes(mg, "P_sell"), "PT_bytes=%d" % sell_bytes(mg, "PT_sell"))

rng = np.random.default_rng(5)
# subdivision hierarchies: coded transfers; k = 1 / 3 (narrow kernel), 8 / 64 (wide kernel); fp64 and mixed-precision solves
for k in (1, 3, 8, 64):
    p = subdiv_problem(kind="mcf", k=k, n_sub=3)
    mg = smg.Hierarchy.from_prolongs(p["Ps"])
    mg.precompute(p["A"], p["known"])
    pieces("subdiv", mg, k, rng)
    for prec in ("f64", "mixed"):
        conv, z, rh = mg.solve(p["RHS"], p["z0"], p["known_val"], smg.SolveOpts(tol=1e-9, max_iter=30, precision=prec))
        print("solve", k, prec, conv, len(rh), h(z), h(np.asarray(rh)))
# a Poisson problem with a pinned boundary (the column drops of P_full leave the codes' value set as it is)
p = subdiv_problem(kind="poisson", k=2, n_sub=3)
mg = smg.Hierarchy.from_prolongs(p["Ps"])
mg.precompute(p["A"], p["known"])
pieces("poisson", mg, 2, rng)
conv, z, rh = mg.solve(p["RHS"], p["z0"], p["known_val"], smg.SolveOpts(tol=1e-9, max_iter=30))
print("solve poisson", conv, len(rh), h(z), h(np.asarray(rh)))
# decimated hierarchy (many distinct weights: the value array stays)
V, F = M.read_smgm("ogre_sim.smgm"); V = M.normalize_unit_area(V, F)
mg = smg.mg_precompute(V, F, 0.25, 100, 1)
Mb = M.massmatrix(V, F, "barycentric"); A = (Mb - 0.01 * M.cotmatrix(V, F)).tocsr(); A.sort_indices()
mg.precompute(A)
pieces("decimated", mg, 1, rng)
# several subdivision meshes in one handle
ms, As, Bs = [], [], []
for mesh in ("ogre_sim.smgm", "bunny.smgm"):
    q = subdiv_problem(mesh=mesh, kind="mcf", k=1, n_sub=2)
    m = smg.Hierarchy.from_prolongs(q["Ps"]); ms.append(m); As.append(q["A"]); Bs.append(q["RHS"])
u = smg.Hierarchy.union(ms)
Au = sp.block_diag(As, format="csr"); Au.sort_indices()
u.precompute(Au)
Bu = np.asfortranarray(np.concatenate(Bs, axis=0))
conv, z, rh = u.solve(Bu, np.zeros_like(Bu), None, smg.SolveOpts(tol=1e-9, max_iter=40))
print("union", conv, len(rh), h(z), h(np.asarray(rh)))
"""


def _run(root, codes):
    env = dict(os.environ)
    env["SMG_TRANSFER_CODES"] = codes
    r = subprocess.run([sys.executable, "-c", _CHILD, root], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    return [ln for ln in r.stdout.splitlines() if ln.startswith(("subdiv", "solve", "poisson", "decimated", "union"))]


def _strip(ln):
    return " ".join(w for w in ln.split() if not w.startswith(("P_bytes=", "PT_bytes=")))


def _bytes(ln, what):
    return int([w for w in ln.split() if w.startswith(what + "=")][0].split("=")[1])


def test_transfer_codes_do_not_change_a_bit():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    on, off = _run(root, "1"), _run(root, "0")
    assert len(on) == 16 and len(off) == 16, (on, off)
    assert [_strip(a) for a in on] == [_strip(b) for b in off]
    assert all(ln.split()[3] == "True" for ln in on if ln.startswith("solve") and ln.split()[2] == "f64")
    for a, b in zip(on, off):
        if a.startswith(("subdiv", "poisson")):
            # coded: the value arrays of P and PT are gone (8 bytes per slot of 12)
            assert _bytes(a, "P_bytes") < 0.5 * _bytes(b, "P_bytes") and _bytes(a, "PT_bytes") < 0.5 * _bytes(b, "PT_bytes"), (a, b)
        elif a.startswith("decimated"):
            # more than 4 distinct weights: the old layout
            assert _bytes(a, "P_bytes") == _bytes(b, "P_bytes") and _bytes(a, "PT_bytes") == _bytes(b, "PT_bytes"), (a, b)
