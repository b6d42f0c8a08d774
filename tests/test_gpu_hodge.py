"""GPU (-m gpu): the Helmholtz-Hodge decomposition of per-face fields (include/smg.h: smg_hodge_*).

The host references are tests/hodge_np.py -- the method in the kernels' operation order with direct solves -- and the library's own host twin
(smg_hodge_host), which compiles the text the kernels compile.  The kernels are held launcher by launcher (smg_debug_hodge, guarded buffers, every
output pre-filled with sentinels): right-hand sides, parts, energy terms, energies and fields bit for bit against the restatement and against
the host twin.  Only +, -, *, / and sqrt occur, so there is nothing to bound.

End to end against HodgeNp's direct solves with opts.tol = 1e-12 |rhs|_F over the solve's columns (all rows, as the library forms its default).
The solve ends at a true residual |r|_2 < tol per handle (smg_solve_pcg replaces the recurrence's norm by the true one before it ends), and
|u - u_exact|_2 <= |r|_2 / lambda_min(-L_uu) <= tol / lambda_min, lambda_min from scipy.sparse.linalg.eigsh inside the test:

    E2E        max |u - u_np| <= 10 tol / lambda_min(-L_uu), the same for v with its own system (closed: the same system, one 2k-column solve whose
               tol is over all 2k columns).  The factor 10 covers the direct solve's own error and whatever separates PCG's recurrence from the
               true residual; the observed ratio max |u - u_np| / (tol / lambda_min) is printed.
    PARTS      a face's G differs by at most |grad e| <= 3 max |W_fi| max |e| = dG, R by dR alike, H by dG + dR (each a vector norm);
               Xt carries no solve: its energy has the restatement's bits.  An energy sum A_f |P_f|^2 moves by at most
               2 sqrt(E_np sum A) d + sum A d^2 + 4 nF eps E_np (Cauchy-Schwarz and the rounding of a sum of nF terms).
    ONE SOLVE  k fields at once against k single-field queries: both are within E2E of the exact potentials, the single query's tol is the
               smaller one, so they differ by at most twice the k-field bound.
    IDENTITIES on the device's output with default options (tol = 1e-10 |rhs|_F): tests/test_hodge_host.py's PYTHAGORAS and WITH_H with the
               default tolerance in place of |r|_2, and the torus' d alpha share >= 0.99.
    ROUND TRIP decompose(field(u0, v0)) against u0 - u0[0] and v0 within E2E."""
import ctypes as C
import gc
import json

import numpy as np
import pytest

import hodge_np as N
from test_hodge_host import GOLDEN, INVALID
from test_gpu_parity import smg  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

NONFINITE = -4
EPS = N.EPS
PYRAMIDS = ("pyramid255", "pyramid256", "pyramid257")


def hook_run(smg):
    def run(op, V, F, **kw):
        rc, bad, out = N.hook(smg, op, V, F, **kw)
        assert rc == 0 and bad == 0, (rc, bad)
        return out
    return run


def host_run(smg):
    def run(op, V, F, **kw):
        rc, out = N.host(smg, op, V, F, **kw)
        assert rc == 0
        return out
    return run


# ---- kernels, launcher by launcher -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", N.LAUNCHER_MESHES + PYRAMIDS)
def test_hook_against_restatement_and_host_twin(smg, name):
    """every launcher alone, k = 1, 3, 8: no guard touched, nothing past the extent, nothing of it left at the sentinel (hodge_np._call)"""
    for k in (1, 3, 8):
        dev = N.check_launchers(hook_run(smg), name, k)
        V, F = N.shape(name)
        X = N.smooth_field(V, F, k)
        u0, v0 = N.potentials(V, k)
        host = host_run(smg)
        for out, (op, kw) in zip(dev, ((N.HODGE_RHS, dict(X=X)), (N.HODGE_PARTS, dict(X=X, u=u0, v=v0)), (N.HODGE_FIELD, dict(u=u0, v=v0)))):
            assert np.array_equal(out, host(op, V, F, k=k, **kw)), (name, k, op)


# ---- the objects ----------------------------------------------------------------------------------------------------------------------------------
COARSEST = {"icosphere3": 50, "torus": 50, "square": 20, "square, one level": 500, "bunny.smgm": 200}


def build(smg, case):
    name = case.split(",")[0]
    V, F = N.shape(name)
    mg = smg.mg_precompute(V, F, 0.25, COARSEST[case], 1)
    assert (mg.n_levels == 1) == case.endswith("one level")
    ref = N.HodgeNp(V, F, L=smg.mesh.cotmatrix(V, F))                          # the library's own L: the system's bits
    return V, F, mg, smg.HodgeDecomposition(mg, V, F), ref, ref.lam_min()


@pytest.fixture(scope="module")
def objects(smg):
    cache = {}

    def get(case):
        if case not in cache:
            cache[case] = build(smg, case)
        return cache[case]
    yield get
    cache.clear()
    gc.collect()


def rhs_norms(ref, X):
    """|rhs|_F of the u solve and of the v solve as the library forms them: closed, the one solve's 2k columns; with boundary, b's and c's"""
    b, c, _ = N.rhs(ref.V, ref.F, X)
    if ref.closed:
        both = float(np.sqrt(np.sum(b * b) + np.sum(c * c)))
        return both, both
    return float(np.linalg.norm(b)), float(np.linalg.norm(c))


def e2e_bounds(ref, lam, X, rel=1e-12):
    """(the E2E bound of u, of v, tol) of a query at tol = rel |rhs|_F; with boundary the two solves share opts, so the smaller norm sets tol"""
    tol = rel * min(rhs_norms(ref, X))
    return 10.0 * tol / lam[0], 10.0 * tol / lam[1], tol


def tight(smg, tol):
    return smg.SolveOpts(tol=tol, max_iter=100)


def decompose_tight(smg, obj, ref, X, parts=False):
    """one query at the tol of e2e_bounds"""
    return obj.decompose(X, parts=parts, opts=tight(smg, e2e_bounds(ref, (1.0, 1.0), X)[2]))


@pytest.mark.parametrize("case", ["icosphere3", "torus", "square", "square, one level", "bunny.smgm"])
def test_end_to_end_against_direct_solves(smg, objects, case):
    V, F, mg, obj, ref, lam = objects(case)
    assert obj.is_closed == ref.closed
    k, nF = 3, F.shape[0]
    X = N.smooth_field(V, F, k)
    d = ref.decompose(X)
    bu, bv, tol = e2e_bounds(ref, lam, X)
    u, v, P, E, cyc = obj.decompose(X, parts=True, opts=tight(smg, tol))
    eu, ev = np.abs(u - d["u"]).max(), np.abs(v - d["v"]).max()
    print("%s: closed %s, cycles %s, lambda_min %.3e / %.3e, tol %.3e" % (case, ref.closed, cyc.tolist(), lam[0], lam[1], tol))
    print("  max |u - u_np| = %.2e (bound %.2e, ratio to tol / lambda_min %.3f); max |v - v_np| = %.2e (bound %.2e, ratio %.3f)"
          % (eu, bu, eu / (bu / 10.0), ev, bv, ev / (bv / 10.0)))
    assert np.all(cyc < 100)                                                   # converged
    assert eu <= bu and ev <= bv
    assert np.all(u[0] == 0.0) and np.all(v[ref.bnd] == 0.0) and (not ref.closed or np.all(v[0] == 0.0))
    # parts and energies
    W, _, A = N.rest_faces(V, F)
    maxW = float(np.sqrt((W * W).sum(axis=2)).max())
    dG, dR = 3.0 * maxW * bu, 3.0 * maxW * bv
    Pd, Pn = P.reshape(k, nF, 9), d["parts"]
    err = [float(np.linalg.norm(Pd[:, :, 3 * e:3 * e + 3] - Pn[:, :, 3 * e:3 * e + 3], axis=2).max()) for e in range(3)]
    print("  parts: max |G - G_np| = %.2e (bound %.2e), R %.2e (bound %.2e), H %.2e (bound %.2e)" % (err[0], dG, err[1], dR, err[2], dG + dR))
    assert err[0] <= dG and err[1] <= dR and err[2] <= dG + dR
    En, Atot = d["energy"], float(A.sum())
    assert np.array_equal(E[:, 0], En[:, 0])
    for e, dd in ((1, dG), (2, dR), (3, dG + dR)):
        bound = 2.0 * np.sqrt(En[:, e] * Atot) * dd + Atot * dd * dd + 4 * nF * EPS * En[:, e]
        print("  energy %d: max |E - E_np| = %.2e (bound %.2e)" % (e, np.abs(E[:, e] - En[:, e]).max(), bound.min()))
        assert np.all(np.abs(E[:, e] - En[:, e]) <= bound)


@pytest.mark.parametrize("k", [1, 3, 4, 5, 8])
def test_closed_mesh_is_one_solve(smg, objects, k):
    """k fields are one 2k-column solve: 2, 6, 8, 10 and 16 columns, below, at and between the wide kernels' sizes"""
    V, F, mg, obj, ref, lam = objects("icosphere3")
    X = N.smooth_field(V, F, k)
    bound = 2.0 * e2e_bounds(ref, lam, X)[0]
    u, v, E, cyc = decompose_tight(smg, obj, ref, X)
    assert cyc[0] == cyc[1] and cyc[0] < 100
    worst = 0.0
    for s in range(k):
        us, vs, Es, cs = decompose_tight(smg, obj, ref, X[s:s + 1])
        assert cs[0] == cs[1] and cs[0] < 100
        worst = max(worst, np.abs(u[:, s] - us[:, 0]).max(), np.abs(v[:, s] - vs[:, 0]).max())
    print("k = %d (%d columns): %d cycles; max difference from the single-field queries %.2e (bound %.2e)" % (k, 2 * k, cyc[0], worst, bound))
    assert worst <= bound


@pytest.mark.parametrize("case", ["icosphere3", "torus", "square", "bunny.smgm"])
def test_identities_with_default_options(smg, objects, case):
    V, F, mg, obj, ref, lam = objects(case)
    k, nF = 3, F.shape[0]
    X = N.smooth_field(V, F, k)
    if case == "torus":
        X = np.concatenate([X[:2], N.dalpha_field(V, F)])
    nu, nv = rhs_norms(ref, X)
    u, v, P, E, cyc = obj.decompose(X, parts=True)
    _, _, A = N.rest_faces(V, F)
    Pd = P.reshape(k, nF, 9)
    G, R, H = Pd[:, :, :3], Pd[:, :, 3:6], Pd[:, :, 6:]
    gr, gh, rh = np.abs(N.inner(A, G, R)), np.abs(N.inner(A, G, H)), np.abs(N.inner(A, R, H))
    defect = np.abs(E[:, 0] - E[:, 1] - E[:, 2] - E[:, 3])
    bound = 2 * (gh + rh + gr) + 4 * nF * EPS * E[:, 0]
    bgh, brh = np.linalg.norm(u, axis=0) * 1e-10 * nu, np.linalg.norm(v, axis=0) * 1e-10 * nv
    bgr = 4 * nF * EPS * np.sqrt(E[:, 1] * E[:, 2])
    print("%s: cycles %s, shares %s" % (case, cyc.tolist(), (E[:, 1:] / E[:, [0]]).round(5).tolist()))
    print("  Pythagoras defect %s (bound %s)\n  |<G, H>| %s (bound %s)\n  |<R, H>| %s (bound %s)\n  |<G, R>| %s (bound %s)"
          % (defect, bound, gh, bgh, rh, brh, gr, bgr))
    assert np.all(cyc < 100)
    assert np.all(defect <= bound) and np.all(gh <= bgh) and np.all(rh <= brh) and np.all(gr <= bgr)
    if case == "torus":
        assert E[2, 3] / E[2, 0] >= 0.99
    if case == "icosphere3":
        assert E[0, 3] / E[0, 0] <= 0.01


# ---- field ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["icosphere3", "square"])
def test_field_and_round_trip(smg, objects, case):
    V, F, mg, obj, ref, lam = objects(case)
    k = 3
    u0, v0 = N.potentials(V, k)
    v0 = v0 - v0[[0]] if ref.closed else v0
    v0[ref.bnd] = 0.0
    X = obj.field(u0, v0)
    assert np.array_equal(X, N.field(V, F, u0, v0))
    assert np.array_equal(obj.field(u0[:, 0], v0[:, 0]), X[0])
    bu, bv, _ = e2e_bounds(ref, lam, X)
    u, v, E, cyc = decompose_tight(smg, obj, ref, X)
    eu, ev = np.abs(u - (u0 - u0[[0]])).max(), np.abs(v - v0).max()
    print("%s: round trip max |u - (u0 - u0[0])| = %.2e (bound %.2e), max |v - v0| = %.2e (bound %.2e), H shares %s, cycles %s"
          % (case, eu, bu, ev, bv, (E[:, 3] / E[:, 0]).tolist(), cyc.tolist()))
    assert np.all(cyc < 100) and eu <= bu and ev <= bv


# ---- determinism, blocks, memory ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pcg", [1, 0])
@pytest.mark.parametrize("name", ["icosphere3", "square"])
def test_same_calls_same_bits(smg, name, pcg):
    """two objects, the same calls: the same bits, with PCG and with the stationary loop, with graphs on and off"""
    V, F = N.shape(name)
    mg = smg.mg_precompute(V, F, 0.25, COARSEST[name], 1)
    X = N.smooth_field(V, F, 3)
    u0, v0 = N.potentials(V, 2)
    runs = []
    for use_graph in (1, 1, 0):
        obj = smg.HodgeDecomposition(mg, V, F)
        obj.set_solver(pcg)
        opts = smg.SolveOpts(tol=1e-9, max_iter=30, use_graph=use_graph)
        a = obj.decompose(X, parts=True, opts=opts)
        b = obj.decompose(X[:1], opts=opts)
        runs.append(list(a) + list(b) + [obj.field(u0, v0)])
    for other in runs[1:]:
        for x, y in zip(runs[0], other):
            assert np.array_equal(x, y)


def raw_decompose(smg, obj, X, k, memspace, u, ld_u, v, ld_v, parts, energy, cycles, opts=None):
    ptr = lambda a: a if a is None or isinstance(a, int) else a.ctypes.data   # noqa: E731
    return smg._lib.load().smg_hodge_decompose(obj.g, ptr(X), k, memspace, None if opts is None else C.byref(opts.c), ptr(u), ld_u, ptr(v), ld_v, ptr(parts),
                                               None if energy is None else energy.ctypes.data_as(C.POINTER(C.c_double)),
                                               None if cycles is None else cycles.ctypes.data_as(C.POINTER(C.c_int)))


@pytest.mark.parametrize("case", ["icosphere3", "square"])
def test_host_and_device_blocks(smg, objects, case):
    """SMG_HOST and SMG_DEVICE blocks with padded leading dimensions give the same bits; rows past nV are untouched"""
    import torch
    V, F, mg, obj, ref, lam = objects(case)
    n, nF, k = V.shape[0], F.shape[0], 2
    X = N.smooth_field(V, F, k)
    u, v, P, E, cyc = obj.decompose(X, parts=True)
    ld = n + 5
    uh, vh = np.full((ld, k), -2.0, order="F"), np.full((ld + 2, k), -3.0, order="F")
    Ph, Eh, ch = np.zeros((k, nF, 9)), np.zeros(4 * k), np.zeros(2, dtype=np.int32)
    assert raw_decompose(smg, obj, X, k, 0, uh, ld, vh, ld + 2, Ph, Eh, ch) == 0
    assert np.array_equal(uh[:n], u) and np.all(uh[n:] == -2.0) and np.array_equal(vh[:n], v) and np.all(vh[n:] == -3.0)
    assert np.array_equal(Ph.reshape(P.shape), P) and np.array_equal(Eh.reshape(k, 4), E) and np.array_equal(ch, cyc)
    Xd = torch.from_numpy(X).cuda()
    ud = torch.full((k, ld), -1.0, dtype=torch.float64, device="cuda")
    vd = torch.full((k, ld), -1.0, dtype=torch.float64, device="cuda")
    Pd = torch.zeros((k, nF, 9), dtype=torch.float64, device="cuda")
    Ed = np.zeros(4 * k)
    torch.cuda.synchronize()
    assert raw_decompose(smg, obj, Xd.data_ptr(), k, 1, ud.data_ptr(), ld, vd.data_ptr(), ld, Pd.data_ptr(), Ed, None) == 0
    got_u, got_v = ud.cpu().numpy(), vd.cpu().numpy()
    assert np.array_equal(got_u[:, :n].T, u) and np.all(got_u[:, n:] == -1.0) and np.array_equal(got_v[:, :n].T, v) and np.all(got_v[:, n:] == -1.0)
    assert np.array_equal(Pd.cpu().numpy().reshape(P.shape), P) and np.array_equal(Ed.reshape(k, 4), E)
    # the field from device blocks equals the field from host blocks
    Xf = torch.zeros((k, nF, 3), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    assert smg._lib.load().smg_hodge_field(obj.g, ud.data_ptr(), ld, vd.data_ptr(), ld, k, 1, Xf.data_ptr()) == 0
    assert np.array_equal(Xf.cpu().numpy(), obj.field(u, v))
    # energy, parts and cycles are optional
    assert raw_decompose(smg, obj, X, k, 0, uh, ld, vh, ld + 2, None, None, None) == 0 and np.array_equal(uh[:n], u)


def test_non_finite_field_is_refused_and_the_object_recovers(smg, objects):
    V, F, mg, obj, ref, lam = objects("icosphere3")
    n, nF, k = V.shape[0], F.shape[0], 2
    X = N.smooth_field(V, F, k)
    bad = X.copy()
    bad[1, 77, 2] = np.nan
    u, v = np.full((n, k), N.SENTINEL, order="F"), np.full((n, k), N.SENTINEL, order="F")
    P, E, cyc = np.full((k, nF, 9), N.SENTINEL), np.full(4 * k, N.SENTINEL), np.full(2, -77, dtype=np.int32)
    assert raw_decompose(smg, obj, bad, k, 0, u, n, v, n, P, E, cyc) == NONFINITE
    assert smg._lib.load().smg_last_error().decode() == "smg_hodge_decompose: the right-hand side is not finite"
    assert np.all(u == N.SENTINEL) and np.all(v == N.SENTINEL) and np.all(P == N.SENTINEL) and np.all(E == N.SENTINEL) and np.all(cyc == -77)
    fresh = smg.HodgeDecomposition(mg, V, F)
    for x, y in zip(obj.decompose(X, parts=True), fresh.decompose(X, parts=True)):
        assert np.array_equal(x, y)


def test_device_bytes_are_live_buffers_and_do_not_grow(smg):
    live = smg._lib.load().smg_device_bytes_live
    for name in ("icosphere3", "square"):
        V, F = N.shape(name)
        mg = smg.mg_precompute(V, F, 0.25, COARSEST[name], 1)                 # the caller's hierarchy stays alive throughout
        X = N.smooth_field(V, F, 3)
        gc.collect()
        before = live()
        obj = smg.HodgeDecomposition(mg, V, F)
        obj.decompose(X, parts=True)
        obj.decompose(X, parts=True)
        second = obj.device_bytes()
        for _ in range(8):
            obj.decompose(X, parts=True)
        counted, held = obj.device_bytes(), live() - before
        print("%s: device_bytes %d after the second query, %d after the tenth, live DevBuf bytes held %d" % (name, second, counted, held))
        del obj
        gc.collect()
        assert 0 < counted == held and counted == second and live() == before


def test_live_refusals(smg, objects):
    """the refusals that need an object: code and text as recorded in tests/golden/hodge_refusals.json, group "live"; nothing is written"""
    golden = json.load(open(GOLDEN))["live"]
    L = smg._lib.load()
    V, F, mg, obj, ref, lam = objects("icosphere3")
    n, nF = V.shape[0], F.shape[0]
    X = np.full((1, nF, 3), 0.5)
    u, v = np.full((n, 1), N.SENTINEL, order="F"), np.full((n, 1), N.SENTINEL, order="F")
    dec = lambda X=X, u=u, v=v, k=1, mem=0, ld_u=n, ld_v=n: raw_decompose(smg, obj, X, k, mem, u, ld_u, v, ld_v, None, None, None)   # noqa: E731
    ptr = lambda a: None if a is None else a.ctypes.data                                                                              # noqa: E731
    fld = lambda X=X, u=u, v=v, k=1, mem=0, ld_u=n, ld_v=n: L.smg_hodge_field(obj.g, ptr(u), ld_u, ptr(v), ld_v, k, mem, ptr(X))      # noqa: E731
    calls = {}
    for tag, fn in (("decompose", dec), ("field", fld)):
        calls.update({
            tag + " without X": lambda fn=fn: fn(X=None), tag + " without u": lambda fn=fn: fn(u=None), tag + " without v": lambda fn=fn: fn(v=None),
            tag + " with k = 0": lambda fn=fn: fn(k=0), tag + " with a bad memspace": lambda fn=fn: fn(mem=2),
            tag + " with ld_u < nV": lambda fn=fn: fn(ld_u=n - 1), tag + " with ld_v < nV": lambda fn=fn: fn(ld_v=n - 1)})
    assert set(calls) == set(golden)
    for name, call in calls.items():
        rc = call()
        assert [rc, L.smg_last_error().decode()] == golden[name] and rc == INVALID, name
    assert np.all(u == N.SENTINEL) and np.all(v == N.SENTINEL) and np.all(X == 0.5)
