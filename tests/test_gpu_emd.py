"""GPU (-m gpu): the earth mover's distance on a mesh (include/smg.h: smg_emd_*).

The host references are tests/emd_np.py -- the method in the kernels' operation order with direct solves -- and the library's own host twin
(smg_emd_host), which compiles the text the kernels compile.  The kernels are held launcher by launcher (smg_debug_emd, guarded buffers, every
output pre-filled with sentinels): geometry, right-hand sides, the update, the bounds' terms, sums and maxima, the potential, the flow and the
residual bit for bit against the restatement and against the host twin.  Only +, -, *, /, sqrt and max occur, so there is nothing to bound.

End to end against EmdNp's direct solves (the library's own L), t iterations at inner_rel_tol = 1e-12.  <P, Q> = sum_f A_f P_f . Q_f, |P|_A its
norm; res_t = |weak divergence of J_t - b|_2 over the unknown rows, which is the solve's residual of iteration t, as each side reports it;
lambda = lambda_min(-L_uu) from scipy.sparse.linalg.eigsh inside the test.  With an exact solve J is the A-orthogonal projection of Y = Z - U onto
the fields of divergence b and Z = shrink(T), 2 Z - T are non-expansive, so the relaxed iteration is non-expansive in T = Z + U under | |_A; a
solve with residual res moves grad phi by sqrt(res . (-L_uu)^-1 res) <= |res|_2 / sqrt(lambda).  Hence, alpha >= 1,

    E2E     |T_dev - T_np|_A and |J_dev - J_np|_A <= E_t = FACTOR sum_{s <= t} alpha (res_dev,s + res_np,s) / sqrt(lambda)
            The bound is the one for T; the test asserts it for J, which stands in for T: the state Z, U is not readable through the ABI, the
            flow is.  J_t is the A-orthogonal projection of Y_{t-1} = 2 Z_{t-1} - T_{t-1}, a non-expansive image of T_{t-1}, plus this
            iteration's solve error, so |J_dev,t - J_np,t|_A <= |T_dev,t-1 - T_np,t-1|_A + (res_dev,t + res_np,t) / sqrt(lambda) <= E_t.
            E_t sums the residuals of both sides, the restatement's direct solves included (about 1e-13): the reference is not exact either.
    UPPER   |upper_dev - upper_np| <= sqrt(sum A) E_t                                   (| |a| - |b| | <= |a - b|, Cauchy-Schwarz)
    LOWER   |lower_dev - lower_np| <= dq + |lower_np| max(1, gmax_np) rho E_t / sqrt(A_min),  dq = rho |b|_2 E_t / sqrt(lambda):
            |b . dphi| <= |b|_2 |dphi|_2 <= |b|_2 |grad dphi|_A / sqrt(lambda); a face's gradient moves by at most |grad dphi|_A / sqrt(A_f);
            |1 / x - 1 / y| <= |x - y| for x, y >= 1
    COLUMNS k columns of one query against k single queries: both runs are the same iteration with their own solves, so they differ by at most
            the bound with the two runs' residuals, which is at most twice the larger one's

FACTOR = 1: the derived bound as it stands (DESIGN.md section 30 records the measured ratios)."""
import ctypes as C
import gc
import json

import numpy as np
import pytest

import emd_np as N
from test_emd_host import GOLDEN, INVALID
from test_gpu_parity import smg  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

EPS = N.EPS
FACTOR = 1.0
COARSEST = {"icosphere3": 50, "torus": 50, "square": 20, "square, one level": 500}


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
@pytest.mark.parametrize("name", N.LAUNCHER_MESHES + N.PYRAMIDS)
def test_hook_against_restatement_and_host_twin(smg, name):
    """every launcher alone, k = 1, 3, 8: no guard touched, nothing past the extent, nothing of it left at the sentinel (emd_np._call)"""
    for k in (1, 3, 8):
        dev = N.check_launchers(hook_run(smg), name, k)
        hst = N.check_launchers(host_run(smg), name, k)
        for op, (a, b) in enumerate(zip(dev, hst)):
            assert np.array_equal(a, b), (name, k, op)


# ---- the objects ----------------------------------------------------------------------------------------------------------------------------------
def build(smg, case, **params):
    name = case.split(",")[0]
    V, F = N.shape(name)
    mg = smg.mg_precompute(V, F, 0.25, COARSEST[case], 1)
    assert (mg.n_levels == 1) == case.endswith("one level")
    ref = N.EmdNp(V, F, L=smg.mesh.cotmatrix(V, F))                            # the library's own L: the system's bits
    return V, F, mg, smg.EarthMover(mg, V, F, **params), ref, ref.lam_min()


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


@pytest.fixture(scope="module")
def torch_cuda():
    """torch with its device context open: the import and the first use of the device take about ten seconds when this file runs alone, and
    belong to no test's own time"""
    import torch
    torch.zeros(1, device="cuda")
    torch.cuda.synchronize()
    return torch


def stepwise(obj, mu0, mu1, steps, **kw):
    """`steps` iterations as `steps` warm one-iteration queries: the last result, and the absolute residual of every iteration (steps x k)"""
    nb = np.linalg.norm(np.asarray(mu1).reshape(obj.n, -1) - np.asarray(mu0).reshape(obj.n, -1), axis=0)
    keep = obj.params.max_iter
    obj.set_params(max_iter=1)
    res = []
    try:
        for t in range(steps):
            r = obj.distance(mu0, mu1, warm=t > 0, **(kw if t == steps - 1 else {}))
            assert r.iterations == 1
            res.append(r.residual * nb)
    finally:
        obj.set_params(max_iter=keep)
    return r, np.array(res)


def drift(res_a, res_b, alpha, lam):
    """E_t of the header per column"""
    return FACTOR * alpha * (res_a + res_b).sum(axis=0) / np.sqrt(lam)


@pytest.mark.parametrize("case", ["icosphere3", "square", "square, one level"])
def test_end_to_end_against_direct_solves(smg, objects, case):
    V, F, mg, obj, ref, lam = objects(case)
    k, steps = 3, 30
    mu0, mu1 = N.pairs(V, F, k)
    b = mu1 - mu0
    obj.set_params(inner_rel_tol=1e-12)
    try:
        r, res_dev = stepwise(obj, mu0, mu1, steps, potential=True, flow=True)
    finally:
        obj.set_params(inner_rel_tol=N.DEFAULTS["inner_rel_tol"])
    d = ref.solve(mu0, mu1, n_iter=steps, history=True)
    res_np = np.array([h[2] for h in d["his"]])
    _, rho, nb = N.column_setup(b, ref.area, N.DEFAULTS["rho_scale"])
    A, alpha = ref.A, N.DEFAULTS["alpha"]
    E = drift(res_dev, res_np, alpha, lam)
    dJ = r.flow - N.flow(V, F, d["J"])
    eJ = np.sqrt(np.sum(A[None] * np.sum(dJ * dJ, axis=2), axis=1))
    bu = np.sqrt(A.sum()) * E
    bl = rho * nb * E / np.sqrt(lam) + np.abs(d["lower"]) * np.maximum(1.0, d["gmax"]) * rho * E / np.sqrt(A.min())
    eu, el = np.abs(r.upper - d["upper"]), np.abs(r.lower - d["lower"])
    print("%s: lambda_min %.3e, residuals dev %.2e np %.2e (largest), E %s" % (case, lam, res_dev.max(), res_np.max(), E))
    print("  |J - J_np|_A %s (ratio to E %s)\n  |upper - upper_np| %s (bound %s)\n  |lower - lower_np| %s (bound %s)" % (eJ, eJ / E, eu, bu, el, bl))
    assert np.all(eJ <= E) and np.all(eu <= bu) and np.all(el <= bl)
    assert np.all(r.potential[0] == 0.0)
    g = N.grad2(ref.W2, F, r.potential)
    assert np.all(np.sqrt(g[:, :, 0] ** 2 + g[:, :, 1] ** 2).max(axis=1) <= 1.0 + 4 * EPS)
    assert np.array_equal(np.array([N.fixed_sum(t) for t in (b * r.potential).T]), r.lower)


def test_convergence_with_default_parameters(smg, objects):
    """icosphere(3), blobs: a gap <= 1e-2 within 1.5 times the restatement's 121 iterations, rounded up to a multiple of check_every"""
    V, F, mg, obj, ref, lam = objects("icosphere3")
    mu0, mu1 = N.blobs(V, F)
    r = obj.distance(mu0, mu1, potential=True)
    nb, psi = np.linalg.norm(mu1 - mu0), np.linalg.norm(r.potential)
    print("icosphere3 blobs: %d iterations, upper %.6f lower %.6f gap %.3e residual %.2e" % (r.iterations, r.upper[0], r.lower[0], r.gap[0], r.residual[0]))
    assert r.iterations <= 190 and r.iterations % 10 == 0 and r.gap[0] <= 1e-2
    assert r.lower[0] <= 1.408243 + 1e-6 + r.residual[0] * nb * psi            # below the restatement's upper bound at a gap of 1e-3 (six digits)
    assert r.upper[0] + r.residual[0] * nb * psi >= 1.406911 - 1e-6            # above its lower bound there


@pytest.mark.parametrize("case", ["icosphere3", "square"])
def test_certificate_swap_and_halving_with_a_fixed_inner_loop(smg, objects, case):
    """the stationary loop at three cycles per solve is linear in its right-hand side operation by operation: swapping mu0 and mu1 keeps the bits
    of both bounds, halving b halves them; the certificate lower <= upper + res |psi|_2 holds whatever the solve's accuracy"""
    V, F, mg, obj, ref, lam = objects(case)
    mu0, mu1 = N.pairs(V, F, 3)
    nb = np.linalg.norm(mu1 - mu0, axis=0)
    opts = smg.SolveOpts(tol=0.0, max_iter=3)
    obj.set_solver(0)
    obj.set_params(max_iter=20)
    try:
        a = obj.distance(mu0, mu1, potential=True, opts=opts)
        s = obj.distance(mu1, mu0, potential=True, opts=opts)
        h = obj.distance(0.5 * mu0, 0.5 * mu1, potential=True, opts=opts)
    finally:
        obj.set_solver(1)
        obj.set_params(max_iter=N.DEFAULTS["max_iter"])
    slack = a.residual * nb * np.linalg.norm(a.potential, axis=0)
    print("%s: upper %s lower %s residual %s" % (case, a.upper, a.lower, a.residual))
    assert a.iterations == s.iterations == h.iterations == 20
    assert np.all(a.lower <= a.upper + slack) and np.all(a.upper > 0.0)
    assert np.array_equal(a.upper, s.upper) and np.array_equal(a.lower, s.lower) and np.array_equal(a.potential, -s.potential)
    assert np.array_equal(0.5 * a.upper, h.upper) and np.array_equal(0.5 * a.lower, h.lower) and np.array_equal(a.potential, h.potential)


def test_swap_and_halving_with_pcg_within_the_bound(smg, objects):
    """nothing holds PCG's scalars to being odd in b operation by operation, so with the default solver the swapped and the halved query are two runs of the same
    iteration with their own solves: -J of the swapped and 2 J of the halved run are within E of J, E from the two runs' residuals (the halved
    run's doubled); upper follows.  10 iterations."""
    V, F, mg, obj, ref, lam = objects("icosphere3")
    mu0, mu1 = N.pairs(V, F, 3)
    steps, A, alpha = 10, ref.A, N.DEFAULTS["alpha"]
    norm = lambda dJ: np.sqrt(np.sum(A[None] * np.sum(dJ * dJ, axis=2), axis=1))   # noqa: E731
    a, res_a = stepwise(obj, mu0, mu1, steps, flow=True)
    s, res_s = stepwise(obj, mu1, mu0, steps, flow=True)
    h, res_h = stepwise(obj, 0.5 * mu0, 0.5 * mu1, steps, flow=True)
    Es, Eh = drift(res_a, res_s, alpha, lam), drift(res_a, 2.0 * res_h, alpha, lam)
    es, eh = norm(a.flow + s.flow), norm(a.flow - 2.0 * h.flow)
    print("icosphere3: |J + J_swapped|_A %s (bound %s); |J - 2 J_halved|_A %s (bound %s)" % (es, Es, eh, Eh))
    assert np.all(es <= Es) and np.all(eh <= Eh)
    assert np.all(np.abs(a.upper - s.upper) <= np.sqrt(A.sum()) * Es) and np.all(np.abs(a.upper - 2.0 * h.upper) <= np.sqrt(A.sum()) * Eh)


@pytest.mark.parametrize("k", [1, 3, 8])
def test_columns_against_single_queries(smg, objects, k):
    """COLUMNS of the header, 10 iterations"""
    V, F, mg, obj, ref, lam = objects("icosphere3")
    mu0, mu1 = N.pairs(V, F, k)
    steps, A, alpha = 10, ref.A, N.DEFAULTS["alpha"]
    r, res = stepwise(obj, mu0, mu1, steps, flow=True)
    worst = 0.0
    for c in range(k):
        rc, resc = stepwise(obj, mu0[:, c], mu1[:, c], steps, flow=True)
        E = drift(res[:, [c]], resc, alpha, lam)[0]
        dJ = r.flow[c] - rc.flow[0]
        eJ = np.sqrt(np.sum(A * np.sum(dJ * dJ, axis=1)))
        worst = max(worst, eJ / E)
        assert eJ <= E and abs(r.upper[c] - rc.upper[0]) <= np.sqrt(A.sum()) * E, (k, c)
    print("k = %d: largest |J_k - J_1|_A / E = %.3f" % (k, worst))


# ---- determinism, blocks, memory ---------------------------------------------------------------------------------------------------------------------
def results(r):
    return [r.upper, r.lower, np.array([r.iterations]), r.residual, r.potential, r.flow]


@pytest.mark.parametrize("pcg", [1, 0])
def test_same_calls_same_bits(smg, pcg):
    """two objects, the same calls: the same bits, with PCG and with the stationary loop, with graphs on and off"""
    V, F = N.shape("icosphere3")
    mg = smg.mg_precompute(V, F, 0.25, COARSEST["icosphere3"], 1)
    mu0, mu1 = N.pairs(V, F, 3)
    runs = []
    for use_graph in (1, 1, 0):
        obj = smg.EarthMover(mg, V, F, max_iter=20)
        obj.set_solver(pcg)
        opts = smg.SolveOpts(tol=1e-9, max_iter=30, use_graph=use_graph)
        a = obj.distance(mu0, mu1, potential=True, flow=True, opts=opts)
        b = obj.distance(mu0, mu1, warm=True, potential=True, flow=True, opts=opts)
        c = obj.distance(mu0[:, 0], mu1[:, 0], potential=True, flow=True, opts=opts)
        runs.append(results(a) + results(b) + results(c))
    for other in runs[1:]:
        for x, y in zip(runs[0], other):
            assert np.array_equal(x, y)
    assert not np.array_equal(runs[0][0], runs[0][6])                          # the warm call went on from the kept state


def raw_solve(smg, obj, mu0, ld0, mu1, ld1, k, memspace, upper, lower, n_iter=None, residual=None, potential=None, ld_p=0, flow=None, warm=0, opts=None):
    ptr = lambda a: a if a is None or isinstance(a, int) else a.ctypes.data   # noqa: E731
    dp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))   # noqa: E731
    return smg._lib.load().smg_emd_solve(obj.o, ptr(mu0), ld0, ptr(mu1), ld1, k, memspace, None if opts is None else C.byref(opts.c), warm, dp(upper), dp(lower),
                                         None if n_iter is None else C.byref(n_iter), dp(residual), ptr(potential), ld_p, ptr(flow))


@pytest.mark.parametrize("case", ["icosphere3", "square"])
def test_host_and_device_blocks(smg, objects, torch_cuda, case):
    """SMG_HOST and SMG_DEVICE blocks with padded leading dimensions give the same bits; rows past nV are untouched"""
    torch = torch_cuda
    V, F, mg, obj, ref, lam = objects(case)
    n, nF, k = V.shape[0], F.shape[0], 2
    mu0, mu1 = N.pairs(V, F, k)
    obj.set_params(max_iter=20)
    try:
        want = obj.distance(mu0, mu1, potential=True, flow=True)
        ld = n + 5
        m0h, m1h = np.full((ld, k), np.nan, order="F"), np.full((ld + 2, k), np.nan, order="F")
        m0h[:n], m1h[:n] = mu0, mu1
        Ph, Jh = np.full((ld, k), -2.0, order="F"), np.zeros((k, nF, 3))
        up, lo, res, nit = np.zeros(k), np.zeros(k), np.zeros(k), C.c_int(0)
        assert raw_solve(smg, obj, m0h, ld, m1h, ld + 2, k, 0, up, lo, nit, res, Ph, ld, Jh) == 0
        assert np.array_equal(up, want.upper) and np.array_equal(lo, want.lower) and np.array_equal(res, want.residual) and nit.value == want.iterations
        assert np.array_equal(Ph[:n], want.potential) and np.all(Ph[n:] == -2.0) and np.array_equal(Jh, want.flow)
        m0d = torch.full((k, ld), float("nan"), dtype=torch.float64, device="cuda")
        m1d = torch.full((k, ld), float("nan"), dtype=torch.float64, device="cuda")
        m0d[:, :n], m1d[:, :n] = torch.from_numpy(mu0.T.copy()).cuda(), torch.from_numpy(mu1.T.copy()).cuda()
        Pd = torch.full((k, ld), -1.0, dtype=torch.float64, device="cuda")
        Jd = torch.zeros((k, nF, 3), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        up2, lo2 = np.zeros(k), np.zeros(k)
        assert raw_solve(smg, obj, m0d.data_ptr(), ld, m1d.data_ptr(), ld, k, 1, up2, lo2, potential=Pd.data_ptr(), ld_p=ld, flow=Jd.data_ptr()) == 0
        got = Pd.cpu().numpy()
        assert np.array_equal(up2, want.upper) and np.array_equal(lo2, want.lower)
        assert np.array_equal(got[:, :n].T, want.potential) and np.all(got[:, n:] == -1.0) and np.array_equal(Jd.cpu().numpy(), want.flow)
    finally:
        obj.set_params(max_iter=N.DEFAULTS["max_iter"])


def test_non_finite_mass_is_refused_and_the_object_recovers(smg, objects):
    V, F, mg, obj, ref, lam = objects("icosphere3")
    n, nF, k = V.shape[0], F.shape[0], 2
    mu0, mu1 = N.pairs(V, F, k)
    bad = np.asfortranarray(mu1.copy())
    bad[77, 1] = np.nan
    m0 = np.asfortranarray(mu0)
    up, lo, res, nit = np.full(k, N.SENTINEL), np.full(k, N.SENTINEL), np.full(k, N.SENTINEL), C.c_int(-77)
    P, J = np.full((n, k), N.SENTINEL, order="F"), np.full((k, nF, 3), N.SENTINEL)
    obj.set_params(max_iter=20)
    try:
        assert raw_solve(smg, obj, m0, n, bad, n, k, 0, up, lo, nit, res, P, n, J) == INVALID
        assert smg._lib.load().smg_last_error().decode() == json.load(open(GOLDEN))["live"]["solve with a NaN mass"][1]
        assert all(np.all(a == N.SENTINEL) for a in (up, lo, res, P, J)) and nit.value == -77
        fresh = smg.EarthMover(mg, V, F, max_iter=20)
        for x, y in zip(results(obj.distance(mu0, mu1, potential=True, flow=True)), results(fresh.distance(mu0, mu1, potential=True, flow=True))):
            assert np.array_equal(x, y)
    finally:
        obj.set_params(max_iter=N.DEFAULTS["max_iter"])


def test_zero_column_and_zero_query(smg, objects):
    """a column with b = 0 returns upper = lower = 0 beside a live one; a query of zero columns alone iterates nothing"""
    V, F, mg, obj, ref, lam = objects("icosphere3")
    mu0, mu1 = N.pairs(V, F, 1)
    obj.set_params(max_iter=10)
    try:
        two = obj.distance(np.concatenate([mu0, mu0], axis=1), np.concatenate([mu1, mu0], axis=1), potential=True, flow=True)
        none = obj.distance(mu0, mu0, potential=True, flow=True)
    finally:
        obj.set_params(max_iter=N.DEFAULTS["max_iter"])
    assert two.iterations == 10 and two.upper[0] > 0.0 and two.upper[1] == 0.0 and two.lower[1] == 0.0 and two.residual[1] == 0.0
    assert np.all(two.potential[:, 1] == 0.0) and np.all(two.flow[1] == 0.0)
    assert none.iterations == 0 and none.upper[0] == 0.0 and none.lower[0] == 0.0 and np.all(none.potential == 0.0) and np.all(none.flow == 0.0)


def test_device_bytes_are_live_buffers_and_do_not_grow(smg):
    live = smg._lib.load().smg_device_bytes_live
    for name in ("icosphere3", "square"):
        V, F = N.shape(name)
        mg = smg.mg_precompute(V, F, 0.25, COARSEST[name], 1)                 # the caller's hierarchy stays alive throughout
        mu0, mu1 = N.pairs(V, F, 3)
        gc.collect()
        before = live()
        obj = smg.EarthMover(mg, V, F, max_iter=10)
        obj.distance(mu0, mu1, potential=True, flow=True)
        obj.distance(mu0, mu1, potential=True, flow=True)
        second = obj.device_bytes()
        for _ in range(8):
            obj.distance(mu0, mu1, warm=True, potential=True, flow=True)
        counted, held = obj.device_bytes(), live() - before
        print("%s: device_bytes %d after the second query, %d after the tenth, live DevBuf bytes held %d" % (name, second, counted, held))
        del obj
        gc.collect()
        assert 0 < counted == held and counted == second and live() == before


def test_live_refusals(smg, objects):
    """the refusals that need an object: code and text as recorded in tests/golden/emd_refusals.json, group "live"; nothing is written"""
    golden = json.load(open(GOLDEN))["live"]
    L = smg._lib.load()
    V, F, mg, obj, ref, lam = objects("icosphere3")
    n = V.shape[0]
    mu0, mu1 = (np.asfortranarray(m) for m in N.pairs(V, F, 2))
    nan, inf, more = mu1.copy(order="F"), mu0.copy(order="F"), np.zeros((n, 2), order="F")
    nan[77, 1], inf[5, 0] = np.nan, np.inf
    one = np.zeros((n, 2), order="F")
    one[1], more[2] = 1.0, 2.0
    up, lo = np.full(2, N.SENTINEL), np.full(2, N.SENTINEL)
    P = np.full((n, 2), N.SENTINEL, order="F")

    def sol(mu0=mu0, mu1=mu1, k=2, mem=0, ld0=n, ld1=n, ld_p=n, upper=up, lower=lo):
        return raw_solve(smg, obj, mu0, ld0, mu1, ld1, k, mem, upper, lower, potential=P, ld_p=ld_p)
    p = L.smg_emd_params_default()

    def setp(null=False, **kw):
        q = type(p)(*[getattr(p, f) for f, _ in p._fields_])
        for key, val in kw.items():
            setattr(q, key, val)
        return L.smg_emd_set_params(obj.o, None if null else C.byref(q))
    calls = {"solve without mu0": lambda: sol(mu0=None), "solve without mu1": lambda: sol(mu1=None), "solve without upper": lambda: sol(upper=None),
             "solve without lower": lambda: sol(lower=None), "solve with k = 0": lambda: sol(k=0), "solve with a bad memspace": lambda: sol(mem=2),
             "solve with ld0 < nV": lambda: sol(ld0=n - 1), "solve with ld1 < nV": lambda: sol(ld1=n - 1), "solve with ld_p < nV": lambda: sol(ld_p=n - 1),
             "solve with a NaN mass": lambda: sol(mu1=nan), "solve with an infinite mass": lambda: sol(mu0=inf),
             "solve with masses that differ": lambda: sol(mu0=one, mu1=more), "set_params without p": lambda: setp(null=True),
             "set_params with alpha = 2": lambda: setp(alpha=2.0), "set_params with check_every = 0": lambda: setp(check_every=0)}
    assert set(calls) == set(golden)
    for name, call in calls.items():
        rc = call()
        assert [rc, L.smg_last_error().decode()] == golden[name] and rc == INVALID, name
    assert np.all(up == N.SENTINEL) and np.all(lo == N.SENTINEL) and np.all(P == N.SENTINEL)
    assert obj.params.alpha == 1.7
