"""GPU (-m gpu): two-species reaction-diffusion on a surface (include/smg.h: smg_rd_*).

The host references are tests/rd_np.py -- the method in the kernels' operation order with direct solves -- and the library's own host twin
(smg_rd_host), which compiles the text the kernels compile.  The kernels are held launcher by launcher (smg_debug_rd, guarded buffers, every output
pre-filled with sentinels) bit for bit against the restatement and against the host twin: only +, -, *, max and fabs occur, so there is nothing
to bound.

End to end against RdNp's direct solves (the library's own L).  m = the barycentric masses, A_D = M + dt D (-L), | | the 2-norm of one column
unless marked, eps = 2^-52.

    ONE STEP   from equal states the right-hand sides m u*, m v* are equal bit for bit (the launcher test), so the two solves' outputs differ by
               |u_dev - u_np| <= b = (10 tol + res_np) / min_i m_i per column              (the issue's statement)
               -L is positive semi-definite, so lambda_min(A_D) >= min m; tol = the solve's stopping tolerance as an absolute residual norm (the
               tests pass it: 1e-12 |rhs|_F of the first step); res_np = the direct solve's residual.  Dv == 0: v' = v* bit for bit.
    CHAIN      states that differ by E at a step's start, E = the M-norm sqrt(sum m (du^2 + dv^2)) of one column's difference.  The reaction acts
               vertex by vertex: d(u*, v*) = (I + dt J_i) d(u, v) + O(|d|^2) with J_i the reaction's 2 x 2 Jacobian at the restatement's state
               (react_substeps = 1 in every chained test), so |d(u*, v*)|_M <= g E, g = max_i sigma_max(I + dt J_i) -- the spectral norm of
               the step matrix, from numpy.  A_D^-1 M is M-self-adjoint with eigenvalues 1 / (1 + dt D lambda) <= 1: the exact solve does not
               increase the M-norm.  Each solve adds its own error, b in the 2-norm, at most sqrt(max m) b in the M-norm; the reaction kernel's
               rounding on the two different inputs adds at most 64 eps |(u, v)|_M (10 multiply-adds per cubic, two cubics, one update); the
               quadratic remainder adds dt H E_2^2 <= dt H E^2 / min m, H = the sum over both cubics of the absolute second derivatives.
                   E' = g E + sqrt(max m) sqrt(b_u^2 + b_v^2) + 64 eps |(u, v)|_M + dt H E^2 / min m,       |d(u, v)|_2 <= E / sqrt(min m)
               (rd_np.Chain; with s sub-steps g is the product of the sub-steps' norms and the rounding term carries s.)
               Chained from E = 0.  The bound grows like g^n; with the tests' dt it stays far below 1e-3 of the amplitude over 20 steps, so it
               is asserted at every step (the test prints it beside the observed error and fails if it ever exceeds 1e-3 of the amplitude).
    CLOSED     the homogeneous state and the eigenmode have closed forms (tests/test_rd_host.py); the device is held to them through the
               restatement: |dev - closed| <= CHAIN + |np - closed|, and |np - closed| is the restatement's own test, asserted here too with the
               CPU file's bound.
    COLUMNS    k columns of one run against single-column objects, one 2k-column solve against its single-simulation runs, and an object whose
               dt was set by set_params against a fresh one: both sides are the same steps with their own solves, each within CHAIN of the
               restatement: within twice CHAIN."""
import ctypes as C
import gc
import json

import numpy as np
import pytest

import rd_np as N
from test_gpu_parity import smg  # noqa: F401  (fixture)
from test_rd_host import GOLDEN, INVALID, closed_homogeneous, eigenmode_bounds, homogeneous_bounds, recurrence, schnakenberg_mode

pytestmark = pytest.mark.gpu

COARSEST = {"icosphere3": 50, "torus": 50, "square": 20}
NONFINITE = -4
CASES = {"two": dict(Du=0.02, Dv=0.01), "one": dict(Du=0.02, Dv=0.02), "v alone": dict(Du=0.02, Dv=0.0)}


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
    """every launcher alone, k = 1, 3, 8 and react_substeps = 1, 3: no guard touched, nothing past the extent, nothing of it left at the sentinel
    (rd_np._call).  icosphere1 has 42 vertices: a wavefront holds fewer than 64 and the waves of different columns share a block"""
    for k in (1, 3, 8):
        for n_sub in (1, 3):
            dev = N.check_launchers(hook_run(smg), name, k, n_sub)
            hst = N.check_launchers(host_run(smg), name, k, n_sub)
            for op, (a, b) in enumerate(zip(dev, hst)):
                assert np.array_equal(a, b), (name, k, n_sub, op)


# ---- the objects ----------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def meshes(smg):
    cache = {}

    def get(name):
        if name not in cache:
            V, F = N.shape(name)
            mg = smg.mg_precompute(V, F, 0.25, COARSEST[name], 1)
            assert mg.n_levels >= 2
            cache[name] = (V, F, mg, smg.mesh.cotmatrix(V, F))                  # the library's own L: the system's bits
        return cache[name]
    yield get
    cache.clear()
    gc.collect()


def gray_scott_state(smg, V, k):
    """(u, v nV x k, coeff k x 20): the usual start, u near 1 and v near 0 with smooth column-dependent patches, and k different (F, kappa) pairs"""
    s = np.arange(k)[None, :]
    bump = np.exp(-8.0 * ((V[:, [0]] - 0.3 * np.cos(s)) ** 2 + (V[:, [1]] - 0.3 * np.sin(s)) ** 2))
    u, v = 1.0 - 0.5 * bump, 0.25 * bump + 0.01 * np.cos(3.0 * V[:, [2]] + s)
    Fk = [(0.030 + 0.004 * c, 0.055 + 0.002 * c) for c in range(k)]
    return np.ascontiguousarray(u), np.ascontiguousarray(v), np.stack([smg.reactions.gray_scott(f, kap) for f, kap in Fk])


def rhs_tol(ref, rel=1e-12):
    """rel |rhs|_F of the restatement's current state, both species together: the absolute tolerance the tests pass to every solve"""
    sums = N.react(ref.m, ref.u, ref.v, ref.coeff, ref.p["dt"], ref.p["react_substeps"])[3]
    return rel * float(np.sqrt(sums.sum()))


Chain, distance = N.Chain, N.distance


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("name", ["icosphere3", "torus", "square"])
def test_one_step_against_direct_solves(smg, meshes, name, case):
    """ONE STEP of the header in each of the three handle cases, k = 3 Gray-Scott columns; Dv == 0: v' bit for bit; the histories against the
    fixed-order sums and maxima of the read-back states, bit for bit; the second entry of cycles is 0 when there is no second solve"""
    V, F, mg, L = meshes(name)
    k, dt = 3, 0.5
    u0, v0, coeff = gray_scott_state(smg, V, k)
    ref = N.RdNp(V, F, L=L, dt=dt, **CASES[case])
    assert ref.case == case
    ref.set_state(u0, v0, coeff)
    tol = rhs_tol(ref)
    obj = smg.ReactionDiffusion(mg, V, F, dt=dt, **CASES[case])
    obj.set_state(u0, v0, coeff)
    mass, change, cyc = obj.step(1, opts=smg.SolveOpts(tol=tol, max_iter=100))
    u, v = obj.state()
    ref.step(1)
    b = (10.0 * tol + ref.res) / ref.m.min()
    err = np.concatenate([np.linalg.norm(u - ref.u, axis=0), np.linalg.norm(v - ref.v, axis=0)])
    solved = slice(0, k) if case == "v alone" else slice(0, 2 * k)
    print("%s, %s: tol %.2e, res_np %.2e, min m %.3e; |dev - np|_2 per column %s, largest ratio to (10 tol + res_np) / min m %.4f; cycles %s"
          % (name, case, tol, ref.res.max(), ref.m.min(), err, float(np.max(err[solved] / b[solved])), cyc[0]))
    assert np.all(err[solved] <= b[solved])
    if case == "v alone":
        assert np.array_equal(v, ref.v) and np.array_equal(v, N.substeps(coeff, u0, v0, dt, 1)[1])
    assert (cyc[0, 1] > 0) == (case == "two") and cyc[0, 0] > 0
    _, _, sums, mx = N.close(ref.m, u0, v0, u, v)
    assert np.array_equal(mass[0], sums) and np.array_equal(change[0], mx)


def run_chained(smg, mg, V, F, L, u0, v0, coeff, steps, closed=None, label="", **params):
    """`steps` single steps of an object and of the restatement from equal states; CHAIN asserted at every step, and that it stays below 1e-3 of
    the amplitude.  closed(n) -> (u, v, bound) of the closed form after n steps: CLOSED of the header.  Returns (the object, the restatement,
    the last bound)"""
    ref = N.RdNp(V, F, L=L, **params)
    ref.set_state(u0, v0, coeff)
    tol = rhs_tol(ref)
    opts = smg.SolveOpts(tol=tol, max_iter=100)
    obj = smg.ReactionDiffusion(mg, V, F, **params)
    obj.set_state(u0, v0, coeff)
    chain = Chain(ref, tol)
    amp = np.sqrt(np.sum(ref.u ** 2 + ref.v ** 2, axis=0))
    worst, bound = 0.0, None
    for n in range(1, steps + 1):
        chain.before()
        ref.step(1)
        bound = chain.after()
        obj.step(1, opts=opts)
        u, v = obj.state()
        err = distance(u, v, ref.u, ref.v)
        line = "%s step %2d: |dev - np|_2 %s, CHAIN %s (g %s)" % (label, n, err, bound, chain.g)
        assert np.all(bound <= 1e-3 * amp), "the chained bound is useless at step %d: %s" % (n, bound)
        assert np.all(err <= bound), line
        worst = max(worst, float(np.max(err / bound)))
        if closed is not None:
            cu, cv, cb = closed(n)
            e_np, e_dev = distance(ref.u, ref.v, cu, cv), distance(u, v, cu, cv)
            line += "; |np - closed|_2 %s (bound %s), |dev - closed|_2 %s" % (e_np, cb, e_dev)
            assert np.all(e_np <= cb) and np.all(e_dev <= bound + cb), line
        if n in (1, steps):
            print(line)
    print("%s: largest |dev - np|_2 over CHAIN in %d steps %.4f" % (label, steps, worst))
    return obj, ref, bound


@pytest.mark.parametrize("model", ["gray_scott", "schnakenberg"])
@pytest.mark.parametrize("name", ["icosphere3", "torus", "square"])
def test_a_homogeneous_state_follows_the_scalar_recurrence(smg, meshes, name, model):
    """CLOSED of the header: u = a, v = b over 20 steps against (a, b) <- (a, b) + dt R(a, b); |np - closed| within HOMOGENEOUS of
    tests/test_rd_host.py"""
    V, F, mg, L = meshes(name)
    n = V.shape[0]
    coeff, a, b, params = closed_homogeneous(smg, model)
    ab = recurrence(coeff, a, b, params["dt"], 1, 20)
    ref = N.RdNp(V, F, L=L, **params)
    ref.set_state(np.full(n, a), np.full(n, b), coeff)
    bounds = homogeneous_bounds(ref, ab, 20)

    def closed(step):
        return np.full((n, 1), ab[step][0]), np.full((n, 1), ab[step][1]), bounds[step]
    run_chained(smg, mg, V, F, L, np.full(n, a), np.full(n, b), coeff, 20, closed=closed, label="%s, %s, homogeneous" % (name, model), **params)


def test_an_eigenmode_follows_the_2x2_recurrence(smg, meshes):
    """CLOSED of the header on icosphere(3): u = alpha phi, v = beta phi with -L phi = lambda M phi from a dense eigh of the library's L, a
    Schnakenberg linearisation whose Turing band contains lambda_3: amplitudes (diag(1 / (1 + dt D lambda)) (I + dt J))^n (alpha, beta);
    |np - closed| within EIGENMODE of tests/test_rd_host.py; the components along the other eigenvectors at most sqrt(max m) times the distance
    to the closed form"""
    V, F, mg, L = meshes("icosphere3")
    mode = schnakenberg_mode(smg, V, F, L)
    phi, lam, T = mode["phi"], mode["lam"], mode["step_matrix"]
    cols = np.array([3])
    assert 1.2 < lam[3] < 3.0
    amps = [np.array([[1.0], [-0.5]])]
    for _ in range(20):
        amps.append(T(lam[3]) @ amps[-1])
    assert np.linalg.norm(amps[20]) > np.linalg.norm(amps[0]), "lambda_3 is inside the Turing band: the mode grows"
    u0, v0 = phi[:, cols] * amps[0][0], phi[:, cols] * amps[0][1]
    ref = N.RdNp(V, F, L=L, **mode["params"])
    ref.set_state(u0, v0, mode["coeff"])
    bounds = eigenmode_bounds(ref, mode, cols, amps, 20)

    def closed(step):
        return phi[:, cols] * amps[step][0], phi[:, cols] * amps[step][1], bounds[step]
    obj, ref, chain = run_chained(smg, mg, V, F, L, u0, v0, mode["coeff"], 20, closed=closed, label="icosphere3, eigenmode 3", **mode["params"])
    u, v = obj.state()
    x = mode["m"][:, None] * np.concatenate([u, v], axis=1)
    others = np.delete(phi, 3, axis=1).T @ x
    print("icosphere3, eigenmode 3 (lambda %.6f): amplitudes %s -> %s (closed form %s); largest component along another eigenvector %.3e (bound %.3e)"
          % (lam[3], amps[0][:, 0], phi[:, 3] @ x, amps[20][:, 0], np.abs(others).max(), np.sqrt(mode["m"].max()) * (chain[0] + bounds[20][0])))
    assert np.abs(others).max() <= np.sqrt(mode["m"].max()) * (chain[0] + bounds[20][0])


def test_zero_reaction_from_a_constant_state_stops_after_one_step(smg, meshes):
    """stop_change ends a zero-reaction run from a constant state after its first step, n_done == 1; with stop_change == 0 the same run goes on"""
    V, F, mg, L = meshes("torus")
    n = V.shape[0]
    for case in CASES:
        obj = smg.ReactionDiffusion(mg, V, F, dt=0.1, stop_change=1e-6, **CASES[case])
        obj.set_state(np.full(n, 1.0), np.full(n, 2.0), np.zeros(20))
        mass, change, cyc = obj.step(5)
        assert obj.n_done == 1 and mass.shape == (1, 2) and np.all(change <= 1e-6), (case, change)
        obj.set_params(stop_change=0.0)
        assert obj.step(3)[0].shape == (3, 2) and obj.n_done == 3


def single_runs(smg, mg, V, F, u0, v0, coeff, steps, opts, **params):
    us, vs = [], []
    for c in range(u0.shape[1]):
        o = smg.ReactionDiffusion(mg, V, F, **params)
        o.set_state(u0[:, c], v0[:, c], coeff[c])
        o.step(steps, opts=opts)
        u, v = o.state()
        us.append(u[:, 0]), vs.append(v[:, 0])
    return np.stack(us, axis=1), np.stack(vs, axis=1)


def chain_bound(V, F, L, u0, v0, coeff, steps, **params):
    ref = N.RdNp(V, F, L=L, **params)
    ref.set_state(u0, v0, coeff)
    tol = rhs_tol(ref)
    chain, bound = Chain(ref, tol), None
    for _ in range(steps):
        chain.before()
        ref.step(1)
        bound = chain.after()
    return tol, bound, ref


def test_one_2k_column_solve_against_single_simulations(smg, meshes):
    """COLUMNS of the header, Du == Dv: k = 3 simulations as ONE 6-column solve per step against three single-simulation objects (a 2-column
    solve each), 5 steps: within twice CHAIN"""
    V, F, mg, L = meshes("icosphere3")
    u0, v0, coeff = gray_scott_state(smg, V, 3)
    params = dict(dt=0.5, **CASES["one"])
    tol, bound, ref = chain_bound(V, F, L, u0, v0, coeff, 5, **params)
    opts = smg.SolveOpts(tol=tol, max_iter=100)
    obj = smg.ReactionDiffusion(mg, V, F, **params)
    obj.set_state(u0, v0, coeff)
    _, _, cyc = obj.step(5, opts=opts)
    u, v = obj.state()
    su, sv = single_runs(smg, mg, V, F, u0, v0, coeff, 5, opts, **params)
    d = distance(u, v, su, sv)
    print("Du == Dv, 5 steps: |block - singles|_2 %s, twice CHAIN %s; against the restatement: block %s, singles %s; cycles %s"
          % (d, 2 * bound, distance(u, v, ref.u, ref.v), distance(su, sv, ref.u, ref.v), cyc[:, 0]))
    assert np.all(cyc[:, 1] == 0) and np.all(d <= 2 * bound)


def test_eight_gray_scott_columns_against_single_objects(smg, meshes):
    """COLUMNS of the header: k = 8 columns with eight different (F, kappa) pairs against eight single-column objects, 5 steps, two handles"""
    V, F, mg, L = meshes("icosphere3")
    u0, v0, coeff = gray_scott_state(smg, V, 8)
    assert len({tuple(c) for c in coeff}) == 8
    params = dict(dt=0.5, **CASES["two"])
    tol, bound, ref = chain_bound(V, F, L, u0, v0, coeff, 5, **params)
    opts = smg.SolveOpts(tol=tol, max_iter=100)
    obj = smg.ReactionDiffusion(mg, V, F, **params)
    obj.set_state(u0, v0, coeff)
    obj.step(5, opts=opts)
    u, v = obj.state()
    su, sv = single_runs(smg, mg, V, F, u0, v0, coeff, 5, opts, **params)
    d = distance(u, v, su, sv)
    print("k = 8 Gray-Scott columns, 5 steps: |block - singles|_2 %s, twice CHAIN %s; block against the restatement %s" % (d, 2 * bound, distance(u, v, ref.u, ref.v)))
    assert np.all(d <= 2 * bound) and np.all(distance(u, v, ref.u, ref.v) <= bound)


@pytest.mark.parametrize("case", list(CASES))
def test_set_params_to_a_new_dt_against_a_fresh_object(smg, meshes, case):
    """COLUMNS of the header: an object created with dt = 0.25 and set to dt = 0.5 (a value-only re-precompute), then 3 steps, against a fresh
    object created with dt = 0.5: within twice CHAIN; whether bitwise is printed.  A change of the handle case is refused"""
    V, F, mg, L = meshes("torus")
    u0, v0, coeff = gray_scott_state(smg, V, 2)
    params = dict(dt=0.5, **CASES[case])
    tol, bound, ref = chain_bound(V, F, L, u0, v0, coeff, 3, **params)
    opts = smg.SolveOpts(tol=tol, max_iter=100)
    outs = []
    for first_dt in (0.25, 0.5):
        o = smg.ReactionDiffusion(mg, V, F, **dict(params, dt=first_dt))
        o.set_state(u0, v0, coeff)
        if first_dt != 0.5:
            o.step(1, opts=opts)                                              # the old matrices are used once before they are replaced
            o.set_params(dt=0.5)
            o.set_state(u0, v0, coeff)
        o.step(3, opts=opts)
        outs.append(o.state())
    d = distance(outs[0][0], outs[0][1], outs[1][0], outs[1][1])
    print("%s: set_params(dt) against a fresh object, 3 steps: |difference|_2 %s, twice CHAIN %s, bitwise %s"
          % (case, d, 2 * bound, np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])))
    assert np.all(d <= 2 * bound)
    other = {"two": dict(Dv=0.02), "one": dict(Dv=0.0), "v alone": dict(Dv=0.02)}[case]
    with pytest.raises(smg.SmgError) as e:
        o.set_params(**other)
    assert e.value.code == INVALID and "smg_rd_set_params" in str(e.value)


def test_a_nan_is_refused_and_the_state_is_kept(smg, meshes):
    """a NaN in the initial u: SMG_ERR_NONFINITE at step 0, n_done == 0, nothing written past the first history row; after a valid set_state the
    next call equals a fresh object's to the bit"""
    V, F, mg, L = meshes("icosphere3")
    Lc = smg._lib.load()
    k = 2
    u0, v0, coeff = gray_scott_state(smg, V, k)
    obj = smg.ReactionDiffusion(mg, V, F, dt=0.5, **CASES["two"])
    obj.set_state(u0, v0, coeff)
    obj.step(2)
    bad = u0.copy()
    bad[77, 1] = np.nan
    obj.set_state(bad, v0, coeff)
    mass, change, cyc = np.full((3, 2 * k), N.SENTINEL), np.full((3, k), N.SENTINEL), np.full((3, 2), -7, dtype=np.int32)
    nd = C.c_int(-1)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    rc = Lc.smg_rd_step(obj.o, 3, None, mass.ctypes.data_as(dp), change.ctypes.data_as(dp), cyc.ctypes.data_as(ip), C.byref(nd))
    assert rc == NONFINITE and nd.value == 0 and b"smg_rd_step" in Lc.smg_last_error() and b"step 0" in Lc.smg_last_error()
    assert np.all(mass[1:] == N.SENTINEL) and np.all(change[1:] == N.SENTINEL) and np.all(cyc[1:] == -7)
    with pytest.raises(smg.SmgError) as e:
        obj.step(3)
    assert e.value.code == NONFINITE and obj.n_done == 0
    ku, kv = obj.state()
    assert np.isnan(ku[77, 1]) and np.array_equal(np.delete(ku, 77, axis=0), np.delete(bad, 77, axis=0)) and np.array_equal(kv, v0)
    obj.set_state(u0, v0, coeff)
    fresh = smg.ReactionDiffusion(mg, V, F, dt=0.5, **CASES["two"])
    fresh.set_state(u0, v0, coeff)
    for x, y in zip(obj.step(2), fresh.step(2)):
        assert np.array_equal(x, y)
    for x, y in zip(obj.state(), fresh.state()):
        assert np.array_equal(x, y)


def test_same_calls_same_bits(smg, meshes):
    """two runs of 10 Gray-Scott steps give identical bits, graphs on and off, in each handle case"""
    V, F, mg, L = meshes("icosphere3")
    u0, v0, coeff = gray_scott_state(smg, V, 3)
    for case in CASES:
        runs = []
        for use_graph in (1, 1, 0):
            obj = smg.ReactionDiffusion(mg, V, F, dt=0.5, react_substeps=2, **CASES[case])
            obj.set_state(u0, v0, coeff)
            out = obj.step(10, opts=smg.SolveOpts(tol=1e-9, max_iter=30, use_graph=use_graph))
            runs.append(list(out) + list(obj.state()))
        for other in runs[1:]:
            for x, y in zip(runs[0], other):
                assert np.array_equal(x, y), case


def test_device_bytes_are_live_buffers(smg):
    """smg_rd_device_bytes equals the library's count of live bytes attributable to the object in all three handle cases, does not grow with
    further steps, and the count returns to its start after destroy"""
    live = smg._lib.load().smg_device_bytes_live
    for name, case in (("icosphere3", "two"), ("square", "one"), ("torus", "v alone")):
        V, F = N.shape(name)
        mg = smg.mg_precompute(V, F, 0.25, COARSEST[name], 1)                  # the caller's hierarchy stays alive throughout
        u0, v0, coeff = gray_scott_state(smg, V, 3)
        gc.collect()
        before = live()
        obj = smg.ReactionDiffusion(mg, V, F, dt=0.5, **CASES[case])
        obj.set_state(u0, v0, coeff)
        obj.step(2)
        second = obj.device_bytes()
        obj.step(8)
        counted, held = obj.device_bytes(), live() - before
        print("%s, %s: device_bytes %d after the second step, %d after the tenth, live DevBuf bytes held %d" % (name, case, second, counted, held))
        del obj
        gc.collect()
        assert 0 < counted == held and counted == second and live() == before


def test_live_refusals(smg, meshes):
    """the refusals that need an object: code and text as recorded in tests/golden/rd_refusals.json, group "live"; nothing is written"""
    golden = json.load(open(GOLDEN))["live"]
    Lc = smg._lib.load()
    V, F, mg, L = meshes("icosphere3")
    n = V.shape[0]
    u0, v0, coeff = gray_scott_state(smg, V, 2)
    u0, v0 = np.asfortranarray(u0), np.asfortranarray(v0)
    out = np.full((n, 2), N.SENTINEL, order="F")
    cp = coeff.ctypes.data_as(C.POINTER(C.c_double))
    cbad = coeff.copy()
    cbad[1, 13] = np.inf
    empty, obj = smg.ReactionDiffusion(mg, V, F, dt=0.5, **CASES["two"]), smg.ReactionDiffusion(mg, V, F, dt=0.5, **CASES["two"])
    obj.set_state(u0, v0, coeff)
    p = obj.params

    def setp(**kw):
        q = type(p)(*[getattr(p, f) for f, _ in p._fields_])
        for key, val in kw.items():
            setattr(q, key, val)
        return Lc.smg_rd_set_params(obj.o, C.byref(q))
    U, W, O = u0.ctypes.data, v0.ctypes.data, out.ctypes.data
    calls = {"set_state null block": lambda: Lc.smg_rd_set_state(empty.o, U, None, n, 2, cp, 0),
             "set_state null coefficients": lambda: Lc.smg_rd_set_state(empty.o, U, W, n, 2, None, 0),
             "set_state k zero": lambda: Lc.smg_rd_set_state(empty.o, U, W, n, 0, cp, 0),
             "set_state memspace": lambda: Lc.smg_rd_set_state(empty.o, U, W, n, 2, cp, 2),
             "set_state leading dimension": lambda: Lc.smg_rd_set_state(empty.o, U, W, n - 1, 2, cp, 0),
             "set_state non-finite coefficient": lambda: Lc.smg_rd_set_state(empty.o, U, W, n, 2, cbad.ctypes.data_as(C.POINTER(C.c_double)), 0),
             "step before set_state": lambda: Lc.smg_rd_step(empty.o, 1, None, None, None, None, None),
             "step n_steps zero": lambda: Lc.smg_rd_step(obj.o, 0, None, None, None, None, None),
             "state before set_state": lambda: Lc.smg_rd_state(empty.o, O, O, n, 0),
             "state null block": lambda: Lc.smg_rd_state(obj.o, O, None, n, 0),
             "state memspace": lambda: Lc.smg_rd_state(obj.o, O, O, n, 3),
             "state leading dimension": lambda: Lc.smg_rd_state(obj.o, O, O, n - 1, 0),
             "set_params handle case": lambda: setp(Dv=0.0),
             "set_params dt": lambda: setp(dt=0.0)}
    assert set(calls) == set(golden)
    for name, call in calls.items():
        rc = call()
        assert [rc, Lc.smg_last_error().decode()] == golden[name] and rc == INVALID, name
    assert np.all(out == N.SENTINEL)
    u, v = obj.state()
    assert np.array_equal(u, u0) and np.array_equal(v, v0) and obj.params.dt == 0.5


def test_the_timing_hook_times_both_launchers(smg):
    """smg_debug_rd_time: a positive time for both launchers on a mesh of more than one block, k = 3"""
    Lc = smg._lib.load()
    V, F = N.shape("icosphere3")
    Fp, Vp = F.ctypes.data_as(C.POINTER(C.c_int)), V.ctypes.data_as(C.POINTER(C.c_double))
    ms = C.c_double(-1.0)
    for op, n_sub in ((N.RD_REACT, 1), (N.RD_REACT, 4), (N.RD_CLOSE, 1)):
        assert Lc.smg_debug_rd_time(op, V.shape[0], F.shape[0], 3, Fp, Vp, n_sub, 3, C.byref(ms)) == 0 and 0.0 < ms.value < 1e3, (op, ms.value)
