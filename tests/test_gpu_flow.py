"""GPU (-m gpu): the conformalized mean-curvature flow and its sphere map (include/smg.h: smg_flow_*).

The host references are tests/flow_np.py -- the method in the kernels' operation order with direct solves -- and the library's own host twin
(smg_flow_host), which compiles the text the kernels compile.  The kernels are held launcher by launcher (smg_debug_flow, guarded buffers, every
output pre-filled with sentinels): masses, right-hand sides, matrix values, the normalisation, the sphericity's sums, S and sigma bit for bit
against the restatement and against the host twin.  Only +, -, *, / and sqrt occur, so there is nothing to bound.

End to end against the restatement's direct solves at tol = 1e-12 |b|_F, max |U - U_np| / bounding-box diagonal after every step and the same
relative figure for the sphericity history.  By the project's rule (tests/test_gpu_morph.py) the bound is 100 x the maximum measured on an
MI355X rounded up to a power of ten and in no case above 1e-8.  Measured (profiles/flow_gpu_tests.log): positions 2.71e-13
diagonals over 10 steps on the squashed icosphere(3) and 3.47e-14 over 5 steps on bunny_15K_init; sphericity 2.59e-13 and 2.11e-14 relative;
8 to 10 loop entries per solve.  100 x 2.71e-13 rounds up to 1e-10: E2E_BOUND = 1e-10.

Default options (tol = 5e-7, the reference's): 20 steps on bunny_15K_init, then the sphere map.  DEFAULT_REL: the solve stops at an absolute
residual of 5e-7 where |b|_F is about 4e-3, a relative residual near 1e-4 per step on a warm start; the sphericity near the sphere is a
difference of radii that are equal to within 7e-3, so a relative change of the positions of 1e-4 may move it by 1e-4 / 7e-3, about 1.5 %, per step
and the steps contract towards the same limit rather than add up: 10 % is the margin for the sphericity.  sigma1 / sigma2 is a ratio of lengths of
order 1 and moves with the positions themselves: 1 %.  Measured on the MI355X: sphericity 6.837837e-3 against 6.832093e-3 (8.4e-4 relative), mean
sigma1 / sigma2 1.070300 against 1.070294 (6e-6), no flipped face, 4 loop entries in every one of the 20 solves."""
import ctypes as C
import gc
import json

import numpy as np
import pytest

import flow_np as N
from test_arap_host import bbox_diag
from test_flow_host import GOLDEN, INVALID
from test_gpu_parity import smg  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

NONFINITE = -4
E2E_BOUND = 1e-10                   # see the header
DEFAULT_REL = dict(sphericity=0.10, mean_ratio=0.01)       # see the header


def hook_run(smg):
    def run(op, U, F, **kw):
        rc, bad, out = N.hook(smg, op, U, F, **kw)
        assert rc == 0 and bad == 0, (rc, bad)
        return out
    return run


# ---- kernels, launcher by launcher -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", N.LAUNCHER_MESHES)
def test_hook_against_restatement_and_host_twin(smg, name):
    dev = hook_run(smg)
    N.check_launchers(dev, name)
    V, F = N.shape(name)
    U = N.wobbled(name)
    csr = N.cotan_csr(name)
    for op, kw in ((N.FLOW_SYSTEM, dict(csr=csr, delta=0.0125)), (N.FLOW_NORMALIZE, {}), (N.FLOW_SPHERICITY, {}), (N.FLOW_SPHERE, dict(V0=V))):
        rc, host = N.host(smg, op, U, F, **kw)
        assert rc == 0 and np.array_equal(dev(op, U, F, **kw), host), op


# ---- the objects ----------------------------------------------------------------------------------------------------------------------------------
def build(smg, name, coarsest=50, **params):
    V, F = N.shape(name)
    mg = smg.mg_precompute(V, F, 0.25, coarsest, 1)
    return V, F, mg, smg.MeanCurvatureFlow(mg, V, F, **params)


def reference(smg, name, n_steps, delta=N.DELTA):
    """the restatement's states U_0 .. U_n and its sphericity history, with the library's own L of the normalised rest mesh: the system's bits"""
    V, F = N.shape(name)
    ref = N.FlowNp(V, F, delta=delta, L=smg.mesh.cotmatrix(N.normalize(V, F), F))
    states, his = [ref.U.copy()], []
    for _ in range(n_steps):
        his.append(ref.step(1)[0])
        states.append(ref.U.copy())
    his.append(N.sphericity(ref.U, F)[0])
    return ref, states, np.array(his)


@pytest.fixture(scope="module")
def refs(smg):
    cache = {}

    def get(name, n_steps):
        if name not in cache:
            cache[name] = reference(smg, name, n_steps)
        return cache[name]
    yield get
    cache.clear()
    gc.collect()


def tight(smg, U, F):
    b = N.mass(U, F)[:, None] * U
    return smg.SolveOpts(tol=1e-12 * float(np.linalg.norm(b)), max_iter=100)


@pytest.mark.parametrize("name,n_steps,coarsest", [("squashed", 10, 50), ("bunny_15K_init.smgm", 5, 500)])
def test_end_to_end_against_direct_solves(smg, refs, name, n_steps, coarsest):
    V, F, mg, flow = build(smg, name, coarsest)
    _, states, his_np = refs(name, 20 if name.startswith("bunny") else n_steps)
    assert np.array_equal(flow.positions(), states[0])                      # the rest mesh is normalised by the step's own kernel
    worst_u = worst_s = 0.0
    for t in range(n_steps):
        his, cyc = flow.step(1, opts=tight(smg, states[t], F))
        U = flow.positions()
        eu = np.abs(U - states[t + 1]).max() / bbox_diag(states[t + 1])
        es = max(abs(his[0] - his_np[t]) / his_np[t], abs(his[1] - his_np[t + 1]) / his_np[t + 1])
        print("%s step %d: %d cycles, max |U - U_np| / diagonal = %.2e, sphericity %.6e (restatement %.6e, relative %.2e)"
              % (name, t, cyc[0], eu, his[1], his_np[t + 1], es))
        worst_u, worst_s = max(worst_u, eu), max(worst_s, es)
        assert cyc[0] < 100
    print("%s: maxima over %d steps: positions %.2e diagonals, sphericity %.2e relative (bound %.0e)" % (name, n_steps, worst_u, worst_s, E2E_BOUND))
    assert worst_u <= E2E_BOUND and worst_s <= E2E_BOUND


def test_default_options_reach_the_sphere(smg, refs):
    name = "bunny_15K_init.smgm"
    V, F, mg, flow = build(smg, name, 500)
    ref, states, his_np = refs(name, 20)
    his, cyc = flow.step(20)
    S, sigma, stats = flow.sphere()
    _, sig_np, _, stats_np = N.sphere(states[20], ref.V0, F)
    max_iter = smg.SolveOpts().c.max_iter
    print("default options: sphericity %.6e (restatement %.6e), mean sigma1 / sigma2 %.6f (restatement %.6f), max %.3f, flipped %d, cycles %s"
          % (his[-1], his_np[-1], stats["mean_ratio"], stats_np[0], stats["max_ratio"], stats["flipped"], cyc.tolist()))
    assert his.size == 21 and cyc.size == 20 and stats["flipped"] == 0
    assert abs(his[-1] - his_np[-1]) <= DEFAULT_REL["sphericity"] * his_np[-1]
    assert abs(stats["mean_ratio"] - stats_np[0]) <= DEFAULT_REL["mean_ratio"] * stats_np[0]
    assert np.all(cyc < max_iter) and stats["sphericity"] == his[-1]
    assert np.abs(np.linalg.norm(S, axis=1) - 1.0).max() <= 4 * N.EPS and np.all(sigma[:, 0] >= sigma[:, 1]) and np.all(sigma[:, 1] > 0.0)


# ---- the value-only path, determinism, memory ------------------------------------------------------------------------------------------------------
def test_value_only_steps_and_set_params(smg):
    V, F, mg, a = build(smg, "squashed")
    a.step(2)
    after_two = a.device_bytes()
    a.step(1)
    U3 = a.positions()
    a.step(7)
    assert a.device_bytes() == after_two                                     # ten steps allocate nothing after the second
    a.set_positions(U3)
    a.set_params(delta=0.02)
    his_a, cyc_a = a.step(2)
    b = smg.MeanCurvatureFlow(mg, V, F, delta=0.02)                           # a fresh object created with that delta, brought to the same state
    b.set_positions(U3)
    his_b, cyc_b = b.step(2)
    assert np.array_equal(his_a, his_b) and np.array_equal(cyc_a, cyc_b) and np.array_equal(a.positions(), b.positions())
    a.set_params(delta=0.01)
    a.set_positions(U3)
    assert not np.array_equal(a.step(2)[0], his_a)                           # and the step does depend on delta


@pytest.mark.parametrize("pcg", [1, 0])
def test_same_calls_same_bits(smg, pcg):
    V, F = N.shape("squashed")
    mg = smg.mg_precompute(V, F, 0.25, 50, 1)
    runs = []
    for _ in range(2):
        flow = smg.MeanCurvatureFlow(mg, V, F)
        flow.set_solver(pcg)
        his, cyc = flow.step(4)
        S, sigma, stats = flow.sphere()
        runs.append((his, cyc, flow.positions(), S, sigma, np.array(list(stats.values()), dtype=np.float64)))
    for x, y in zip(*runs):
        assert np.array_equal(x, y)


def test_device_bytes_are_live_buffers_and_destroy_frees_them(smg):
    live = smg._lib.load().smg_device_bytes_live
    V, F = N.shape("squashed")
    mg = smg.mg_precompute(V, F, 0.25, 50, 1)                                  # the caller's hierarchy stays alive throughout
    gc.collect()
    before = live()
    flow = smg.MeanCurvatureFlow(mg, V, F)
    flow.step(2)
    flow.sphere()
    counted, held = flow.device_bytes(), live() - before
    print("flow: device_bytes %d, live DevBuf bytes held %d" % (counted, held))
    del flow
    gc.collect()
    assert 0 < counted == held and live() == before


# ---- the ends of a call ----------------------------------------------------------------------------------------------------------------------------
def raw_step(smg, flow, n, his_len=None):
    """smg_flow_step through the C ABI on sentinel-filled arrays -> (rc, n_done, his, cycles)"""
    L = smg._lib.load()
    his = np.full(his_len or n + 1, N.SENTINEL)
    cyc = np.full(max(n, 1), -77, dtype=np.int32)
    done = C.c_int(-5)
    rc = L.smg_flow_step(flow.f, n, None, his.ctypes.data_as(C.POINTER(C.c_double)), cyc.ctypes.data_as(C.POINTER(C.c_int)), C.byref(done))
    return rc, done.value, his, cyc


def test_non_finite_state_is_refused_and_reset_recovers(smg):
    V, F, mg, flow = build(smg, "squashed")
    fresh = smg.MeanCurvatureFlow(mg, V, F)
    want = fresh.step(2)
    U = flow.positions()
    U[17, 1] = np.nan
    flow.set_positions(U)
    rc, done, his, cyc = raw_step(smg, flow, 3)
    assert rc == NONFINITE and done == 0
    assert smg._lib.load().smg_last_error().decode() == "smg_flow_step: non-finite sphericity at step 0"
    assert np.isnan(his[0]) and np.all(his[1:] == N.SENTINEL) and np.all(cyc == -77)
    flow.reset()
    got = flow.step(2)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(flow.positions(), fresh.positions())
    # no array at all, and n_steps = 0 only measures
    assert smg._lib.load().smg_flow_step(flow.f, 1, None, None, None, None) == 0
    rc, done, his, cyc = raw_step(smg, flow, 0)
    assert rc == 0 and done == 0 and np.isfinite(his[0]) and his[0] != N.SENTINEL and np.all(cyc == -77)


def test_stop_sphericity_ends_the_call(smg):
    V, F, mg, flow = build(smg, "squashed")
    his, cyc = flow.step(6)
    stop = 0.5 * (his[3] + his[4])
    assert np.all(his[:4] > stop) and his[4] <= stop                           # the history is not monotone (it rises on the first step): step 4 is the first at or below
    flow.reset()
    flow.set_params(stop_sphericity=stop)
    got, cyc2 = flow.step(6)
    assert got.size == 5 and cyc2.size == 4 and np.array_equal(got, his[:5]) and np.array_equal(cyc2, cyc[:4])
    again, none = flow.step(3)                                                 # already below: nothing is done
    assert again.size == 1 and none.size == 0 and again[0] == his[4]


def test_host_and_device_blocks(smg):
    import torch
    V, F, mg, flow = build(smg, "squashed")
    L = smg._lib.load()
    n = V.shape[0]
    flow.step(1)
    U = flow.positions()
    ld = n + 5
    Up = np.full((ld, 3), -2.0, order="F")
    assert L.smg_flow_positions(flow.f, 0, Up.ctypes.data, ld) == 0
    assert np.array_equal(Up[:n], U) and np.all(Up[n:] == -2.0)
    Ud = torch.full((3, ld), -1.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    flow.positions_device(Ud.data_ptr(), ld)
    got = Ud.cpu().numpy()
    assert np.array_equal(got[:, :n].T, U) and np.all(got[:, n:] == -1.0)
    want = flow.step(2)
    end = flow.positions()
    for setter in (lambda: L.smg_flow_set_positions(flow.f, Up.ctypes.data, ld, 0), lambda: flow.set_positions_device(Ud.data_ptr(), ld)):
        flow.reset()
        assert setter() in (0, None)
        assert np.array_equal(flow.positions(), U)
        got = flow.step(2)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(flow.positions(), end)
    # the sphere map into device blocks equals the one into host blocks
    S, sigma, stats = flow.sphere()
    Sd = torch.full((3, ld), -1.0, dtype=torch.float64, device="cuda")
    sd = torch.zeros((2, F.shape[0]), dtype=torch.float64, device="cuda")
    st = np.zeros(4)
    torch.cuda.synchronize()
    assert L.smg_flow_sphere(flow.f, 1, Sd.data_ptr(), ld, sd.data_ptr(), st.ctypes.data_as(C.POINTER(C.c_double))) == 0
    assert np.array_equal(Sd.cpu().numpy()[:, :n].T, S) and np.array_equal(sd.cpu().numpy().T, sigma) and st[0] == stats["mean_ratio"]


def test_live_refusals(smg):
    """the refusals that need an object: code and text as recorded in tests/golden/flow_refusals.json, group "live"; the state is left alone"""
    golden = json.load(open(GOLDEN))["live"]
    L = smg._lib.load()
    V, F, mg, flow = build(smg, "squashed")
    Vs, Fs, mgs, square = build(smg, "square", 20)                             # 169 vertices: a coarsest level of 20 leaves two levels
    Vt, Ft, mgt, torus = build(smg, "torus")
    n = V.shape[0]
    X, st = np.zeros((n, 3), order="F"), np.zeros(4)
    dp = C.POINTER(C.c_double)
    p2 = smg._lib.FlowParamsC(0.01, 0, 0.0)
    p3 = smg._lib.FlowParamsC(0.0, 1, 0.0)
    calls = {
        "step with n_steps < 0": lambda: L.smg_flow_step(flow.f, -1, None, None, None, None),
        "positions with a bad memspace": lambda: L.smg_flow_positions(flow.f, 2, X.ctypes.data, n),
        "set_positions with a bad memspace": lambda: L.smg_flow_set_positions(flow.f, X.ctypes.data, n, -1),
        "positions with ld < nV": lambda: L.smg_flow_positions(flow.f, 0, X.ctypes.data, n - 1),
        "set_positions with ld < nV": lambda: L.smg_flow_set_positions(flow.f, X.ctypes.data, n - 1, 0),
        "sphere with a bad memspace": lambda: L.smg_flow_sphere(flow.f, 2, X.ctypes.data, n, None, st.ctypes.data_as(dp)),
        "sphere with ld < nV": lambda: L.smg_flow_sphere(flow.f, 0, X.ctypes.data, n - 1, None, st.ctypes.data_as(dp)),
        "sphere without stats": lambda: L.smg_flow_sphere(flow.f, 0, X.ctypes.data, n, None, None),
        "sphere on the flat square": lambda: L.smg_flow_sphere(square.f, 0, None, 0, None, st.ctypes.data_as(dp)),
        "sphere on the torus": lambda: L.smg_flow_sphere(torus.f, 0, None, 0, None, st.ctypes.data_as(dp)),
        "set_params with another normalize": lambda: L.smg_flow_set_params(flow.f, C.byref(p2)),
        "set_params with delta = 0": lambda: L.smg_flow_set_params(flow.f, C.byref(p3)),
    }
    assert set(calls) == set(golden)
    before = flow.positions()
    for name, call in calls.items():
        rc = call()
        assert [rc, L.smg_last_error().decode()] == golden[name] and rc == INVALID, name
    assert np.array_equal(flow.positions(), before)
    # the flow itself runs on a mesh with a boundary and on a torus: only the sphere map is refused
    assert np.all(np.isfinite(square.step(2)[0])) and np.all(np.isfinite(torus.step(2)[0]))
