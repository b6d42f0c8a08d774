"""GPU (-m gpu): incompressible flow on a surface in vorticity form (include/smg.h: smg_fluid_*).

The host references are tests/fluid_np.py -- the method in the kernels' operation order with direct solves -- and the library's own host twin
(smg_fluid_host), which compiles the text the kernels compile.  The kernels are held launcher by launcher (smg_debug_fluid, guarded buffers, every
output pre-filled with sentinels): masses, right-hand sides, both forms of the transport with each (a, b) pair, the velocity, the diagnostics' terms,
every sum and maximum and the step's closing arithmetic bit for bit against the restatement and against the host twin.  Only +, -, *, /, max and
fabs occur, so there is nothing to bound.

End to end against FluidNp's direct solves (the library's own L).  lambda = lambda_min(-L) over the unknown rows from scipy.sparse.linalg.eigsh
inside the test; tol = the solve's absolute tolerance; res_np = the direct solve's residual; | | is the maximum norm unless marked; eps = 2^-52;
G = 2 deg + 32 as in tests/test_fluid_host.py; nseg_i = the segments of vertex i; D_i = sum over i's segments of |w_nbr - w_i|.

    PSI      |psi_dev - psi_np|_2 <= e_psi = (10 tol + res_np) / lambda for equal right-hand sides           (the issue's statement)
    PHI      |dPhi| <= (2/3) |dpsi| per segment: Phi_ij = (psi_i + psi_j) / 6 - psi_k / 3
    STAGE    one Euler stage from equal w: |out_dev - out_np|_i <= (dt / m_i) (1/2) (1 + theta) (2/3) e_psi D_i + G eps (|w_i| + dt |adv_i|)
    RATE     |rate_dev - rate_np|_i <= (nseg_i / m_i) (2/3) e_psi + G eps rate_i;  the maximum and the reported cfl = dt rmax follow, and with
             an adaptive step |dt_dev - dt_np| <= cfl |d rmax| / (rmax_np (rmax_np - |d rmax|))
    STEPS    states that differ by at most E = |w_dev - w_np| at the start of a stage (w_n included) differ after it by at most
             (1 + 2 dt (1 + theta) rmax) E + max_i (dt C_i) |dpsi| + |d dt| max_i |adv_i| + G eps max |w|:
               d out_i = dw_i - (dt / m_i) sum (1/2) (Phi - theta |Phi|) (dw_nbr - dw_i)          <= (1 + 2 dt (1 + theta) rate_i) E
                         - (dt / m_i) sum (1/2) d(Phi - theta |Phi|) (w_nbr - w_i)                <= dt C_i |dpsi|,  C_i = (1 + theta) D_i / (3 m_i)
                         + d(dt) adv_i   (adaptive)                                               <= |d dt| |adv_i|, |d dt| of RATE
             (the segments' |Phi| sum to 2 m_i rate_i, inflow being outflow), and |dpsi|_2 <= (2 |m|_2 E + 10 tol + res_np) / lambda because
             the right-hand sides differ by m (dw - dwbar).  A Shu-Osher stage is a convex combination of w_n and such a stage, so the running
             maximum E over the stages obeys the same recursion (walk_step: every term from the restatement's state at that stage).  The factor
             2 |m|_2 / lambda makes E grow by orders of magnitude per step: chained over ten steps from E = 0 the test prints it beside the
             observed error and asserts it, but it exceeds 1e-3 max |w| from the first step on.
    LINEAR   the same recursion's E-free part, B = max_i (dt C_i) e_psi + |d dt|(e_psi) max |adv| + G eps max |w| per stage -- each stage's own
             one-stage bound -- summed over the stages run so far.  It is a first-order estimate, NOT a bound: it neglects how a stage amplifies
             the errors of the earlier ones.  It stays below 1e-3 max |w| over ten steps and is asserted beside STEPS, so that those tests can fail.
    HISTORY  a step that starts from states e_n = |w_dev - w_np| apart (read back before the step) reports cfl and dt within the RATE bounds of
             its stages, E chained through the step's stages from e_n by STEPS; the time after step n is within the sum of the |d dt| so far.
             This is the one-stage bound evaluated at every step on the restatement's state, with the observed distance of the two starts.
    COLUMNS  k columns of one run against k single runs: both are the same steps with their own solves, within twice STEPS and twice LINEAR."""
import ctypes as C
import gc
import json

import numpy as np
import pytest

import fluid_np as N
from test_fluid_host import GOLDEN, INVALID, degree
from test_gpu_parity import smg  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

EPS = N.EPS
COARSEST = {"icosphere3": 50, "torus": 50, "square": 20, "square, one level": 500}
NONFINITE = -4


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
    """every launcher alone, k = 1, 3, 8, theta = 0, 0.3, 1: no guard touched, nothing past the extent, nothing of it left at the sentinel
    (fluid_np._call)"""
    for k, theta in ((1, 0.0), (3, 0.3), (8, 1.0)):
        dev = N.check_launchers(hook_run(smg), name, k, theta)
        hst = N.check_launchers(host_run(smg), name, k, theta)
        for op, (a, b) in enumerate(zip(dev, hst)):
            assert np.array_equal(a, b), (name, k, op)


# ---- the objects ----------------------------------------------------------------------------------------------------------------------------------
def initial(V, k):
    """nV x k: w = z in the first column, smooth fields of the positions in the others"""
    w = N.hodge_np.potentials(V, k)[1].copy()
    w[:, 0] = V[:, 2] if np.ptp(V[:, 2]) > 0 else np.sin(5.0 * V[:, 0]) * np.cos(4.0 * V[:, 1])
    return np.ascontiguousarray(w)


def build(smg, case, **params):
    name = case.split(",")[0]
    V, F = N.shape(name)
    mg = smg.mg_precompute(V, F, 0.25, COARSEST[case], 1)
    assert (mg.n_levels == 1) == case.endswith("one level")
    L = smg.mesh.cotmatrix(V, F)                                               # the library's own L: the system's bits
    return V, F, mg, L


@pytest.fixture(scope="module")
def meshes(smg):
    cache = {}

    def get(case):
        if case not in cache:
            cache[case] = build(smg, case)
        return cache[case]
    yield get
    cache.clear()
    gc.collect()


def sensitivities(ref, psi, w, theta):
    """(C_i, nseg_i / m_i, |adv_i|, rate, rmax) of the header at one stage of the restatement"""
    V, F, m = ref.V, ref.F, ref.m
    vi, vj, vk = F.reshape(-1), F[:, [1, 2, 0]].reshape(-1), F[:, [2, 0, 1]].reshape(-1)
    D = np.zeros(w.shape)
    np.add.at(D, vi, np.abs(w[vj] - w[vi]) + np.abs(w[vk] - w[vi]))
    nseg = 2.0 * np.bincount(vi, minlength=V.shape[0])
    out, rate, _, rmax, _ = N.advect(V, F, psi, w, w, 0.0, 1.0, np.ones(w.shape[1]), theta, m=m, lists=ref.lists)
    adv = np.abs(out - w)
    Ci = (1.0 + theta) * D / (3.0 * m[:, None])
    return Ci, nseg / m, adv, rate.T, rmax


@pytest.mark.parametrize("case", ["icosphere3", "square", "square, one level"])
def test_one_euler_stage_against_direct_solves(smg, meshes, case):
    """PSI, PHI, STAGE and RATE of the header: stages = 1, a fixed step, tol = 1e-12 |rhs|_F"""
    V, F, mg, L = meshes(case)
    n, k, theta, dt = V.shape[0], 3, 0.3, 0.02
    w0 = initial(V, k)
    ref = N.FluidNp(V, F, L=L, theta=theta, stages=1, dt=dt)
    ref.set_vorticity(w0)
    r = N.rhs(V, F, w0, m=(ref.m, ref.msum))
    tol = 1e-12 * np.sqrt(r[6])
    psi_np = ref.stream()
    res_np = float(np.linalg.norm(r[4][ref.I] - ref.Auu @ psi_np[ref.I]))
    lam = ref.lam_min()
    e_psi = (10.0 * tol + res_np) / lam
    obj = smg.SurfaceFluid(mg, V, F, theta=theta, stages=1, dt=dt)
    obj.set_vorticity(w0)
    opts = smg.SolveOpts(tol=tol, max_iter=100)
    psi = obj.stream(opts=opts)
    cfl, time, cyc = obj.step(1, opts=opts)
    out = obj.vorticity()
    cfl_np, time_np = ref.step(1)
    Ci, sm, adv, rate, rmax = sensitivities(ref, psi_np, w0, theta)
    G = 2 * degree(F, n) + 32
    d_psi = np.linalg.norm(psi - psi_np)
    bound = dt * Ci * e_psi + G * EPS * (np.abs(w0) + dt * adv)
    err = np.abs(out - ref.w)
    d_rate = sm.max() * (2.0 / 3.0) * e_psi + G * EPS * rmax
    print("%s: lambda_min %.3e, tol %.2e, res_np %.2e; |dpsi|_2 %.3e over e_psi %.3e = %.3f; max |out - out_np| %.3e, largest ratio to its bound %.3f; "
          "|cfl - cfl_np| %s (bound %s); cycles %s" % (case, lam, tol, res_np, d_psi, e_psi, d_psi / e_psi, err.max(), float(np.max(err / bound)),
                                                       np.abs(cfl - cfl_np)[0], dt * d_rate, cyc))
    assert d_psi <= e_psi
    assert np.all(err <= bound)
    assert np.all(np.abs(cfl - cfl_np) <= dt * d_rate) and np.array_equal(time, time_np)
    known, nb = N.known_rows(F, n)
    assert np.all(psi[known] == 0.0) and obj.closed == (nb == 0)


def walk_step(ref, lam, E, rel_tol=1e-10):
    """one step of the restatement `ref` (adaptive dt), stage by stage, with STEPS, LINEAR and HISTORY of the header from its state at every stage.
    E: the distance of the two states at the step's start.  Advances ref.  Returns (E after the step, the sum of the stages' B, the bounds on
    |dt_dev - dt_np| and on |cfl_dev - cfl_np| per column, the step's cfl and times)"""
    V, F, p = ref.V, ref.F, ref.p
    n, theta, m2 = V.shape[0], p["theta"], float(np.linalg.norm(ref.m))
    G = 2 * degree(F, n) + 32
    wn = ref.w
    w, dtv, d_dt, d_dt0, rm0, Bsum, d_cfl = wn, None, None, None, None, 0.0, 0.0

    def step_of(rm, d_rate):
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(d_rate < rm, p["cfl"] * d_rate / (rm * (rm - d_rate)), np.inf) + 4 * EPS * p["cfl"] / rm
    for s, (a, b) in enumerate(N.PAIRS[p["stages"]]):
        r = N.rhs(V, F, w, m=(ref.m, ref.msum))
        tol = rel_tol * np.sqrt(r[6])
        psi = ref.stream(w)
        res_np = float(np.linalg.norm(r[4][ref.I] - ref.Auu @ psi[ref.I]))
        Ci, sm, adv, rate, rmax = sensitivities(ref, psi, w, theta)
        e_psi = (10.0 * tol + res_np) / lam                                  # equal states
        dpsi = e_psi + 2.0 * m2 * E / lam                                    # states E apart
        d_rate, d_rate0 = sm.max() * (2.0 / 3.0) * dpsi + G * EPS * rmax, sm.max() * (2.0 / 3.0) * e_psi + G * EPS * rmax
        if s == 0:
            rm0 = rmax
            dtv = p["cfl"] / rm0
            d_dt, d_dt0 = step_of(rm0, d_rate), step_of(rm0, d_rate0)
        d_cfl = np.maximum(d_cfl, d_dt * rmax + dtv * d_rate + d_dt * d_rate + 4 * EPS * dtv * rmax)
        dtC, round_ = float(np.max(dtv[None, :] * Ci)), G * EPS * float(np.abs(w).max())
        Bsum += dtC * e_psi + float(np.max(d_dt0)) * float(adv.max()) + round_
        E = (1.0 + 2.0 * (1.0 + theta) * float(np.max(dtv * rmax))) * E + dtC * dpsi + float(np.max(d_dt)) * float(adv.max()) + round_
        w = N.advect(V, F, psi, w, wn, a, b, dtv, theta, m=ref.m, lists=ref.lists)[0]
    cfl_np, time_np = ref.step(1)
    assert np.array_equal(ref.w, w)
    return E, Bsum, d_dt, d_cfl, cfl_np[0], time_np[0]


def steps_bound(V, F, L, w0, steps):
    """(STEPS chained from E = 0 after every step, LINEAR after every step, the restatement after them), default parameters"""
    ref = N.FluidNp(V, F, L=L)
    ref.set_vorticity(w0)
    lam = ref.lam_min()
    E, lin, Es, lins = 0.0, 0.0, [], []
    for step in range(steps):
        E, B = walk_step(ref, lam, E)[:2]
        lin += B
        Es.append(E)
        lins.append(lin)
    return Es, lins, ref


def test_ten_default_steps_follow_the_recursion(smg, meshes):
    """STEPS and LINEAR of the header on icosphere(3), k = 2: the observed error beside both after every step"""
    V, F, mg, L = meshes("icosphere3")
    w0 = initial(V, 2)
    Es, lins, _ = steps_bound(V, F, L, w0, 10)
    ref = N.FluidNp(V, F, L=L)
    ref.set_vorticity(w0)
    obj = smg.SurfaceFluid(mg, V, F)
    obj.set_vorticity(w0)
    worst = 0.0
    for step, (E, lin) in enumerate(zip(Es, lins)):
        ref.step(1)
        cfl, time, cyc = obj.step(1)
        err = float(np.max(np.abs(obj.vorticity() - ref.w)))
        worst = max(worst, err / lin)
        print("step %d: max |w - w_np| %.3e, STEPS %.3e, LINEAR %.3e (%.1e max |w|), cycles %d, cfl %s, time %s" % (step + 1, err, E, lin, lin / np.abs(w0).max(),
                                                                                                         cyc[0], cfl[0], time[0]))
        assert err <= E and err <= lin
    assert lins[-1] <= 1e-3 * np.abs(w0).max()
    print("ten default steps: largest observed error over LINEAR %.3e" % worst)


@pytest.mark.parametrize("case", ["icosphere3", "torus", "square"])
def test_invariants_over_twenty_steps(smg, meshes, case):
    """the reported cfl and time of every step against the restatement's within HISTORY of the header; and on the device's own output: the
    circulation to its rounding bound (CIRCULATION of tests/test_fluid_host.py, summed over the stages, with the state's own extremes), and
    with theta = 1 and cfl = 0.5 the maximum principle with every reported cfl <= 1"""
    V, F, mg, L = meshes(case)
    n, k = V.shape[0], 2
    w0 = initial(V, k)
    m, msum = N.mass(V, F)
    G = 2 * degree(F, n) + 32
    for theta in (0.0, 1.0):
        obj = smg.SurfaceFluid(mg, V, F, theta=theta)
        obj.set_vorticity(w0)
        c0 = obj.diagnostics()["circulation"]
        ref = N.FluidNp(V, F, L=L, theta=theta)
        ref.set_vorticity(w0)
        lam = ref.lam_min()
        cfl, time, cyc, sum_dt, ratio, e_max = [], [], [], 0.0, 0.0, 0.0
        for step in range(20):                                                # HISTORY of the header, step by step
            e_n = float(np.max(np.abs(obj.vorticity() - ref.w)))
            _, _, d_dt, d_cfl, cfl_np, time_np = walk_step(ref, lam, e_n)
            c1, t1, y1 = obj.step(1)
            sum_dt = sum_dt + d_dt
            d_time = sum_dt + 4 * EPS * (step + 1) * time_np
            assert np.all(np.abs(c1[0] - cfl_np) <= d_cfl) and np.all(np.abs(t1[0] - time_np) <= d_time), (case, theta, step)
            ratio = max(ratio, float(np.max(np.abs(c1[0] - cfl_np) / d_cfl)), float(np.max(np.abs(t1[0] - time_np) / d_time)))
            e_max = max(e_max, e_n)
            cfl.append(c1[0]), time.append(t1[0]), cyc.append(y1[0])
        cfl, time, cyc = np.array(cfl), np.array(time), np.array(cyc)
        print("%s theta %.0f: cfl and time against the restatement over 20 steps: largest ratio to the HISTORY bound %.3e (largest |w - w_np| at a step's start %.2e, "
              "last |cfl - cfl_np| %s, |time - time_np| %s)" % (case, theta, ratio, e_max, np.abs(c1[0] - cfl_np), np.abs(t1[0] - time_np)))
        w = obj.vorticity()
        d = obj.diagnostics()
        # per stage G eps (sum m |w| + dt sum_i sum_s |t_s|) with dt sum_s |t_s| <= dt (1 + theta) 2 m_i rate_i max |w| <= 4 m_i max |w| at a stage's
        # cfl <= 1: 5 G eps sum(m) max |w|; max |w| of the stages is taken as at most twice the larger of the first and the last state's
        scale = msum * 2.0 * max(np.abs(w0).max(), np.abs(w).max())
        bound = 20 * 3 * 5 * G * EPS * scale
        print("%s theta %.0f: circulation %s -> %s (bound on the change %.2e), enstrophy %s, energy %s, cfl in [%.3f, %.3f], time %s, cycles %d .. %d"
              % (case, theta, c0, d["circulation"], bound, d["enstrophy"], d["energy"], cfl.min(), cfl.max(), time[-1], cyc.min(), cyc.max()))
        assert cfl.shape == (20, k) and np.all(np.diff(time, axis=0) > 0.0)
        assert np.all(np.abs(d["circulation"] - c0) <= bound)
        if theta == 1.0:
            tol = 60 * G * EPS * np.abs(w0).max()
            assert np.all(cfl <= 1.0)
            assert np.all(w <= w0.max(axis=0) + tol) and np.all(w >= w0.min(axis=0) - tol)
        assert np.array_equal(d["circulation"], N.diag(m, w)[2]) and np.array_equal(d["enstrophy"], N.diag(m, w)[3])


def test_columns_of_one_run_against_single_runs(smg, meshes):
    """COLUMNS of the header: k = 1, 3 and 8 columns as one run of three steps against single-column runs, within twice STEPS and twice LINEAR"""
    V, F, mg, L = meshes("icosphere3")
    w0 = initial(V, 8)
    Es, lins, ref = steps_bound(V, F, L, w0, 3)
    singles = []
    for c in range(8):
        o = smg.SurfaceFluid(mg, V, F)
        o.set_vorticity(w0[:, c])
        o.step(3)
        singles.append(o.vorticity()[:, 0])
    singles = np.stack(singles, axis=1)
    for k in (1, 3, 8):
        o = smg.SurfaceFluid(mg, V, F)
        o.set_vorticity(w0[:, :k])
        o.step(3)
        w = o.vorticity()
        d = np.abs(w - singles[:, :k]).max()
        print("k = %d: max |block - singles| %.3e, twice STEPS %.3e, twice LINEAR %.3e; against the restatement: block %.3e, singles %.3e"
              % (k, d, 2 * Es[-1], 2 * lins[-1], np.abs(w - ref.w[:, :k]).max(), np.abs(singles - ref.w).max()))
        assert d <= 2 * Es[-1] and d <= 2 * lins[-1]


def test_fixed_against_adaptive_step(smg, meshes):
    """a fixed dt equal to the adaptive run's first dt gives the first step's bits; set_params switches between the two"""
    V, F, mg, L = meshes("icosphere3")
    w0 = initial(V, 1)
    a = smg.SurfaceFluid(mg, V, F)
    a.set_vorticity(w0)
    cfl, time, _ = a.step(1)
    wa = a.vorticity()
    b = smg.SurfaceFluid(mg, V, F, dt=float(time[0, 0]))
    b.set_vorticity(w0)
    cfl_b, time_b, _ = b.step(1)
    assert np.array_equal(b.vorticity(), wa) and np.array_equal(time_b, time) and np.array_equal(cfl_b, cfl)
    b.set_params(dt=0.0)
    a.step(1)
    b.step(1)
    assert np.array_equal(b.vorticity(), a.vorticity())


def test_viscosity_on_the_torus(smg, meshes):
    """enstrophy does not increase, the circulation stays within the solves' tolerance; set_params re-precomputes by values; zero and non-zero
    viscosity cannot change"""
    V, F, mg, L = meshes("torus")
    w0 = initial(V, 2)
    m, msum = N.mass(V, F)
    obj = smg.SurfaceFluid(mg, V, F, viscosity=0.05, dt=0.02, theta=1.0)
    obj.set_vorticity(w0)
    d0 = obj.diagnostics()
    ens = [d0["enstrophy"]]
    for _ in range(5):
        obj.step(1)
        ens.append(obj.diagnostics()["enstrophy"])
    d1 = obj.diagnostics()
    ens = np.array(ens)
    # a stage keeps sum m w whatever psi; a viscous solve with residual r moves it by |sum r| <= sqrt(n) |r|_2, |r|_2 <= 10 tol as in PSI,
    # tol = 1e-10 |m w*|_F <= 1e-10 sqrt(k) |m|_2 max |w0| (upwind stages and the M-matrix solve keep the extremes); plus the sums' rounding
    n, G = V.shape[0], 2 * degree(F, V.shape[0]) + 32
    slack = 5 * (np.sqrt(n) * 10 * 1e-10 * np.sqrt(2.0) * np.linalg.norm(m) + 4 * 5 * G * EPS * msum) * np.abs(w0).max()
    print("torus, viscosity 0.05: enstrophy %s, circulation %s -> %s (slack %.2e)" % (ens[:, 0], d0["circulation"], d1["circulation"], slack))
    assert np.all(np.diff(ens, axis=0) <= 0.0)
    assert np.all(np.abs(d1["circulation"] - d0["circulation"]) <= slack)
    before = obj.diagnostics()["enstrophy"]
    obj.set_params(viscosity=0.5)                                              # re-precomputed by values: ten times the diffusion
    obj.step(1)
    after = obj.diagnostics()["enstrophy"]
    assert np.all(after < before) and np.all(before - after > ens[-2] - ens[-1])
    with pytest.raises(smg.SmgError):
        obj.set_params(viscosity=0.0)


def test_the_kernels_depend_on_psi_alone_whichever_solver_made_it(smg, meshes):
    """psi from PCG and psi from the stationary loop, each fed to the transport launcher through the hook with the same w: the outputs are the
    restatement's on that psi bit for bit, so the two solvers' steps differ by what their psi differ and by nothing else; and a psi that both
    solvers are handed gives the same bits"""
    V, F, mg, L = meshes("icosphere3")
    n, nF, k = V.shape[0], F.shape[0], 2
    w0 = initial(V, k)
    dt = np.array([0.02, 0.03])
    psis = []
    for pcg in (1, 0):
        obj = smg.SurfaceFluid(mg, V, F)
        obj.set_solver(pcg)
        obj.set_vorticity(w0)
        psis.append(np.ascontiguousarray(obj.stream(opts=smg.SolveOpts(tol=1e-9, max_iter=100))))
    assert not np.array_equal(psis[0], psis[1])
    outs = []
    for psi in psis + [psis[0]]:
        out = hook_run(smg)(N.FLUID_ADVECT, V, F, k=k, psi=psi, w=w0, wn=w0, a=0.75, b=0.25, dt=dt, theta=0.3)
        for got, want in zip(N.unpack(N.FLUID_ADVECT, out, n, nF, k), N.advect(V, F, psi, w0, w0, 0.75, 0.25, dt, 0.3)):
            assert np.array_equal(got, want)
        outs.append(out)
    assert np.array_equal(outs[0], outs[2]) and not np.array_equal(outs[0], outs[1])


def test_the_timing_hook_times_every_launcher(smg):
    """smg_debug_fluid_time: a positive time for every launcher on a mesh of more than one block, k = 3; its refusals"""
    Lc = smg._lib.load()
    V, F = N.shape("icosphere3")
    Fp, Vp = F.ctypes.data_as(C.POINTER(C.c_int)), V.ctypes.data_as(C.POINTER(C.c_double))
    n, nF = V.shape[0], F.shape[0]
    ms = C.c_double(-1.0)
    for op, ro in ((N.FLUID_RHS, 0), (N.FLUID_ADVECT, 0), (N.FLUID_ADVECT, 1), (N.FLUID_VELOCITY, 0), (N.FLUID_DIAG, 0)):
        assert Lc.smg_debug_fluid_time(op, n, nF, 3, Fp, Vp, ro, 3, C.byref(ms)) == 0 and 0.0 < ms.value < 1e3, (op, ro, ms.value)
    for bad in ((N.FLUID_DT, n, nF, 3, Fp, Vp, 0, 3, C.byref(ms)), (0, n, nF, 0, Fp, Vp, 0, 3, C.byref(ms)), (0, n, nF, 3, Fp, Vp, 0, 0, C.byref(ms)),
                (0, n, nF, 3, None, Vp, 0, 3, C.byref(ms)), (0, n, nF, 3, Fp, Vp, 0, 3, None), (0, n - 1, nF, 3, Fp, Vp, 0, 3, C.byref(ms))):
        assert Lc.smg_debug_fluid_time(*bad) == INVALID and b"smg_debug_fluid_time: " in Lc.smg_last_error()


def test_same_calls_same_bits(smg, meshes):
    """two objects, the same calls: the same bits, with PCG and with the stationary loop, with graphs on and off"""
    V, F, mg, L = meshes("icosphere3")
    w0 = initial(V, 3)
    for pcg in (1, 0):
        runs = []
        for use_graph in (1, 1, 0):
            obj = smg.SurfaceFluid(mg, V, F)
            obj.set_solver(pcg)
            opts = smg.SolveOpts(tol=1e-9, max_iter=30, use_graph=use_graph)
            obj.set_vorticity(w0)
            a = obj.step(2, opts=opts)
            b = obj.step(1, opts=opts)
            runs.append(list(a) + list(b) + [obj.vorticity(), obj.stream(opts=opts), obj.velocity(opts=opts)])
        for other in runs[1:]:
            for x, y in zip(runs[0], other):
                assert np.array_equal(x, y)


@pytest.fixture(scope="module")
def torch_cuda():
    """torch with its device context open: the import and the first use of the device take about ten seconds when this file runs alone, and
    belong to no test's own time"""
    import torch
    torch.zeros(1, device="cuda")
    torch.cuda.synchronize()
    return torch


def test_host_and_device_blocks(smg, meshes, torch_cuda):
    """SMG_HOST and SMG_DEVICE blocks with padded leading dimensions give the same bits; rows past nV are untouched"""
    torch = torch_cuda
    V, F, mg, L = meshes("square")
    Lc = smg._lib.load()
    n, nF, k, ld = V.shape[0], F.shape[0], 2, V.shape[0] + 5
    w0 = initial(V, k)
    want = smg.SurfaceFluid(mg, V, F)
    want.set_vorticity(w0)
    want.step(2)
    ww, wp = want.vorticity(), want.stream()
    obj = smg.SurfaceFluid(mg, V, F)
    wh = np.full((ld, k), np.nan, order="F")
    wh[:n] = w0
    assert Lc.smg_fluid_set_vorticity(obj.o, wh.ctypes.data, ld, k, 0) == 0
    obj.k = k
    obj.step(2)
    oh = np.full((ld, k), -2.0, order="F")
    assert Lc.smg_fluid_vorticity(obj.o, oh.ctypes.data, ld, 0) == 0
    assert np.array_equal(oh[:n], ww) and np.all(oh[n:] == -2.0)
    wd = torch.full((k, ld), float("nan"), dtype=torch.float64, device="cuda")
    wd[:, :n] = torch.from_numpy(w0.T.copy()).cuda()
    od = torch.full((k, ld), -1.0, dtype=torch.float64, device="cuda")
    pd = torch.full((k, ld), -1.0, dtype=torch.float64, device="cuda")
    ud = torch.zeros((k, nF, 3), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    dev = smg.SurfaceFluid(mg, V, F)
    dev.set_vorticity_device(wd.data_ptr(), ld, k)
    dev.step(2)
    dev.vorticity_device(od.data_ptr(), ld)
    assert Lc.smg_fluid_stream(dev.o, None, pd.data_ptr(), ld, 1) == 0
    assert Lc.smg_fluid_velocity(dev.o, None, ud.data_ptr(), 1) == 0
    got, gp = od.cpu().numpy(), pd.cpu().numpy()
    assert np.array_equal(got[:, :n].T, ww) and np.all(got[:, n:] == -1.0)
    assert np.array_equal(gp[:, :n].T, wp) and np.all(gp[:, n:] == -1.0)
    assert want.velocity().shape == (k, nF, 3) and np.all(np.isfinite(ud.cpu().numpy()))


def test_a_nan_is_refused_and_the_state_is_kept(smg, meshes):
    """one NaN in w: SMG_ERR_NONFINITE, n_done = 0, the state as set; the next run equals a fresh object's"""
    V, F, mg, L = meshes("icosphere3")
    w0 = initial(V, 2)
    obj = smg.SurfaceFluid(mg, V, F)
    obj.set_vorticity(w0)
    obj.step(2)
    bad = w0.copy()
    bad[77, 1] = np.nan
    obj.set_vorticity(bad)
    with pytest.raises(smg.SmgError) as e:
        obj.step(3)
    assert e.value.code == NONFINITE and "smg_fluid_step" in str(e.value) and obj.n_done == 0
    kept = obj.vorticity()
    assert np.array_equal(kept[:, 0], bad[:, 0]) and np.isnan(kept[77, 1]) and np.array_equal(np.delete(kept[:, 1], 77), np.delete(bad[:, 1], 77))
    obj.set_vorticity(w0)
    fresh = smg.SurfaceFluid(mg, V, F)
    fresh.set_vorticity(w0)
    for x, y in zip(obj.step(2), fresh.step(2)):
        assert np.array_equal(x, y)
    assert np.array_equal(obj.vorticity(), fresh.vorticity())


def test_device_bytes_are_live_buffers_and_do_not_grow(smg):
    live = smg._lib.load().smg_device_bytes_live
    for name, params in (("icosphere3", {}), ("square", {}), ("torus", dict(viscosity=0.05, dt=0.02))):
        V, F = N.shape(name)
        mg = smg.mg_precompute(V, F, 0.25, COARSEST[name], 1)                 # the caller's hierarchy stays alive throughout
        w0 = initial(V, 3)
        gc.collect()
        before = live()
        obj = smg.SurfaceFluid(mg, V, F, **params)
        obj.set_vorticity(w0)
        obj.step(1)
        obj.velocity()
        obj.diagnostics()
        obj.step(1)
        second = obj.device_bytes()
        for _ in range(8):
            obj.step(1)
        counted, held = obj.device_bytes(), live() - before
        print("%s: device_bytes %d after the second step, %d after the tenth, live DevBuf bytes held %d" % (name, second, counted, held))
        del obj
        gc.collect()
        assert 0 < counted == held and counted == second and live() == before


def test_live_refusals(smg, meshes):
    """the refusals that need an object: code and text as recorded in tests/golden/fluid_refusals.json, group "live"; nothing is written"""
    golden = json.load(open(GOLDEN))["live"]
    Lc = smg._lib.load()
    V, F, mg, L = meshes("icosphere3")
    n = V.shape[0]
    w = np.asfortranarray(initial(V, 2))
    out = np.full((n, 2), N.SENTINEL, order="F")
    dp = out.ctypes.data_as(C.POINTER(C.c_double))
    empty, obj = smg.SurfaceFluid(mg, V, F), smg.SurfaceFluid(mg, V, F)
    obj.set_vorticity(w)
    p = Lc.smg_fluid_params_default()

    def setp(**kw):
        q = type(p)(*[getattr(p, f) for f, _ in p._fields_])
        for key, val in kw.items():
            setattr(q, key, val)
        return Lc.smg_fluid_set_params(obj.o, C.byref(q))
    calls = {"set_vorticity null block": lambda: Lc.smg_fluid_set_vorticity(empty.o, None, n, 2, 0),
             "set_vorticity k zero": lambda: Lc.smg_fluid_set_vorticity(empty.o, w.ctypes.data, n, 0, 0),
             "set_vorticity memspace": lambda: Lc.smg_fluid_set_vorticity(empty.o, w.ctypes.data, n, 2, 2),
             "set_vorticity leading dimension": lambda: Lc.smg_fluid_set_vorticity(empty.o, w.ctypes.data, n - 1, 2, 0),
             "step before set_vorticity": lambda: Lc.smg_fluid_step(empty.o, 1, None, None, None, None, None),
             "step n_steps zero": lambda: Lc.smg_fluid_step(obj.o, 0, None, None, None, None, None),
             "vorticity before set_vorticity": lambda: Lc.smg_fluid_vorticity(empty.o, out.ctypes.data, n, 0),
             "vorticity null block": lambda: Lc.smg_fluid_vorticity(obj.o, None, n, 0),
             "vorticity leading dimension": lambda: Lc.smg_fluid_vorticity(obj.o, out.ctypes.data, n - 1, 0),
             "stream before set_vorticity": lambda: Lc.smg_fluid_stream(empty.o, None, out.ctypes.data, n, 0),
             "stream memspace": lambda: Lc.smg_fluid_stream(obj.o, None, out.ctypes.data, n, 3),
             "velocity null block": lambda: Lc.smg_fluid_velocity(obj.o, None, None, 0),
             "diagnostics null block": lambda: Lc.smg_fluid_diagnostics(obj.o, None, None),
             "set_params viscosity from zero": lambda: setp(viscosity=0.1, dt=0.1),
             "set_params stages": lambda: setp(stages=4)}
    assert set(calls) == set(golden)
    for name, call in calls.items():
        rc = call()
        assert [rc, Lc.smg_last_error().decode()] == golden[name] and rc == INVALID, name
    assert np.all(out == N.SENTINEL) and dp is not None
    assert np.array_equal(obj.vorticity(), w) and obj.params.stages == 3
