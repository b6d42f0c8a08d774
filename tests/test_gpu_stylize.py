"""GPU (-m gpu): cubic and normal-driven stylization (include/smg.h: smg_stylize_*).

The host references are tests/stylize_np.py -- the method with LAPACK SVDs and direct solves, in the kernels' operation order -- and the library's
own host twin (smg_stylize_local_host), which compiles the text the kernels compile.  The kernels are held launcher by launcher
(smg_debug_stylize, guarded buffers): normals, areas and the energy terms of given rotations bit for bit against the restatement; single ADMM
iterations, the whole local step and the normal-driven fit to the bounds of tests/test_stylize_host.py against the restatement, and bit for bit
against the host twin.

Measured on an MI355X: the device equals the host twin bit for bit on every shape and op (fp64 sqrt and division
included), so its maxima against the restatement are the host twin's (tests/test_stylize_host.py); end to end against the restatement see
E2E_BOUND below; cubeness of the device's result equal to the restatement's in the six digits printed on every case (bound 1e-6)."""
import ctypes as C
import gc
import json
import math

import numpy as np
import pytest

import stylize_np as N
from test_arap_host import bbox_diag, rotation_matrix, rotations_np, twist
from test_gpu_parity import smg  # noqa: F401  (fixture)
from test_stylize_host import GOLDEN, INVALID, check_admm_steps, check_fit, check_local

pytestmark = pytest.mark.gpu

EPS = N.EPS
# end to end at tight inner tolerances against the direct solves of the restatement: 100 x the measured maximum (3.00e-10 diagonals, the
# normal-driven run on icosphere(3), whose system -L with ONE pinned vertex is the worst conditioned of the cases; 2.70e-10 cubic there, 1.27e-12
# on bunny.smgm, 2.49e-12 at 252 834 vertices; energies at most 1.11e-11), rounded up to a power of ten
E2E_BOUND = 1e-7


def hook_run(smg):
    def run(op, A, F, P=None, **kw):
        rc, bad, out, it = N.hook(smg, op, A, F, P, **kw)
        assert rc == 0 and bad == 0, (rc, bad)
        return out, it
    return run


def host_run(smg):
    def run(op, A, F, P=None, **kw):
        rc, out, it = N.local_host(smg, op, A, F, P, **kw)
        assert rc == 0
        return out, it
    return run


# ---- kernels, launcher by launcher ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", N.KERNEL_SHAPES)
def test_hook_against_restatement_and_host_twin(smg, name):
    dev, host = hook_run(smg), host_run(smg)
    V, F = N.shape(name)
    A = N.rest(name)
    n = A.n
    nn, aa = N.vertex_normals_areas(V, F)
    ln, la_ = N.unpack(N.STY_NORMALS, dev(N.STY_NORMALS, A, F)[0], n)
    assert np.array_equal(ln, nn) and np.array_equal(la_, aa)
    # single iterations and the whole local step: the bounds and caps of the host twin's test
    check_admm_steps(dev, name)
    check_admm_steps(dev, name, steps=2, Q=rotation_matrix([1.0, -2.0, 0.5], 0.7), lam=np.linspace(0.0, 0.5, n))
    P = N.noisy_pose(V)
    for lambda_ in (0.2, 0.4):
        it = check_local(dev, name, lambda_)
        # the device against the host twin: the same text, bit for bit
        od, oh = dev(N.STY_LOCAL, A, F, P, lambda_=lambda_), host(N.STY_LOCAL, A, F, P, lambda_=lambda_)
        same = np.array_equal(od[0][:17 * n], oh[0]) and np.array_equal(od[1], oh[1])
        print("  device against host twin, lambda %.1f: bit for bit %s, max |difference| %.2e, counts differ at %d" %
              (lambda_, same, np.abs(od[0][:17 * n] - oh[0]).max(), np.sum(od[1] != oh[1])))
        assert same and np.array_equal(it, oh[1])
    Q, lam = rotation_matrix([1.0, -2.0, 0.5], 0.7), np.linspace(0.0, 0.5, n)
    od, oh = dev(N.STY_LOCAL, A, F, P, Q=Q, lam=lam), host(N.STY_LOCAL, A, F, P, Q=Q, lam=lam)
    assert np.array_equal(od[0], oh[0]) and np.array_equal(od[1], oh[1])
    t = N.nearest_axis(nn)
    od, oh = dev(N.STY_LOCAL_TARGETS, A, F, P, targets=t), host(N.STY_LOCAL_TARGETS, A, F, P, targets=t)
    R, terms = N.unpack(N.STY_LOCAL_TARGETS, od[0], n)
    Rn, _, gap = N.local_targets(A, P, nn, aa, N.params(), t)
    check_fit(name + ", normal-driven", R, Rn, gap)
    assert np.array_equal(terms, N.energy_terms(A, P, R, nn, 0.2 * aa, None, t))
    assert np.array_equal(od[0], oh[0]) and np.all(od[1] == 0)
    # the energy terms of given rotations bit for bit, their sum to the bound of a sum and equal across two calls
    for tgt in (None, t):
        o1, o2 = dev(N.STY_ENERGY, A, F, P, targets=tgt, R_in=Rn)[0], dev(N.STY_ENERGY, A, F, P, targets=tgt, R_in=Rn)[0]
        want = N.energy_terms(A, P, Rn, nn, 0.2 * aa, None, tgt)
        assert np.array_equal(o1[:n], want)
        exact = math.fsum(want)
        print("  reduced energy %.17g, |E - fsum| = %.2e (bound %.2e)" % (o1[n], abs(o1[n] - exact), 2 * n * EPS * np.abs(want).sum()))
        assert o1[n] == o2[n] and abs(o1[n] - exact) <= 2 * n * EPS * np.abs(want).sum()
        assert o1[n] == N.fixed_sum(want)


# ---- end to end -----------------------------------------------------------------------------------------------------------------------------
def build(smg, name, n_sub=0, pins=None, **par):
    if n_sub:
        from oracle import mesh_np as M
        V, F = M.read_smgm(name)
        mg, V, F = smg.mg_precompute_subdiv(N.unit_box(V), F, n_sub, ratio=0.25, nVCoarsest=1000)
    else:
        V, F = N.shape(name)
        mg = smg.mg_precompute(V, F, 0.25, 200, 1)
    return V, F, mg, smg.Stylizer(mg, V, F, pins, **par)


@pytest.fixture(scope="module")
def sphere_case(smg):
    return build(smg, "icosphere3")


@pytest.fixture(scope="module")
def bunny_case(smg):
    return build(smg, "bunny.smgm")


def check_run(smg, V, F, sty, n_iter, targets=None, Q=None):
    ref = N.StylizeNp(V, F, L=smg.mesh.cotmatrix(V, F))                      # the library's own L: the system's bits
    ref.targets, ref.Q = targets, Q
    s = ref.A.scale()
    U, E, cyc = sty.run(max_iter=n_iter, opts=smg.SolveOpts(tol=1e-12 * s, max_iter=100))      # the inner solver is PCG (the default)
    Un, En, counts = ref.run(n_iter=n_iter)
    du = np.abs(U - Un).max() / bbox_diag(V)
    de = np.abs(E - En) / np.abs(En)
    c, cn = N.cubeness(U, F), N.cubeness(Un, F)
    st = sty.admm_stats()
    print("n = %d: max |U - U_np| = %.2e diagonals, energy differences %s, cycles %s, cubeness %.6f (restatement %.6f, rest %.6f), ADMM of the last "
          "local step min %d mean %.2f max %d at the cap %d" % (V.shape[0], du, np.array2string(de, precision=2), cyc, c, cn, N.cubeness(V, F),
                                                               st["min"], st["mean"], st["max"], st["at_cap"]))
    assert E.shape == (n_iter + 1,) and np.all(cyc < 100)
    assert du <= E2E_BOUND and np.all(de <= E2E_BOUND)
    assert abs(c - cn) <= 1e-6
    assert np.sum(st["iters"] != counts[-1]) <= 0.01 * V.shape[0]
    return U, E


@pytest.mark.parametrize("case", ["sphere_case", "bunny_case"])
def test_cubic_run_against_restatement(smg, request, case):
    V, F, mg, sty = request.getfixturevalue(case)
    U, E = check_run(smg, V, F, sty, 6)
    assert np.all(E[1:] < E[:-1]) and N.cubeness(U, F) < N.cubeness(V, F)
    assert np.array_equal(U[0], V[0])                                        # vertex 0 is pinned at its rest position


def test_normal_driven_run_against_restatement(smg, sphere_case):
    V, F, mg, sty = sphere_case
    cubic = sty.run(max_iter=3)
    sty.set_targets(N.nearest_axis(sty.normals()[0]))
    try:
        U, E = check_run(smg, V, F, sty, 6, targets=N.nearest_axis(N.vertex_normals_areas(V, F)[0]))
        assert np.all(E[1:] <= E[:-1]) and sty.admm_stats()["max"] == 0
    finally:
        sty.set_targets(None)
    assert all(np.array_equal(x, y) for x, y in zip(cubic, sty.run(max_iter=3)))      # back in the cubic mode, to the bit


def test_frame_against_restatement(smg, sphere_case):
    V, F, mg, sty = sphere_case
    plain = sty.run(max_iter=3)
    Q = rotation_matrix([1.0, 2.0, -0.5], 1.1)
    sty.set_frame(Q)
    try:
        U, _ = check_run(smg, V, F, sty, 6, Q=Q)
        assert np.abs(U - sty.run(max_iter=0)[0]).max() > 1e-3
    finally:
        sty.set_frame(None)
    assert all(np.array_equal(x, y) for x, y in zip(plain, sty.run(max_iter=3)))


def test_run_full_size(smg):
    V, F, mg, sty = build(smg, "bunny_15K_init.smgm", n_sub=2)
    assert V.shape[0] == 252834 and sty.device_bytes() > 0
    check_run(smg, V, F, sty, 3)


# ---- behaviour ------------------------------------------------------------------------------------------------------------------------------
def test_normals_stats_and_counts(smg, sphere_case):
    """the object's normals and areas are the hook's; after run(max_iter = 0) the counts are those of the hook's local step at the rest pose"""
    V, F, mg, sty = sphere_case
    nn, aa = N.vertex_normals_areas(V, F)
    on, oa = sty.normals()
    assert np.array_equal(on, nn) and np.array_equal(oa, aa)
    sty.run(max_iter=0)
    st = sty.admm_stats()
    A = N.ArapRest(smg.mesh.cotmatrix(V, F), V)
    out, it = hook_run(smg)(N.STY_LOCAL, A, F, np.ascontiguousarray(V))
    assert np.array_equal(st["iters"], it)
    assert (st["min"], st["max"], st["at_cap"]) == (it.min(), it.max(), int(np.sum(it >= 100))) and abs(st["mean"] - it.mean()) <= 1e-12


def test_lambda_zero_is_arap(smg):
    """At lambda = 0 a local step from the start state returns the ARAP fit (two ADMM iterations; the restatement's rotations agree to about
    1e-14), so the run with one outer iteration is ArapDeformer.deform from the same start and pins: held to 1e-9 diagonals.  From the second
    local step on the state is carried, as the method is specified: z of the previous outer iteration enters M = S + rho n z^T, and with
    lambda = 0 both residuals pass the stopping test after ONE iteration (r = 0, s = rho |z - z_old| <= 1e-4 |z - z_old|), so that rotation is
    the ARAP fit only to about rho / sigma(S).  The restatement shows the same: after four outer iterations its lambda = 0 run is 3.6e-5
    diagonals from the ARAP restatement.  Measured on the device: one iteration 1.28e-16 diagonals; four iterations 3.65e-5 (energies 5.1e-5),
    and 1.4e-6 from the restatement's own lambda = 0 run (whether a vertex stops after one iteration or two is a discrete decision there), so
    the four-iteration figures are printed, not bounded.  Per-vertex lambda that is zero on half the sphere leaves that half's rotations of a local step from the
    start state at the ARAP fit (bound 1e-12)."""
    V, F = N.shape("icosphere3")
    mg = smg.mg_precompute(V, F, 0.25, 200, 1)
    handles, hp = twist(V)
    Lc = smg.mesh.cotmatrix(V, F)
    A = N.ArapRest(Lc, V)
    o = smg.SolveOpts(tol=1e-12 * A.scale(), max_iter=100)
    arap, sty = smg.ArapDeformer(mg, V, F, handles), smg.Stylizer(mg, V, F, handles, lambda_=0.0)
    Ua, Ea, _ = arap.deform(hp, max_iter=1, opts=o)
    Us, Es, _ = sty.run(hp, max_iter=1, opts=o)
    du = np.abs(Ua - Us).max() / bbox_diag(V)
    print("lambda = 0 against smg_arap, one iteration: max |U - U_arap| = %.2e diagonals, E_0 %.2e, E_1 %.2e" %
          (du, abs(2.0 * Es[0] - Ea[0]) / Ea[0], abs(2.0 * Es[1] - Ea[1]) / Ea[0]))
    assert du <= 1e-9 and abs(2.0 * Es[0] - Ea[0]) <= 1e-9 * Ea[0]
    assert np.all(sty.admm_stats()["iters"] <= 2)
    Ua, Ea, _ = arap.deform(hp, max_iter=4, opts=o)
    Us, Es, _ = sty.run(hp, max_iter=4, opts=o)
    ref = N.StylizeNp(V, F, pins=handles, L=Lc, lambda_=0.0)
    Un, En, _ = ref.run(hp, n_iter=4)
    print("lambda = 0, four iterations: max |U - U_arap| = %.2e diagonals, energies %.2e; against the restatement's lambda = 0 run %.2e, %.2e" %
          (np.abs(Ua - Us).max() / bbox_diag(V), np.abs(2.0 * Es - Ea).max() / Ea.max(), np.abs(Us - Un).max() / bbox_diag(V), (np.abs(Es - En) / En).max()))
    assert np.all(np.isfinite(Us)) and np.all(Es[1:] < Es[:-1])
    lam = np.where(V[:, 0] < 0.5, 0.0, 0.4)
    P = N.noisy_pose(V)
    out, it = hook_run(smg)(N.STY_LOCAL, A, F, P, lam=lam)
    R = N.unpack(N.STY_LOCAL, out, A.n)[0]
    Rn, _, _ = rotations_np(N.covariance(A, P))
    half = lam == 0.0
    print("lambda_i = 0 on %d of %d vertices: max |R - R_arap| = %.2e there, %.2e on the rest" % (half.sum(), A.n, np.abs(R - Rn)[half].max(), np.abs(R - Rn)[~half].max()))
    assert 0 < half.sum() < A.n and np.abs(R - Rn)[half].max() <= 1e-12 and np.all(it[half] == 2)
    assert np.abs(R - Rn)[~half].max() > 1e-3


def test_same_bits(smg, sphere_case):
    import torch
    V, F, mg, sty = sphere_case
    n = V.shape[0]
    live = smg._lib.load().smg_device_bytes_live
    s = N.ArapRest(smg.mesh.cotmatrix(V, F), V).scale()
    handles, hp = twist(V)
    gc.collect()
    before_live = live()
    pinned = smg.Stylizer(mg, V, F, handles)
    a = pinned.run(hp, max_iter=4)
    b = pinned.run(hp, max_iter=4)
    before = pinned.device_bytes()
    assert 0 < before == live() - before_live                                # what it counts is what the library holds for it
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    eager = pinned.run(hp, max_iter=4, opts=smg.SolveOpts(tol=1e-8 * s, max_iter=50, use_graph=0))
    graph = pinned.run(hp, max_iter=4, opts=smg.SolveOpts(tol=1e-8 * s, max_iter=50, use_graph=1))
    assert all(np.array_equal(x, y) for x, y in zip(eager, graph)) and all(np.array_equal(x, y) for x, y in zip(a, graph))
    assert pinned.device_bytes() == before                                   # nothing grows between the second and later calls
    # SMG_DEVICE, padded leading dimensions: the same bits, rows past n untouched
    nh = handles.size
    ld_u, ld_pp, ld_u0 = n + 5, nh + 3, n + 2
    U0 = a[0] + 0.0
    Ud = torch.full((3, ld_u), -1.0, dtype=torch.float64, device="cuda")
    ppd = torch.zeros((3, ld_pp), dtype=torch.float64, device="cuda")
    ppd[:, :nh] = torch.from_numpy(np.ascontiguousarray(hp.T))
    U0d = torch.zeros((3, ld_u0), dtype=torch.float64, device="cuda")
    U0d[:, :n] = torch.from_numpy(np.ascontiguousarray(U0.T))
    Ed, cycd = pinned.run_device(Ud.data_ptr(), ppd.data_ptr(), ld_u=ld_u, U0_ptr=U0d.data_ptr(), ld_u0=ld_u0, ld_pp=ld_pp, max_iter=3)
    torch.cuda.synchronize()
    Uh, Eh, cych = pinned.run(hp, U0=U0, max_iter=3)
    got = Ud.cpu().numpy()
    assert np.array_equal(got[:, :n].T, Uh) and np.all(got[:, n:] == -1.0)
    assert np.array_equal(Ed, Eh) and np.array_equal(cycd, cych)
    # padded host leading dimensions through the C ABI
    L = smg._lib.load()
    Up = np.full((n + 7, 3), -2.0, order="F")
    ppp = np.zeros((nh + 1, 3), order="F")
    ppp[:nh] = hp
    E = np.zeros(4)
    nit = C.c_int()
    assert L.smg_stylize_run(pinned.s, ppp.ctypes.data, nh + 1, None, 0, 0, 3, 0.0, None, Up.ctypes.data, n + 7, E.ctypes.data_as(C.POINTER(C.c_double)),
                             None, C.byref(nit)) == 0
    assert nit.value == 3 and np.array_equal(Up[:n], pinned.run(hp, max_iter=3)[0]) and np.all(Up[n:] == -2.0)
    assert pinned.device_bytes() == before
    del pinned
    gc.collect()
    assert live() == before_live


def test_callers_hierarchy_is_untouched(smg):
    from oracle import mesh_np as M
    V, F = N.shape("bunny.smgm")
    mg = smg.mg_precompute(V, F, 0.25, 200, 1)
    A = (M.massmatrix(V, F, "barycentric") - 0.01 * smg.mesh.cotmatrix(V, F)).tocsr()
    mg.precompute(A, None)
    rhs_ = np.asfortranarray(A @ V)
    o = smg.SolveOpts(tol=1e-10, max_iter=30)
    first = mg.solve(rhs_, np.zeros_like(rhs_, order="F"), None, o)
    smg.Stylizer(mg, V, F).run(max_iter=2)
    second = mg.solve(rhs_, np.zeros_like(rhs_, order="F"), None, o)
    assert first[0] and np.array_equal(first[1], second[1]) and np.array_equal(first[2], second[2])


def test_setters_take_effect_without_a_rebuild(smg, sphere_case):
    V, F, mg, sty = sphere_case
    n = V.shape[0]
    base = sty.run(max_iter=3)
    bytes0 = sty.device_bytes()
    sty.set_params(lambda_=0.4)
    strong = sty.run(max_iter=3)
    fresh = smg.Stylizer(mg, V, F, lambda_=0.4).run(max_iter=3)
    assert all(np.array_equal(x, y) for x, y in zip(strong, fresh)) and not np.array_equal(strong[0], base[0])
    assert N.cubeness(strong[0], F) < N.cubeness(base[0], F) and sty.device_bytes() == bytes0
    sty.set_params(lambda_=0.2, admm_iters=3)
    sty.run(max_iter=1)
    assert sty.admm_stats()["max"] <= 3 and sty.admm_stats()["at_cap"] > 0
    sty.set_params(admm_iters=100)
    assert all(np.array_equal(x, y) for x, y in zip(base, sty.run(max_iter=3)))
    sty.set_lambda(np.full(n, 0.4))                                          # per-vertex weights equal to a uniform one: its bits
    assert all(np.array_equal(x, y) for x, y in zip(strong, sty.run(max_iter=3))) and sty.device_bytes() == bytes0 + 8 * n
    sty.set_lambda(np.where(V[:, 2] > 0.5, 0.4, 0.0))
    half = sty.run(max_iter=3)[0]
    moved = np.linalg.norm(half - V, axis=1)
    assert moved[V[:, 2] > 0.75].mean() > moved[V[:, 2] < 0.25].mean()     # the weighted half is the one that is stylized
    assert not np.array_equal(half, base[0]) and not np.array_equal(half, strong[0])
    sty.set_lambda(None)
    assert all(np.array_equal(x, y) for x, y in zip(base, sty.run(max_iter=3))) and sty.device_bytes() == bytes0


def test_live_object_refusals(smg, sphere_case):
    """the refusals that need an object, with the code and message recorded in tests/golden/stylize_refusals.json (group "live"); the object is
    as usable afterwards as before"""
    V, F, mg, sty = sphere_case
    n, L = V.shape[0], smg._lib.load()
    golden = json.load(open(GOLDEN))["live"]
    dp = C.POINTER(C.c_double)
    before = sty.run(max_iter=2)
    new = smg.Stylizer(mg, V, F)
    lam_neg, lam_nan = np.full(n, 0.1), np.full(n, 0.1)
    lam_neg[2], lam_nan[1] = -0.1, np.nan
    t = np.tile([0.0, 0.0, 1.0], (n, 1))
    t_bad, t_nan = t.copy(), t.copy()
    t_bad[2], t_nan[1, 0] = [0.0, 0.6, 0.9], np.nan
    skew, mirror = np.eye(3) + 1e-6 * np.arange(9).reshape(3, 3), np.diag([1.0, 1.0, -1.0])
    U = np.zeros((n, 3), order="F")
    pp = np.asfortranarray(V[:1])
    run = lambda **k: L.smg_stylize_run(k.get("s", sty.s), pp.ctypes.data, k.get("ld_pp", 1), None, 0, k.get("memspace", 0), k.get("max_iter", 1),   # noqa: E731
                                        k.get("rel_tol", 0.0), None, k.get("U", U.ctypes.data), k.get("ld_u", n), None, None, None)
    bad_p = N.params_c(smg, tau=1.0)
    calls = {"set_params tau one": lambda: L.smg_stylize_set_params(sty.s, C.byref(bad_p)), "set_params null": lambda: L.smg_stylize_set_params(sty.s, None),
             "set_lambda negative": lambda: L.smg_stylize_set_lambda(sty.s, lam_neg.ctypes.data_as(dp)),
             "set_lambda nan": lambda: L.smg_stylize_set_lambda(sty.s, lam_nan.ctypes.data_as(dp)),
             "set_frame not orthonormal": lambda: L.smg_stylize_set_frame(sty.s, skew.ctypes.data_as(dp)),
             "set_frame reflection": lambda: L.smg_stylize_set_frame(sty.s, mirror.ctypes.data_as(dp)),
             "set_targets not unit": lambda: L.smg_stylize_set_targets(sty.s, t_bad.ctypes.data_as(dp)),
             "set_targets nan": lambda: L.smg_stylize_set_targets(sty.s, t_nan.ctypes.data_as(dp)),
             "run bad memspace": lambda: run(memspace=7), "run negative max_iter": lambda: run(max_iter=-1), "run nan rel_tol": lambda: run(rel_tol=float("nan")),
             "run null U": lambda: run(U=None), "run ld_u too small": lambda: run(ld_u=n - 1), "run ld_pp too small": lambda: run(ld_pp=0),
             "admm_stats before a run": lambda: L.smg_stylize_admm_stats(new.s, None, None, None, None, None)}
    assert set(calls) == set(golden)
    for name, f in calls.items():
        rc = f()
        assert [rc, L.smg_last_error().decode()] == golden[name] and rc == INVALID, name
    assert all(np.array_equal(x, y) for x, y in zip(before, sty.run(max_iter=2)))


def test_non_finite_start_is_refused_at_iteration_0(smg, sphere_case):
    """one NaN in U0 at a vertex that is not pinned: E_0 is NaN, so the call ends before any inner solve with SMG_ERR_NONFINITE, n_iter = 0 and
    nothing written past energy_his[0]; the object is as usable afterwards as before (the same bits)"""
    V, F, mg, sty = sphere_case
    n, L = V.shape[0], smg._lib.load()
    before = sty.run(max_iter=2)
    U0 = np.asfortranarray(V.copy())
    U0[n // 2, 1] = np.nan
    U = np.zeros((n, 3), order="F")
    E, cyc, nit = np.full(4, -7.0), np.full(3, -7, dtype=np.int32), C.c_int(-7)
    rc = L.smg_stylize_run(sty.s, None, 0, U0.ctypes.data, n, 0, 3, 0.0, None, U.ctypes.data, n, E.ctypes.data_as(C.POINTER(C.c_double)),
                           cyc.ctypes.data_as(C.POINTER(C.c_int)), C.byref(nit))
    assert rc == -4 and L.smg_last_error() == b"smg_stylize_run: non-finite energy at iteration 0"
    assert nit.value == 0 and np.isnan(E[0]) and np.all(E[1:] == -7.0) and np.all(cyc == -7)
    assert all(np.array_equal(x, y) for x, y in zip(before, sty.run(max_iter=2)))


@pytest.mark.parametrize("case", ["sphere_case", "bunny_case"])
def test_default_opts_and_stopping_rule(smg, request, case):
    V, F, mg, sty = request.getfixturevalue(case)
    U, E, cyc = sty.run(max_iter=10)
    drops = (E[:-1] - E[1:]) / E[:-1]
    print(case, "default opts: cycles %s, relative drops %s" % (cyc, np.array2string(drops, precision=3)))
    assert E.shape == (11,) and cyc.shape == (10,)
    assert np.all(E[1:] < E[:-1]) and np.all(cyc < 50)                       # every inner solve converged
    assert np.array_equal(U[0], V[0])
    rel_tol = 1.0001 * float(np.sort(drops)[len(drops) // 2])                # just above a drop of this run: the rule must end at the first one not above it
    U2, E2, cyc2 = sty.run(max_iter=20, rel_tol=rel_tol)
    drops2 = (E2[:-1] - E2[1:]) / np.abs(E2[:-1])
    print(case, "rel_tol = %.3g: n_iter = %d, drops %s" % (rel_tol, cyc2.size, np.array2string(drops2, precision=3)))
    assert 1 <= cyc2.size < 20 and E2.size == cyc2.size + 1
    assert drops2[-1] <= rel_tol and np.all(drops2[:-1] > rel_tol)
    assert np.array_equal(E2, E[:E2.size])
    U0, E0, cyc0 = sty.run(max_iter=0)
    assert E0.shape == (1,) and cyc0.size == 0 and E0[0] == E[0] and np.array_equal(U0, V)
