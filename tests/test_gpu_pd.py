"""GPU (-m gpu): projective-dynamics membrane steps on the scalar V-cycle (include/smg.h: smg_pd_*).

The host reference is tests/pd_np.py -- the same method with direct solves, in the kernels' operation order.  The kernels are held launcher by
launcher (smg_debug_pd, guarded buffers): F, sigma, T and the energy terms to the restatement within the projection bound of
tests/test_pd_host.py, the right-hand side and the energy sum bit for bit to numpy sums of the DEVICE's per-face outputs in list order (the
fixed sum in its own order), m0 bit for bit to smg_mesh_massmatrix.

End to end (three steps of 10 iterations at inner tolerance 1e-10 |b_0| against the restatement's direct solves) positions are compared
relative to the largest displacement of the run and energies relatively.  The rule: 100 x the measured maximum rounded up to a power of ten,
positions never looser than 1e-6.  Measured on an MI355X: ogre_sim, three steps, PCG: positions <= 2.68e-8, energies
<= 1.48e-10, so STEP_POS_BOUND = 1e-6 (the rule's 1e-5 is looser than the ceiling) and STEP_ENERGY_BOUND = 1e-7; one global system 2.00e-12
(stationary) and 4.88e-13 (PCG) under SOLVE_BOUND; the projection at most 17.6 eps (sigma1 / sigma2)^2 (the fan) under PROJECTION_B = 1e3."""
import ctypes as C
import gc

import numpy as np
import pytest

import pd_np as N
from test_geodesics_host import flat_square
from test_gpu_param import fan, strip
from test_gpu_parity import smg  # noqa: F401  (fixture)
from test_pd_host import PROJECTION_B, projection_errors

pytestmark = pytest.mark.gpu

EPS = N.EPS
NONFINITE = -4          # SMG_ERR_NONFINITE
SOLVE_BOUND = 1e-8          # one global system against the direct solve: the bound of the membrane and ARAP tests for this comparison
STEP_POS_BOUND = 1e-6       # measured 2.68e-8 (ogre_sim, three steps): the rule gives 1e-5, the ceiling 1e-6 holds
STEP_ENERGY_BOUND = 1e-7    # measured 1.48e-10
BAND = (0.9, 1.2)


def hook(smg, op, V, F, P=None, inp=None, n_out=0, **params):
    rc, bad, out = N.pd_hook(smg, op, V.shape[0], F, V, P, inp, n_out, **params)
    assert rc == 0 and bad == 0, (rc, bad)
    return out


def cycling_pose(V, F):
    """the second corner of face f moved along its first edge by 1, 1, 1.6, 1.6, 0.6, 0.6, ...: on the fan (every face's first corner is the hub,
    its second a ring vertex of its own) runs of lanes fall inside the band, above it and below it; the caller counts the outcomes"""
    P = V.copy()
    scale = np.array([1.0, 1.0, 1.6, 1.6, 0.6, 0.6])
    for f in range(F.shape[0]):
        P[F[f, 1]] = V[F[f, 0]] + scale[f % 6] * (V[F[f, 1]] - V[F[f, 0]])
    return P


@pytest.fixture(scope="module")
def kernel_cases():
    """label -> (V, F, [poses]): the hand-made faces, strips at the wave and block edges, a fan (the long corner list), ogre_sim at amp 0.3"""
    out = {}
    hand = N.hand_faces(BAND)
    out["hand"] = (np.tile(N.REST_FACE, (len(hand), 1)), np.arange(3 * len(hand), dtype=np.int32).reshape(-1, 3), [np.concatenate([p for _, p, _ in hand])])
    rng = np.random.default_rng(5)
    for label, (V, F) in [("strip63", strip(63)), ("strip64", strip(64)), ("strip65", strip(65)), ("fan65", fan(65))]:
        used = np.unique(F)                                        # no vertex without a face: it has no mass and no normal (create refuses such a mesh)
        V, F = np.ascontiguousarray(V[used]), np.searchsorted(used, F).astype(np.int32)
        out[label] = (V, F, [cycling_pose(V, F), V + 0.2 * rng.standard_normal(V.shape)])
    V, F = N.load_mesh("ogre_sim.smgm")
    out["ogre_sim"] = (V, F, [N.perturbed(V, F, 0.3)])
    return out


KERNEL_CASES = ["hand", "strip63", "strip64", "strip65", "fan65", "ogre_sim"]


# ---- kernels, launcher by launcher ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", KERNEL_CASES)
def test_kernels_against_restatement(smg, kernel_cases, name):
    V, F, poses = kernel_cases[name]
    nV, nF = V.shape[0], F.shape[0]
    par = dict(sigma_min=BAND[0], sigma_max=BAND[1], stiffness=1.7, density=1.3, dt=2e-2, pressure=3.0, gravity=(0.1, -0.2, -1.0))
    r = N.rest_constants(V, F)
    assert np.array_equal(hook(smg, N.PD_REST, V, F, n_out=4 * nF, **par).reshape(4, nF).T, r)
    m0 = hook(smg, N.PD_MASS, V, F, n_out=nV, **par)
    lib_m0 = np.zeros(nV)
    Fi = np.ascontiguousarray(F, dtype=np.int32)
    assert smg._lib.load().smg_mesh_massmatrix(V.ctypes.data_as(C.POINTER(C.c_double)), nV, Fi.ctypes.data_as(C.POINTER(C.c_int)), nF, 1,
                                               lib_m0.ctypes.data_as(C.POINTER(C.c_double))) == 0
    assert np.array_equal(m0, lib_m0)                                                  # the diagonal the matrix is built with, bit for bit
    lists = N.corner_lists(F, nV)
    c_mass = par["density"] / (par["dt"] * par["dt"])
    print(name, "nV = %d, nF = %d, longest corner list %d" % (nV, nF, np.bincount(F.ravel()).max()))
    for P in poses:
        out = hook(smg, N.PD_FACES, V, F, P, n_out=24 * nF, **par).reshape(24, nF)
        Fg, sigma, T, et, share = out[:6].T, out[6:8].T, out[8:14].T, out[14], out[15:].T
        Fn = N.gradient(r, F, P)
        sn, Tn, guard = N.project(Fn, *BAND)
        etn, shn = N.face_energy(r, par["stiffness"], Fn, Tn), N.corner_shares(r, par["stiffness"], Tn)
        # against the restatement: the host bounds of tests/test_pd_host.py (the guard faces have no SVD bound: they are compared to the rule)
        ok = ~guard
        err, bound, s = projection_errors(T[ok], Fn[ok], BAND)
        assert np.all(np.isfinite(out)) and np.all(np.abs(Fg - Fn) <= 4 * EPS * np.abs(Fn).max(axis=1, keepdims=True))
        assert np.all(err <= bound)                                                    # every unguarded face compared: none is left out
        assert np.all(np.sqrt(np.sum((T - Tn) ** 2, axis=1))[ok] <= bound) and np.allclose(T[guard], Tn[guard], rtol=0, atol=8 * EPS)
        assert np.all(np.abs(sigma - sn)[ok] <= 16 * EPS * ((s[:, 0] / s[:, 1]) ** 2 * s[:, 0])[:, None])
        # (k A / 2) | |F - T|^2 - |F - T'|^2 | <= (k A / 2) (2 |F - T| + |T - T'|) |T - T'| with |T - T'| within the projection bound
        dist = np.sqrt(N.distance2(Fn, Tn))[ok]
        assert np.all(np.abs(et - etn)[ok] <= 0.5 * par["stiffness"] * r[ok, 3] * (2 * dist + bound) * bound + 16 * EPS * etn[ok])
        counts = N.clamp_outcomes(sigma, *BAND)
        print("  |T - T_svd| <= %.2f eps (s1/s2)^2, inside / above / below %s, guard faces %d"
              % ((err / (bound / PROJECTION_B)).max(), counts, guard.sum()))
        if name in ("hand", "ogre_sim") or (name == "fan65" and P is poses[0]):
            assert min(counts) > 0                                                     # the lanes diverge over all three clamp outcomes
        # the step's kernel (MODE 0, the pose as a column-major block) writes the bits MODE 1 writes
        step = hook(smg, N.PD_FACES_STEP, V, F, P, n_out=10 * nF, **par).reshape(10, nF)
        assert np.array_equal(step[0], et) and np.array_equal(step[1:].T, share)
        # the energy terms and the shares are the restatement's expressions of the DEVICE's F and T, bit for bit
        assert np.array_equal(et, N.face_energy(r, par["stiffness"], Fg, T)) and np.array_equal(share, N.corner_shares(r, par["stiffness"], T))
        # |k A (T - T') g_i| <= k A |T - T'|_F |g_i| and |g_0| <= |g_1| + |g_2|
        gnorm = (np.hypot(1.0 / r[:, 0], r[:, 1] / (r[:, 0] * r[:, 2])) + 1.0 / r[:, 2])[ok]
        assert np.all(np.abs(share - shn)[ok] <= (par["stiffness"] * r[ok, 3] * gnorm * bound)[:, None] + 16 * EPS * np.abs(shn[ok]).max(axis=1, keepdims=True))
        # b and the inertia terms: numpy sums of the device's shares in list order
        vel = 0.3 * np.sin(np.arange(3 * nV, dtype=np.float64)).reshape(nV, 3)
        X = V if name == "hand" else P                                                 # a collapsed face has no normal: the forces are taken at rest there
        pr = hook(smg, N.PD_PREDICT, V, F, X, vel.reshape(-1), n_out=6 * nV, **par)
        fext, S = pr[:3 * nV].reshape(nV, 3), pr[3 * nV:].reshape(3, nV).T
        assert np.array_equal(S, N.predict(X, vel, fext, m0, par["dt"], par["density"], par["gravity"]))      # of the DEVICE's pressure force
        fn = N.pressure_fext(X, F, par["pressure"])                                     # the launcher is the membrane's, held bit for bit by its own tests
        assert np.all(np.isfinite(pr)) and np.all(np.abs(fext - fn) <= 1e-10 * np.abs(fn).max())
        Q = P + 0.01 * np.cos(np.arange(3 * nV, dtype=np.float64)).reshape(nV, 3)
        inp = np.concatenate([share.T.reshape(-1), m0, S.T.reshape(-1), Q.T.reshape(-1)])
        vo = hook(smg, N.PD_VERTICES, V, F, None, inp, n_out=5 * nV, **par)
        B, iterm, bsq = N.vertices(share, lists, m0, c_mass, S, Q)
        assert np.array_equal(vo[:3 * nV].reshape(3, nV).T, B) and np.array_equal(vo[3 * nV:4 * nV], iterm) and np.array_equal(vo[4 * nV:], bsq)
        terms = np.concatenate([et, iterm])
        E1 = hook(smg, N.PD_ENERGY, V, F, None, terms, n_out=1, **par)[0]
        assert E1 == N.fixed_sum(terms)                                                # the fixed sum in its own order
        fin = hook(smg, N.PD_FINISH, V, F, P, Q.T.reshape(-1), n_out=6 * nV, **par)
        assert np.array_equal(fin[:3 * nV].reshape(nV, 3), (Q - P) / par["dt"]) and np.array_equal(fin[3 * nV:].reshape(nV, 3), Q)
        st = hook(smg, N.PD_STRAIN, V, F, P, n_out=5 * nF, **par).reshape(5, nF).T
        assert np.array_equal(st, N.strain_terms(r, Fg, sigma, T, *BAND))


# ---- the object -------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ogre(smg):
    V, F = N.load_mesh("ogre_sim.smgm")
    return V, F, smg.mg_precompute(V, F, 0.25, 500, 1)


def tight(smg, tol, use_graph=1):
    return smg.SolveOpts(tol=tol, max_iter=100, use_graph=use_graph)


@pytest.mark.parametrize("pcg", [0, 1], ids=["stationary", "pcg"])
def test_one_global_system_against_the_direct_solve(smg, ogre, pcg):
    """the first global step of the table run: q_1 of the object against the restatement's direct solve"""
    V, F, mg = ogre
    P = N.PdNp(V, F, pressure=5.0)
    S, hp = P.prediction()
    _, B, bnorm = P.local(S, S)
    want = P.solve(B, S, hp)
    pd = smg.ProjectiveDynamics(mg, V, F, pressure=5.0)
    pd.set_solver(pcg)
    E, cyc = pd.step(max_iter=1, opts=tight(smg, 1e-10 * bnorm))
    got = pd.state()[0]
    err = np.linalg.norm(got - want) / np.linalg.norm(want)
    print("pcg %d: |q_1 - direct| / |direct| = %.2e, %d loop entries, |b| = %.3e" % (pcg, err, cyc[0], bnorm))
    assert 0 < cyc[0] < 100 and err <= SOLVE_BOUND


def run_steps(smg, pd, P, bnorm0, n_steps=3, pin_seq=None, use_graph=1):
    """n_steps of 10 iterations on the object and on the restatement; returns the worst position error relative to the largest displacement of
    the run and the worst relative energy error"""
    x0 = P.x.copy()
    worst_x = worst_e = 0.0
    disp = 0.0
    for s in range(n_steps):
        hp = None if pin_seq is None else pin_seq[s]
        En, _ = P.step(pin_pos=hp, n_iter=10)
        Ed, cyc = pd.step(pin_pos=hp, max_iter=10, opts=tight(smg, 1e-10 * bnorm0, use_graph))
        x, v = pd.state()
        disp = max(disp, np.abs(P.x - x0).max())
        worst_x = max(worst_x, np.abs(x - P.x).max() / disp)
        worst_e = max(worst_e, np.abs(Ed / En - 1.0).max())
        print("  step %d: |x - x_np| / displacement %.2e, energies %.2e, loop entries %s" % (s, np.abs(x - P.x).max() / disp, np.abs(Ed / En - 1.0).max(), cyc))
        assert Ed.size == 11 and np.all(cyc > 0)
    return worst_x, worst_e


def test_three_steps_against_the_restatement(smg, ogre):
    V, F, mg = ogre
    P = N.PdNp(V, F, pressure=5.0)
    S, _ = P.prediction()
    bnorm0 = P.local(S, S)[2]
    pd = smg.ProjectiveDynamics(mg, V, F, pressure=5.0)
    pd.set_solver(1)
    wx, we = run_steps(smg, pd, P, bnorm0)
    print("three steps, ogre_sim, PCG: positions %.2e of the largest displacement, energies %.2e" % (wx, we))
    assert wx <= STEP_POS_BOUND and we <= STEP_ENERGY_BOUND


# The inner tolerance of the pinned run.  Its displacements are the pins' 2e-3 per step, and what an inner solve leaves undone sits next to the
# pins: at 1e-10 |b_0| the positions were measured at 1.03e-6 of the largest displacement and the energies at 1.52e-7, both the solver's
# remainder (|b_0| = c_mass |M0 s| carries the positions, of size 1, not the displacement).  The bounds are those of the three-step test; the
# run is held to them at a tolerance two digits tighter.
PIN_TOL = 1e-12


def test_moving_pins_under_gravity(smg):
    V, F = flat_square(24)
    mg = smg.mg_precompute(V, F, 0.25, 100, 1)
    top = np.nonzero(V[:, 1] == V[:, 1].max())[0]
    pins = np.array([top[np.argmin(V[top, 0])], top[np.argmax(V[top, 0])]], dtype=np.int32)
    par = dict(gravity=(0.0, 0.0, -1.0))
    P = N.PdNp(V, F, pins=pins, **par)
    S, _ = P.prediction()
    bnorm0 = P.local(S, S)[2]
    pd = smg.ProjectiveDynamics(mg, V, F, pins=pins, **par)
    seq = [V[pins] + (s + 1) * np.array([0.002, 0.0, 0.001]) for s in range(3)]
    old = V[pins].copy()
    x0 = V.copy()
    worst_x = worst_e = disp = 0.0
    for s in range(3):
        En, _ = P.step(pin_pos=seq[s], n_iter=10)
        Ed, cyc = pd.step(pin_pos=seq[s], max_iter=10, opts=tight(smg, PIN_TOL * bnorm0))
        x, v = pd.state()
        assert np.array_equal(x[pins], seq[s])                                         # the pin rows are pin_pos, bit for bit
        assert np.array_equal(v[pins], (seq[s] - old) / P.p["dt"])                      # (new - old) / h as k_pd_finish computes it
        old = seq[s]
        disp = max(disp, np.abs(P.x - x0).max())
        worst_x = max(worst_x, np.abs(x - P.x).max() / disp)
        worst_e = max(worst_e, np.abs(Ed / En - 1.0).max())
    print("flat_square(24), moving pins: positions %.2e of the largest displacement, energies %.2e" % (worst_x, worst_e))
    assert worst_x <= STEP_POS_BOUND and worst_e <= STEP_ENERGY_BOUND


def device_array(smg, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def test_same_bits_across_graphs_memspaces_and_setters(smg, ogre):
    V, F, mg = ogre
    pins = np.array([0, 17], dtype=np.int32)
    hp = V[pins] + [0.001, 0.0, -0.002]
    x0, v0 = N.perturbed(V, F, 0.02), 0.1 * np.sin(np.arange(V.size, dtype=np.float64)).reshape(V.shape)

    def run(use_graph, device, via_setters=False):
        if via_setters:                         # a stepped object brought to the same parameters and state
            pd = smg.ProjectiveDynamics(mg, V, F, pins=pins, pressure=1.0, sigma_min=1.0, sigma_max=1.0)
            pd.step(max_iter=2)
            pd.set_strain_limits(*BAND)
            pd.set_forces(4.0, (0.0, 0.0, -0.5))
        else:
            pd = smg.ProjectiveDynamics(mg, V, F, pins=pins, pressure=4.0, gravity=(0.0, 0.0, -0.5), sigma_min=BAND[0], sigma_max=BAND[1])
        opts = smg.SolveOpts(tol=1e-9, max_iter=50, use_graph=use_graph)
        out = []
        if device:
            import torch
            dx, dv, dh = device_array(smg, x0), device_array(smg, v0), device_array(smg, hp)
            pd.set_state_device(dx.data_ptr(), dv.data_ptr())
            E1, c1 = pd.step_device(dh.data_ptr(), max_iter=4, opts=opts)
            E2, c2 = pd.step_device(None, max_iter=4, opts=opts)
            ox, ov = torch.zeros_like(dx), torch.zeros_like(dv)
            pd.state_device(ox.data_ptr(), ov.data_ptr())
            torch.cuda.synchronize()
            out = [E1, E2, ox.cpu().numpy(), ov.cpu().numpy()]
        else:
            pd.set_state(x0, v0)
            E1, c1 = pd.step(hp, max_iter=4, opts=opts)
            E2, c2 = pd.step(None, max_iter=4, opts=opts)
            out = [E1, E2, *pd.state()]
        return out + [c1, c2, pd.strain()[0]]

    ref = run(1, False)
    for use_graph, device, setters in ((1, False, False), (0, False, False), (1, True, False), (0, True, False), (1, False, True)):
        got = run(use_graph, device, setters)
        for a, b in zip(ref, got):
            assert np.array_equal(a, b), (use_graph, device, setters)


def test_an_unrelated_handle_solves_the_same_bits_around_a_step(smg, ogre):
    import scipy.sparse as sp
    from oracle import mesh_np as M
    V, F, mg = ogre
    A = (sp.diags(M.massmatrix(V, F, "voronoi").diagonal()) - 1e-3 * M.cotmatrix(V, F)).tocsr()
    other = smg.mg_precompute(V, F, 0.25, 500, 1)
    other.precompute(A)
    rhs = np.sin(np.arange(V.shape[0], dtype=np.float64))[:, None]
    opts = smg.SolveOpts(tol=1e-10, max_iter=30)
    before = other.solve(rhs, np.zeros_like(rhs), opts=opts)
    pd = smg.ProjectiveDynamics(mg, V, F, pressure=5.0)
    pd.step(max_iter=3)
    after = other.solve(rhs, np.zeros_like(rhs), opts=opts)
    for a, b in zip(before, after):
        assert np.array_equal(np.asarray(a), np.asarray(b))


def test_a_nan_in_the_state_is_reported_and_changes_nothing(smg, ogre):
    V, F, mg = ogre
    L = smg._lib.load()
    pd = smg.ProjectiveDynamics(mg, V, F, pressure=5.0)
    x0 = N.perturbed(V, F, 0.02)
    bad = x0.copy()
    bad[1234, 1] = np.nan
    pd.set_state(bad, np.zeros_like(V))
    E = np.full(6, -7.0)
    cyc = np.full(5, -7, dtype=np.int32)
    nit = C.c_int(-7)
    rc = L.smg_pd_step(pd.d, None, 0, 5, 0.0, None, E.ctypes.data_as(C.POINTER(C.c_double)), cyc.ctypes.data_as(C.POINTER(C.c_int)), C.byref(nit))
    assert rc == NONFINITE and nit.value == 0 and b"iteration 0" in L.smg_last_error()
    assert np.isnan(E[0]) and np.all(E[1:] == -7.0) and np.all(cyc == -7)              # nothing is written past energy_his[0]
    x, v = pd.state()
    assert np.array_equal(x, bad, equal_nan=True) and np.array_equal(v, np.zeros_like(V))   # the state is as it was
    pd.set_state(x0, np.zeros_like(V))
    fresh = smg.ProjectiveDynamics(mg, V, F, pressure=5.0)
    fresh.set_state(x0, np.zeros_like(V))
    Ea, ca = pd.step(max_iter=3)
    Eb, cb = fresh.step(max_iter=3)
    assert np.array_equal(Ea, Eb) and np.array_equal(ca, cb)
    for a, b in zip(pd.state(), fresh.state()):
        assert np.array_equal(a, b)


def test_device_bytes_are_live_buffers_and_destroy_frees_them(smg, ogre):
    V, F, mg = ogre
    live = smg._lib.load().smg_device_bytes_live
    gc.collect()
    before = live()
    pd = smg.ProjectiveDynamics(mg, V, F, pins=[3], pressure=5.0)
    pd.step(max_iter=2)
    pd.strain()
    counted, held = pd.device_bytes(), live() - before
    print("pd: device_bytes %d, live DevBuf bytes held %d" % (counted, held))
    del pd
    gc.collect()
    assert 0 < counted == held and live() == before


def test_strain_against_numpy_on_the_device_state(smg, ogre):
    V, F, mg = ogre
    pd = smg.ProjectiveDynamics(mg, V, F, pressure=5.0, sigma_min=BAND[0], sigma_max=BAND[1])
    pd.set_state(N.perturbed(V, F, 0.3), None)
    pd.step(max_iter=2)
    x, _ = pd.state()
    sigma, stats = pd.strain()
    r = N.rest_constants(V, F)
    Fn = N.gradient(r, F, x)
    sn, Tn, guard = N.project(Fn, *BAND)
    s, Tsvd = N.project_svd(Fn, *BAND)
    assert not guard.any()
    assert np.all(np.abs(sigma - s) <= PROJECTION_B * EPS * ((s[:, 0] / s[:, 1]) ** 2 * s[:, 0])[:, None])
    # the count is exact where no face lies within 1e-9 of a band edge: asserted for this pose
    assert np.abs(s - BAND[0]).min() > 1e-9 and np.abs(s - BAND[1]).min() > 1e-9
    inside, above, below = N.clamp_outcomes(s, *BAND)
    assert stats["outside_band"] == F.shape[0] - inside and 0 < inside < F.shape[0]
    assert stats["max_sigma1"] == sigma[:, 0].max() and stats["min_sigma2"] == sigma[:, 1].min()
    mean = np.sum(r[:, 3] * N.distance2(Fn, Tsvd)) / np.sum(r[:, 3])
    print("strain: max sigma1 %.4f, min sigma2 %.4f, outside %d, mean |F - T|^2 %.6e (numpy %.6e)"
          % (stats["max_sigma1"], stats["min_sigma2"], stats["outside_band"], stats["mean_distance2"], mean))
    assert abs(stats["mean_distance2"] / mean - 1.0) <= 1e-10
