"""GPU (-m gpu): feature-preserving denoising on the scalar V-cycle (include/smg.h: smg_denoise_*).

The host reference is tests/denoise_np.py -- the same method with direct solves, written from the formulas.  The kernels are held launcher by
launcher (smg_debug_denoise, guarded buffers).  Every expression of the rest constants, the spacing and the projection is a correctly rounded
+, -, *, / or sqrt with contraction off, so the device gives the restatement's bits (the host twin measured 0 against numpy on every shape,
tests/test_denoise_host.py); the right-hand side and the energy sum are held bit for bit to numpy sums of the DEVICE's per-face outputs in
list order.  The filter calls exp, whose bits may differ between libm and the device: its bound is FILTER_BOUND of tests/test_denoise_host.py
(100 x the maximum measured on the host twin, rounded up to a power of ten), which the device holds with the figures of DESIGN.md section 24.

End to end (10 iterations at inner tolerance 1e-10 |b_0| against the restatement's direct solves) positions are compared relative to the
largest displacement of the run and energies relatively; the rule is the same 100 x.  Measured on an MI355X: noisy cube
positions 1.03e-9, energies 1.61e-11; ogre_sim positions 5.35e-10, energies 5.05e-11: RUN_POS_BOUND = 1e-6, RUN_ENERGY_BOUND = 1e-8.  The filter
on the device: at most 1.00 eps after 1 iteration and 5.25 eps after 5 (ogre_sim); one global system 7.44e-13 (stationary) and 5.25e-13 (PCG)."""
import ctypes as C
import gc

import numpy as np
import pytest

import denoise_np as N
from test_denoise_host import FILTER_BOUND, kernel_shapes
from test_gpu_parity import smg  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

EPS = N.EPS
NONFINITE = -4              # SMG_ERR_NONFINITE
SOLVE_BOUND = 1e-8          # one global system against the direct solve: the bound tests/test_gpu_pd.py holds for the same kind of matrix and tolerance
RUN_POS_BOUND = 1e-6        # measured 1.03e-9 (noisy cube): 100 x, rounded up to a power of ten
RUN_ENERGY_BOUND = 1e-8     # measured 5.05e-11 (ogre_sim)


def hook(smg, op, V, F, P=None, inp=None, n_out=0, **params):
    rc, bad, out = N.hook(smg, op, V.shape[0], F, V, P, inp, n_out, **params)
    assert rc == 0 and bad == 0, (rc, bad)
    return out


@pytest.fixture(scope="module")
def shapes():
    return kernel_shapes()


KERNEL_CASES = ["strip63", "strip64", "strip65", "fan65", "tetrahedron", "square", "ogre_sim"]


# ---- kernels, launcher by launcher ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", KERNEL_CASES)
def test_kernels_against_restatement(smg, shapes, name):
    V, F = shapes[name]
    nV, nF = V.shape[0], F.shape[0]
    r = N.rest_constants(V, F)
    ptr, idx = N.face_neighbours(F, nV)
    slots = N.row_slots(ptr, idx)
    print(name, "nV = %d, nF = %d, longest row %d, longest corner list %d" % (nV, nF, np.diff(ptr).max(), np.bincount(F.ravel()).max()))
    rd = hook(smg, N.DN_REST, V, F, n_out=10 * nF).reshape(10, nF).T
    print("  rest planes: max error %.2e of the largest entry of the face" % (np.abs(rd - r).max(axis=1) / np.abs(r).max(axis=1)).max())
    assert np.array_equal(rd, r)
    sd = hook(smg, N.DN_SPACING, V, F, n_out=nF)
    assert np.array_equal(sd, N.spacing_terms(r, slots))
    sigma_s = N.sigma_s_rule(r, ptr, slots)
    for iters in (1, 5):
        md = hook(smg, N.DN_FILTER, V, F, None, r[:, :3].T.reshape(-1), n_out=3 * nF, sigma_s=sigma_s, normal_iters=iters).reshape(3, nF).T
        mn = N.filter_normals(r, slots, r[:, :3], sigma_s, N.DEFAULTS["sigma_r"], iters)
        err = np.abs(md - mn).max() / EPS
        print("  filter, %d iterations: max |m - m_np| = %.2f eps (bound %g eps)" % (iters, err, FILTER_BOUND[iters]))
        assert np.all(np.isfinite(md)) and err <= FILTER_BOUND[iters]
        assert np.all(np.abs(np.sqrt(np.sum(md * md, axis=1)) - 1.0) <= 4 * EPS)
    # the projection of a perturbed pose against the DEVICE's filtered normals
    X = V + 0.05 * N.mean_edge(V, F) * np.random.default_rng(7).standard_normal(V.shape)
    po = hook(smg, N.DN_PROJECT, V, F, X, md.T.reshape(-1), n_out=10 * nF).reshape(10, nF)
    et, share, big = N.project(r, F, X, md)
    print("  projection: max share error %.2e of the largest term of the face" % (np.abs(po[1:].T - share).max(axis=1) / big).max())
    assert np.array_equal(po[0], et) and np.array_equal(po[1:].T, share)
    # b, the fidelity terms and the mass: numpy sums of the device's shares in list order
    fidelity = 1.7
    vo = hook(smg, N.DN_RHS, V, F, None, np.concatenate([po[1:].reshape(-1), X.T.reshape(-1)]), n_out=6 * nV, fidelity=fidelity)
    m0 = vo[5 * nV:]
    lib_m0 = np.zeros(nV)
    Fi = np.ascontiguousarray(F, dtype=np.int32)
    assert smg._lib.load().smg_mesh_massmatrix(V.ctypes.data_as(C.POINTER(C.c_double)), nV, Fi.ctypes.data_as(C.POINTER(C.c_int)), nF, 1,
                                               lib_m0.ctypes.data_as(C.POINTER(C.c_double))) == 0
    assert np.array_equal(m0, lib_m0)                                                  # the diagonal the matrix is built with, bit for bit
    B, iterm, bsq = N.vertices(po[1:].T, N.corner_lists(F, nV), m0, fidelity, V, X)
    assert np.array_equal(vo[:3 * nV].reshape(3, nV).T, B) and np.array_equal(vo[3 * nV:4 * nV], iterm) and np.array_equal(vo[4 * nV:5 * nV], bsq)
    terms = np.concatenate([po[0], iterm])
    assert hook(smg, N.DN_ENERGY, V, F, None, terms, n_out=1)[0] == N.fixed_sum(terms)  # the fixed sum in its own order


def test_hand_made_rows(smg):
    """face 0 of the mirrored triple has two neighbours of equal weight: with opposite normals the sum is zero and m_0 stays, bit for bit; with its
    own normal everywhere the field is a fixed point; no iteration returns the input bits"""
    V, F = N.mirrored_triple()
    nF = F.shape[0]
    m_in = np.array([[0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [-1.0, 0.0, 0.0]])
    for iters in (1, 2):
        out = hook(smg, N.DN_FILTER, V, F, None, m_in.T.reshape(-1), n_out=3 * nF, sigma_s=1.5, normal_iters=iters).reshape(3, nF).T
        assert np.array_equal(out[0], m_in[0]) and np.array_equal(out, N.filter_normals(N.rest_constants(V, F), N.row_slots(*N.face_neighbours(F, 7)), m_in, 1.5, 0.35, iters))
    same = np.tile([0.0, 1.0, 0.0], (nF, 1))
    assert np.array_equal(hook(smg, N.DN_FILTER, V, F, None, same.T.reshape(-1), n_out=3 * nF, sigma_s=1.5, normal_iters=3).reshape(3, nF).T, same)
    odd = np.array([[0.6, 0.8, 0.0], [0.0, 0.28, 0.96], [1.0, 0.0, 0.0]])
    assert np.array_equal(hook(smg, N.DN_FILTER, V, F, None, odd.T.reshape(-1), n_out=3 * nF, sigma_s=1.5, normal_iters=0).reshape(3, nF).T, odd)


# ---- the object -------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ogre(smg):
    D, Vn, F, m, X, E = N.reference_run("ogre_sim.smgm")
    return Vn, F, smg.mg_precompute(Vn, F, 0.25, 500, 1)


def tight(smg, tol, use_graph=1):
    return smg.SolveOpts(tol=tol, max_iter=100, use_graph=use_graph)


@pytest.mark.parametrize("pcg", [0, 1], ids=["stationary", "pcg"])
def test_one_global_system_against_the_direct_solve(smg, ogre, pcg):
    """the first global step after the filter: x_1 of the object against the restatement's direct solve"""
    V, F, mg = ogre
    D = N.reference_run("ogre_sim.smgm")[0]
    _, B, bnorm = D.local(D.V)
    want = D.lu.solve(B)
    dn = smg.Denoiser(mg, V, F)
    dn.set_solver(pcg)
    dn.filter()
    got, E, cyc = dn.update(max_iter=1, opts=tight(smg, 1e-10 * bnorm))
    err = np.linalg.norm(got - want) / np.linalg.norm(want)
    print("pcg %d: |x_1 - direct| / |direct| = %.2e, %d loop entries, |b| = %.3e" % (pcg, err, cyc[0], bnorm))
    assert 0 < cyc[0] < 100 and err <= SOLVE_BOUND


def compare_run(smg, name, mg):
    D, Vn, F, m, Xn, En = N.reference_run(name)
    bnorm = D.local(D.V)[2]
    dn = smg.Denoiser(mg, Vn, F)
    assert dn.sigma_s == D.sigma_s                                                     # the rule's fixed-order sum, bit for bit
    X, E, cyc = dn.run(max_iter=10, opts=tight(smg, 1e-10 * bnorm))
    disp = np.abs(Xn - Vn).max()
    ex, ee = np.abs(X - Xn).max() / disp, np.abs(E / En - 1.0).max()
    print("%s: positions %.2e of the largest displacement %.3e, energies %.2e, loop entries %s" % (name, ex, disp, ee, cyc))
    print("  E =", np.array2string(E, precision=6))
    assert E.size == 11 and np.all(cyc > 0)
    assert ex <= RUN_POS_BOUND and ee <= RUN_ENERGY_BOUND
    assert np.all(np.diff(E) <= 1e-9 * E[:-1])                                         # descent, to what the inner solves leave undone
    return X


def test_run_on_the_noisy_cube(smg):
    Vc, F, Ps = N.cube(4)
    X = compare_run(smg, "cube", smg.Hierarchy.from_prolongs(Ps))
    clean = N.rest_constants(np.asarray(Vc), F)[:, :3]
    noisy_err, err = N.normal_error_deg(N.reference_run("cube")[1], F, clean), N.normal_error_deg(X, F, clean)
    print("noisy cube: mean normal error %.2f -> %.2f degrees, ratio %.3f" % (noisy_err, err, err / noisy_err))
    assert err <= 0.25 * noisy_err


def test_run_on_ogre_sim(smg, ogre):
    compare_run(smg, "ogre_sim.smgm", ogre[2])


def device_array(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def test_same_bits_across_calls_graphs_and_memspaces(smg, ogre):
    V, F, mg = ogre
    X0 = V + 0.01 * N.mean_edge(V, F) * np.sin(np.arange(V.size, dtype=np.float64)).reshape(V.shape)

    def run(dn, use_graph, device):
        opts = smg.SolveOpts(tol=1e-9, max_iter=50, use_graph=use_graph)
        if device:
            import torch
            dx0, dX, dm = device_array(X0), device_array(np.zeros_like(V)), device_array(np.zeros((F.shape[0], 3)))
            dn.filter_device(None, dm.data_ptr())
            E1, c1 = dn.update_device(dX.data_ptr(), dx0.data_ptr(), max_iter=3, opts=opts)
            torch.cuda.synchronize()
            X1, m = dX.cpu().numpy(), dm.cpu().numpy()
            E2, c2 = dn.run_device(dX.data_ptr(), max_iter=3, opts=opts)
            torch.cuda.synchronize()
            return [m, X1, E1, c1, dX.cpu().numpy(), E2, c2]
        m = dn.filter()
        X1, E1, c1 = dn.update(X0, max_iter=3, opts=opts)
        X2, E2, c2 = dn.run(max_iter=3, opts=opts)
        return [m, X1, E1, c1, X2, E2, c2]

    dn = smg.Denoiser(mg, V, F)
    ref = run(dn, 1, False)
    for got in (run(dn, 1, False), run(smg.Denoiser(mg, V, F), 0, False), run(smg.Denoiser(mg, V, F), 1, True), run(dn, 0, True)):
        for a, b in zip(ref, got):
            assert np.array_equal(a, b)


def test_set_filter_back_to_the_defaults_gives_the_fresh_bits(smg, ogre):
    V, F, mg = ogre
    fresh, dn = smg.Denoiser(mg, V, F), smg.Denoiser(mg, V, F)
    rule = dn.sigma_s
    want = fresh.run(max_iter=2)
    dn.set_filter(3.0 * rule, 0.5, 3)
    assert dn.sigma_s == 3.0 * rule
    other = dn.run(max_iter=2)
    assert not np.array_equal(other[0], want[0])
    dn.set_filter(-1.0, 0.0, -1)                                                       # keeps all three
    assert dn.sigma_s == 3.0 * rule and np.array_equal(dn.run(max_iter=2)[0], other[0])
    dn.set_filter(rule, 0.35, 20)
    for a, b in zip(dn.run(max_iter=2), want):
        assert np.array_equal(a, b)
    dn.set_filter(normal_iters=0)                                                      # no iteration: the latched normals are the mesh's own
    assert np.array_equal(dn.filter(), N.rest_constants(V, F)[:, :3])


def test_a_nan_in_x0_is_reported_and_changes_nothing(smg, ogre):
    V, F, mg = ogre
    L = smg._lib.load()
    dn, fresh = smg.Denoiser(mg, V, F), smg.Denoiser(mg, V, F)
    m = dn.filter()
    assert np.array_equal(m, fresh.filter())
    bad = V.copy()
    bad[1234, 1] = np.nan
    X = np.full(V.shape, -7.0)
    E = np.full(6, -7.0)
    cyc = np.full(5, -7, dtype=np.int32)
    nit = C.c_int(-7)
    rc = L.smg_denoise_update(dn.d, bad.ctypes.data, 0, 5, 0.0, None, X.ctypes.data, E.ctypes.data_as(C.POINTER(C.c_double)),
                              cyc.ctypes.data_as(C.POINTER(C.c_int)), C.byref(nit))
    assert rc == NONFINITE and nit.value == 0 and b"iteration 0" in L.smg_last_error()
    assert np.isnan(E[0]) and np.all(E[1:] == -7.0) and np.all(cyc == -7) and np.all(X == -7.0)   # nothing is written past energy_his[0]
    for a, b in zip(dn.update(max_iter=3), fresh.update(max_iter=3)):
        assert np.array_equal(a, b)


def test_an_unrelated_handle_solves_the_same_bits_around_a_run(smg, ogre):
    import scipy.sparse as sp
    from oracle import mesh_np as M
    V, F, mg = ogre
    A = (sp.diags(M.massmatrix(V, F, "voronoi").diagonal()) - 1e-3 * M.cotmatrix(V, F)).tocsr()
    other = smg.mg_precompute(V, F, 0.25, 500, 1)
    other.precompute(A)
    rhs = np.sin(np.arange(V.shape[0], dtype=np.float64))[:, None]
    opts = smg.SolveOpts(tol=1e-10, max_iter=30)
    before = other.solve(rhs, np.zeros_like(rhs), opts=opts)
    smg.Denoiser(mg, V, F).run(max_iter=3)
    after = other.solve(rhs, np.zeros_like(rhs), opts=opts)
    for a, b in zip(before, after):
        assert np.array_equal(np.asarray(a), np.asarray(b))


def test_device_bytes_are_live_buffers_and_destroy_frees_them(smg, ogre):
    V, F, mg = ogre
    live = smg._lib.load().smg_device_bytes_live
    gc.collect()
    before = live()
    dn = smg.Denoiser(mg, V, F)
    dn.run(max_iter=2)
    counted, held = dn.device_bytes(), live() - before
    print("denoise: device_bytes %d, live DevBuf bytes held %d" % (counted, held))
    del dn
    gc.collect()
    assert 0 < counted == held and live() == before
