"""GPU (-m gpu): the StVK and tension-field StVK materials of the membrane time step (include/smg.h: smg_membrane_set_material; DESIGN.md
section 20).

The host reference is the term-by-term restatement of tests/membrane_materials_np.py (checked on the CPU by tests/test_membrane_materials_host.py).
The new face kernels k_membrane_faces_mat<MODE, MAT> are held through smg_debug_membrane_material (guarded buffers): hand-made single faces in
each tension-field branch, strips whose lanes cycle through the three branches across the 64-lane block edge, the per-face outputs on the two
fixtures, the assembly in list order, one Newton system, one time step, and switching materials on a live object.

Every bound that is not bit-equality is meant to be 100 x the maximum measured on an MI355X, rounded up to a power of ten (the convention of
DESIGN.md section 19).  NOT MEASURED YET on an MI355X: until the first GPU run the per-face bounds are the host twin's (the same text compiled
for the host, tests/test_membrane_materials_host.py: 100 x its measured maxima), and the bounds of the Newton system and of the step are the
neo-Hookean ones of the same mesh and tolerances (tests/test_gpu_membrane.py); DESIGN.md section 20 says the same.  W, G and the unfixed H are
compared per face, relative to the largest-magnitude term that enters the face's sum in the restatement (for a wrinkled face that includes
the 1 / denom^3 term)."""
import json

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from denoise_np import edge_shapes
from test_gpu_membrane import check_sums
from test_gpu_parity import smg  # noqa: F401  (fixture)
from membrane_materials_np import (MATERIAL_NAMES, PURE, SLACK, STVK, TENSION_FIELD, WRINKLED, MaterialNp, fan_mesh, fan_pose, hook_material,
                                   infer_branch, relative_errors, strip_mesh, strip_pose)
from test_membrane_host import (MEM_ENERGY, MEM_FACES, MEM_FACES_RAW, MEM_GRADIENT, MEM_MATRIX, MEM_PRESSURE, corner_lists, eig_fix, lists, load_mesh,
                                matrix_values_np, perturbed_pose, scalar_pattern, unpack_upper)
from test_membrane_materials_host import GOLDEN

pytestmark = pytest.mark.gpu

MATERIALS = (STVK, TENSION_FIELD)
# per-face W, G, unfixed H against the restatement: the host twin measures 2.2e-15, 4.2e-15, 1.1e-14
W_BOUND, G_BOUND, H_BOUND = 1e-12, 1e-12, 1e-11
FIX_BOUND = 1e-12           # |H' - Q fix(Lambda) Q^T|_F / |.|_F against LAPACK on the device's unfixed blocks: the host twin measures 5.3e-15
SLACK_BOUND = 1e-13         # slack faces, |H' - eig_value I_9|_F / eig_value: the host twin measures 4.0e-16
# |dx - dx_np| / |dx_np| of one Newton system on ogre_sim from the perturbed pose, tol 1e-10 |b| (neo-Hookean from the rest pose: 4.1e-11)
SOLVE_BOUND = 1e-8
STEP_POS_BOUND, STEP_OBJ_BOUND = 1e-7, 1e-13      # a step of three Newton iterations: positions over the largest displacement; objectives


def call(smg, mat, op, V0, F, P, inp, n_out, **params):
    rc, bad, out = hook_material(smg, mat, op, V0, F, P, inp, n_out, **params)
    assert rc == 0 and bad == 0, (rc, bad, smg._lib.load().smg_last_error())
    assert not np.any(np.isnan(out))
    return out


def device_faces(smg, mat, V, F, P, fixed):
    nF = F.shape[0]
    o = call(smg, mat, MEM_FACES if fixed else MEM_FACES_RAW, V, F, P, None, 55 * nF)
    return o[:nF], o[nF:10 * nF].reshape(9, nF), o[10 * nF:].reshape(45, nF)


def compare_faces(smg, mb, V, F, P, label, expect_branch=None):
    """every per-face output of the material's kernels at P against the restatement; returns the five maxima (W, G, H, fix, slack)"""
    mat = mb.material
    p = mb.p
    nF = F.shape[0]
    assert mb.margins_ok(P)[0], label                                                   # the condition of the comparison: no face near a boundary
    W, G, H, br, sW, sG, sH = mb.faces_detail(P)
    Wd, Gd, Hd = device_faces(smg, mat, V, F, P, False)
    assert np.array_equal(call(smg, mat, MEM_ENERGY, V, F, P, None, nF), Wd)           # the line search's kernel: the same bits
    Hu = unpack_upper(Hd)
    eW, eG, eH = relative_errors(Wd, W, sW), relative_errors(Gd.T, G, sG), relative_errors(Hu, H, sH)
    if mat == TENSION_FIELD:                                                            # the branch every lane took, none left out
        got, near, far = infer_branch(mb, P, Wd, Hu, sH)
        assert np.array_equal(got, br), (label, np.nonzero(got != br)[0][:10])
        live = br != SLACK
        assert near.max() <= H_BOUND and (not live.any() or far[live].min() > 1e3 * H_BOUND)      # the other formula is far away
        assert not Gd[:, br == SLACK].any()
    if expect_branch is not None:
        assert np.array_equal(br, expect_branch), (label, br)
    ref_fix, lam = eig_fix(Hu, p["eig_floor"], p["eig_value"])                          # LAPACK on the DEVICE's unfixed blocks
    assert not np.any((lam >= 1e-8) & (lam <= 1e-4))
    Wf, Gf, Hf = device_faces(smg, mat, V, F, P, True)
    assert np.array_equal(Wf, Wd) and np.array_equal(Gf, Gd)
    Hfu = unpack_upper(Hf)
    eF = (np.linalg.norm(Hfu - ref_fix, axis=(1, 2)) / np.linalg.norm(ref_fix, axis=(1, 2))).max()
    sl = br == SLACK
    eS = np.linalg.norm(Hfu[sl] - p["eig_value"] * np.eye(9), axis=(1, 2)).max() / p["eig_value"] if sl.any() else 0.0
    lmin = np.linalg.eigvalsh(Hfu).min()
    print(label, MATERIAL_NAMES[mat], "W %.2e G %.2e H %.2e fix %.2e slack %.2e lambda_min %.6e branches %s"
          % (eW, eG, eH, eF, eS, lmin, np.bincount(br, minlength=3)))
    assert lmin >= p["eig_floor"] * (1 - 1e-9)
    return np.array([eW, eG, eH, eF, eS])


def within_bounds(worst):
    return worst[0] <= W_BOUND and worst[1] <= G_BOUND and worst[2] <= H_BOUND and worst[3] <= FIX_BOUND and worst[4] <= SLACK_BOUND


@pytest.fixture(scope="module")
def ogre():
    """ogre_sim: per material the restatement and its step of three Newton iterations from rest with direct solves"""
    V, F = load_mesh("ogre_sim.smgm")
    out = {"V": V, "F": F}
    for mat in MATERIALS:
        mb = MaterialNp(V, F, mat)
        _, _, info = mb.step(V.copy(), np.zeros(3 * V.shape[0]), newton_iters=3)
        out[mat] = (mb, info)
    return out


# ---- 1: hand-made single faces, one per branch; a two-triangle square ---------------------------------------------------------------------------
REST_TRIANGLE = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.2, 0.9, 0.0]])
ROTATION = np.array([[0.8, 0.0, 0.6], [0.0, 1.0, 0.0], [-0.6, 0.0, 0.8]])
STRETCHES = [((1.1, 1.2), PURE), ((0.9, 0.8), SLACK), ((1.3, 0.7), WRINKLED)]      # principal stretches: both > 1; both < 1; one > 1, one well below the transition


@pytest.mark.parametrize("mat", MATERIALS)
def test_single_faces_in_each_branch(smg, mat):
    worst = np.zeros(5)
    F = np.array([[0, 1, 2]], dtype=np.int32)
    for (sx, sy), branch in STRETCHES:
        P = (REST_TRIANGLE * [sx, sy, 1.0]) @ ROTATION.T + [0.3, -0.2, 0.1]
        mb = MaterialNp(REST_TRIANGLE, F, mat)
        expect = np.array([branch if mat == TENSION_FIELD else PURE])
        worst = np.maximum(worst, compare_faces(smg, mb, REST_TRIANGLE, F, P, "triangle %s" % ((sx, sy),), expect))
    Vq = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [1.0, 1.0, 0.0], [0.0, 1.0, 0.0]])
    Fq = np.array([[0, 1, 2], [0, 2, 3]], dtype=np.int32)
    mb = MaterialNp(Vq, Fq, mat)
    for (sx, sy), _ in STRETCHES:
        Pq = (Vq * [sx, sy, 1.0]) @ ROTATION.T
        Pq[2] += [0.0, 0.05, 0.1]                                                  # the shared diagonal's far corner out of the plane
        worst = np.maximum(worst, compare_faces(smg, mb, Vq, Fq, Pq, "square %s" % ((sx, sy),)))
    worst = np.maximum(worst, compare_faces(smg, mb, Vq, Fq, Vq, "square at rest", np.array([PURE, PURE])))
    assert within_bounds(worst), worst


# ---- 2: strips across the block edge and a fan; consecutive lanes cycle through the three branches ----------------------------------------------
@pytest.mark.parametrize("mat", MATERIALS)
def test_strips_and_a_fan_with_divergent_lanes(smg, mat):
    worst = np.zeros(5)
    for label, (V, F), pose in [("strip %d" % n, strip_mesh(n), strip_pose) for n in (63, 64, 65)] + [("fan 65", fan_mesh(65), fan_pose)]:
        P = pose(V)
        mb = MaterialNp(V, F, mat)
        br = MaterialNp(V, F, TENSION_FIELD).branches(P)[0]
        assert np.all(br[1:] != br[:-1]) and np.all(br[2:] != br[:-2]) and np.bincount(br, minlength=3).min() >= 21      # period 3 in the lanes
        assert mb.margins_ok(P, rel=1e-2)[0]
        worst = np.maximum(worst, compare_faces(smg, mb, V, F, P, label, br if mat == TENSION_FIELD else None))
        worst = np.maximum(worst, compare_faces(smg, mb, V, F, V, label + " at rest", np.zeros(F.shape[0], dtype=np.int64)))
    assert within_bounds(worst), worst


# ---- 3: the per-face outputs on the fixtures ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mat", MATERIALS)
def test_face_kernels_against_the_restatement(smg, ogre, mat):
    V, F = ogre["V"], ogre["F"]
    mb, info = ogre[mat]
    Pp = perturbed_pose(V, F)
    worst = np.zeros(5)
    for label, P in (("rest", V), ("perturbed", Pp), ("1.02 x perturbed", 1.02 * Pp), ("after Newton iteration 1", info["poses"][1])):
        worst = np.maximum(worst, compare_faces(smg, mb, V, F, P, "ogre_sim " + label, np.zeros(F.shape[0], dtype=np.int64) if label == "rest" else None))
        if label == "rest":
            Wd, Gd, _ = device_faces(smg, mat, V, F, V, False)
            assert not Wd.any() and not Gd.any()                                    # exactly zero
    Vb, Fb = load_mesh("bunny_15K_init.smgm")
    worst = np.maximum(worst, compare_faces(smg, MaterialNp(Vb, Fb, mat), Vb, Fb, perturbed_pose(Vb, Fb), "bunny_15K_init perturbed"))
    print(MATERIAL_NAMES[mat], "worst W %.2e G %.2e H %.2e fix %.2e slack %.2e" % tuple(worst))
    assert within_bounds(worst), worst


def test_tension_field_at_rest_is_stvk_bit_for_bit(smg, ogre):
    V, F = ogre["V"], ogre["F"]
    for fixed in (False, True):
        for x, y in zip(device_faces(smg, STVK, V, F, V, fixed), device_faces(smg, TENSION_FIELD, V, F, V, fixed)):
            assert np.array_equal(x, y)


def test_material_0_of_the_hook_is_the_neo_hookean_kernel(smg, ogre):
    from test_membrane_host import hook
    V, F = ogre["V"], ogre["F"]
    P = perturbed_pose(V, F)
    for op, n in ((MEM_FACES, 55), (MEM_FACES_RAW, 55), (MEM_ENERGY, 1)):
        rc, bad, ref = hook(smg, op, V, F, P, None, n * F.shape[0])
        assert rc == 0 and bad == 0
        assert np.array_equal(call(smg, 0, op, V, F, P, None, n * F.shape[0]), ref)


# ---- 4: the assembly in list order ----------------------------------------------------------------------------------------------------------------
def device_mass(smg, mat, V, F, P):
    nF, nV = F.shape[0], V.shape[0]
    o = call(smg, mat, MEM_PRESSURE, None, F, P, None, 6 * nF + 4 * nV)
    return o[6 * nF:6 * nF + nV], o[6 * nF + nV:]


@pytest.mark.parametrize("mat", MATERIALS)
def test_sums_are_bitwise_the_documented_ones(smg, ogre, mat):
    """the downstream kernels are unchanged, so one pose is enough: matrix values, gradient and b are numpy sums of the DEVICE's per-face outputs
    in list order"""
    V, F = ogre["V"], ogre["F"]
    mb, _ = ogre[mat]
    nV, p = V.shape[0], mb.p
    P = perturbed_pose(V, F)
    lsts = lists(smg, F, nV)
    mass0, _ = device_mass(smg, mat, V, F, V)
    _, fext = device_mass(smg, mat, V, F, P)
    _, Gd, Hd = device_faces(smg, mat, V, F, P, True)
    val = call(smg, mat, MEM_MATRIX, None, F, None, np.concatenate([Hd.reshape(-1), mass0]), 9 * lsts[1].shape[0])
    assert np.array_equal(val, matrix_values_np(Hd, mass0, lsts, p["dt"], p["mass_scale"]))
    rng = np.random.default_rng(3)
    qdot, qdot0 = rng.standard_normal(3 * nV), rng.standard_normal(3 * nV)
    o = call(smg, mat, MEM_GRADIENT, None, F, None, np.concatenate([Gd.reshape(-1), mass0, qdot, qdot0, fext]), 6 * nV)
    g_np = np.zeros((nV, 3))
    for rows, ts in corner_lists(F, nV):
        f, j = ts // 3, ts % 3
        for l in range(3):
            g_np[rows, l] += Gd[3 * j + l, f]
    g_np = g_np.reshape(-1)
    mv = np.repeat(p["mass_scale"] * mass0, 3)
    b_np = -((mv * (qdot - qdot0) + p["dt"] * g_np) + p["dt"] * fext)
    assert np.array_equal(o[:3 * nV], g_np) and np.array_equal(o[3 * nV:], b_np)


@pytest.mark.parametrize("name", ["fan65", "strip255"])
@pytest.mark.parametrize("mat", MATERIALS)
def test_sums_on_edge_shapes(smg, mat, name):
    """the summing launchers are shared by the three materials: the same sums from these materials' face outputs on the fan (a 65-long block
    list and corner list) and on a strip with 257 vertices and 255 faces, at rest and perturbed"""
    V, F = edge_shapes()[name]
    check_sums(smg, "%s %s" % (name, MATERIAL_NAMES[mat]), V, F, MaterialNp(V, F, mat), [V, perturbed_pose(V, F)], mat=mat, restatement=False)


# ---- 5: one Newton system -----------------------------------------------------------------------------------------------------------------------------
def device_system(smg, mat, V, F, P, qdot, qdot0, fext_pose):
    nV = V.shape[0]
    lsts = lists(smg, F, nV)
    mass0, _ = device_mass(smg, mat, V, F, V)
    _, fext = device_mass(smg, mat, V, F, fext_pose)
    _, Gd, Hd = device_faces(smg, mat, V, F, P, True)
    val = call(smg, mat, MEM_MATRIX, None, F, None, np.concatenate([Hd.reshape(-1), mass0]), 9 * lsts[1].shape[0])
    o = call(smg, mat, MEM_GRADIENT, None, F, None, np.concatenate([Gd.reshape(-1), mass0, qdot, qdot0, fext]), 6 * nV)
    rowptr, col = scalar_pattern(lsts[0], lsts[1])
    return sp.csr_matrix((val, col, rowptr), shape=(3 * nV, 3 * nV)), o[3 * nV:]


@pytest.mark.parametrize("mat", MATERIALS)
def test_one_newton_system(smg, ogre, mat):
    """ogre_sim at the perturbed pose (velocity 0): the system assembled by the device, solved by the stationary loop and by PCG to
    tol = 1e-10 |b|, against the restatement's system solved directly"""
    V, F = ogre["V"], ogre["F"]
    mb, _ = ogre[mat]
    nV = V.shape[0]
    P = perturbed_pose(V, F)
    zero = np.zeros(3 * nV)
    _, Hn, bn, _ = mb.system(P, zero, zero, mb.pressure_force(P))
    dxn = spla.spsolve(Hn.tocsc(), bn)
    mg = smg.mg_precompute_block(V, F)
    H0, _ = device_system(smg, mat, V, F, V, zero, zero, V)
    mg.precompute(H0)                                                   # the pattern; the next precompute is the value-only path
    H, b = device_system(smg, mat, V, F, P, zero, zero, P)
    mg.precompute(H)
    assert mg.block_size() == 3
    worst = 0.0
    for pcg in (False, True):
        opts = smg.SolveOpts(tol=1e-10 * np.linalg.norm(b), max_iter=100)
        conv, z, his = (mg.solve_pcg if pcg else mg.solve)(b.reshape(-1, 1), zero.reshape(-1, 1), None, opts)
        err = np.linalg.norm(z[:, 0] - dxn) / np.linalg.norm(dxn)
        print(MATERIAL_NAMES[mat], "%s: %d loop entries, |dx - dx_np| / |dx_np| = %.2e" % ("PCG" if pcg else "stationary", len(his), err))
        assert conv
        worst = max(worst, err)
    assert worst <= SOLVE_BOUND


# ---- 6: one time step --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mat", MATERIALS)
def test_step_against_the_restatement(smg, ogre, mat):
    V, F = ogre["V"], ogre["F"]
    mb, info = ogre[mat]
    mg = smg.mg_precompute_block(V, F)
    sim = smg.MembraneSim(mg, V, F, material=MATERIAL_NAMES[mat], newton_iters=3)
    assert sim.material == MATERIAL_NAMES[mat]
    sim.set_solver(1)
    opts = smg.SolveOpts(tol=1e-10 * info["bnorm"][0], max_iter=100)
    r = sim.step(opts)
    pos, qdot = sim.state()
    ref = info["poses"][3]
    e_pos = np.abs(pos - ref).max() / np.abs(ref - V).max()
    obj = np.array(info["objective"])
    e_obj = np.abs(r["objective"] - obj).max() / np.abs(obj).max()
    print(MATERIAL_NAMES[mat], "pos %.2e objective %.2e alpha %s cycles %s" % (e_pos, e_obj, r["alpha"], r["cycles"]))
    assert np.array_equal(r["alpha"], info["alpha"]) and np.all(r["alpha"] == 1.0)
    assert e_pos <= STEP_POS_BOUND and e_obj <= STEP_OBJ_BOUND
    sim.set_state()                                                        # the same inputs give the same bits
    r2 = sim.step(opts)
    pos2, qdot2 = sim.state()
    assert all(np.array_equal(r[k], r2[k]) for k in ("objective", "alpha", "cycles")) and np.array_equal(pos, pos2) and np.array_equal(qdot, qdot2)


# ---- 7: switching materials ----------------------------------------------------------------------------------------------------------------------------
def test_switching_materials(smg, ogre):
    V, F = ogre["V"], ogre["F"]
    L = smg._lib.load()
    mg = smg.mg_precompute_block(V, F)

    def result(sim):
        r = sim.step()
        return [r["objective"], r["alpha"], r["cycles"], *sim.state()]

    same = lambda x, y: all(np.array_equal(a, b) for a, b in zip(x, y))   # noqa: E731
    untouched = smg.MembraneSim(mg, V, F, newton_iters=2)
    assert untouched.material == "neo_hookean"
    first = result(untouched)
    reset = smg.MembraneSim(mg, V, F, newton_iters=2)
    reset.set_material(0)
    assert same(first, result(reset))                                       # set_material(0) on a fresh object: the bits of an untouched one
    # a refused value leaves the material alone; code and text are the golden file's
    want = json.load(open(GOLDEN))["on an object"]
    for bad in (3, -1):
        rc = L.smg_membrane_set_material(untouched.m, bad)
        assert [rc, L.smg_last_error().decode()] == want["set_material(%d)" % bad]
        assert untouched.material == "neo_hookean"
    # the stepped object goes on with the tension field; a fresh tension-field object given the same state returns the same bits
    state = untouched.state()
    untouched.set_material("tension_field")
    assert untouched.material == "tension_field" and same(state, untouched.state())     # the state is kept
    a = result(untouched)
    fresh = smg.MembraneSim(mg, V, F, newton_iters=2)
    fresh.set_material(2)
    fresh.set_state(*state)
    b = result(fresh)
    assert same(a, b)
    assert not same(a[-2:], first[-2:])
    # ... and the material really is another one: stepped from the same state with StVK the positions differ
    other = smg.MembraneSim(mg, V, F, material="stvk", newton_iters=2)
    other.set_state(*state)
    assert not np.array_equal(result(other)[3], a[3])
