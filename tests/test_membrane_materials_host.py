"""CPU: the StVK and tension-field StVK materials of the membrane time step (include/smg.h: smg_membrane_set_material) -- the
term-by-term numpy restatement (tests/membrane_materials_np.py) against finite differences and against the anchors of the reference's
configuration, the population of the three tension-field branches and the distance of every compared pose from a branch boundary, the shared
per-face maths compiled for the host against the restatement, and the ABI: symbols, refusals, the neo-Hookean bits, the registers of the new
face kernels, and a stand-alone sanitized program.
PARITY UNPINNED, as for tests/test_membrane_host.py: the reference's 06 example cannot be compiled here."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import mesh_np as M
from membrane_materials_np import (MATERIAL_NAMES, PURE, SLACK, STVK, TENSION_FIELD, WRINKLED, MaterialNp, faces_host_material, hook_material,
                                   relative_errors)
from test_membrane_host import INVALID, MEM_FACES, MESHES, NO_DEVICE, agrees, eig_fix, faces_host, load_mesh, perturbed_pose

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "membrane_material_refusals.json")
MATERIALS = (STVK, TENSION_FIELD)

# smg_membrane_faces_host_material against the restatement, per face relative to the largest term of the face's sum; the 6 x 6 Jacobi fix
# against LAPACK on the same unfixed blocks (relative Frobenius); slack faces |H' - eig_value I_9|_F / eig_value.  Each bound is 100 x the
# maximum measured on the host over both meshes, both materials and the four poses, rounded up to a power of ten:
# measured 2.2e-15, 4.2e-15, 1.1e-14, 5.3e-15, 4.0e-16
HOST_W_BOUND, HOST_G_BOUND, HOST_H_BOUND, HOST_FIX_BOUND, HOST_SLACK_BOUND = 1e-12, 1e-12, 1e-11, 1e-12, 1e-13


@pytest.fixture(scope="module")
def steps():
    """per (mesh, material): the restatement and two restated steps of four Newton iterations from rest (direct solves, the reference's defaults)"""
    out = {}
    for name in MESHES:
        V, F = load_mesh(name)
        for mat in MATERIALS:
            mb = MaterialNp(V, F, mat)
            pos, qdot, info0 = mb.step(V.copy(), np.zeros(3 * V.shape[0]), newton_iters=4)
            _, _, info1 = mb.step(pos, qdot, newton_iters=4)
            out[name, mat] = (V, F, mb, info0, info1)
    return out


def compared_poses(V, F, info0):
    """rest, the perturbed pose, 1.02 x it, and the restatement's iterate after one Newton iteration from rest"""
    P = perturbed_pose(V, F)
    return [("rest", V), ("perturbed", P), ("1.02 x perturbed", 1.02 * P), ("after Newton iteration 1", info0["poses"][1])]


# ---- 2: the restatement against finite differences, per face ------------------------------------------------------------------------------------
@pytest.mark.parametrize("mat", MATERIALS)
@pytest.mark.parametrize("name", MESHES)
def test_restatement_against_finite_differences_per_face(name, mat):
    """Central differences along a random direction d (every vertex moves by exactly eps = 1e-6 sqrt(mean double area): a unit vector per vertex),
    per face with d_f the face's nine entries:  (W_f(P + eps d) - W_f(P - eps d)) / (2 eps) against G_f . d_f, and
    |(G_f(P + eps d) - G_f(P - eps d)) / (2 eps) - H_f d_f|_2; both relative to the largest such quantity of the mesh (max |G_f . d_f|,
    max |H_f d_f|_2): the deviation of a face in units of the mesh's largest response, which does not blow up on the faces whose own
    gradient vanishes (wrinkled faces with lambda_1 -> 0, slack faces).  Poses: the perturbed pose and 1.02 x it.
    The tension-field Hessian is discontinuous across branches: a face whose branch at P +- eps d differs from its branch at P is left out, at
    most 0.5 % of a mesh; StVK leaves none out.  Bound 1e-7 on every remaining face.  What is left of it is the quotient's truncation error on
    wrinkled faces close to lambda_1 = lambda_2, where every derivative gains a factor 1 / denom: (eps |dM| / denom)^2 with denom down to
    1.5e-3 here; everywhere else the deviations are 1e-9 and below."""
    V, F = load_mesh(name)
    mb = MaterialNp(V, F, mat)
    eps = 1e-6 * np.sqrt(np.mean(M.doublearea(V, F)))
    d = np.random.default_rng(1).standard_normal(V.shape)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    df = d[F].reshape(F.shape[0], 9)
    for scale in (1.0, 1.02):
        P = scale * perturbed_pose(V, F)
        W, G, H, br, *_ = mb.faces_detail(P)
        Wp, Gp, _, brp, *_ = mb.faces_detail(P + eps * d)
        Wm, Gm, _, brm, *_ = mb.faces_detail(P - eps * d)
        keep = (brp == br) & (brm == br)
        left_out = int(np.sum(~keep))
        gd = np.einsum("fi,fi->f", G, df)
        Hd = np.einsum("fij,fj->fi", H, df)
        eG = np.abs((Wp - Wm) / (2 * eps) - gd)[keep] / np.abs(gd).max()
        eH = np.linalg.norm((Gp - Gm) / (2 * eps) - Hd, axis=1)[keep] / np.linalg.norm(Hd, axis=1).max()
        print(name, MATERIAL_NAMES[mat], "x %.2f: gradient %.2e, Hessian %.2e (%d faces above 1e-8), %d of %d faces left out"
              % (scale, eG.max(), eH.max(), int(np.sum(eH > 1e-8)), left_out, F.shape[0]))
        assert left_out <= 0.005 * F.shape[0]
        if mat == STVK:
            assert left_out == 0
        assert eG.max() <= 1e-7 and eH.max() <= 1e-7


# ---- 3: the three branches are populated; no compared pose is near a branch boundary or the floor ----------------------------------------------
BRANCH_COUNTS = {   # (pure, slack, wrinkled) at the perturbed pose and at the tension-field restatement's iterate after one Newton iteration from rest
    "ogre_sim.smgm": ((1830, 710, 2532), (3417, 218, 1437)),
    "bunny_15K_init.smgm": ((11496, 4330, 15778), (17973, 1397, 12234)),
}


@pytest.mark.parametrize("name", MESHES)
def test_branches_are_populated_and_no_pose_is_near_a_boundary(steps, name):
    smallest = np.inf
    for mat in MATERIALS:
        V, F, mb, info0, info1 = steps[name, mat]
        for label, P in compared_poses(V, F, info0):
            ok, denom_over_s = mb.margins_ok(P)
            smallest = min(smallest, denom_over_s)
            assert ok, (name, mat, label)
            _, _, H, br, *_ = mb.faces_detail(P)
            lam = np.linalg.eigvalsh(H)
            assert not np.any((lam >= 1e-8) & (lam <= 1e-4)), (name, mat, label)     # the condition of every comparison of fixed blocks
            if label == "rest":
                assert np.all(br == PURE)                                           # M == 0 exactly: l1 >= 0 and l2 >= transition l1 hold with equality
        for info in (info0, info1):
            assert sum(info["band"]) == 0 and len(info["band"]) == 4               # ... and along two restated steps of four iterations
    V, F, mb, info0, _ = steps[name, TENSION_FIELD]
    counts = [tuple(int(c) for c in np.bincount(mb.branches(P)[0], minlength=3)) for P in (perturbed_pose(V, F), info0["poses"][1])]
    print(name, "pure / slack / wrinkled:", counts, "smallest denom / s: %.2e" % smallest)
    assert tuple(counts) == BRANCH_COUNTS[name]
    assert all(min(c) > 0 for c in counts)


# ---- 4: restated steps, the anchors ----------------------------------------------------------------------------------------------------------------
ANCHORS = {   # |b| over the four Newton iterations of step 0, the objective before the first and after the last
    ("ogre_sim.smgm", STVK): ([(50.47, 4), (0.1648, 4), (1.389e-3, 4), (6.72e-5, 3)], (-1179247.3, 8), (-1180449.86, 9)),
    ("ogre_sim.smgm", TENSION_FIELD): ([(50.47, 4), (3.263, 4), (0.5478, 4), (0.0168, 3)], (-1179247.3, 8), (-1180461.86, 9)),
    ("bunny_15K_init.smgm", STVK): ([(7.852, 4), (1.691, 4), (0.0561, 3), (8.945e-3, 4)], (-115249.873, 9), (-115635.472, 9)),
    ("bunny_15K_init.smgm", TENSION_FIELD): ([(7.852, 4), (2.192, 4), (4.372, 4), (1.112, 4)], (-115249.873, 9), (-115652.946, 9)),
}


@pytest.mark.parametrize("mat", MATERIALS)
@pytest.mark.parametrize("name", MESHES)
def test_restated_steps_and_anchors(steps, name, mat):
    V, F, mb, info0, info1 = steps[name, mat]
    bn, first, last = ANCHORS[name, mat]
    print(name, MATERIAL_NAMES[mat], "|b|", info0["bnorm"], "objective", info0["objective"], "alpha", info0["alpha"])
    for k, (ref, digits) in enumerate(bn):
        assert agrees(info0["bnorm"][k], ref, digits), (k, info0["bnorm"][k], ref)
    assert agrees(info0["objective"][0], *first) and agrees(info0["objective"][-1], *last)
    for info in (info0, info1):
        assert np.all(np.array(info["alpha"]) == 1.0)
        assert np.all(np.diff(info["objective"]) <= 0)                              # the objective never rises


# ---- 5: the shared maths on the host --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MESHES)
def test_shared_maths_on_the_host(smg_mod, steps, name):
    """smg_membrane_inl.hpp compiled for the host against the restatement: W, G and the unfixed H per face, relative to the largest-magnitude
    term that enters the face's sum (for a wrinkled face that includes the 1 / denom^3 term); the 6 x 6 Jacobi fix against LAPACK's
    Q fix(Lambda) Q^T of the SAME unfixed blocks; slack faces come out as eig_value I_9."""
    worst = np.zeros(5)
    rest = {}
    for mat in MATERIALS:
        V, F, mb, info0, _ = steps[name, mat]
        for label, P in compared_poses(V, F, info0):
            W, G, H, br, sW, sG, sH = mb.faces_detail(P)
            Wl, Gl, Hl = faces_host_material(smg_mod, V, P, F, mat, 0)
            assert np.array_equal(faces_host_material(smg_mod, V, P, F, mat, 0, derivs=False), Wl)           # energy only: the same text
            if label == "rest":
                assert not Wl.any() and not Gl.any() and not W.any() and not G.any()                          # exactly zero
                rest[mat] = (Wl, Gl, Hl)
            eW, eG, eH = relative_errors(Wl, W, sW), relative_errors(Gl, G, sG), relative_errors(Hl, H, sH)
            slack_l = (Wl == 0.0) & (np.abs(Hl).reshape(len(Wl), -1).max(axis=1) == 0.0) & (np.abs(Gl).max(axis=1) == 0.0)
            if label != "rest":
                assert np.array_equal(slack_l, br == SLACK)
            ref, lam = eig_fix(Hl, mb.p["eig_floor"], mb.p["eig_value"])
            assert not np.any((lam >= 1e-8) & (lam <= 1e-4))
            Wf, Gf, Hf = faces_host_material(smg_mod, V, P, F, mat, 1)
            assert np.array_equal(Wf, Wl) and np.array_equal(Gf, Gl)
            eF = (np.linalg.norm(Hf - ref, axis=(1, 2)) / np.linalg.norm(ref, axis=(1, 2))).max()
            lmin = np.linalg.eigvalsh(Hf).min()
            sl = br == SLACK
            eS = np.linalg.norm(Hf[sl] - mb.p["eig_value"] * np.eye(9), axis=(1, 2)).max() / mb.p["eig_value"] if sl.any() else 0.0
            print(name, MATERIAL_NAMES[mat], label, "W %.2e G %.2e H %.2e fix %.2e slack %.2e lambda_min %.6e" % (eW, eG, eH, eF, eS, lmin))
            worst = np.maximum(worst, [eW, eG, eH, eF, eS])
            assert lmin >= mb.p["eig_floor"] * (1 - 1e-9)
    assert all(np.array_equal(x, y) for x, y in zip(rest[STVK], rest[TENSION_FIELD]))      # at rest the tension-field block IS the StVK block
    print(name, "worst W %.2e G %.2e H %.2e fix %.2e slack %.2e" % tuple(worst))
    assert worst[0] <= HOST_W_BOUND and worst[1] <= HOST_G_BOUND and worst[2] <= HOST_H_BOUND
    assert worst[3] <= HOST_FIX_BOUND and worst[4] <= HOST_SLACK_BOUND


# ---- 6: ABI and behaviour ----------------------------------------------------------------------------------------------------------------------------
def test_abi_present_and_typed(smg_mod):
    L = smg_mod._lib.load()
    sig = L._smg_signatures
    ip, dp, vp, i = C.POINTER(C.c_int), C.POINTER(C.c_double), C.c_void_p, C.c_int
    prm = C.POINTER(smg_mod._lib.MembraneParamsC)
    want = {"smg_membrane_set_material": (i, [vp, i]), "smg_membrane_material": (i, [vp]),
            "smg_membrane_faces_host_material": (i, [dp, dp, i, ip, i, prm, i, i, dp, dp, dp]),
            "smg_debug_membrane_material": (i, [i, i, i, i, ip, dp, dp, dp, prm, dp, ip])}
    for name, (res, args) in want.items():
        assert hasattr(L, name) and sig[name] == (res, args), name
        assert getattr(L, name).restype is res and list(getattr(L, name).argtypes) == args
    assert L.smg_membrane_material(None) == 0
    assert L.smg_version() >= 510
    sim = smg_mod.MembraneSim
    assert sim.MATERIALS == ("neo_hookean", "stvk", "tension_field") and hasattr(sim, "set_material") and isinstance(sim.material, property)
    with pytest.raises(ValueError):
        sim._material_id("rubber")
    txt = open(os.path.join(ROOT, "surface_multigrid_code_amd", "csrc", "mg_api.hpp")).read()
    assert "smg_membrane_set_material" in txt


def collect_refusals(smg):
    """every refusal that needs no device: (code, smg_last_error())"""
    from test_geodesics_host import icosphere
    L = smg._lib.load()
    V, F = icosphere(1)
    nF = F.shape[0]
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    prm = smg.membrane_params()
    W = np.zeros(nF)
    out = {}

    def record(label, rc):
        out[label] = [int(rc), L.smg_last_error().decode()]

    for mat in (0, 1, 2, 3, -1):
        record("set_material(NULL, %d)" % mat, L.smg_membrane_set_material(None, mat))
    for mat in (3, -1):
        Fi = np.ascontiguousarray(F, dtype=np.int32)
        record("faces_host_material, material %d" % mat,
               L.smg_membrane_faces_host_material(V.ctypes.data_as(dp), V.ctypes.data_as(dp), V.shape[0], Fi.ctypes.data_as(ip), nF, C.byref(prm), mat, 0,
                                                  W.ctypes.data_as(dp), None, None))
        record("debug hook, material %d" % mat, hook_material(smg, mat, MEM_FACES, V, F, V, None, 55 * nF)[0])
    Fi = np.ascontiguousarray(F, dtype=np.int32)
    record("faces_host_material, null W",
           L.smg_membrane_faces_host_material(V.ctypes.data_as(dp), V.ctypes.data_as(dp), V.shape[0], Fi.ctypes.data_as(ip), nF, C.byref(prm), 1, 0, None, None, None))
    record("debug hook, unknown op", hook_material(smg, 1, 8, V, F, V, None, 55 * nF)[0])
    record("debug hook, the pose missing", hook_material(smg, 2, MEM_FACES, V, F, None, None, 55 * nF)[0])
    return out


def test_refusals_match_the_golden_file(smg_mod):
    got = collect_refusals(smg_mod)
    want = json.load(open(GOLDEN))
    for label, (code, text) in want["no device needed"].items():
        assert got[label] == [code, text], (label, got[label])
        assert code == INVALID and text.split(":")[0] in ("smg_membrane_set_material", "smg_membrane_faces_host_material", "smg_debug_membrane_material")
    assert sorted(got) == sorted(want["no device needed"])
    if smg_mod._lib.load().smg_device_count() == 0:
        from test_geodesics_host import icosphere
        V, F = icosphere(1)
        for mat in (0, 1, 2):
            assert hook_material(smg_mod, mat, MEM_FACES, V, F, V, None, 55 * F.shape[0])[0] == NO_DEVICE


def write_golden():      # python -c "import sys; sys.path[:0] = ['.', 'tests']; import test_membrane_materials_host as t; t.write_golden()"
    import surface_multigrid_code_amd as smg
    want = {"no device needed": collect_refusals(smg),
            "on an object": {"set_material(3)": [INVALID, "smg_membrane_set_material: material 3 is not 0 (neo-Hookean), 1 (StVK) or 2 (tension-field StVK)"],
                             "set_material(-1)": [INVALID, "smg_membrane_set_material: material -1 is not 0 (neo-Hookean), 1 (StVK) or 2 (tension-field StVK)"]}}
    json.dump(want, open(GOLDEN, "w"), indent=1, sort_keys=True)


@pytest.mark.parametrize("name", MESHES)
def test_material_0_has_the_bits_of_faces_host(smg_mod, name):
    V, F = load_mesh(name)
    for P in (V, perturbed_pose(V, F)):
        for fix in (0, 1):
            for x, y in zip(faces_host(smg_mod, V, P, F, fix), faces_host_material(smg_mod, V, P, F, 0, fix)):
                assert np.array_equal(x, y)


def test_material_face_kernels_keep_everything_in_registers():
    """the ISA notes of k_membrane_faces_mat<MODE, MAT> (the build's flags, device side only), exactly one kernel per (mode, material): no
    scratch and no spills in any mode of either material; at most 168 VGPRs (512 / 168 = 3 waves per SIMD, the budget of the neo-Hookean kernel)
    with the fix and without, 64 (8 waves) for the energy alone.  DESIGN.md section 20: 52 / 142 / 160 (StVK), 56 / 142 / 156 (tension field)."""
    from surface_multigrid_code_amd import build as B
    src = os.path.join(B.CSRC, "smg_membrane_device.hip")
    asm = subprocess.check_output([B._hipcc()] + B.FLAGS + ["--cuda-device-only", "-S", src, "-o", "-"], text=True)
    for mat in (1, 2):
        for mode, cap in ((0, 64), (1, 168), (2, 168)):
            notes = re.findall(r"\.name:\s+(\S*k_membrane_faces_matILi%dELi%dE\S*)(.*?)\.wavefront_size" % (mode, mat), asm, flags=re.S)
            assert len(notes) == 1
            body = notes[0][1]
            field = lambda k: int(re.search(r"\.%s:\s+(\d+)" % k, body).group(1))   # noqa: E731
            print("k_membrane_faces_mat<%d, %d>: vgpr_count %d, private_segment_fixed_size %d, vgpr_spill_count %d"
                  % (mode, mat, field("vgpr_count"), field("private_segment_fixed_size"), field("vgpr_spill_count")))
            assert field("private_segment_fixed_size") == 0 and field("vgpr_spill_count") == 0
            assert field("vgpr_count") <= cap


def test_stand_alone_program_under_asan_ubsan(tmp_path):
    """tests/membrane_material_asan_driver.cpp (its own main) calls smg_membrane_faces_host_material on a small strip for the three materials.  It
    is compiled with -fsanitize=address,undefined and linked with the sanitized host objects of the library (the device objects unchanged) and
    the static sanitizer runtimes into one program, which is run directly: no sanitizer in anything python loads, nothing preloaded."""
    from surface_multigrid_code_amd import build as B
    B.build_sanitized()                                                            # lib/obj_asan/*.o: the host translation units under the sanitizers
    objs = [os.path.join(B.LIBDIR, "obj" if s.endswith(".hip") else "obj_asan", os.path.splitext(s)[0] + ".o") for s in B.SOURCES]
    exe = str(tmp_path / "membrane_material_asan_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-fno-omit-frame-pointer",
                           "-fno-sanitize-recover=undefined", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "membrane_material_asan_driver.cpp")] + objs +
                          ["-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib", "-lpthread", "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1:abort_on_error=0:protect_shadow_gap=0:detect_odr_violation=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    out = r.stdout + r.stderr
    assert "AddressSanitizer" not in out and "runtime error:" not in out, out[-4000:]
    assert r.returncode == 0 and "MEMBRANE_MATERIAL_DRIVER OK" in out, out[-4000:]
    zero = dict(re.findall(r"material (\d): \d+ faces, (\d+) with W == 0", out))
    assert zero["0"] == "0" and zero["1"] == "0" and int(zero["2"]) > 0                # the strip has slack faces, which only the tension field zeroes
