"""CPU: Born traces and Gauss-Newton products of the wave object (include/smg.h: smg_wave_gauss_newton) -- the ABI and its refusals without a GPU,
the library's host twin (smg_wave_born_host) against the numpy restatement (tests/wave_gn_np.py) bit for bit, and the restatement's J d and
H d = J' J d against derivatives and identities that do not use them.

The two setups are those the derivation was checked on: icosphere(2) free and sinkhorn_np.regular_square(8) clamped, non-uniform speed and sigma,
dt = 0.05, 8 forced steps, k = 3, three Ricker sources, four receiver slots with one vertex twice, noisy observed traces, direct solves.

    DERIVATIVE  the traces are evaluated once more in complex arithmetic (wave_adjoint_np.misfit_complex's states) at speed + i h d, h = 1e-30:
                Im traces / h is J d with no subtraction.  Asserted within 1e-12 of the largest entry, the scale tests/test_wave_adjoint_host.py
                uses for complex-step comparisons (measured here: 4.5e-14 on the sphere, 9.5e-15 on the square).
    IDENTITIES  <d, H d> = sum (J d)^2 per column and <w, H d> = <J w, J d>: the adjoint pass is the exact transpose of the tangent run.  Asserted
                within relative 1e-12 (measured here: at most 1.5e-15 and at most 1.2e-14).
    LINEARITY   H (2 d1 - 3 d2) against 2 H d1 - 3 H d2, per column relative to the norm of the left side.  Both sides are sums of the same
                products rounded in another order; measured 4.7e-16 to 2.0e-15 on the two setups, asserted at 100 times the largest measured
                value, 2.0e-13 (no looser than 1e-10).
    ROUTE       H d against grad_speed of wave_adjoint_np.gradient with observed = traces - J d, whose residual is J d up to the rounding of
                the subtraction, eps |traces| per entry.  d is scaled so that max |J d| is 5e-2 max |traces|; the subtraction then costs about
                eps / 5e-2 = 4.4e-15 relative.  Measured 1.4e-16 to 9.6e-16 per column relative to |H d|, asserted at 100 times the largest, 9.6e-14
                (no looser than 1e-10).
    TAYLOR      traces(speed + h d) - traces(speed) - h J d = O(h^2): from h = 1e-3 to 5e-4 its norm per column falls by a factor within
                4 +- 0.1, on a one-signed d (tests/test_wave_adjoint_host.py: TAYLOR uses the same direction and range).
    ZERO        the product is exactly 0.0 on clamped rows although boundary corners are receivers; d = 0 gives exact zeros, every
                right-hand side exactly 0.0 (every solve skipped) and curvature 0.0."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import sinkhorn_np
import wave_adjoint_np as A
import wave_gn_np as G
import wave_np as N
from test_wave_host import INVALID, NO_DEVICE, ROOT, check_cases, launcher_cases, ricker_signal

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wave_gn_refusals.json")
SYMBOLS = ("smg_wave_gauss_newton", "smg_wave_born_host", "smg_debug_wave_born")
STEPS, DT, K = 8, 0.05, 3
LINEARITY, ROUTE = 2.0e-13, 9.6e-14   # 100 times the largest measured value (header), both inside 1e-10


# ---- the ABI and its refusals --------------------------------------------------------------------------------------------------------------------
def test_abi_present(smg_mod):
    L = smg_mod._lib.load()
    for name in SYMBOLS:
        assert hasattr(L, name)
    assert L.smg_version() >= 552
    assert hasattr(smg_mod.WaveEquation, "gauss_newton") and hasattr(smg_mod, "WaveGaussNewton")


def null_object_cases(smg):
    L = smg._lib.load()
    X = np.ones(8)
    dp = X.ctypes.data_as(C.POINTER(C.c_double))
    return [("null object: gauss_newton", lambda: (L.smg_wave_gauss_newton(None, dp, 8, 1, None, dp, 8, None, None, None), L.smg_last_error().decode()), False)]


def host_twin_cases(smg, call=None, prefix="host twin"):
    """the operand checks smg_wave_born_host and smg_debug_wave_born share"""
    call = call or (lambda *a, **k: G.host(smg, *a, **k)[0])
    L = smg._lib.load()
    V, F = N.shape("icosphere1")
    n = V.shape[0]
    u, v, w = N.test_state(V, F, 3)
    Fo = np.array(F)
    Fo[1, 2] = n
    ok = dict(k=3, d_cols=1, b=u, e=v, fd=w[:, :1])
    thunks = {
        "out missing": lambda: call(V, F, over=dict(out=None), **ok),
        "F missing": lambda: call(V, F, over=dict(F=None), **ok),
        "no vertex": lambda: call(V, F, over=dict(nV=0), **ok),
        "no face": lambda: call(V, F, over=dict(nF=0), **ok),
        "b missing": lambda: call(V, F, **dict(ok, b=None)),
        "e missing": lambda: call(V, F, **dict(ok, e=None)),
        "fd missing": lambda: call(V, F, **dict(ok, fd=None)),
        "k zero": lambda: call(V, F, **dict(ok, k=0)),
        "k negative": lambda: call(V, F, **dict(ok, k=-3)),
        "d_cols zero": lambda: call(V, F, **dict(ok, d_cols=0)),
        "d_cols two of three": lambda: call(V, F, **dict(ok, d_cols=2, fd=w[:, :2])),
        "clamped two": lambda: call(V, F, clamped=2, **ok),
        "face index": lambda: call(V, Fo, **ok),
        "order: operands before k": lambda: call(V, F, **dict(ok, e=None, k=0)),
        "order: k before d_cols": lambda: call(V, F, **dict(ok, k=0, d_cols=2)),
        "order: d_cols before clamped": lambda: call(V, F, clamped=2, **dict(ok, d_cols=0)),
        "order: clamped before faces": lambda: call(V, Fo, clamped=2, **ok),
    }
    return [("%s: %s" % (prefix, k), (lambda f=f: (f(), L.smg_last_error().decode())), False) for k, f in thunks.items()]


def test_refusals_keep_code_and_message(smg_mod):
    """every refusal of the call on a missing object and of the host twin's operand checks, with the code and the smg_last_error() text recorded in
    tests/golden/wave_gn_refusals.json.  The refusals that need a live object (group "live") are checked by tests/test_gpu_wave_gn.py; here their
    record is held to the order and the wording the contract sets.  Every message carries its entry point's name."""
    golden = json.load(open(GOLDEN))
    assert check_cases(smg_mod, null_object_cases(smg_mod), golden["null"]) == set(golden["null"])
    assert check_cases(smg_mod, host_twin_cases(smg_mod), golden["host"]) == set(golden["host"])
    h = golden["host"]
    assert h["host twin: order: operands before k"] == h["host twin: e missing"]
    assert h["host twin: order: k before d_cols"] == h["host twin: k zero"]
    assert h["host twin: order: d_cols before clamped"] == h["host twin: d_cols zero"]
    assert h["host twin: order: clamped before faces"] == h["host twin: clamped two"]
    assert all(v[1].startswith("smg_wave_born_host: ") for v in h.values())
    assert golden["null"]["null object: gauss_newton"] == [INVALID, "smg_wave_gauss_newton: null object"]
    live = golden["live"]
    for name, (code, msg) in live.items():
        assert code == INVALID and msg.startswith("smg_wave_gauss_newton: "), name
    assert "smg_wave_gradient" in live["before any gradient call"][1]
    assert "vertex 5, column 1" in live["non-finite d"][1]
    assert live["order: the point before d"] == live["before any gradient call"]
    assert live["order: d before d_cols"] == live["d missing"]
    assert live["order: d_cols before ldd"] == live["d_cols two of three"]
    assert live["order: ldd before a non-finite d"] == live["ldd below nV"]
    assert live["order: a non-finite d before the outputs"] == live["non-finite d"]
    assert live["order: the outputs before ld"] == live["every output missing"]


def test_hook_refuses_what_the_host_twin_refuses(smg_mod):
    golden = json.load(open(GOLDEN))["host"]
    hook = lambda *a, **k: G.hook(smg_mod, *a, **k)[0]   # noqa: E731
    for name, thunk, _ in host_twin_cases(smg_mod, hook, "hook"):
        rc, msg = thunk()
        want = golden[name.replace("hook: ", "host twin: ")]
        assert [rc, msg] == [want[0], want[1].replace("smg_wave_born_host", "smg_debug_wave_born")], name
    if smg_mod._lib.load().smg_device_count() == 0:
        V, F = N.shape("icosphere1")
        u, v, w = N.test_state(V, F, 1)
        assert G.hook(smg_mod, V, F, k=1, d_cols=1, b=u, e=v, fd=w)[0] == NO_DEVICE


# ---- the host twin against the restatement -------------------------------------------------------------------------------------------------------
def host_run(smg):
    def run(V, F, **kw):
        rc, out = G.host(smg, V, F, **kw)
        assert rc == 0
        return out
    return run


@pytest.mark.parametrize("k", [1, 3, 8])
@pytest.mark.parametrize("name", N.LAUNCHER_MESHES + N.PYRAMIDS)
def test_host_twin_against_restatement(smg_mod, name, k):
    """d_cols = 1 and k, free and clamped, fd of both signs and a zero column of d, bit for bit"""
    for clamped in sorted({cl for cl, _ in launcher_cases(name)}):
        for d_cols in sorted({1, k}):
            G.check_launcher(host_run(smg_mod), name, k, d_cols, clamped)


# ---- the restatement's J d and H d ---------------------------------------------------------------------------------------------------------------
CASES = ["sphere", "square"]


def run_case(smg, key, corners=False):
    """(the restatement, its gradient -- the linearisation point --, u0, v0, the signal, observed); corners: the receiver list of
    wave_adjoint_np.receiver_list, which holds vertex 0 and vertex nV - 1"""
    clamped = key == "square"
    V, F = sinkhorn_np.regular_square(8) if clamped else N.shape("icosphere2")
    speed, sigma = N.nonuniform(V)
    ref = N.WaveNp(V, F, speed=speed, sigma=sigma, dt=DT, clamped=int(clamped))
    u0, v0, _ = N.test_state(V, F, K, clamped)
    src = N.test_lists(V, F, 3, clamped)
    ref.src, ref.rec = src, A.receiver_list(V, F, clamped) if corners else np.concatenate([src[::-1], src[:1]]).astype(np.int32)
    sig = ricker_signal(smg, STEPS, DT, 3, K)
    obs = 0.05 * np.random.default_rng(7).standard_normal((STEPS, ref.rec.size, K))
    ref.set_state(u0, v0)
    return ref, A.gradient(ref, STEPS, sig, obs), u0, v0, sig, obs


def dots(x, y):
    """per column"""
    k = x.shape[-1]
    return np.sum((x * y).reshape(-1, k), axis=0)


@pytest.mark.parametrize("key", CASES)
def test_born_traces_against_complex_step(smg_mod, key):
    """DERIVATIVE of the header: one direction for every shot (d_cols = 1) and one per shot (d_cols = k), two random directions each"""
    ref, r, u0, v0, sig, _ = run_case(smg_mod, key)
    n, h = u0.shape[0], 1e-30
    rng = np.random.default_rng(11)
    worst = 0.0
    for cols in (1, K, 1, K):
        d = rng.standard_normal((n, cols))
        Jd = G.born_traces(ref, r.e, d)
        cs = np.zeros(Jd.shape)
        for c in range(cols):
            t = G.traces_complex(ref, u0, v0, STEPS, sig, speed=ref.speed + 1j * h * d[:, c]).imag / h
            if cols == 1:
                cs = t
            else:
                cs[:, :, c] = t[:, :, c]
        worst = max(worst, float(np.max(np.abs(Jd - cs)) / np.max(np.abs(cs))))
        assert np.max(np.abs(Jd - cs)) <= 1e-12 * np.max(np.abs(cs)), (key, cols)
    print("%s: largest |J d - complex step| over the largest entry %.2e (asserted: 1e-12)" % (key, worst))


@pytest.mark.parametrize("key", CASES)
def test_curvature_and_symmetry_identities(smg_mod, key):
    """IDENTITIES of the header, d_cols = 1 and k"""
    ref, r, u0, *_ = run_case(smg_mod, key)
    n = u0.shape[0]
    rng = np.random.default_rng(13)
    worst = [0.0, 0.0]
    for cols in (1, K):
        d, w = rng.standard_normal((n, cols)), rng.standard_normal((n, cols))
        gd, gw = G.gauss_newton(ref, r, d), G.gauss_newton(ref, r, w, product=False)
        quad, sq = dots(np.broadcast_to(d, (n, K)) if cols == 1 else d, gd.product), dots(gd.born_traces, gd.born_traces)
        cross, want = dots(np.broadcast_to(w, (n, K)) if cols == 1 else w, gd.product), dots(gw.born_traces, gd.born_traces)
        worst = [max(worst[0], float(np.max(np.abs(quad - sq) / sq))), max(worst[1], float(np.max(np.abs(cross - want) / np.abs(want))))]
        assert np.all(np.abs(quad - sq) <= 1e-12 * sq) and np.all(sq > 0.0), (key, cols)
        assert np.all(np.abs(quad - gd.curvature) <= 1e-12 * gd.curvature), (key, cols)
        assert np.all(np.abs(cross - want) <= 1e-12 * np.abs(want)), (key, cols)
    print("%s: <d, H d> against sum (J d)^2 relative %.2e, <w, H d> against <J w, J d> relative %.2e (asserted: 1e-12)" % (key, worst[0], worst[1]))


@pytest.mark.parametrize("key", CASES)
def test_product_is_linear(smg_mod, key):
    """LINEARITY of the header"""
    ref, r, u0, *_ = run_case(smg_mod, key)
    n = u0.shape[0]
    rng = np.random.default_rng(17)
    d1, d2 = rng.standard_normal((n, K)), rng.standard_normal((n, K))
    left = G.gauss_newton(ref, r, 2.0 * d1 - 3.0 * d2).product
    right = 2.0 * G.gauss_newton(ref, r, d1).product - 3.0 * G.gauss_newton(ref, r, d2).product
    rel = np.linalg.norm(left - right, axis=0) / np.linalg.norm(left, axis=0)
    print("%s: |H (2 d1 - 3 d2) - (2 H d1 - 3 H d2)| / |H (2 d1 - 3 d2)| per column %s (asserted: %.1e)" % (key, rel, LINEARITY))
    assert np.all(rel <= LINEARITY)


@pytest.mark.parametrize("key", CASES)
def test_product_against_the_gradient_route(smg_mod, key):
    """ROUTE of the header"""
    ref, r, u0, v0, sig, _ = run_case(smg_mod, key)
    n = u0.shape[0]
    d = np.random.default_rng(19).standard_normal((n, 1))
    d = d * (5e-2 * np.max(np.abs(r.traces)) / np.max(np.abs(G.born_traces(ref, r.e, d))))
    gn = G.gauss_newton(ref, r, d)
    assert np.max(np.abs(gn.born_traces)) >= 1e-2 * np.max(np.abs(r.traces))
    ref.set_state(u0, v0)
    other = A.gradient(ref, STEPS, sig, r.traces - gn.born_traces).grad_speed
    rel = np.linalg.norm(gn.product - other, axis=0) / np.linalg.norm(gn.product, axis=0)
    print("%s: |H d - grad_speed(observed = traces - J d)| / |H d| per column %s (asserted: %.1e)" % (key, rel, ROUTE))
    assert np.all(rel <= ROUTE)


@pytest.mark.parametrize("key", CASES)
def test_taylor_remainder_of_the_traces_falls_by_four(smg_mod, key):
    """TAYLOR of the header: h = 1e-3 and 5e-4"""
    ref, r, u0, v0, sig, _ = run_case(smg_mod, key)
    d = (1.0 + 0.5 * np.cos(3.0 * ref.V[:, 0] + ref.V[:, 1])) / 1.5
    Jd = G.born_traces(ref, r.e, d)

    def traces(h):
        other = N.WaveNp(ref.V, ref.F, speed=ref.speed + h * d, sigma=ref.sigma, dt=DT, clamped=ref.p["clamped"])
        other.src, other.rec = ref.src, ref.rec
        other.set_state(u0, v0)
        return other.step(STEPS, sig)[1]
    rem = [np.linalg.norm((traces(h) - r.traces - h * Jd).reshape(-1, K), axis=0) for h in (1e-3, 5e-4)]
    print("%s: remainders %s and %s, ratio %s" % (key, rem[0], rem[1], rem[0] / rem[1]))
    assert np.all(np.abs(rem[0] / rem[1] - 4.0) <= 0.1)


def test_clamped_rows_and_a_zero_direction_give_exact_zeros(smg_mod):
    """ZERO of the header"""
    ref, r, u0, *_ = run_case(smg_mod, "square", corners=True)
    kn, n = ref.known, u0.shape[0]
    assert kn[0] and kn[-1] and 0 in ref.rec and n - 1 in ref.rec
    gn = G.gauss_newton(ref, r, np.random.default_rng(23).standard_normal((n, K)))
    assert np.all(gn.product[kn] == 0.0) and np.any(gn.product[~kn] != 0.0) and np.all(gn.curvature > 0.0)
    assert all(ss > 0.0 for ss, _ in gn.tangent + gn.adjoint)
    zero = G.gauss_newton(ref, r, np.zeros((n, 1)))
    assert np.all(zero.product == 0.0) and np.all(zero.born_traces == 0.0) and np.all(zero.curvature == 0.0)
    assert all(ss == 0.0 and np.all(res == 0.0) for ss, res in zero.tangent + zero.adjoint) and len(zero.tangent) == len(zero.adjoint) == STEPS


def test_one_truncated_newton_step_on_the_restatement(smg_mod):
    """NEWTON: what tests/test_gpu_wave_gn.py asserts on the device is what the restatement shows here, on the same start (icosphere3, k = 2, the
    library's own L, the non-uniform speed, no damping, the data from a 20 percent speed bump, five conjugate-gradient iterations, damping 1e-3):
    the full step is accepted, the misfit falls from 6.952e-2 to 1.492e-3, and one steepest-descent step from the same start reaches 5.312e-2,
    35.6 times higher -- more than the factor 1.2 to spare that lets the device test assert the comparison too"""
    V, F = N.shape("icosphere3")
    speed = N.nonuniform(V)[0]
    L = smg_mod.mesh.cotmatrix(V, F)
    u0, v0, _ = N.test_state(V, F, 2, False)
    src = N.test_lists(V, F, 3, False)
    rec = np.concatenate([src[::-1], src[:1]]).astype(np.int32)
    sig = ricker_signal(smg_mod, STEPS, DT, 3, 2)
    true = speed * (1.0 + 0.2 * np.exp(-4.0 * np.sum((V - V[rec[0]]) ** 2, axis=1)))

    def make(spd):
        ref = N.WaveNp(V, F, L=L, speed=spd, dt=DT, clamped=0)
        ref.src, ref.rec = src, rec
        return ref
    made = make(true)
    made.set_state(u0, v0)
    engine = G.NpEngine(make, u0, v0, STEPS, sig, made.step(STEPS, sig)[1])
    step, sd = G.newton_step(engine, speed.copy()), G.descent_step(engine, speed.copy())
    print("one truncated-Newton step: misfit %.6e -> %.6e, alpha %g after %s halvings, lambda %.3e, <d, H d> per iteration %s; one steepest-descent step: %.6e"
          % (step["J"], step["Jt"], step["alpha"], step["found"], step["lam"], step["curvatures"], sd["Jt"]))
    assert step["found"] == 0 and sd["found"] is not None and all(c > 0.0 for c in step["curvatures"]) and step["slope"] < 0.0
    assert abs(step["J"] - 6.952e-2) <= 1e-5 and abs(step["Jt"] - 1.492e-3) <= 1e-6 and abs(sd["Jt"] - 5.312e-2) <= 1e-5
    assert 1.2 * step["Jt"] < sd["Jt"] < sd["J"]


# ---- the kernel's registers, the host maths under sanitizers -------------------------------------------------------------------------------------
def test_kernel_keeps_everything_in_registers():
    """the ISA notes of k_wave_born (the build's flags, device side only): no scratch, no spills, no contraction"""
    from surface_multigrid_code_amd import build as B
    src = os.path.join(B.CSRC, "smg_wave_born_device.hip")
    asm = subprocess.check_output([B._hipcc()] + B.FLAGS + ["--cuda-device-only", "-S", src, "-o", "-"], text=True, stderr=subprocess.DEVNULL)
    notes = dict(re.findall(r"\.name:\s+(\S*k_wave_born\S*)(.*?)\.wavefront_size", asm, flags=re.S))
    assert len(notes) == 1
    for kernel, body in notes.items():
        field = lambda k: int(re.search(r"\.%s:\s+(\d+)" % k, body).group(1))   # noqa: E731
        print("%s: vgpr_count %d, sgpr_count %d, private_segment_fixed_size %d" % (kernel, field("vgpr_count"), field("sgpr_count"), field("private_segment_fixed_size")))
        assert field("private_segment_fixed_size") == 0 and field("vgpr_spill_count") == 0 and field("sgpr_spill_count") == 0 and field("vgpr_count") <= 32
    for word in ("v_fma_f64", "v_fmac_f64"):
        assert word not in asm, "no contraction"


def test_host_maths_under_sanitizers(tmp_path):
    """tests/wave_gn_asan_driver.cpp, a stand-alone program: the host twin's loops (smg::wave_born_host_plane and wave_born_host of
    csrc/smg_wave_born_inl.hpp, what smg_wave_born_host runs after its checks) on exactly-sized heap arrays, under AddressSanitizer and
    UndefinedBehaviorSanitizer (static runtimes: run directly, nothing preloaded, nothing loaded into python)"""
    exe = str(tmp_path / "wave_gn_asan_driver")
    csrc = os.path.join(ROOT, "surface_multigrid_code_amd", "csrc")
    srcs = [os.path.join(ROOT, "tests", "wave_gn_asan_driver.cpp"), os.path.join(csrc, "smg_mesh.cpp"), os.path.join(csrc, "smg_sparse.cpp")]
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-ffp-contract=off", "-pthread", "-I" + csrc] + srcs + ["-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    run = subprocess.run([exe], env=env, capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0 and run.stdout.count("ok 1") == 24 and "ERROR" not in run.stderr
