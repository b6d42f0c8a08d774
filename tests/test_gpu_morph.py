"""GPU (-m gpu): gradient-domain morphing (include/smg.h: smg_morph_*).

The host references are tests/morph_np.py -- the method with LAPACK SVDs and direct solves, in the kernels' operation order -- and the library's
own host twin (smg_morph_faces_host), which compiles the text the kernels compile.  The kernels are held launcher by launcher (smg_debug_morph,
guarded buffers, every output pre-filled with sentinels): face gradients, right-hand sides from given gradients, pins and starts bit for bit
against the restatement; polar factors, rotation vectors and the interpolated right-hand side to the bounds of tests/test_morph_host.py
(ROT_BOUND, OMEGA_BOUND = 16 x 6.66e-16 measured on the CPU, INTERP_C = 8 x 0.822 measured on the CPU: see that file's header).

Exact answers (reconstruct returns the pose, interpolate ends at the rest pose and the pose, rigid and uniformly scaled poses, transfer from the
target itself and from a scaled source) are held to PROP_BOUND diagonals at tol = 1e-12 |b|_F: the residual bound times a condition number of
(-L)_uu of at most 1e4 on these meshes (pins at vertex 0; the restatement's direct solves are within 3e-13).

End to end against the restatement's direct solves, max |U - U_np| / bounding-box diagonal, measured on an MI355X (DESIGN.md section 26,
profiles/morph_gpu_tests.log): 1.59e-10 on the flat square (169 vertices, two loop entries: its coarsest level is the mesh itself, and the same
figure separates the device from the exact answers there), 9.76e-12 on icosphere(1), 1.26e-14 on icosphere(3), 8.32e-14 on the torus, 1.35e-13
on bunny.smgm; reconstruct and transfer at most 1.64e-11 beside the square's 1.59e-10.  By the project's rule the bound is 100 x the measured
maximum rounded up to a power of ten, 1e-7, and in no case above 1e-8: E2E_BOUND = 1e-8.  With the default options (1e-10 |b|_F) the device is
within 1.56e-12 of the restatement on the larger meshes.  Launchers on the MI355X: rotations and stretches equal the host twin's bit for bit,
omega is within 6.66e-16 of the twin's and 5.77e-15 of scipy's (bound 1.066e-14), the interpolated right-hand side within 0.845 of the scale
(bound 6.58)."""
import ctypes as C
import gc
import json

import numpy as np
import pytest

import morph_np as N
from test_arap_host import bbox_diag, twist
from test_gpu_parity import smg  # noqa: F401  (fixture)
from test_morph_host import GOLDEN, INVALID, affine_source, check_launchers, rigid_pose

pytestmark = pytest.mark.gpu

NONFINITE = -4
PROP_BOUND = 1e-8
E2E_BOUND = 1e-8                    # measured maximum 1.59e-10: see the header
SETS_BOUND = 1e-8                   # a k = 5 call against the five k = 1 calls: the loop stops on the norm over all columns, so bits may differ


def hook_run(smg):
    def run(op, V0, F, **kw):
        rc, bad, out = N.hook(smg, op, V0, F, **kw)
        assert rc == 0 and bad == 0, (rc, bad)
        return out
    return run


# ---- kernels, launcher by launcher -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,k", list(zip(N.CASES, (1, 2, 5, 1, 2))) + [(N.CASES[1], 5), (N.CASES[0], 2)])
def test_hook_against_restatement(smg, case, k):
    check_launchers(hook_run(smg), case[0], case[1], k, device=True)


@pytest.mark.parametrize("case", N.CASES)
def test_hook_against_host_twin(smg, case):
    """the same text on both sides: everything that calls no sin, cos or atan2 bit for bit"""
    V, F = N.shape(case[0])
    X = N.pose(*case)
    n, nF, k = V.shape[0], F.shape[0], 2
    Xs = np.stack([X, N.blend(V, X, 0.5)])
    dev = hook_run(smg)
    host = lambda op, **kw: N.faces_host(smg, op, V, F, **kw)[1]   # noqa: E731
    Jd = dev(N.MORPH_FACE_GRADIENT, V, F, k=k, X=Xs)
    assert np.array_equal(Jd, host(N.MORPH_FACE_GRADIENT, k=k, X=Xs))
    assert np.array_equal(dev(N.MORPH_RHS_GRADIENT, V, F, k=k, inp=Jd), host(N.MORPH_RHS_GRADIENT, k=k, inp=Jd))
    pd, ph = dev(N.MORPH_FACE_POLAR, V, F, X=X), host(N.MORPH_FACE_POLAR, X=X)
    Rd, omd, Sd = N.unpack(N.MORPH_FACE_POLAR, pd, n, nF, 1)
    Rh, omh, Sh = N.unpack(N.MORPH_FACE_POLAR, ph, n, nF, 1)
    print("%s: rotations bit for bit %s, stretches %s; max |omega - omega_host| = %.2e" %
          (case[0], np.array_equal(Rd, Rh), np.array_equal(Sd, Sh), np.abs(omd - omh).max()))
    assert np.array_equal(Rd, Rh) and np.array_equal(Sd, Sh)
    assert np.abs(omd - omh).max() <= 16 * N.EPS * np.pi              # atan2 alone differs: a few ulps of an angle below pi


# ---- the objects ----------------------------------------------------------------------------------------------------------------------------------
def build(smg, name, pins=(0,)):
    V, F = N.shape(name)
    mg = smg.mg_precompute(V, F, 0.25, 50, 1)
    ref = N.MorphNp(V, F, pins=pins, L=smg.mesh.cotmatrix(V, F))                   # the library's own L: the system's bits
    return V, F, mg, smg.Morpher(mg, V, F, pins), ref


@pytest.fixture(scope="module")
def objects(smg):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = build(smg, name)
        return cache[name]
    yield get
    cache.clear()
    gc.collect()


def tight(smg, B):
    return smg.SolveOpts(tol=1e-12 * float(np.linalg.norm(B)), max_iter=100)


def err(U, want, V):
    return np.abs(U - want).max() / bbox_diag(V)


# ---- exact answers ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", N.CASES)
def test_reconstruct_returns_the_pose(smg, objects, case):
    V, F, mg, mo, ref = objects(case[0])
    X = N.pose(*case)
    J = N.gradient(V, F, X)
    B, _ = N.rhs(V, F, J[None])
    U, cyc = mo.reconstruct(J, pin_pos=X[[0]][None], opts=tight(smg, B))
    print("%s: reconstruct %.2e diagonals from the pose, %d cycles" % (case[0], err(U[0], X, V), cyc))
    assert cyc < 100 and err(U[0], X, V) <= PROP_BOUND


@pytest.mark.parametrize("case", N.CASES)
def test_interpolate_ends(smg, objects, case):
    V, F, mg, mo, ref = objects(case[0])
    X = N.pose(*case)
    _, B = ref.interpolate(X, [0.0, 1.0])
    U, cyc = mo.interpolate(X, [0.0, 1.0], opts=tight(smg, B))
    print("%s: interpolate t = 0 %.2e, t = 1 %.2e diagonals, %d cycles" % (case[0], err(U[0], V, V), err(U[1], X, V), cyc))
    assert cyc < 100 and err(U[0], V, V) <= PROP_BOUND and err(U[1], X, V) <= PROP_BOUND


@pytest.mark.parametrize("name", ["icosphere3", "torus"])
def test_interpolate_rigid_and_scale(smg, objects, name):
    V, F, mg, mo, ref = objects(name)
    ts = [0.25, 0.5, 1.5]
    X = rigid_pose(V, 2.4)
    U, cyc = mo.interpolate(X, ts, opts=tight(smg, ref.interpolate(X, ts)[1]))
    worst = max(err(U[c], rigid_pose(V, 2.4 * t), V) for c, t in enumerate(ts))
    s = 1.7
    X = V[0] + s * (V - V[0])
    U, cyc2 = mo.interpolate(X, ts, opts=tight(smg, ref.interpolate(X, ts)[1]))
    worst_s = max(err(U[c], V[0] + (1.0 + t * (s - 1.0)) * (V - V[0]), V) for c, t in enumerate(ts))
    print("%s: rigid pose %.2e, uniform scale %.2e diagonals; cycles %d, %d" % (name, worst, worst_s, cyc, cyc2))
    assert max(cyc, cyc2) < 100 and worst <= PROP_BOUND and worst_s <= PROP_BOUND


def test_transfer(smg, objects):
    V, F, mg, mo, ref = objects("icosphere3")
    X = N.pose("icosphere3", "twist")
    Un, B = ref.transfer(V, X[None])
    o = tight(smg, B)
    same, _ = mo.transfer(V, X)
    same_t, _ = mo.transfer(V, X, opts=o)
    one, _ = mo.interpolate(X, [1.0], pin_pos=V[[0]][None], opts=o)
    print("transfer of the target itself against interpolate at t = 1: %.2e diagonals" % err(same_t[0], one[0], V))
    assert err(same_t[0], one[0], V) <= PROP_BOUND and err(same[0], one[0], V) <= 1e-6
    # an affine pose of a uniformly scaled copy of the target: V B^T, the restatement's closed form
    S0, S1, Bm = affine_source(V, general=False)
    U, _ = mo.transfer(S0, S1, opts=tight(smg, ref.transfer(S0, S1[None])[1]))
    print("transfer from a scaled source: %.2e diagonals from V B^T" % err(U[0], N.exact_transfer(V, ref.pins, Bm), V))
    assert err(U[0], N.exact_transfer(V, ref.pins, Bm), V) <= PROP_BOUND
    # a sheared copy with its own face list (a relabelling of the vertices): the restatement's value, which is no affine map
    S0, S1, Bm = affine_source(V, general=True)
    perm = np.random.default_rng(3).permutation(V.shape[0])
    inv = np.argsort(perm)
    S0p, S1p, Fs = S0[perm], S1[perm], inv[F].astype(np.int32)                        # vertex i of the target is vertex inv[i] of the source
    Un, B = ref.transfer(S0p, S1p[None], Fs)
    U, _ = mo.transfer(S0p, S1p, Fs, opts=tight(smg, B))
    print("transfer from a sheared, relabelled source: %.2e diagonals from the restatement, %.2e from V B^T" %
          (err(U[0], Un[0], V), err(U[0], N.exact_transfer(V, ref.pins, Bm), V)))
    assert err(U[0], Un[0], V) <= PROP_BOUND
    assert np.array_equal(Un, ref.transfer(S0, S1[None])[0])                           # the relabelling changes nothing: the same faces, the same bits


# ---- end to end ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,k", list(zip(N.CASES, (5, 2, 1, 5, 2))))
def test_against_restatement(smg, objects, case, k):
    V, F, mg, mo, ref = objects(case[0])
    X = N.pose(*case)
    ts = list(N.TIMES[:k])
    Un, B = ref.interpolate(X, ts)
    U, cyc = mo.interpolate(X, ts, opts=tight(smg, B))
    Ud, cycd = mo.interpolate(X, ts)
    worst = err(U, Un, V)
    print("%s, %s, k = %d: interpolate max |U - U_np| = %.2e diagonals (%d cycles); default opts %.2e (%d cycles)" %
          (case[0], case[1], k, worst, cyc, err(Ud, Un, V), cycd))
    Js = np.stack([N.gradient(V, F, N.blend(V, X, t)) for t in ts])
    Rn, Bn = ref.reconstruct(Js)
    R, cycr = mo.reconstruct(Js, opts=tight(smg, Bn))
    Tn, Bt = ref.transfer(V, np.stack([N.blend(V, X, t) for t in ts]))
    T, cyct = mo.transfer(V, np.stack([N.blend(V, X, t) for t in ts]), opts=tight(smg, Bt))
    print("  reconstruct %.2e (%d cycles), transfer %.2e (%d cycles)" % (err(R, Rn, V), cycr, err(T, Tn, V), cyct))
    assert max(cyc, cycd, cycr, cyct) < 100                                            # every solve converged
    assert worst <= E2E_BOUND and err(R, Rn, V) <= E2E_BOUND and err(T, Tn, V) <= E2E_BOUND
    assert err(Ud, Un, V) <= 1e-6                                                      # tol = 1e-10 |b|_F


def test_five_sets_against_five_calls(smg, objects):
    V, F, mg, mo, ref = objects("icosphere3")
    X = N.pose("icosphere3", "twist")
    n, nF = V.shape[0], F.shape[0]
    ts = np.array(N.TIMES)
    dev = hook_run(smg)
    R, om, S6 = N.unpack(N.MORPH_FACE_POLAR, dev(N.MORPH_FACE_POLAR, V, F, X=X), n, nF, 1)
    fac = np.concatenate([om.ravel(), S6.ravel()])
    B5, q5 = N.unpack(N.MORPH_RHS_INTERP, dev(N.MORPH_RHS_INTERP, V, F, k=5, t=ts, inp=fac), n, nF, 5)
    U5, _ = mo.interpolate(X, ts)
    for c, t in enumerate(ts):
        B1, q1 = N.unpack(N.MORPH_RHS_INTERP, dev(N.MORPH_RHS_INTERP, V, F, k=1, t=[t], inp=fac), n, nF, 1)
        assert np.array_equal(B1, B5[:, 3 * c:3 * c + 3]) and np.array_equal(q1[0], q5[c])
        U1, _ = mo.interpolate(X, [t])
        assert err(U1[0], U5[c], V) <= SETS_BOUND
    assert np.array_equal(mo.interpolate(X, ts[:1])[0][0], mo.interpolate(X, [ts[0]])[0][0])


# ---- determinism, memory, refusals --------------------------------------------------------------------------------------------------------------
def test_same_bits_and_memory(smg, objects):
    import torch
    V, F, mg, _, ref = objects("icosphere3")
    X = N.pose("icosphere3", "twist")
    n, nF = V.shape[0], F.shape[0]
    live = smg._lib.load().smg_device_bytes_live
    handles, hp = twist(V)
    nh = handles.size
    ts = np.array([0.25, 0.5])
    k = ts.size
    gc.collect()
    before_live = live()
    mo = smg.Morpher(mg, V, F, handles)
    a = mo.interpolate(X, ts)
    b = mo.interpolate(X, ts)
    assert np.array_equal(a[0], b[0]) and a[1] == b[1]
    J = np.stack([N.gradient(V, F, N.blend(V, X, t)) for t in ts])
    r1, r2 = mo.reconstruct(J), mo.reconstruct(J)
    t1, t2 = mo.transfer(V, X), mo.transfer(V, X)
    assert np.array_equal(r1[0], r2[0]) and np.array_equal(t1[0], t2[0])
    counted = mo.device_bytes()
    assert 0 < counted == live() - before_live                               # what it counts is what the library holds for it
    tol = 1e-10 * float(np.linalg.norm(N.MorphNp(V, F, pins=handles).interpolate(X, ts)[1]))
    eager = mo.interpolate(X, ts, opts=smg.SolveOpts(tol=tol, max_iter=100, use_graph=0))
    graph = mo.interpolate(X, ts, opts=smg.SolveOpts(tol=tol, max_iter=100, use_graph=1))
    assert np.array_equal(eager[0], graph[0]) and eager[1] == graph[1]
    assert mo.device_bytes() == counted                                      # nothing grows between the second and later calls
    # SMG_DEVICE, padded leading dimensions, caller-given pins and start: the same bits, rows past n untouched
    ld_u, ld_pp, ld_u0 = n + 5, nh + 3, n + 2
    pp = np.stack([hp, hp + 0.01])
    U0 = np.stack([V, X])
    want = mo.interpolate(X, ts, pin_pos=pp, U0=U0)
    cols = lambda A: np.ascontiguousarray(A.transpose(0, 2, 1).reshape(3 * A.shape[0], -1))   # noqa: E731  (sets x rows x 3 -> 3 sets x rows: column-major)
    Ud = torch.full((3 * k, ld_u), -1.0, dtype=torch.float64, device="cuda")
    ppd = torch.zeros((3 * k, ld_pp), dtype=torch.float64, device="cuda")
    ppd[:, :nh] = torch.from_numpy(cols(pp))
    U0d = torch.zeros((3 * k, ld_u0), dtype=torch.float64, device="cuda")
    U0d[:, :n] = torch.from_numpy(cols(U0))
    Xd = torch.from_numpy(np.array(X)).cuda()
    torch.cuda.synchronize()
    cyc = mo.interpolate_device(Xd.data_ptr(), ts, Ud.data_ptr(), ld_u=ld_u, pp_ptr=ppd.data_ptr(), ld_pp=ld_pp, U0_ptr=U0d.data_ptr(), ld_u0=ld_u0)
    got = Ud.cpu().numpy()
    assert np.array_equal(got[:, :n], cols(want[0])) and np.all(got[:, n:] == -1.0) and cyc == want[1]
    # the defaults on the device, and the other two queries there
    Ud.fill_(-1.0)
    mo.interpolate_device(Xd.data_ptr(), ts, Ud.data_ptr(), ld_u=ld_u)
    assert np.array_equal(Ud.cpu().numpy()[:, :n], cols(a[0]))
    Jd = torch.from_numpy(np.ascontiguousarray(J)).cuda()
    mo.reconstruct_device(Jd.data_ptr(), k, Ud.data_ptr(), ld_u=ld_u)
    assert np.array_equal(Ud.cpu().numpy()[:, :n], cols(r1[0]))
    Vd = torch.from_numpy(np.array(V)).cuda()
    Ud.fill_(-1.0)
    mo.transfer_device(Vd.data_ptr(), n, Xd.data_ptr(), 1, Ud.data_ptr(), ld_u=ld_u)
    got = Ud.cpu().numpy()
    assert np.array_equal(got[:3, :n], cols(t1[0])) and np.all(got[3:] == -1.0)
    assert mo.device_bytes() == counted
    # padded host leading dimensions through the C ABI
    L = smg._lib.load()
    Up = np.full((n + 7, 3 * k), -2.0, order="F")
    assert L.smg_morph_interpolate(mo.m, np.ascontiguousarray(X).ctypes.data, ts.ctypes.data_as(C.POINTER(C.c_double)), k, None, 0, None, 0, 0, None,
                                   Up.ctypes.data, n + 7, None) == 0
    assert np.array_equal(Up[:n], cols(a[0]).T) and np.all(Up[n:] == -2.0)
    # a larger k grows the blocks once; the stationary loop is another solver with the same answer
    mo.interpolate(X, N.TIMES)
    grown = mo.device_bytes()
    assert grown > counted and grown == live() - before_live
    mo.interpolate(X, N.TIMES)
    assert mo.device_bytes() == grown and np.array_equal(mo.interpolate(X, ts)[0], a[0])
    mo.set_solver(0)
    assert err(mo.interpolate(X, ts)[0], a[0], V) <= 1e-6
    del mo
    gc.collect()
    assert live() == before_live


def test_callers_hierarchy_is_untouched(smg):
    from oracle import mesh_np as M
    V, F = N.shape("icosphere3")
    mg = smg.mg_precompute(V, F, 0.25, 50, 1)
    A = (M.massmatrix(V, F, "barycentric") - 0.01 * smg.mesh.cotmatrix(V, F)).tocsr()
    mg.precompute(A, None)
    rhs_ = np.asfortranarray(A @ V)
    o = smg.SolveOpts(tol=1e-10, max_iter=30)
    first = mg.solve(rhs_, np.zeros_like(rhs_, order="F"), None, o)
    smg.Morpher(mg, V, F).interpolate(N.pose("icosphere3", "twist"), [0.5])
    second = mg.solve(rhs_, np.zeros_like(rhs_, order="F"), None, o)
    assert first[0] and np.array_equal(first[1], second[1]) and np.array_equal(first[2], second[2])


def test_non_finite_input_is_refused_before_the_solve(smg, objects):
    """one NaN in X: SMG_ERR_NONFINITE, U untouched, and the object's next call equals a fresh object's to the bit"""
    V, F, mg, mo, ref = objects("icosphere3")
    X = N.pose("icosphere3", "twist")
    n, L = V.shape[0], smg._lib.load()
    ts = np.array([0.25, 0.5])
    bad = np.array(X)
    bad[n // 2, 1] = np.nan
    U = np.full((n, 6), -7.0, order="F")
    cyc = C.c_int(-7)
    rc = L.smg_morph_interpolate(mo.m, bad.ctypes.data, ts.ctypes.data_as(C.POINTER(C.c_double)), 2, None, 0, None, 0, 0, None, U.ctypes.data, n, C.byref(cyc))
    assert rc == NONFINITE and L.smg_last_error() == b"smg_morph_interpolate: the right-hand side is not finite"
    assert np.all(U == -7.0) and cyc.value == -7
    Jbad = N.gradient(V, F, X)
    Jbad[7, 1, 2] = np.inf
    assert L.smg_morph_reconstruct(mo.m, Jbad.ctypes.data, 1, None, 0, None, 0, 0, None, U.ctypes.data, n, None) == NONFINITE and np.all(U == -7.0)
    assert L.smg_morph_transfer(mo.m, np.ascontiguousarray(V).ctypes.data, n, None, bad.ctypes.data, 1, None, 0, None, 0, 0, None, U.ctypes.data, n,
                                None) == NONFINITE and np.all(U == -7.0)
    after = mo.interpolate(X, ts)
    fresh = smg.Morpher(mg, V, F).interpolate(X, ts)
    assert np.array_equal(after[0], fresh[0]) and after[1] == fresh[1]


def test_live_object_refusals(smg, objects):
    """the refusals that need an object, with the code and message recorded in tests/golden/morph_refusals.json (group "live"); the object is as
    usable afterwards as before"""
    V, F, mg, mo, ref = objects("icosphere3")
    X = np.ascontiguousarray(N.pose("icosphere3", "twist"))
    Vc = np.ascontiguousarray(V)
    n, nF, L = V.shape[0], F.shape[0], smg._lib.load()
    assert n == 642
    golden = json.load(open(GOLDEN))["live"]
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    ts = np.array([0.25, 0.5])
    before = mo.interpolate(X, ts)
    J = np.ascontiguousarray(np.stack([N.gradient(V, F, X)] * 2))
    U, blk, ppb = np.zeros((n, 6), order="F"), np.zeros((n, 6), order="F"), np.zeros((1, 6), order="F")
    Fo, Fn = np.array(F), np.array(F)
    Fo[1, 2], Fn[5, 0] = n, -1

    def tail(a):
        return (ppb.ctypes.data if "ld_pp" in a else None, a.get("ld_pp", 1), blk.ctypes.data if "ld_u0" in a else None, a.get("ld_u0", n),
                a.get("memspace", 0), None, a.get("U", U.ctypes.data), a.get("ld_u", n), None)

    def reconstruct(**a):
        return L.smg_morph_reconstruct(mo.m, a.get("inp", J.ctypes.data), a.get("k", 2), *tail(a))

    def interpolate(**a):
        t = a.get("t", ts)
        return L.smg_morph_interpolate(mo.m, a.get("inp", X.ctypes.data), None if t is None else np.asarray(t, dtype=np.float64).ctypes.data_as(dp),
                                       a.get("k", 2), *tail(a))

    def transfer(**a):
        Fs = a.get("Fs")
        return L.smg_morph_transfer(mo.m, a.get("inp", Vc.ctypes.data), a.get("nVs", n), None if Fs is None else Fs.ctypes.data_as(ip),
                                    None if a.get("S1", 1) is None else X.ctypes.data, a.get("k", 1), *tail(a))

    calls = {}
    for name, f in (("reconstruct", reconstruct), ("interpolate", interpolate), ("transfer", transfer)):
        calls.update({name + " null input": lambda f=f: f(inp=None), name + " null U": lambda f=f: f(U=None), name + " k zero": lambda f=f: f(k=0),
                      name + " k negative": lambda f=f: f(k=-2), name + " bad memspace": lambda f=f: f(memspace=7),
                      name + " ld_u too small": lambda f=f: f(ld_u=n - 1), name + " ld_pp too small": lambda f=f: f(ld_pp=0),
                      name + " ld_u0 too small": lambda f=f: f(ld_u0=n - 1)})
    calls.update({"interpolate null t": lambda: interpolate(t=None), "interpolate t nan": lambda: interpolate(t=[0.5, np.nan]),
                  "interpolate t inf": lambda: interpolate(t=[np.inf, 0.5]), "interpolate order: k before t": lambda: interpolate(k=0, t=[np.nan, 0.5]),
                  "transfer null S1": lambda: transfer(S1=None), "transfer nVs zero": lambda: transfer(nVs=0),
                  "transfer Fs null, nVs differs": lambda: transfer(nVs=n - 1), "transfer source face past the end": lambda: transfer(Fs=Fo),
                  "transfer source face negative": lambda: transfer(Fs=Fn), "transfer order: ld before faces": lambda: transfer(Fs=Fo, ld_u=n - 1)})
    assert set(calls) == set(golden)
    for name, f in calls.items():
        rc = f()
        assert [rc, L.smg_last_error().decode()] == golden[name] and rc == INVALID, name
    after = mo.interpolate(X, ts)
    assert np.array_equal(before[0], after[0]) and before[1] == after[1]
