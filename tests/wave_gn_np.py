"""The numpy / scipy restatement of the wave object's Born traces and Gauss-Newton products (include/smg.h: smg_wave_gauss_newton), in the kernels'
operation order, with direct solves on tests/wave_np.py's WaveNp and the adjoint pieces of tests/wave_adjoint_np.py; the ctypes wrappers of
smg_wave_born_host and smg_debug_wave_born.

    plane     fd = fac d,  fac = (-2.0 mt) / speed                 d: nV x d_cols, d_cols 1 or k; column c reads column c % d_cols
    born      x = b + fd e;  b = x;  rsq = x x                     off the known rows; a known row keeps its b and rsq
    tangent   from du = dv = 0, for n = 0 .. N - 1: b = rhs(du, dv), born with e_n, A w = b (|b|_F^2 == 0.0: w = 0), advance, record: J d
    product   the adjoint pass with rho = J d: H d = fac G

Only + and * occur in the kernel: the library's host twin and its kernel are held to this file bit for bit.  Vertex blocks are nV x k arrays here
(the library's are column-major); term planes are k x nV."""
import ctypes as C

import numpy as np

import wave_adjoint_np as A
import wave_np as N
from wave_np import SENTINEL, fixed_sum


# ---- the kernel's expression ---------------------------------------------------------------------------------------------------------------------
def plane(fac, d):
    """fd (nV x d_cols) = fac d, one multiply per entry"""
    return fac[:, None] * np.asarray(d, dtype=np.float64).reshape(fac.shape[0], -1)


def born(known, fd, e, b, rsq):
    """(b' nV x k, rsq' k x nV, the sum of rsq') of k_wave_born and its reduction; b, rsq: what k_wave_rhs or k_wave_advance left"""
    k = b.shape[1]
    cols = np.arange(k) % fd.shape[1]
    x = b + fd[:, cols] * e
    bn, rn = np.array(b), np.array(rsq)
    bn[~known] = x[~known]
    rn[:, ~known] = (x * x).T[:, ~known]
    return bn, rn, fixed_sum(rn.reshape(-1))


# ---- the method with direct solves ---------------------------------------------------------------------------------------------------------------
def born_traces(ref, e, d, records=None):
    """J d (N x n_rec x k) of the tangent run over the history e = [e_n] on `ref`'s direct solves; ref's own state is not touched.  records (a
    list): (|b|_F^2, the solve's residuals) per step are appended"""
    dt, q2 = ref.p["dt"], ref.q2
    n, k = e[0].shape
    fd = plane(A.factor(ref.mt, ref.speed), d)
    du, dv, T = np.zeros((n, k)), np.zeros((n, k)), []
    for t in range(len(e)):
        b, rsq, _, _ = N.rhs(ref.mt, ref.s2, ref.known, dt, du, dv)
        b, _, ss = born(ref.known, fd, e[t], b, rsq)
        w, res = (np.zeros((n, k)), np.zeros(k)) if ss == 0.0 else ref.solve(b)
        du, dv, _, _ = N.advance(ref.mt, q2, w, du, dv)
        T.append(du[ref.rec])
        if records is not None:
            records.append((ss, res))
    return np.stack(T)


def backward(ref, e, rho, records=None):
    """the unscaled sum_n y e_n of the adjoint pass over the history e with the residuals rho (N x n_rec x k): wave_adjoint_np.gradient's loop
    without the signal's gradient; records (a list): (|g|_F^2, the solve's residuals) per step in the order they ran"""
    n, k = e[0].shape
    steps = len(e)
    groups = A.group(ref.rec, ref.known)
    p, q, G = A.inject(np.zeros((n, k)), rho[steps - 1], groups), np.zeros((n, k)), np.zeros((n, k))
    for t in range(steps - 1, -1, -1):
        g, _, ss = A.rhs(ref.known, ref.q2, p, q)
        y, res = (np.zeros((n, k)), np.zeros(k)) if ss == 0.0 else ref.solve(g)
        if records is not None:
            records.append((ss, res))
        p, q, G = A.advance(ref.mt, ref.s2, ref.p["dt"], ref.q2, y, e[t], p, q, G)
        if t >= 1:
            p = A.inject(p, rho[t - 1], groups)
    return G


def gauss_newton(ref, r, d, product=True):
    """smg_wave_gauss_newton on the restatement: r = wave_adjoint_np.gradient(ref, ...) is the linearisation point (its history r.e), d: nV or
    nV x k.  -> Result with born_traces, curvature (k: the fixed-order sums of the Born traces' squares), product (nV x k or None), and
    tangent, adjoint: the per-step (|rhs|_F^2, residuals) records"""
    out = A.Result()
    out.tangent, out.adjoint = [], []
    out.born_traces = born_traces(ref, r.e, d, out.tangent)
    rho, _, out.curvature = A.residual(out.born_traces, None)
    out.product = A.scale(A.factor(ref.mt, ref.speed), backward(ref, r.e, rho, out.adjoint)) if product else None
    return out


def traces_complex(ref, u0, v0, n_steps, signal_=None, speed=None):
    """the traces (n_steps x n_rec x k, complex) of the scheme in complex arithmetic: Im traces(speed + i h d) / h is J d"""
    states = []
    A.misfit_complex(ref, u0, v0, n_steps, signal_, None, speed=speed, states=states)
    return np.stack([u[ref.rec] for u, _ in states[1:]])


# ---- the library's side, shared with tests/test_gpu_wave_gn.py -----------------------------------------------------------------------------------
def out_size(nV, k):
    return 2 * nV * k + 1


def unpack(out, nV, k):
    nk = nV * k
    return out[:nk].reshape(k, nV).T, out[nk:2 * nk].reshape(k, nV), out[2 * nk]


def _call(fn, with_guard, V, F, k=1, d_cols=1, clamped=0, b=None, e=None, fd=None, over=None, pad=64):
    """`pad` doubles of sentinel follow the extent in `out`: nothing past the extent may be written"""
    ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
    nV, nF = V.shape[0], F.shape[0]
    F = np.ascontiguousarray(F, dtype=np.int32)
    cols = lambda a: None if a is None else np.ascontiguousarray(np.asarray(a, dtype=np.float64).T).reshape(-1)   # noqa: E731  (column-major)
    keep_ = [cols(b), cols(e), cols(fd)]
    arr = lambda a, ty=dp: None if a is None else a.ctypes.data_as(ty)   # noqa: E731
    size = out_size(nV, max(k, 0))
    out = np.full(size + pad, SENTINEL)
    bad = C.c_int(-1)
    q = dict(nV=nV, nF=nF, k=k, d_cols=d_cols, F=arr(F, ip), clamped=int(clamped), b=arr(keep_[0]), e=arr(keep_[1]), fd=arr(keep_[2]), out=arr(out))
    q.update(over or {})
    args = [q[key] for key in ("nV", "nF", "k", "d_cols", "F", "clamped", "b", "e", "fd", "out")]
    rc = fn(*args, C.byref(bad)) if with_guard else fn(*args)
    if rc == 0:
        assert np.all(out[size:] == SENTINEL), "the call wrote past its extent"
        assert not np.any(out[:size] == SENTINEL), "the call left a part of its extent unwritten"
    return rc, bad.value, out[:size]


def host(smg, V, F, **kw):
    """one call of smg_wave_born_host; returns (rc, out)"""
    rc, _, out = _call(smg._lib.load().smg_wave_born_host, False, V, F, **kw)
    return rc, out


def hook(smg, V, F, **kw):
    """one call of smg_debug_wave_born; returns (rc, guard hits, out)"""
    return _call(smg._lib.load().smg_debug_wave_born, True, V, F, **kw)


def operands(name, k, d_cols, clamped):
    """(V, F, known, b, e, fd): b a right-hand side as k_wave_rhs leaves it (0 on the known rows), e a history block, fd with entries of both signs
    and, where d_cols > 1, a zero column"""
    V, F = N.shape(name)
    n = V.shape[0]
    known = N.known_mask(F, n, clamped)
    u, v, _ = N.test_state(V, F, k, clamped)
    speed, sigma = N.nonuniform(V)
    mt, s2 = N.planes(N.mass(V, F)[0], speed, sigma, 0.03)
    b = N.rhs(mt, s2, known, 0.03, u, v)[0]
    e = A.adjoint_state(V, F, k, clamped)[3]
    d = np.ascontiguousarray(np.sin(3.0 * V[:, [0]] + 2.0 * V[:, [1]] + 0.7 * np.arange(d_cols)[None, :]))
    if d_cols > 1:
        d[:, 1] = 0.0
    fd = plane(A.factor(mt, speed), d)
    assert np.any(fd > 0.0) and np.any(fd < 0.0)
    return V, F, known, b, e, fd


def check_launcher(run, name, k, d_cols, clamped):
    """`run(V, F, **operands) -> out` on one mesh against the restatement, bit for bit; shared by the host twin's and the device's tests"""
    V, F, known, b, e, fd = operands(name, k, d_cols, clamped)
    n = V.shape[0]
    out = run(V, F, k=k, d_cols=d_cols, clamped=int(clamped), b=b, e=e, fd=fd)
    rsq0 = np.zeros((k, n))
    rsq0[:, ~known] = (b * b).T[:, ~known]
    want = born(known, fd, e, b, rsq0)
    tag = (name, k, d_cols, clamped)
    for got, w_ in zip(unpack(out, n, k), want):
        assert np.array_equal(got, w_), tag
    assert not np.array_equal(want[0], b) and np.array_equal(want[0][known], b[known]) and np.all(want[1][:, known] == 0.0), tag
    if d_cols > 1:
        assert np.array_equal(want[0][:, 1], b[:, 1]), tag                   # b + 0.0 e == b: the zero column of d leaves its column of b
    return out


# ---- one truncated-Newton step, on any engine: the restatement's (below) or the device's (tests/test_gpu_wave_gn.py) ------------------------------
def newton_step(engine, speed, iters=5, damping=1e-3, c=1e-4, halvings=20):
    """one Gauss-Newton step with `iters` conjugate-gradient iterations on (sum_shots H + lambda I) x = -g from x = 0, lambda = damping times the
    first <d, H d> / |d|^2, then Armijo backtracking from alpha = 1: speed + alpha x is accepted when J(trial) <= J + c alpha <g, x>.
    engine.gradient(speed) -> (J, g); engine.product(d) -> sum_shots H d at the speed of the last gradient call; engine.misfit(speed) -> J.
    -> dict(J, g, x, lam, alpha, found: the halvings or None, Jt, trial, curvatures: <d, H d> per iteration)"""
    J, g = engine.gradient(speed)
    x, r = np.zeros(g.shape), -g
    d, rr, lam, curv = r.copy(), float(r @ r), None, []
    for _ in range(iters):
        Hd = engine.product(d)
        dHd = float(d @ Hd)
        if lam is None:
            lam = damping * dHd / float(d @ d)
        curv.append(dHd)
        q = Hd + lam * d
        a = rr / float(d @ q)
        x, r = x + a * d, r - a * q
        rr, old = float(r @ r), rr
        d = r + (rr / old) * d
    alpha, found, Jt, trial, slope = 1.0, None, None, None, float(g @ x)
    for h in range(halvings + 1):
        trial = speed + alpha * x
        if trial.min() > 0.0:
            Jt = engine.misfit(trial)
            if Jt <= J + c * alpha * slope:
                found = h
                break
        alpha *= 0.5
    return dict(J=J, g=g, x=x, lam=lam, alpha=alpha, found=found, Jt=Jt, trial=trial, curvatures=curv, slope=slope)


def descent_step(engine, speed, c=1e-4, halvings=20):
    """one steepest-descent step with the backtracking of tests/test_gpu_wave_gradient.py's DESCENT -> dict(J, alpha, found, Jt)"""
    J, g = engine.gradient(speed)
    alpha, found, Jt = 0.05 * speed.min() / np.abs(g).max(), None, None
    for h in range(halvings + 1):
        Jt = engine.misfit(speed - alpha * g)
        if Jt <= J - c * alpha * float(g @ g):
            found = h
            break
        alpha *= 0.5
    return dict(J=J, alpha=alpha, found=found, Jt=Jt)


class NpEngine:
    """the engine of newton_step on the restatement: V, F, L, sigma, the lists, the start state, the signal and the data are fixed"""

    def __init__(self, make_ref, u0, v0, steps, sig, data):
        self.make_ref, self.u0, self.v0, self.steps, self.sig, self.data = make_ref, u0, v0, steps, sig, data
        self.ref = self.r = None

    def gradient(self, speed):
        self.ref = self.make_ref(speed)
        self.ref.set_state(self.u0, self.v0)
        self.r = A.gradient(self.ref, self.steps, self.sig, self.data)
        return float(self.r.misfit.sum()), self.r.grad_speed.sum(axis=1)

    def product(self, d):
        return gauss_newton(self.ref, self.r, d).product.sum(axis=1)

    def misfit(self, speed):
        ref = self.make_ref(speed)
        ref.set_state(self.u0, self.v0)
        return float(A.gradient(ref, self.steps, self.sig, self.data, backward=False).misfit.sum())
