"""The numpy / scipy restatement of the wave object's adjoint pass (include/smg.h: smg_wave_gradient), in the kernels' operation order, with direct
solves on tests/wave_np.py's WaveNp; the ctypes wrappers of smg_wave_adjoint_host and smg_debug_wave_adjoint; the misfit in complex arithmetic for
complex-step derivatives.

    keep      e = dt v - (0.5 s2) (u' - u)
    residual  rho = trace - observed (observed missing: trace);  sq = rho rho;  J = 0.5 (the fixed-order sum of a column's sq)
    inject    p = p + (rho[s_0] + rho[s_1] + ...)          a vertex's slots in ascending order; a receiver on a known row contributes nothing
    rhs       g = p + q2 q;  gsq = g g                     both 0.0 on a known row
    solve     A y = g                                      the matrix of the forward step
    advance   G = G + y e;  t = mt y;  p' = (s2 t - p) - (2.0 q2) q;  q' = dt t - q
    signal    x = a y[src];  gs[n] = gs[n] + x;  gs[n + 1] = gs[n + 1] + x
    scale     grad_speed = ((-2.0 mt) / speed) G

Only +, - and * occur in the kernels: the library's host twin and its kernels are held to this file bit for bit.  Vertex blocks are nV x k arrays
here (the library's are column-major); term planes are k x entries; trace and signal rows are (slot) x column."""
import ctypes as C

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import wave_np as N
from wave_np import SENTINEL, fixed_sum

KEEP, RESIDUAL, INJECT, RHS, ADVANCE, SIGNAL, SCALE = range(7)


# ---- the kernels' expressions --------------------------------------------------------------------------------------------------------------------
def keep(s2, dt, u, v, u1):
    d = u1 - u
    return dt * v - (0.5 * s2)[:, None] * d


def residual(trace, observed):
    """(rho rows x slots x k, sq k x (rows x slots), the k fixed-order sums) of k_wave_adj_residual and its reductions"""
    rho = np.array(trace) if observed is None else trace - observed
    k = rho.shape[-1]
    sq = np.ascontiguousarray((rho * rho).reshape(-1, k).T)
    return rho, sq, np.array([fixed_sum(t) for t in sq])


def group(idx, known):
    """[(vertex, its slots ascending)] in ascending vertex order, without the vertices on a known row: wave_group_receivers"""
    idx = np.asarray(idx)
    return [(int(v), np.flatnonzero(idx == v)) for v in np.unique(idx) if not known[v]]


def inject(p, rho_row, groups):
    """p + R' rho for one trace row (slots x k)"""
    p = np.array(p)
    for v, slots in groups:
        x = np.array(rho_row[slots[0]])
        for s in slots[1:]:
            x = x + rho_row[s]
        p[v] = p[v] + x
    return p


def rhs(known, q2, p, q):
    """(g nV x k, gsq k x nV, the sum of gsq)"""
    g = p + q2 * q
    g[known] = 0.0
    gsq = np.ascontiguousarray((g * g).T)
    return g, gsq, fixed_sum(gsq.reshape(-1))


def advance(mt, s2, dt, q2, y, e, p, q, G):
    Gn = G + y * e
    t = mt[:, None] * y
    pn = (s2[:, None] * t - p) - (2.0 * q2) * q
    qn = dt * t - q
    return pn, qn, Gn


def signal(a, y, idx, gs0, gs1):
    x = a * y[idx]
    return gs0 + x, gs1 + x


def factor(mt, speed):
    n = mt.shape[0]
    return (-2.0 * mt) / (np.ones(n) if speed is None else np.broadcast_to(np.asarray(speed, dtype=np.float64), (n,)))


def scale(fac, G):
    return fac[:, None] * G


# ---- the method with direct solves ---------------------------------------------------------------------------------------------------------------
class Result:
    pass


def gradient(ref, n_steps, signal_=None, observed=None, backward=True, after_step=None):
    """smg_wave_gradient on the restatement `ref` (a wave_np.WaveNp with its state, sources and receivers set), direct solves.  -> Result with
    misfit (k), grad_speed, grad_u0, grad_v0 (nV x k), grad_signal ((n_steps + 1) x n_src x k or None), traces, and for the bounds of
    BOUND below the per-step records fwd = [(u_n, v_n, u_n+1, v_n+1, b, res)], e = [e_n], rho, and bwd = [(n, g, y, res,
    p, q before the step)] in the order the steps ran.  `ref` is left n_steps steps on"""
    dt, q2, a = ref.p["dt"], ref.q2, ref.a
    r = Result()
    r.fwd, r.e, T = [], [], []
    for t in range(n_steps):
        _, tr = ref.step(1, None if signal_ is None else signal_[t:t + 2])
        r.fwd.append((ref.u0, ref.v0, ref.u, ref.v, ref.b, ref.res))
        r.e.append(keep(ref.s2, dt, ref.u0, ref.v0, ref.u))
        T.append(tr[0])
        if after_step is not None:
            after_step(t)
    r.traces = np.stack(T)
    r.rho, _, sums = residual(r.traces, observed)
    r.misfit = 0.5 * sums
    r.grad_speed = r.grad_u0 = r.grad_v0 = r.grad_signal = None
    r.bwd = []
    if not backward:
        return r
    n, k = ref.u.shape
    groups = group(ref.rec, ref.known)
    p, q, y, G = inject(np.zeros((n, k)), r.rho[n_steps - 1], groups), np.zeros((n, k)), np.zeros((n, k)), np.zeros((n, k))
    gs = None if signal_ is None else np.zeros((n_steps + 1, ref.src.size, k))
    for t in range(n_steps - 1, -1, -1):
        g, _, ss = rhs(ref.known, q2, p, q)
        if ss == 0.0:
            y, res = np.zeros((n, k)), np.zeros(k)
        else:
            y, res = ref.solve(g)
        r.bwd.append((t, g, y, res, p, q))
        p, q, G = advance(ref.mt, ref.s2, dt, q2, y, r.e[t], p, q, G)
        if gs is not None:
            gs[t], gs[t + 1] = signal(a, y, ref.src, gs[t], gs[t + 1])
        if t >= 1:
            p = inject(p, r.rho[t - 1], groups)
    r.grad_speed, r.grad_u0, r.grad_v0, r.grad_signal = scale(factor(ref.mt, ref.speed), G), p, q, gs
    return r


# ---- how far two evaluations of the gradient can be apart: BOUND of tests/test_gpu_wave_gradient.py and tests/test_wave_adjoint_host.py ----------
def gradient_bound(ref, r, norms, tol, chain):
    """BOUND: the distance between the restatement's gradient `r` (direct solves) and another evaluation of the same call whose solves stop at the
    absolute residual `tol` (0: exact answers) and whose forward states are within chain[n - 1] of the restatement's (u_n, v_n), n = 1 .. N (the 2-norm
    of one column's u and v together: wave_np.Chain).  | | is the 2-norm of one column, eps = 2^-52, mu = min 0.5 s2 mt, M = the largest number of
    slots of one vertex, lambda_n = (p, q) before step n - 1 runs (lambda_N = R' rho_N), C_0 = 0.

    The adjoint recursion is lambda_n = S' lambda_n+1 + (R' rho_n, 0) with S the forward step map, so the two evaluations' lambda are apart by
    eps_n <= sum_(j >= n) |S^(j - n)|_2 delta_j (the norms of wave_np.step_map), delta_j the injection of step j:
        beta_j  = (10 tol + res_np) / mu + 8 eps |(|p| + q2 |q|)| / mu          the two solves, and g = p + q2 q rounded differently on each side
        delta_j = max(mt) sqrt(max(s2)^2 + dt^2) beta_j                          y enters p as s2 mt y and q as dt mt y
                  + 8 eps sqrt(|(|s2 mt y| + |p| + 2 q2 |q|)|^2 + |(dt |mt y| + |q|)|^2)      the roundings of p' and q'
                  + M C_j + 2 eps (M |rho_j| + |p|)                   (j >= 1) rho = R u - observed, |R' R|_2 <= M; the slots' sum and the add
        delta_N = M C_N + 2 eps M |rho_N|
    From these
        |dy_j|   <= sqrt(1 + q2^2) eps_(j+1) / mu + beta_j                                      y_j = A^-1 (p + q2 q) of lambda_(j+1)
        |de_j|   <= dt C_j + 0.5 max(s2) (C_(j+1) + C_j) + 4 eps |(dt |v| + 0.5 s2 (|u'| + |u|))|    e_j = dt v_j - 0.5 s2 (u_(j+1) - u_j)
        state    = eps_0                                                                         (grad_u0, grad_v0) together
        speed    = max|fac| (sum_j (|dy_j| max|e_j| + max|y_j| |de_j|) + (N + 1) eps sum_j |y_j e_j|) + 2 eps |grad_speed|
        signal_n = a (|dy_n| + |dy_(n-1)|) + 4 eps |grad_signal_n|                              over the sources
    -> dict(state=k values, speed=k values, signal=(N + 1) x k)"""
    EPS = N.EPS
    col = lambda x: np.linalg.norm(x, axis=0)   # noqa: E731
    n_steps, k = len(r.fwd), r.misfit.size
    dt, q2, a, mu = ref.p["dt"], ref.q2, ref.a, ref.mu
    Cn = [np.zeros(k)] + [np.asarray(c, dtype=np.float64) * np.ones(k) for c in chain]
    M = float(np.max(np.unique(ref.rec, return_counts=True)[1]))
    smax, cA = float(ref.s2.max()), float(ref.mt.max()) * np.sqrt(float(ref.s2.max()) ** 2 + dt * dt)
    rho_norm = lambda n: col(r.rho[n - 1].reshape(-1, k))   # noqa: E731  (rho_n is trace row n - 1)
    delta, beta = {n_steps: M * Cn[n_steps] + 2.0 * EPS * M * rho_norm(n_steps)}, {}
    rec = {t: (g, y, res, p, q) for t, g, y, res, p, q in r.bwd}
    for j in range(n_steps):
        g, y, res, p, q = rec[j]
        t = ref.mt[:, None] * np.abs(y)
        beta[j] = (10.0 * tol + res) / mu + 8.0 * EPS * col(np.abs(p) + q2 * np.abs(q)) / mu
        delta[j] = cA * beta[j] + 8.0 * EPS * np.sqrt(col(ref.s2[:, None] * t + np.abs(p) + 2.0 * q2 * np.abs(q)) ** 2 + col(dt * t + np.abs(q)) ** 2)
        if j >= 1:
            delta[j] = delta[j] + M * Cn[j] + 2.0 * EPS * (M * rho_norm(j) + col(p))
    eps_ = {n: sum(norms[j - n] * delta[j] for j in range(n, n_steps + 1)) for n in range(n_steps + 1)}
    dy, dG, mag = {}, np.zeros(k), np.zeros(k)
    for j in range(n_steps):
        g, y, res, p, q = rec[j]
        u0, v0, u1, _, _, _ = r.fwd[j]
        dy[j] = np.sqrt(1.0 + q2 * q2) * eps_[j + 1] / mu + beta[j]
        de = dt * Cn[j] + 0.5 * smax * (Cn[j + 1] + Cn[j]) + 4.0 * EPS * col(dt * np.abs(v0) + 0.5 * ref.s2[:, None] * (np.abs(u1) + np.abs(u0)))
        dG = dG + dy[j] * np.max(np.abs(r.e[j]), axis=0) + np.max(np.abs(y), axis=0) * de
        mag = mag + col(y * r.e[j])
    fmax = float(np.max(np.abs(factor(ref.mt, ref.speed))))
    out = dict(state=eps_[0], speed=fmax * (dG + (n_steps + 1) * EPS * mag) + 2.0 * EPS * col(r.grad_speed))
    if r.grad_signal is not None:
        zero = np.zeros(k)
        out["signal"] = np.stack([a * (dy.get(n, zero) + dy.get(n - 1, zero)) + 4.0 * EPS * col(r.grad_signal[n]) for n in range(n_steps + 1)])
    return out


def misfit_complex(ref, u0, v0, n_steps, signal_=None, observed=None, speed=None, states=None):
    """J (k complex values) of `n_steps` steps from (u0, v0) with the scheme's operations in complex arithmetic -- complex direct solves, rho rho
    without a conjugate -- so that Im J(x + i h d) / h is the derivative along d: `speed`, u0, v0 and signal_ may be complex.  ref supplies the
    mesh, the masses, sigma, the lists and dt; states (a list): (u_n, v_n), n = 0 .. n_steps, are appended"""
    n = ref.V.shape[0]
    spd = np.ones(n) if speed is None and ref.speed is None else np.broadcast_to(np.asarray(ref.speed if speed is None else speed), (n,))
    mt = ref.m / (spd * spd)
    dt, q2, a, s2 = ref.p["dt"], ref.q2, ref.a, ref.s2
    A = (sp.diags(0.5 * s2 * mt) + a * ref.C.astype(np.complex128)).tocsr()
    lu = spla.splu(A[ref.free][:, ref.free].tocsc().astype(np.complex128))
    u, v = np.asarray(u0, dtype=np.complex128), np.asarray(v0, dtype=np.complex128)
    J = np.zeros(u.shape[1], dtype=np.complex128)
    if states is not None:
        states.append((u, v))
    for t in range(n_steps):
        b = mt[:, None] * (s2[:, None] * u + dt * v)
        if signal_ is not None:
            b[ref.src] = b[ref.src] + a * (signal_[t] + signal_[t + 1])
        w = np.zeros(b.shape, dtype=np.complex128)
        w[ref.free] = lu.solve(np.ascontiguousarray(b[ref.free]))
        u1 = w - u
        v = q2 * (u1 - u) - v
        u = u1
        rho = u[ref.rec] - (0.0 if observed is None else observed[t])
        J = J + 0.5 * np.sum(rho * rho, axis=0)
        if states is not None:
            states.append((u, v))
    return J


# ---- test operands -------------------------------------------------------------------------------------------------------------------------------
def receiver_list(V, F, clamped=False):
    """six slots: vertex 0 and vertex nV - 1 (on the clamped boundary or not), an interior vertex twice, vertex 0 again, the first usable vertex"""
    n = V.shape[0]
    ok = np.setdiff1d(np.arange(n), N.boundary_vertices(np.asarray(F))) if clamped else np.arange(n)
    return np.array([0, n - 1, ok[len(ok) // 2], ok[0], ok[len(ok) // 2], 0], dtype=np.int32)


def adjoint_state(V, F, k, clamped=False):
    """(y, p, q, e, G as nV x k): smooth fields; y, p, q, G are 0 on the boundary when clamped, as in a run"""
    u, v, w = N.test_state(V, F, k, clamped)
    c = np.arange(k)[None, :]
    e = np.ascontiguousarray(np.sin(2.0 * V[:, [0]] - V[:, [2]] + 0.5 * c) + 0.1)
    G = np.ascontiguousarray(0.5 * np.cos(V[:, [1]] + 2.0 * V[:, [0]] - c))
    if clamped:
        G[N.boundary_vertices(np.asarray(F))] = 0.0
    return w, u, v, e, G


# ---- the library's side, shared with tests/test_gpu_wave_gradient.py -----------------------------------------------------------------------------
OPERANDS = {KEEP: "ccc", RESIDUAL: "rr", INJECT: "cr", RHS: "cc", ADVANCE: "ccccc", SIGNAL: "crr", SCALE: "c"}   # c: nV x k column-major; r: rows, row-major


def out_size(op, nV, k, n_idx, n_rows):
    nk, ent = nV * k, n_rows * n_idx
    return {KEEP: nk, RESIDUAL: 2 * ent * k + k, INJECT: nk, RHS: 2 * nk + 1, ADVANCE: 3 * nk, SIGNAL: 2 * n_idx * k, SCALE: nk}[op]


def unpack(op, out, nV, k, n_idx, n_rows):
    """the outputs of an op in the restatement's shapes"""
    nk, ent = nV * k, n_rows * n_idx
    col = lambda j: out[j * nk:(j + 1) * nk].reshape(k, nV).T   # noqa: E731
    if op in (KEEP, INJECT, SCALE):
        return (col(0),)
    if op == RESIDUAL:
        return out[:ent * k].reshape(n_rows, n_idx, k), out[ent * k:2 * ent * k].reshape(k, ent), out[2 * ent * k:]
    if op == RHS:
        return col(0), out[nk:2 * nk].reshape(k, nV), out[2 * nk]
    if op == ADVANCE:
        return col(0), col(1), col(2)
    return out[:n_idx * k].reshape(n_idx, k), out[n_idx * k:].reshape(n_idx, k)


def _call(fn, with_guard, op, V, F, k=1, speed=None, sigma=None, clamped=0, dt=0.5, x=(), idx=None, n_rows=0, over=None, pad=64):
    """`pad` doubles of sentinel follow the op's extent in `out`: nothing past the extent may be written"""
    ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
    nV, nF = V.shape[0], F.shape[0]
    F = np.ascontiguousarray(F, dtype=np.int32)
    rows = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64).reshape(-1)                 # noqa: E731
    cols = lambda a: None if a is None else np.ascontiguousarray(np.asarray(a, dtype=np.float64).T).reshape(-1)   # noqa: E731  (column-major)
    kinds = OPERANDS.get(op, "ccccc")
    xs = [(cols if kinds[j] == "c" else rows)(x[j]) if j < len(x) and j < len(kinds) else None for j in range(5)]
    ints = None if idx is None else np.ascontiguousarray(idx, dtype=np.int32).reshape(-1)
    keep_ = [rows(V), rows(speed), rows(sigma)]
    arr = lambda a, ty=dp: None if a is None else a.ctypes.data_as(ty)   # noqa: E731
    n_idx = 0 if ints is None else ints.size
    size = out_size(op, nV, max(k, 0), n_idx, n_rows) if op in OPERANDS else 1
    out = np.full(size + pad, SENTINEL)
    bad = C.c_int(-1)
    q = dict(nV=nV, nF=nF, k=k, F=arr(F, ip), V=arr(keep_[0]), speed=arr(keep_[1]), sigma=arr(keep_[2]), clamped=int(clamped), dt=float(dt), x0=arr(xs[0]),
             x1=arr(xs[1]), x2=arr(xs[2]), x3=arr(xs[3]), x4=arr(xs[4]), idx=arr(ints, ip), n_idx=n_idx, n_rows=int(n_rows), out=arr(out))
    q.update(over or {})
    args = [op] + [q[key] for key in ("nV", "nF", "k", "F", "V", "speed", "sigma", "clamped", "dt", "x0", "x1", "x2", "x3", "x4", "idx", "n_idx", "n_rows", "out")]
    rc = fn(*args, C.byref(bad)) if with_guard else fn(*args)
    if rc == 0:
        assert np.all(out[size:] == SENTINEL), "op %d wrote past its extent" % op
        assert not np.any(out[:size] == SENTINEL), "op %d left a part of its extent unwritten" % op
    return rc, bad.value, out[:size]


def host(smg, op, V, F, **kw):
    """one call of smg_wave_adjoint_host; returns (rc, out)"""
    rc, _, out = _call(smg._lib.load().smg_wave_adjoint_host, False, op, V, F, **kw)
    return rc, out


def hook(smg, op, V, F, **kw):
    """one call of smg_debug_wave_adjoint; returns (rc, guard hits, out)"""
    return _call(smg._lib.load().smg_debug_wave_adjoint, True, op, V, F, **kw)


def check_launchers(run, name, k, clamped):
    """all seven ops of `run(op, V, F, **operands) -> out` on one mesh against the restatement, bit for bit; shared by the host twin's and the
    device's tests.  The receiver list holds vertex 0, vertex nV - 1 and duplicates; the residual is taken with and without observed traces.
    Returns the outputs for a comparison of the two."""
    V, F = N.shape(name)
    n = V.shape[0]
    y, p, q, e, G = adjoint_state(V, F, k, clamped)
    u, v, w = N.test_state(V, F, k, clamped)
    speed, sigma = N.nonuniform(V)
    dt = 0.03
    mt, s2 = N.planes(N.mass(V, F)[0], speed, sigma, dt)
    a, q2 = 0.25 * dt * dt, 2.0 / dt
    known = N.known_mask(F, n, clamped)
    rec = receiver_list(V, F, clamped)
    src = N.test_lists(V, F, 3, clamped)
    assert 0 in rec and n - 1 in rec and np.unique(rec).size < rec.size
    rng = np.random.default_rng(n + 10 * k)
    rows = 3
    tr, ob = rng.standard_normal((rows, rec.size, k)), rng.standard_normal((rows, rec.size, k))
    gs0, gs1 = rng.standard_normal((src.size, k)), rng.standard_normal((src.size, k))
    eq = np.array_equal
    common = dict(k=k, speed=speed, sigma=sigma, clamped=int(clamped), dt=dt)
    tag = (name, k, clamped)
    outs = [run(KEEP, V, F, x=(u, v, w), **common)]
    assert eq(unpack(KEEP, outs[-1], n, k, 0, 0)[0], keep(s2, dt, u, v, w)), tag + ("keep",)
    for observed in (ob, None):
        outs.append(run(RESIDUAL, V, F, x=(tr, observed), idx=rec, n_rows=rows, **common))
        for got, want in zip(unpack(RESIDUAL, outs[-1], n, k, rec.size, rows), residual(tr, observed)):
            assert eq(got, want), tag + ("residual",)
    outs.append(run(INJECT, V, F, x=(p, tr[1]), idx=rec, **common))
    want = inject(p, tr[1], group(rec, known))
    assert eq(unpack(INJECT, outs[-1], n, k, rec.size, 0)[0], want) and not eq(want, p), tag + ("inject",)
    assert eq(want[known], p[known]), "a receiver on a clamped row contributes nothing"
    outs.append(run(RHS, V, F, x=(p, q), **common))
    want = rhs(known, q2, p, q)
    for got, w_ in zip(unpack(RHS, outs[-1], n, k, 0, 0), want):
        assert eq(got, w_), tag + ("rhs",)
    assert np.all(want[0][known] == 0.0) and np.all(want[1][:, known] == 0.0)
    outs.append(run(ADVANCE, V, F, x=(y, p, q, e, G), **common))
    want = advance(mt, s2, dt, q2, y, e, p, q, G)
    for got, w_ in zip(unpack(ADVANCE, outs[-1], n, k, 0, 0), want):
        assert eq(got, w_), tag + ("advance",)
    assert not clamped or all(np.all(w_[known] == 0.0) for w_ in want), "exact zeros on the clamped rows"
    outs.append(run(SIGNAL, V, F, x=(y, gs0, gs1), idx=src, **common))
    for got, w_ in zip(unpack(SIGNAL, outs[-1], n, k, src.size, 0), signal(a, y, src, gs0, gs1)):
        assert eq(got, w_), tag + ("signal",)
    for spd in (speed, None):
        outs.append(run(SCALE, V, F, x=(G,), **dict(common, speed=spd)))
        mt_ = N.planes(N.mass(V, F)[0], spd, sigma, dt)[0]
        assert eq(unpack(SCALE, outs[-1], n, k, 0, 0)[0], scale(factor(mt_, spd), G)), tag + ("scale",)
    return outs
