"""numpy wrappers of the kernel test hooks (include/smg.h: the handle-free smg_debug_eig_gram, smg_debug_eig_combine, smg_debug_eig_residual,
smg_debug_krylov, smg_debug_union, smg_debug_fixed_reduce; on a handle smg_debug_cycle_f32, smg_debug_convert_f32; read-only, which kernel variants run: smg_debug_wgs_launches,
smg_debug_wgs_level_plan, smg_debug_deep_launches, smg_debug_gs_colour_wpb) and the rounding-error bounds the tests hold them to.

Every wrapper asserts that the hook succeeded and that no guard region around a device buffer changed (no write out of place)."""
import ctypes as C
import math

import numpy as np

U = 2.0 ** -53                     # unit roundoff of fp64
KRY_OPS = dict(zr_zq=0, direction=1, pq=2, step=3, precond_in=4, widen=5)
KRY_NVEC = dict(zr_zq=3, direction=2, pq=2, step=4, precond_in=3, widen=1)
KS_RZ, KS_RZ_PREV, KS_ALPHA, KS_BETA = range(4)
EIG_MAX_GROUPS, KRY_MAX_GROUPS = 256, 512


def gamma(N):
    """gamma_N = N u / (1 - N u): the relative bound of any summation order of N terms in fp64 (Higham, Accuracy and Stability, 3.1)"""
    return N * U / (1.0 - N * U)


def sentinel(shape, dtype=np.float64):
    """an array of 0x5B bytes: a value no kernel computes from the tests' data"""
    a = np.empty(shape, dtype=dtype)
    a.view(np.uint8)[...] = 0x5B
    return a


def _p(a, t=C.c_double):
    if a is None:
        return None
    assert a.flags.c_contiguous
    return a.ctypes.data_as(C.POINTER(t))


def _c(a, dtype=np.float64):
    return None if a is None else np.ascontiguousarray(a, dtype=dtype)


def eig_groups(n):
    return max(1, min((n + 1023) // 1024, EIG_MAX_GROUPS))


def kry_groups(n, k):
    ct = min(k, 64)
    R = 256 // ct
    return max(1, min((n + R * 8 - 1) // (R * 8), KRY_MAX_GROUPS))


def gram(L, Sa, Sb=None, w=None, sym=False, done=0, G=None):
    """G = Sa^T diag(w) Sb for Sa, Sb of shape (nb, n, m); sym: Sb = Sa.  G: the array uploaded as the output (default zeros)."""
    Sa = _c(Sa)
    nb_a, n, m = Sa.shape
    Sb = None if sym else _c(Sb)
    nb_b = nb_a if sym else Sb.shape[0]
    G = np.zeros((nb_a * m, nb_b * m)) if G is None else _c(G).copy()
    w = _c(w)
    groups, bad = C.c_int(-1), C.c_int(-1)
    rc = L.smg_debug_eig_gram(n, m, nb_a, _p(Sa), nb_b, _p(Sb), _p(w), int(sym), done, _p(G), C.byref(groups), C.byref(bad))
    assert rc == 0, L.smg_last_error()
    assert bad.value == 0, "a guard region around a device buffer was overwritten"
    assert groups.value == eig_groups(n)
    return G


def combine(L, S, AS, Cm, make_p=True, done=0, outs=None):
    """X, AX, P, AP for S, AS of shape (nb, n, m) and C of shape (nb m, 2m); P, AP are None without make_p"""
    S, AS, Cm = _c(S), _c(AS), _c(Cm)
    nb, n, m = S.shape
    outs = [np.zeros((n, m)) for _ in range(4)] if outs is None else [_c(o).copy() for o in outs]
    X, AX, P, AP = outs
    bad = C.c_int(-1)
    rc = L.smg_debug_eig_combine(n, m, nb, _p(S), _p(AS), _p(Cm), int(make_p), done, _p(X), _p(AX), _p(P) if make_p else None,
                                 _p(AP) if make_p else None, C.byref(bad))
    assert rc == 0, L.smg_last_error()
    assert bad.value == 0, "a guard region around a device buffer was overwritten"
    return X, AX, P, AP


def residual(L, X, AX, mass, lam, f32=False, done=0, outs=None):
    """(b0, u0, b32, u32, res): outs = the arrays uploaded as the outputs (default: sentinels)"""
    X, AX, mass, lam = _c(X), _c(AX), _c(mass), _c(lam)
    n, m = X.shape
    if outs is None:
        outs = [sentinel((n, m)), sentinel((n, m)), sentinel((n, m), np.float32), sentinel((n, m), np.float32), sentinel(m)]
    b0, u0, b32, u32, res = [o.copy() for o in outs]
    groups, bad = C.c_int(-1), C.c_int(-1)
    rc = L.smg_debug_eig_residual(n, m, _p(X), _p(AX), _p(mass), _p(lam), int(f32), done, _p(b0), _p(u0), _p(b32, C.c_float), _p(u32, C.c_float),
                                  _p(res), C.byref(groups), C.byref(bad))
    assert rc == 0, L.smg_last_error()
    assert bad.value == 0, "a guard region around a device buffer was overwritten"
    assert groups.value == eig_groups(n)
    return b0, u0, b32, u32, res


def krylov(L, op, vecs, s=None, restart=None, e=None, tol=0.0, done=0):
    """one PCG launcher (e: the float input of widen): returns (vecs after, s after, restart after, ctrl),
    ctrl = dict(sumsq, r0 = r_his[0], n_his, done, status)"""
    vecs = [_c(v).copy() for v in vecs]
    assert len(vecs) == KRY_NVEC[op]
    n, k = vecs[0].shape
    v = vecs + [None] * (4 - len(vecs))
    s = None if s is None else _c(s).copy()
    e = None if e is None else _c(e, np.float32).copy()
    rs = None if restart is None else C.c_int(restart)
    cd = (C.c_double * 2)(7.0, 7.0)
    ci = (C.c_int * 3)(7, 7, 7)
    groups, bad = C.c_int(-1), C.c_int(-1)
    rc = L.smg_debug_krylov(KRY_OPS[op], n, k, _p(v[0]), _p(v[1]), _p(v[2]), _p(v[3]), _p(e, C.c_float), _p(s),
                            None if rs is None else C.byref(rs), tol, done, cd, ci, C.byref(groups), C.byref(bad))
    assert rc == 0, L.smg_last_error()
    assert bad.value == 0, "a guard region around a device buffer was overwritten"
    assert groups.value == kry_groups(n, k)
    ctrl = dict(sumsq=cd[0], r0=cd[1], n_his=ci[0], done=ci[1], status=ci[2])
    return vecs, s, (None if rs is None else rs.value), ctrl


FIXED_OPS = dict(SUM=0, MAX=1)


def fixed_reduce(L, op, term):
    """(launch_fixed_sum's or launch_fixed_max's result over term, the chunk count launched) through smg_debug_fixed_reduce; the chunk scratch
    holds exactly that many doubles and the result one, each between guards"""
    term = _c(term).reshape(-1)
    out = sentinel(1)
    groups, bad = C.c_int(-1), C.c_int(-1)
    rc = L.smg_debug_fixed_reduce(FIXED_OPS[op], term.size, _p(term), _p(out), C.byref(groups), C.byref(bad))
    assert rc == 0, L.smg_last_error()
    assert bad.value == 0, "a guard region around a device buffer was overwritten"
    return out[0], groups.value


UNION_OPS = dict(SUMSQ_DECIDE=0, RESTORE=1, COARSE=2)


def _union_call(L, op, m, n, k, a, tol=0.0, done=0, cap=0, ctrl_d=None, ctrl_i=None):
    """smg_debug_union with the arrays of dict a (missing ones: NULL); asserts success and untouched guards"""
    bad = C.c_int(-1)
    g = lambda name, t=C.c_double: _p(a.get(name), t)
    rc = L.smg_debug_union(UNION_OPS[op], m, n, k, g("rptr", C.c_int), g("rows", C.c_int), g("r"), g("u"), g("zsave"), g("ss"), g("mdone", C.c_int),
                           g("nhis", C.c_int), g("his"), cap, g("Ainv"), g("moff", C.c_longlong), g("mlda", C.c_int), g("mrow0", C.c_int),
                           g("row_member", C.c_int), g("b"), tol, done, ctrl_d, ctrl_i, g("r_his"), C.byref(bad))
    assert rc == 0, L.smg_last_error()
    assert bad.value == 0, "a guard region around a device buffer was overwritten"


def union_sumsq_decide(L, rptr, rows, r, u, zsave, ss, mdone, nhis, his, tol, done=0, status=0, n_his=0, his_cap=None, r_last=-1.0, r_his=None):
    """launch_union_sumsq_decide on n x k blocks r, u, zsave and the members' state (his: m x cap); the control block starts from the given
    done / status / n_his / his_cap / r_last and a history r_his (default: his_cap sentinels).  Returns a dict of everything after the launches:
    r, u, zsave, ss, mdone, nhis, his, r_his and the control block's done, status, n_his, r_last, r_prev, sumsq."""
    r, u, zsave = _c(r).copy(), _c(u).copy(), _c(zsave).copy()
    n, k = r.shape
    his = _c(his).copy()
    m, cap = his.shape
    his_cap = cap if his_cap is None else his_cap
    a = dict(rptr=_c(rptr, np.int32), rows=_c(rows, np.int32), r=r, u=u, zsave=zsave, ss=_c(ss).copy(), mdone=_c(mdone, np.int32).copy(),
             nhis=_c(nhis, np.int32).copy(), his=his, r_his=sentinel(max(his_cap, 1)) if r_his is None else _c(r_his).copy())
    assert len(a["rptr"]) == m + 1 and len(a["ss"]) == len(a["mdone"]) == len(a["nhis"]) == m and len(a["r_his"]) >= his_cap
    ci, cd = (C.c_int * 4)(n_his, status, his_cap, -7), (C.c_double * 3)(r_last, 7.0, 7.0)
    _union_call(L, "SUMSQ_DECIDE", m, n, k, a, tol, done, cap, cd, ci)
    a.update(n_his=ci[0], status=ci[1], done=ci[3], r_last=cd[0], r_prev=cd[1], sumsq=cd[2])
    return a


def union_restore(L, rptr, rows, u, zsave, mdone, done=0):
    """launch_union_restore: returns (u, zsave, mdone) after the launch"""
    u, zsave = _c(u).copy(), _c(zsave).copy()
    n, k = u.shape
    a = dict(rptr=_c(rptr, np.int32), rows=_c(rows, np.int32), u=u, zsave=zsave, mdone=_c(mdone, np.int32).copy())
    _union_call(L, "RESTORE", len(a["mdone"]), n, k, a, done=done)
    return a["u"], a["zsave"], a["mdone"]


def union_coarse(L, blocks, members, b, u, done=0):
    """launch_blockdiag_gemv_add on the members' dense blocks (blocks[i]: lda_i x lda_i with the matrix of member i's members[i] rows in the
    leading part), laid side by side as the handle lays them: returns (u, b) after the launches"""
    b, u = _c(b).copy(), _c(u).copy()
    n, k = u.shape
    sizes = [int(np.asarray(B).shape[0]) for B in blocks]
    moff = np.concatenate([[0], np.cumsum([s * s for s in sizes])[:-1]]).astype(np.int64)
    mrow0 = np.concatenate([[0], np.cumsum(members)]).astype(np.int32)
    assert mrow0[-1] == n and len(members) == len(blocks)
    a = dict(Ainv=np.concatenate([_c(B).ravel() for B in blocks]), moff=moff, mlda=np.asarray(sizes, np.int32), mrow0=mrow0,
             row_member=np.repeat(np.arange(len(blocks), dtype=np.int32), members), b=b, u=u)
    _union_call(L, "COARSE", len(blocks), n, k, a, done=done)
    return a["u"], a["b"]


F32_OPS = dict(A=0, RESID=1, RESTRICT=2, PROLONG_ADD=3, RELAX=4, COARSE=5, VCYCLE=6)
F32_IN_LEVEL = dict(A=0, RESID=0, RESTRICT=0, PROLONG_ADD=1, RELAX=0, COARSE=0, VCYCLE=0)     # level of in0 relative to lv
F32_OUT_LEVEL = dict(A=0, RESID=0, RESTRICT=1, PROLONG_ADD=0, RELAX=0, COARSE=0, VCYCLE=0)    # ... of out


def _f32_block(a, rows, name):
    a = np.asarray(a)
    if a.ndim == 1:
        a = a[:, None]
    assert a.dtype == np.float32, "%s: the fp32 pieces take float32 blocks (round them where the cycle rounds them)" % name
    assert a.shape[0] == rows, "%s: expected %d rows, got %d (the C ABI takes bare pointers)" % (name, rows, a.shape[0])
    return np.asfortranarray(a)


def _fp(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_float))


def cycle_f32(mg, op, lv, in0, in1=None, out=None, pre=0, post=0, done=0, check=True):
    """One piece of the fp32 V-cycle on hierarchy mg (smg_debug_cycle_f32), blocks in the caller's numbering of their level.
    out: what is uploaded to the buffers the op writes (the iterate of PROLONG_ADD / RELAX / COARSE / VCYCLE; default zeros).
    Returns the output block -- RESTRICT: the pair (PT r, the zeroed coarse iterate), `out` a pair likewise -- after asserting
    (check) that no buffer the op only reads has changed and, with done = 1, that no fp32 vector of any level has (the second iterate and
    the update vector of the Jacobi-type levels and the coarser levels of a cycle included)."""
    L = mg.L
    if op == "COARSE":
        lv = mg.n_levels - 1
    rows_in, rows_out = mg.rows(lv + F32_IN_LEVEL[op]), mg.rows(lv + F32_OUT_LEVEL[op])
    in0 = _f32_block(in0, rows_in, op)
    k = in0.shape[1]
    in1 = None if in1 is None else _f32_block(in1, rows_in, op)
    if op == "RESTRICT":
        pair = (np.zeros((rows_out, k), np.float32),) * 2 if out is None else out
        o = np.concatenate([_f32_block(x, rows_out, op).ravel(order="F") for x in pair])
    else:
        o = (np.zeros((rows_out, k), np.float32, order="F") if out is None else _f32_block(out, rows_out, op).copy(order="F"))
        assert o.shape[1] == k
    changed = C.c_int(-1)
    rc = L.smg_debug_cycle_f32(mg.h, F32_OPS[op], lv, k, pre, post, done, _fp(in0), _fp(in1), _fp(o), C.byref(changed))
    assert rc == 0, L.smg_last_error()
    if check:
        assert not changed.value & 1, "%s on level %d: a buffer the op only reads was written" % (op, lv)
        assert not changed.value & 4, "%s on level %d with done = 1: an fp32 vector of the cycle (some level's fp32 b / u / r / t / d) was written" % (op, lv)
        assert changed.value == 0, changed.value
    if op == "RESTRICT":
        return o[:rows_out * k].reshape((rows_out, k), order="F"), o[rows_out * k:].reshape((rows_out, k), order="F")
    return o


def residual_to_f32(mg, r, done=0, outs=None):
    """(b32, u32) = ((float) r, 0) on level 0 (smg_debug_convert_f32); outs: what is uploaded as b32, u32 (default: sentinels)"""
    r = np.asfortranarray(np.asarray(r, dtype=np.float64).reshape(mg.rows(0), -1))
    k = r.shape[1]
    b32, u32 = [_f32_block(o, mg.rows(0), "RESIDUAL_TO_F32").copy(order="F") for o in (outs or (sentinel(r.shape, np.float32),) * 2)]
    changed = C.c_int(-1)
    rc = mg.L.smg_debug_convert_f32(mg.h, 0, k, done, _p(r.T), None, None, _fp(b32), _fp(u32), C.byref(changed))
    assert rc == 0, mg.L.smg_last_error()
    assert changed.value == 0, "RESIDUAL_TO_F32: the input changed or the launch wrote behind the block (inputs_changed = %d)" % changed.value
    return b32, u32


def add_correction(mg, z, e, done=0):
    """z + (double) e on level 0 (smg_debug_convert_f32)"""
    z = np.asfortranarray(np.asarray(z, dtype=np.float64).reshape(mg.rows(0), -1)).copy(order="F")
    e = _f32_block(e, mg.rows(0), "ADD_CORRECTION")
    changed = C.c_int(-1)
    rc = mg.L.smg_debug_convert_f32(mg.h, 1, z.shape[1], done, None, _fp(e), _p(z.T), None, None, C.byref(changed))
    assert rc == 0, mg.L.smg_last_error()
    assert changed.value == 0, "ADD_CORRECTION: the input changed or the launch wrote behind the block (inputs_changed = %d)" % changed.value
    return z


def schur_partition(mg):
    """block_of_row of the handle's Schur-complement coarse solver (smg_debug_schur_partition): interior block per coarsest-level row, -1 = separator"""
    nb, ns = C.c_int(-1), C.c_int(-1)
    out = np.full(mg.rows(mg.n_levels - 1), -3, np.int32)
    rc = mg.L.smg_debug_schur_partition(mg.h, C.byref(nb), C.byref(ns), _p(out, C.c_int))
    assert rc == 0, mg.L.smg_last_error()
    assert out.min() >= -1 and (out == -1).sum() == ns.value and out.max() == nb.value - 1, "not a partition"
    return out


def wgs_level_plan(mg, lv, k, from_host=False):
    """(n_pieces, nb_max, rim_pitch) of the wave Gauss-Seidel plan of level lv -- the one relax() sweeps with for k columns in the handle's present
    state (nothing is built), or from_host: the plan as the first sweep would build it, built on the host -- or None"""
    a, b, c = C.c_int(-1), C.c_int(-1), C.c_int(-1)
    rc = mg.L.smg_debug_wgs_level_plan(mg.h, lv, k, int(from_host), C.byref(a), C.byref(b), C.byref(c))
    assert rc == 0, mg.L.smg_last_error()
    return (a.value, b.value, c.value) if a.value > 0 else None


def wgs_launches(L, n_pieces, nb_max, rim_pitch, k):
    """(NBMAX, RIMI, [(KB, groups), ...]): the k_wgs launches of one piece colour in this process (smg_debug_wgs_launches)"""
    nbm, ri, n = C.c_int(-1), C.c_int(-1), C.c_int(-1)
    out = np.full(2 * (k + 1), -1, np.int32)
    rc = L.smg_debug_wgs_launches(n_pieces, nb_max, rim_pitch, k, C.byref(nbm), C.byref(ri), _p(out, C.c_int), k + 1, C.byref(n))
    assert rc == 0, L.smg_last_error()
    assert 1 <= n.value <= k
    la = [(int(out[2 * i]), int(out[2 * i + 1])) for i in range(n.value)]
    assert sum(kb * g for kb, g in la) == k and all(1 <= kb <= 4 and g >= 1 for kb, g in la), la
    return nbm.value, ri.value, la


def deep_launches(mg, lv, which, mode, k):
    """(w_max, [(columns, NBMAX class of k_sell_deep or 0 = k_sell), ...]): the launches of A x (mode "A") or b - A x ("RESID") with k <= 4 fp64
    columns on the device image which ("A", "P", "PT") of level lv in this process (smg_debug_deep_launches)"""
    w, n = C.c_int(-1), C.c_int(-1)
    out = np.full(2 * (k + 1), -1, np.int32)
    rc = mg.L.smg_debug_deep_launches(mg.h, lv, {"A": 0, "P": 1, "PT": 2}[which], {"A": 0, "RESID": 1}[mode], k, C.byref(w), _p(out, C.c_int), k + 1, C.byref(n))
    assert rc == 0, mg.L.smg_last_error()
    return w.value, [(int(out[2 * i]), int(out[2 * i + 1])) for i in range(n.value)]


def gs_colour_wpb(mg, lv, n_slices):
    """(waves per workgroup, panel pitch, lower width): a one-column Gauss-Seidel colour launch of n_slices slices on the image level lv sweeps on, in
    this process (smg_debug_gs_colour_wpb)"""
    wpb, stride, w_lo = C.c_int(-1), C.c_int(-1), C.c_int(-1)
    rc = mg.L.smg_debug_gs_colour_wpb(mg.h, lv, n_slices, C.byref(wpb), C.byref(stride), C.byref(w_lo))
    assert rc == 0, mg.L.smg_last_error()
    return wpb.value, stride.value, w_lo.value


def exact_dot(a, b):
    """sum_i a_i b_i correctly rounded: every product split into four exact fp64 products (Veltkamp), summed by math.fsum"""
    return math.fsum(_exact_products(a, b))


def _exact_products(a, b):
    # Veltkamp split: x = hi + lo with 26-bit halves, so hi*hi, hi*lo, lo*lo are exact
    def split(x):
        c = (2.0 ** 27 + 1.0) * x
        hi = c - (c - x)
        return hi, x - hi
    ah, al = split(np.asarray(a, dtype=np.float64))
    bh, bl = split(np.asarray(b, dtype=np.float64))
    return np.concatenate([(ah * bh).ravel(), (ah * bl).ravel(), (al * bh).ravel(), (al * bl).ravel()])
