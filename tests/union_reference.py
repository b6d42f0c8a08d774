"""numpy restatement of what only a union handle runs (csrc/smg_union_device.hip), no GPU: the per-member sum of squares in the kernel's own
order, the break test of every member, the restore of the ended members, the block-diagonal coarse product, and the loop they form
(csrc/smg_cycle.cpp: enqueue_residual_ss / enqueue_cycle_part for a union).  Blocks are n x k arrays; a member is the list of its rows.

The launchers are held to these functions by tests/test_gpu_union_kernels.py (through smg_debug_union), the loop to UnionLoop; on the CPU
tests/test_union_host.py holds the functions to fsum and UnionLoop to the stand-alone oracle of every member."""
import math

import numpy as np

from kernel_hooks import exact_dot

THREADS = 1024                      # k_union_sumsq: one workgroup of 1024 threads per member
R_MAX = 1.7e308                     # k_union_decide: a residual above this counts as not finite


def member_sumsq(r, rows_i, k):
    """ss of one member as k_union_sumsq forms it: thread t adds the squares of positions t, t + 1024, ... of the row list (columns ascending
    inside a row, product and addition separate), then the tree red[t] += red[t + o], o = 512 ... 1."""
    r = np.asarray(r, dtype=np.float64).reshape(-1, k)
    rows_i = np.asarray(rows_i, dtype=np.int64)
    red = np.zeros(THREADS)
    with np.errstate(over="ignore", invalid="ignore"):
        for p0 in range(0, len(rows_i), THREADS):
            chunk = r[rows_i[p0:p0 + THREADS]]                  # thread t holds row p0 + t
            for c in range(k):
                sq = chunk[:, c] * chunk[:, c]
                red[:len(sq)] = red[:len(sq)] + sq
        o = THREADS // 2
        while o > 0:
            red[:o] = red[:o] + red[o:2 * o]
            o >>= 1
    return red[0]


class UnionState:
    """what k_union_decide reads and writes: the members' mdone / nhis / his (m x cap) and the handle's control block"""

    def __init__(self, m, cap, his_cap=None, done=0, status=0, n_his=0, r_last=-1.0, mdone=None, nhis=None, his=None, r_his=None):
        self.m, self.cap = m, cap
        self.mdone = np.zeros(m, np.int32) if mdone is None else np.array(mdone, np.int32)
        self.nhis = np.zeros(m, np.int32) if nhis is None else np.array(nhis, np.int32)
        self.his = np.zeros((m, cap)) if his is None else np.array(his, np.float64).reshape(m, cap)
        self.his_cap = cap if his_cap is None else his_cap
        self.r_his = np.zeros(self.his_cap) if r_his is None else np.array(r_his, np.float64)
        self.done, self.status, self.n_his = done, status, n_his
        self.r_last, self.r_prev, self.sumsq = r_last, -1.0, -1.0


def decide(st, ss, tol):
    """k_union_decide, line by line"""
    if st.done:
        return st
    tot, all_ended = 0.0, 1
    with np.errstate(over="ignore", invalid="ignore"):
        for i in range(st.m):
            if not st.mdone[i]:
                r = float(np.sqrt(np.float64(ss[i])))
                j = int(st.nhis[i])
                if j < st.cap:
                    st.his[i, j] = r
                st.nhis[i] = j + 1
                if not (r == r) or r > R_MAX:
                    st.mdone[i] = 2
                elif r < tol:
                    st.mdone[i] = 1
            if st.mdone[i] != 2:
                tot = float(np.float64(tot) + np.float64(ss[i]))
            if not st.mdone[i]:
                all_ended = 0
        r = float(np.sqrt(np.float64(tot)))
    j = st.n_his
    if j < st.his_cap:
        st.r_his[j] = r
    st.n_his = j + 1
    st.r_prev, st.r_last = st.r_last, r
    st.sumsq = tot
    if all_ended or st.status != 0:
        st.done = 1
    return st


def restore(u, zsave, rows, rptr, mdone, k):
    """k_union_restore: the rows of every ended member get zsave back; returns the new block"""
    u = np.array(u, dtype=np.float64).reshape(-1, k)
    zsave = np.asarray(zsave).reshape(-1, k)
    for i in range(len(rptr) - 1):
        if mdone[i]:
            ri = rows[rptr[i]:rptr[i + 1]]
            u[ri] = zsave[ri]
    return u


def blockdiag_exact(blocks, mrow0, b, u):
    """u + (member's block) b_i per row: every dot product correctly rounded (exact_dot), then one addition.  blocks[i]: lda_i x lda_i, of
    which the leading n_i x n_i part multiplies.  Also returns sum |a| |b| per entry, what the rounding bound scales with."""
    b, u = np.asarray(b, dtype=np.float64), np.asarray(u, dtype=np.float64)
    out, mag = u.copy(), np.zeros_like(u)
    for i, Ai in enumerate(blocks):
        r0, r1 = mrow0[i], mrow0[i + 1]
        ni = r1 - r0
        for row in range(ni):
            for c in range(b.shape[1]):
                out[r0 + row, c] = u[r0 + row, c] + exact_dot(Ai[row, :ni], b[r0:r1, c])
                mag[r0 + row, c] = math.fsum(np.abs(Ai[row, :ni]) * np.abs(b[r0:r1, c]))
    return out, mag


class UnionLoop:
    """The loop of a union solve: per step the residual vector, member_sumsq and decide (zsave <- u happens in the same launch), a cycle on the
    WHOLE block, then restore.  resid(z) -> the residual block, cycle(z) -> the block after one V-cycle; rows_of_member[i]: member i's rows."""

    def __init__(self, resid, cycle, rows_of_member, tol, max_iter):
        self.resid, self.cycle, self.tol, self.max_iter = resid, cycle, tol, max_iter
        self.members = [np.asarray(r, dtype=np.int64) for r in rows_of_member]
        self.rows = np.concatenate(self.members)
        self.rptr = np.concatenate([[0], np.cumsum([len(r) for r in self.members])]).astype(np.int64)

    def run(self, z0, stops=None):
        """stops: None -- the break tests decide from resid; or per member (iteration, code) / None: the member ends at that iteration with
        mdone = code, as a run elsewhere decided (resid is then not called and the histories are not formed).  Returns a dict: zs (z_0 ... ,
        z_j the iterate whose residual is history entry j), z (the last of them), st (UnionState), stop (per member: iteration or None)."""
        z = np.array(z0, dtype=np.float64)
        if z.ndim == 1:
            z = z[:, None]
        k, m = z.shape[1], len(self.members)
        st = UnionState(m, max(self.max_iter, 1))
        zs, stop = [z.copy()], [None] * m
        zsave = np.zeros_like(z)
        for it in range(self.max_iter):
            before = st.mdone.copy()
            zsave[self.rows] = z[self.rows]                                        # k_union_sumsq, every member, ended or not
            if stops is None:
                r = self.resid(z)
                decide(st, [member_sumsq(r, ri, k) for ri in self.members], self.tol)
            else:
                for i in range(m):
                    if not st.mdone[i]:
                        st.nhis[i] += 1
                        if stops[i] is not None and stops[i][0] == it:
                            st.mdone[i] = stops[i][1]
                st.n_his += 1
                st.done = int(all(st.mdone))
            for i in range(m):
                if st.mdone[i] and not before[i]:
                    stop[i] = it
            if st.done:
                break
            z = restore(self.cycle(z), zsave, self.rows, self.rptr, st.mdone, k)
            zs.append(z.copy())
        return dict(zs=zs, z=z, st=st, stop=stop)


def tol_is_clear_of_the_histories(histories, tol):
    """the condition of every comparison of stop iterations: no member's last two residuals lie within 1e-3 relative of tol, so a history that
    differs in the last bits stops at the same entry"""
    return all(abs(r - tol) > 1e-3 * tol for rh in histories for r in rh[-2:])


def _split(x):
    c = (2.0 ** 27 + 1.0) * x
    hi = c - (c - x)
    return hi, x - hi


def residual_twofold(A, B, z):
    """B - A z as an unevaluated sum hi + lo of two float64 blocks (error-free products, compensated additions): good to about 2^-100 of
    |B| + |A||z| per entry, so that norms taken from it are the correctly rounded ones for every purpose of a bound in units of 2^-53.  Also
    returns |B| + |A||z| and the longest row.  A: scipy CSR, B and z: n x k."""
    A = A.tocsr()
    n, k = B.shape
    lens = np.diff(A.indptr)
    W = int(lens.max()) if n else 0
    col, val = np.zeros((n, W), np.int64), np.zeros((n, W))
    slot = np.arange(A.nnz) - np.repeat(A.indptr[:-1], lens)
    row = np.repeat(np.arange(n), lens)
    col[row, slot], val[row, slot] = A.indices, A.data
    zh, zl = _split(np.asarray(z, dtype=np.float64))
    hi, lo, mag = np.array(B, dtype=np.float64), np.zeros((n, k)), np.abs(B)
    for s in range(W):
        a = -val[:, s][:, None]
        ah, al = _split(a)
        c = col[:, s]
        x = z[c]
        p = a * x
        e = ((ah * zh[c] - p) + ah * zl[c] + al * zh[c]) + al * zl[c]        # a x = p + e exactly
        t = hi + p
        bb = t - hi
        lo = lo + ((hi - (t - bb)) + (p - bb)) + e                           # hi + p = t + (that) exactly
        hi = t + lo
        lo = lo - (hi - t)
        mag = mag + np.abs(p)
    return hi, lo, mag, W


def norm_twofold(hi, lo):
    """the 2-norm of hi + lo, rounded once at the end"""
    hi, lo = np.ravel(hi), np.ravel(lo)
    h1, h2 = _split(hi)
    return math.sqrt(math.fsum(np.concatenate([h1 * h1, 2.0 * (h1 * h2), h2 * h2, 2.0 * (hi * lo), lo * lo])))


# ---- hand-written cases of the break test: the CPU lane holds decide() to the expected values, the GPU lane holds k_union_decide to decide().
# ss: what k_union_sumsq left; tol; the state before (defaults: nobody ended, empty histories, cap 4, status 0); expect: the state after --
# his: {(member, entry): value} names every history entry that changes.
NAN, INF = float("nan"), float("inf")
_SQ70 = [float((i + 1) ** 2) for i in range(70)]
DECIDE_CASES = [
    dict(name="r_equals_tol_does_not_stop", ss=[0.25], tol=0.5,
         expect=dict(mdone=[0], nhis=[1], done=0, n_his=1, sumsq=0.25, his={(0, 0): 0.5})),
    dict(name="r_below_tol_stops", ss=[0.25, 1.0], tol=0.5000000000000001,
         expect=dict(mdone=[1, 0], nhis=[1, 1], done=0, n_his=1, sumsq=1.25, his={(0, 0): 0.5, (1, 0): 1.0})),
    dict(name="one_member_below_tol_ends_the_handle", ss=[0.0625], tol=0.5,
         expect=dict(mdone=[1], nhis=[1], done=1, n_his=1, sumsq=0.0625, his={(0, 0): 0.25})),
    dict(name="nan_fails_that_member_only", ss=[NAN, 4.0], tol=0.5,
         expect=dict(mdone=[2, 0], nhis=[1, 1], done=0, n_his=1, sumsq=4.0, his={(0, 0): NAN, (1, 0): 2.0})),
    dict(name="inf_fails_that_member_only", ss=[9.0, INF, 0.0625], tol=0.5,
         expect=dict(mdone=[0, 2, 1], nhis=[1, 1, 1], done=0, n_his=1, sumsq=9.0625, his={(0, 0): 3.0, (1, 0): INF, (2, 0): 0.25})),
    dict(name="ended_members_record_nothing", ss=[9.0, NAN, 16.0], tol=0.5, mdone=[1, 2, 0], nhis=[3, 1, 2],
         expect=dict(mdone=[1, 2, 0], nhis=[3, 1, 3], done=0, n_his=1, sumsq=25.0, his={(2, 2): 4.0})),
    dict(name="nhis_at_the_cap", ss=[1.0, 4.0, 9.0], tol=0.5, nhis=[3, 4, 5],
         expect=dict(mdone=[0, 0, 0], nhis=[4, 5, 6], done=0, n_his=1, sumsq=14.0, his={(0, 3): 1.0})),
    dict(name="status_ends_the_handle", ss=[4.0, 4.0], tol=0.5, status=-1,
         expect=dict(mdone=[0, 0], nhis=[1, 1], done=1, n_his=1, sumsq=8.0, his={(0, 0): 2.0, (1, 0): 2.0})),
    dict(name="all_ended", ss=[1.0, 4.0, 4.0], tol=0.5, mdone=[1, 2, 1], nhis=[2, 1, 3], n_his=3, his_cap=4, r_last=7.0,
         expect=dict(mdone=[1, 2, 1], nhis=[2, 1, 3], done=1, n_his=4, sumsq=5.0, his={}, r_prev=7.0)),
    dict(name="handle_history_at_its_cap", ss=[4.0], tol=0.5, n_his=2, his_cap=2,
         expect=dict(mdone=[0], nhis=[1], done=0, n_his=3, sumsq=4.0, his={(0, 0): 2.0})),
    dict(name="done_on_entry_changes_nothing", ss=[0.0625, NAN], tol=0.5, done=1, n_his=1,
         expect=dict(mdone=[0, 0], nhis=[0, 0], done=1, n_his=1, his={})),
    dict(name="seventy_members", ss=_SQ70, tol=35.0,
         expect=dict(mdone=[1] * 34 + [0] * 36, nhis=[1] * 70, done=0, n_his=1, sumsq=116795.0, his={(i, 0): float(i + 1) for i in range(70)})),
]


def state_of_case(case, fill=None):
    """the UnionState a case starts from; fill: what the histories hold before (default zeros; the GPU lane passes sentinels)"""
    m, cap = len(case["ss"]), case.get("cap", 4)
    his_cap = case.get("his_cap", cap)
    his = np.zeros((m, cap)) if fill is None else fill((m, cap))
    r_his = np.zeros(his_cap) if fill is None else fill(his_cap)
    return UnionState(m, cap, his_cap=his_cap, done=case.get("done", 0), status=case.get("status", 0), n_his=case.get("n_his", 0),
                      r_last=case.get("r_last", -1.0), mdone=case.get("mdone"), nhis=case.get("nhis"), his=his, r_his=r_his)
