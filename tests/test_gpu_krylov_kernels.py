"""GPU (-m gpu): the vector kernels of the V-cycle-preconditioned conjugate gradient solve (csrc/smg_krylov_device.hip) one launcher at a time,
through the handle-free hook smg_debug_krylov of include/smg.h.

References as in tests/test_gpu_eig_kernels.py: small integers make every column sum exact, so a correct kernel returns numpy's integer result
bit for bit whatever order it sums in; real data is held to the rigorous bound 2 gamma_N of any summation order; elementwise updates and the
scalar recurrences are compared bitwise with numpy's unfused expressions (-ffp-contract=off).  The widths are the edges of the reduction
launches: one and two 64-column groups (blockIdx.y), k <= 1024 and k > 1024 (the two summation paths of the |r|^2 finalize); the row counts
are the steps of kry_groups (8 rows a thread) and past its cap of 512 chunks."""
import numpy as np
import pytest

from kernel_hooks import KS_ALPHA, KS_BETA, KS_RZ, KS_RZ_PREV, KRY_MAX_GROUPS, gamma, krylov, kry_groups, sentinel
from test_gpu_parity import smg  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

KS = [1, 2, 3, 5, 8, 63, 64, 65, 100, 128, 1024, 1025, 1100]


@pytest.fixture(scope="module")
def L(smg):
    return smg._lib.load()


def ints(rng, shape, lo=-8, hi=8):
    return rng.integers(lo, hi + 1, size=shape).astype(np.float64)


def row_counts(k):
    """1 row, the kry_groups steps (8 rows per thread of a chunk), and past the chunk cap where the block stays small"""
    rpc = 8 * (256 // min(k, 64))
    ns = [1, 7, rpc - 1, rpc, rpc + 1, 3 * rpc + 5]
    if k <= 128:
        ns.append(KRY_MAX_GROUPS * rpc + 37)
    return sorted(set(ns))


def slots(rng, k):
    s = np.empty((4, k))
    s[KS_RZ] = rng.uniform(0.5, 2.0, k)
    s[KS_RZ_PREV] = rng.uniform(0.5, 2.0, k) * rng.choice([-1.0, 1.0], k)
    s[KS_ALPHA] = rng.uniform(-2.0, 2.0, k)
    s[KS_BETA] = rng.uniform(-2.0, 2.0, k)
    return s


def colsum(a, b):
    """exact column sums of integer blocks"""
    return np.sum(a.astype(np.int64) * b.astype(np.int64), axis=0).astype(np.float64)


def test_row_counts_cover_the_cap():
    for k in KS:
        ns = row_counts(k)
        assert any(kry_groups(n, k) == 2 for n in ns) and kry_groups(ns[1], k) == 1
        if k <= 128:
            assert kry_groups(ns[-1], k) == KRY_MAX_GROUPS and kry_groups(ns[-2], k) < KRY_MAX_GROUPS


@pytest.mark.parametrize("k", KS)
def test_dots_and_scalars_exact(L, k):
    """z.r, z.q -> rz, beta; p.q -> alpha, rz_prev; x += alpha p, r -= alpha q and |r|^2 -> the history: exact integer data"""
    rng = np.random.default_rng(k)
    for n in row_counts(k):
        z, r, q, p, x = (ints(rng, (n, k)) for _ in range(5))
        # ---- zr_zq
        s = slots(rng, k)
        s[KS_RZ_PREV, ::3] = 0.0                              # rz_prev == 0: beta = 0
        (z1, r1, q1), s1, rs, ctrl = krylov(L, "zr_zq", [z, r, q], s=s, restart=0)
        assert np.array_equal(z1, z) and np.array_equal(r1, r) and np.array_equal(q1, q)
        rz, zq = colsum(z, r), colsum(z, q)
        with np.errstate(divide="ignore", invalid="ignore"):
            beta = np.where(s[KS_RZ_PREV] == 0.0, 0.0, -s[KS_ALPHA] * zq / s[KS_RZ_PREV])
        assert np.array_equal(s1[KS_RZ], rz), n
        assert s1[KS_BETA].tobytes() == beta.tobytes(), n
        assert np.array_equal(s1[[KS_RZ_PREV, KS_ALPHA]], s[[KS_RZ_PREV, KS_ALPHA]]) and rs == 0
        assert ctrl == dict(sumsq=-1.0, r0=-1.0, n_his=0, done=0, status=0)
        # after a restart beta is 0 whatever rz_prev is, and the flag is cleared
        _, s2, rs, _ = krylov(L, "zr_zq", [z, r, q], s=s, restart=1)
        assert rs == 0 and np.array_equal(s2[KS_RZ], rz)
        assert np.all(s2[KS_BETA] == 0.0) and not np.signbit(s2[KS_BETA]).any()
        # ---- pq
        q2 = q.copy()
        q2[:, ::4] = 0.0                                      # p.q == 0: alpha = 0
        (p1, q3), s3, _, _ = krylov(L, "pq", [p, q2], s=s, restart=1)
        assert np.array_equal(p1, p) and np.array_equal(q3, q2)
        pq = colsum(p, q2)
        with np.errstate(divide="ignore", invalid="ignore"):
            alpha = np.where(pq == 0.0, 0.0, s[KS_RZ] / pq)
        assert s3[KS_ALPHA].tobytes() == alpha.tobytes(), n
        assert s3[KS_RZ_PREV].tobytes() == s[KS_RZ].tobytes()
        assert np.array_equal(s3[[KS_RZ, KS_BETA]], s[[KS_RZ, KS_BETA]])
        # ---- step + decide, integer alpha: every value exact
        s4 = s.copy()
        s4[KS_ALPHA] = rng.integers(-2, 3, k)
        (x1, r1, p1, q1), s5, _, ctrl = krylov(L, "step", [x, r, p, q], s=s4, tol=0.0)
        xn, rn = x + s4[KS_ALPHA] * p, r - s4[KS_ALPHA] * q
        assert np.array_equal(x1, xn) and np.array_equal(r1, rn) and np.array_equal(p1, p) and np.array_equal(q1, q)
        sumsq = float(np.sum(colsum(rn, rn)))
        assert ctrl["sumsq"] == sumsq and ctrl["r0"] == np.sqrt(sumsq), (n, ctrl, sumsq)
        assert ctrl["n_his"] == 1 and ctrl["done"] == 0 and ctrl["status"] == 0
        assert np.array_equal(s5, s4)


@pytest.mark.parametrize("k", [1, 3, 64, 65, 1024, 1100])
def test_dots_real_data_within_bound_and_deterministic(L, k):
    rng = np.random.default_rng(50 + k)
    n = row_counts(k)[-1] if k <= 128 else 97
    z = rng.standard_normal((n, k)) * 10.0 ** rng.uniform(-6, 6, (1, k))
    r, q, p, x = (rng.standard_normal((n, k)) for _ in range(4))
    s = slots(rng, k)
    N = n + 2
    runs = [krylov(L, "zr_zq", [z, r, q], s=s, restart=0)[1] for _ in range(2)]
    assert runs[0].tobytes() == runs[1].tobytes()
    rz = np.sum(z * r, axis=0)
    assert np.all(np.abs(runs[0][KS_RZ] - rz) <= 2 * gamma(N) * np.sum(np.abs(z * r), axis=0))
    runs = [krylov(L, "pq", [p, q], s=s)[1] for _ in range(2)]
    assert runs[0].tobytes() == runs[1].tobytes()
    pq = np.sum(p * q, axis=0)
    bound = 2 * gamma(N) * np.sum(np.abs(p * q), axis=0)
    alpha = runs[0][KS_ALPHA]
    assert np.all(np.abs(s[KS_RZ] / alpha - pq) <= bound + 4 * 2.0 ** -53 * np.abs(pq))
    runs = [krylov(L, "step", [x, r, p, q], s=s) for _ in range(2)]
    assert runs[0][3] == runs[1][3] and runs[0][0][1].tobytes() == runs[1][0][1].tobytes()
    rn = r - s[KS_ALPHA] * q
    assert np.array_equal(runs[0][0][1], rn) and np.array_equal(runs[0][0][0], x + s[KS_ALPHA] * p)
    ss = np.sum(rn * rn)
    assert abs(runs[0][3]["sumsq"] - ss) <= 2 * gamma(n + k + 2) * ss
    assert runs[0][3]["r0"] == np.sqrt(runs[0][3]["sumsq"])


@pytest.mark.parametrize("k", [1, 5, 64, 65, 1100])
def test_direction_bitwise(L, k):
    rng = np.random.default_rng(60 + k)
    for n in (1, 33, 1001):
        z, p = rng.standard_normal((n, k)), rng.standard_normal((n, k))
        s = slots(rng, k)
        s[KS_BETA, ::2] = 0.0
        p[:, ::2] = np.where(rng.random((n, (k + 1) // 2)) < 0.5, np.nan, np.inf)     # never read where beta == 0
        (z1, p1), s1, _, ctrl = krylov(L, "direction", [z, p], s=s)
        with np.errstate(invalid="ignore"):
            want = np.where(s[KS_BETA] == 0.0, z, z + s[KS_BETA] * p)
        assert p1.tobytes() == want.tobytes() and np.array_equal(z1, z) and np.array_equal(s1, s)
        assert np.isfinite(p1[:, ::2]).all()


@pytest.mark.parametrize("k", [1, 3, 64, 1025])
def test_precond_in_and_widen_bitwise(L, k):
    rng = np.random.default_rng(70 + k)
    n = 517
    r = rng.standard_normal((n, k)) * 10.0 ** rng.uniform(-300, 300, (n, k))
    (r1, b0, u0), _, _, _ = krylov(L, "precond_in", [r, sentinel((n, k)), sentinel((n, k))])
    assert r1.tobytes() == r.tobytes() and b0.tobytes() == r.tobytes() and np.all(u0 == 0.0) and not np.signbit(u0).any()
    e = (rng.standard_normal((n, k)) * 10.0 ** rng.uniform(-44, 38, (n, k))).astype(np.float32)
    e.flat[:6] = [np.inf, -np.inf, 1e-45, -1e-45, np.finfo(np.float32).max, 0.0]
    (z,), _, _, _ = krylov(L, "widen", [sentinel((n, k))], e=e)
    assert z.tobytes() == e.astype(np.float64).tobytes()


def test_break_test_and_nonfinite(L):
    rng = np.random.default_rng(80)
    n, k = 300, 3
    x, r, p, q = (ints(rng, (n, k)) for _ in range(4))
    s = slots(rng, k)
    s[KS_ALPHA] = [1.0, -2.0, 0.0]
    rn = r - s[KS_ALPHA] * q
    r0 = np.sqrt(float(np.sum(colsum(rn, rn))))
    for tol, done in ((np.nextafter(r0, np.inf), 1), (r0, 0), (r0 / 2, 0)):     # r < tol ends the loop
        ctrl = krylov(L, "step", [x, r, p, q], s=s, tol=tol)[3]
        assert ctrl["r0"] == r0 and ctrl["done"] == done and ctrl["status"] == 0 and ctrl["n_his"] == 1, (tol, ctrl)
    for bad in (np.nan, np.inf):
        q2 = q.copy()
        q2[n // 2, 1] = bad
        ctrl = krylov(L, "step", [x, r, p, q2], s=s, tol=1e300)[3]
        assert ctrl["status"] == -1 and ctrl["done"] == 1 and ctrl["n_his"] == 1 and not np.isfinite(ctrl["r0"])


@pytest.mark.parametrize("k", [1, 65, 1100])
def test_done_leaves_every_output(L, k):
    rng = np.random.default_rng(90 + k)
    n = 200
    s = slots(rng, k)
    vec = lambda: sentinel((n, k))
    stopped = dict(sumsq=-1.0, r0=-1.0, n_his=0, done=1, status=0)
    for op, nv in (("zr_zq", 3), ("direction", 2), ("pq", 2), ("step", 4), ("precond_in", 3), ("widen", 1)):
        vecs = [rng.standard_normal((n, k)) for _ in range(nv - 1)] + [vec()]
        e = rng.standard_normal((n, k)).astype(np.float32) if op == "widen" else None
        out, s1, rs, ctrl = krylov(L, op, vecs, s=None if op in ("precond_in", "widen") else s, restart=1, e=e, tol=1e300, done=1)
        for a, b in zip(out, vecs):
            assert a.tobytes() == b.tobytes(), op
        assert s1 is None or s1.tobytes() == s.tobytes()
        assert rs == 1 and ctrl == stopped, (op, ctrl)
