"""GPU (-m gpu): the block kernels of the LOBPCG eigensolver (csrc/smg_eig_device.hip) one at a time, through the handle-free hooks of
include/smg.h (smg_debug_eig_gram, smg_debug_eig_combine, smg_debug_eig_residual).

Two kinds of reference, both independent of the order in which a kernel sums, so they hold for any correct rewrite (MFMA, other chunks):
  - exact: small integers (and powers of two), so every product and partial sum is exact in fp64 and a correct kernel returns numpy's
    integer result bit for bit -- a lost, doubled or misplaced row or column fails loudly;
  - real data: |dev - ref| <= 2 gamma_N (|Sa|^T |w| |Sb|) entry by entry, the rigorous bound of any summation order of N terms (gamma_N of
    tests/kernel_hooks.py) for both the kernel and the fp64 reference.
Elementwise results are compared bitwise with numpy's unfused expression (the library is built with -ffp-contract=off).  The shapes are the
edges of the tiles (64 x 64 Gram tiles, 16-column combine chunks, 256 / m row lanes) and of the row chunks (eig_groups: 1024 rows a chunk, at
most 256 chunks)."""
import numpy as np
import pytest

from kernel_hooks import combine, eig_groups, gamma, gram, residual, sentinel
from test_gpu_parity import smg  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

MS = [1, 3, 8, 12, 16, 21, 22, 32, 48, 63, 64]
NS = [31, 32, 33, 1023, 1024, 1025, 2049]
BIG_N = 256 * 1024 + 1000          # past the chunk cap: 256 chunks of 1028 rows, the last one 1004


@pytest.fixture(scope="module")
def L(smg):
    return smg._lib.load()


def ints(rng, shape, lo=-8, hi=8):
    return rng.integers(lo, hi + 1, size=shape).astype(np.float64)


def gram_ref(Sa, Sb, w=None):
    """exact for integer data: the product in int64"""
    A = np.concatenate(list(Sa), axis=1).astype(np.int64)
    B = np.concatenate(list(Sb), axis=1).astype(np.int64)
    if w is not None:
        A = A * w.astype(np.int64)[:, None]
    return (A.T @ B).astype(np.float64)


def gram_bound_check(G, Sa, Sb, w):
    A, B = np.concatenate(list(Sa), axis=1), np.concatenate(list(Sb), axis=1)
    wv = np.ones(A.shape[0]) if w is None else w
    ref = (A * wv[:, None]).T @ B
    bound = 2 * gamma(A.shape[0] + 2) * ((np.abs(A) * np.abs(wv)[:, None]).T @ np.abs(B))
    err = np.abs(G - ref)
    assert np.all(err <= bound), (err.max(), np.unravel_index(np.argmax(err - bound), err.shape))


# ---- Gram: G = Sa^T diag(w) Sb ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m", MS)
def test_gram_exact_integer(L, m):
    rng = np.random.default_rng(m)
    for n in sorted(set([m] + NS)):
        for nb_a, nb_b in [(1, 1), (2, 2), (3, 3), (1, 3), (3, 2)]:
            Sa, Sb, w = ints(rng, (nb_a, n, m)), ints(rng, (nb_b, n, m)), ints(rng, n)
            for ww in (None, w):
                G = gram(L, Sa, Sb, ww, G=sentinel((nb_a * m, nb_b * m)))
                assert np.array_equal(G, gram_ref(Sa, Sb, ww)), (n, nb_a, nb_b, ww is None)
            Gs = gram(L, Sa, w=w, sym=True, G=sentinel((nb_a * m, nb_a * m)))
            assert np.array_equal(Gs, gram_ref(Sa, Sa, w)), (n, nb_a, "sym")


@pytest.mark.parametrize("m", [1, 3])
def test_gram_exact_past_the_chunk_cap(L, m):
    rng = np.random.default_rng(10 + m)
    n = BIG_N
    assert eig_groups(n) == 256 and -(-n // 256) > 1024 and n % -(-n // 256) != 0
    for nb in (1, 3):
        Sa, Sb, w = ints(rng, (nb, n, m)), ints(rng, (nb, n, m)), ints(rng, n)
        assert np.array_equal(gram(L, Sa, Sb, w), gram_ref(Sa, Sb, w))
        assert np.array_equal(gram(L, Sa, w=w, sym=True), gram_ref(Sa, Sa, w))


@pytest.mark.parametrize("m", [1, 8, 21, 22, 64])
def test_gram_real_data_within_bound_and_symmetric(L, m):
    rng = np.random.default_rng(20 + m)
    for n in (33, 1025, 2049):
        for nb in (1, 2, 3):
            Sa = rng.standard_normal((nb, n, m)) * 10.0 ** rng.uniform(-3, 3, (nb, 1, m))
            Sb = rng.standard_normal((1, n, m))
            mass = 10.0 ** rng.uniform(-8, 3, n)            # the range of a lumped mass on a graded mesh
            for w in (None, mass):
                gram_bound_check(gram(L, Sa, Sb, w), Sa, Sb, w)
                G = gram(L, Sa, Sa, w)
                Gs = gram(L, Sa, w=w, sym=True)
                assert np.array_equal(Gs, Gs.T)
                gram_bound_check(Gs, Sa, Sa, w)
                gram_bound_check(G, Sa, Sa, w)


def test_gram_small_n_against_correctly_rounded_sums(L):
    """n = 5: the entries against math.fsum of exact product splits (the correctly rounded result), within 2 gamma_n of |Sa|^T |Sb|"""
    from kernel_hooks import exact_dot
    rng = np.random.default_rng(3)
    n, m = 5, 22
    S = rng.standard_normal((3, n, m))
    G = gram(L, S, sym=True)
    A = np.concatenate(list(S), axis=1)
    absb = np.abs(A).T @ np.abs(A)
    for i in range(A.shape[1]):
        for j in range(A.shape[1]):
            assert abs(G[i, j] - exact_dot(A[:, i], A[:, j])) <= gamma(n + 1) * absb[i, j]


@pytest.mark.parametrize("m,nb,n", [(8, 1, 100), (22, 3, 1025), (64, 3, 2049), (3, 2, 40)])
def test_gram_nan_stays_in_its_row_and_column(L, m, nb, n):
    """smg_eigs' SMG_ERR_NONFINITE needs NaN to reach G -- and only where it belongs: a padding slot that computed 0 x NaN would spread it"""
    rng = np.random.default_rng(m + n)
    S = rng.standard_normal((nb, n, m))
    w = 10.0 ** rng.uniform(-2, 2, n)
    q = nb * m
    for c in sorted({0, m - 1, q - 1, q // 2}):
        for row in (0, n - 1):
            T = S.copy()
            T[c // m, row, c % m] = np.nan
            for G in (gram(L, T, w=w, sym=True), gram(L, T, T, w)):
                nan = np.isnan(G)
                assert nan[c, :].all() and nan[:, c].all()
                nan[c, :] = nan[:, c] = False
                assert not nan.any(), (c, row, np.argwhere(nan)[:4])
            # non-symmetric, NaN in Sa only: row c of G and nowhere else
            G = gram(L, T, S[:1], w)
            nan = np.isnan(G)
            assert nan[c, :].all() and nan.sum() == m


def test_gram_done_leaves_output(L):
    rng = np.random.default_rng(4)
    for m, nb, n in [(22, 3, 2049), (64, 3, 1025), (1, 1, 31)]:
        S = rng.standard_normal((nb, n, m))
        G0 = sentinel((nb * m, nb * m))
        for sym in (False, True):
            G = gram(L, S, None if sym else S, sym=sym, done=1, G=G0)
            assert G.tobytes() == G0.tobytes()


def test_gram_deterministic(L):
    rng = np.random.default_rng(5)
    n, m = BIG_N, 2
    S = rng.standard_normal((3, n, m))
    w = 10.0 ** rng.uniform(-8, 3, n)
    a = gram(L, S, w=w, sym=True)
    b = gram(L, S, w=w, sym=True)
    assert a.tobytes() == b.tobytes()
    S = rng.standard_normal((3, 2049, 64))
    a, b = gram(L, S, S[:1]), gram(L, S, S[:1])
    assert a.tobytes() == b.tobytes()


# ---- combine: X = S Cx, AX = AS Cx, P = S' Cp, AP = AS' Cp ---------------------------------------------------------------------------------

def combine_ref(S, AS, Cm):
    nb, n, m = S.shape
    Si = np.concatenate(list(S), axis=1).astype(np.int64)
    ASi = np.concatenate(list(AS), axis=1).astype(np.int64)
    Ci = Cm.astype(np.int64)
    Cp = Ci[:, m:].copy()
    Cp[:m] = 0                     # S' leaves out block 0
    f = lambda a: a.astype(np.float64)
    return f(Si @ Ci[:, :m]), f(ASi @ Ci[:, :m]), f(Si @ Cp), f(ASi @ Cp)


@pytest.mark.parametrize("m", MS + [17])
def test_combine_exact_integer(L, m):
    rng = np.random.default_rng(100 + m)
    for n in sorted(set([m, 31, 33, 1025, 2049])):
        for nb in (1, 2, 3):
            S, AS, Cm = ints(rng, (nb, n, m)), ints(rng, (nb, n, m)), ints(rng, (nb * m, 2 * m))
            Cm[:m, m:] = np.nan    # the Cp rows of block 0 are never read
            ref = combine_ref(S, AS, np.nan_to_num(Cm))
            outs = [sentinel((n, m)) for _ in range(4)]
            X, AX, P, AP = combine(L, S, AS, Cm, make_p=True, outs=outs)
            for got, want in zip((X, AX, P, AP), ref):
                assert np.array_equal(got, want), (n, nb)
            X2, AX2, P2, AP2 = combine(L, S, AS, Cm, make_p=False, outs=outs)
            assert np.array_equal(X2, ref[0]) and np.array_equal(AX2, ref[1])


def test_combine_exact_past_the_chunk_cap(L):
    rng = np.random.default_rng(7)
    n, m = BIG_N, 3
    S, AS, Cm = ints(rng, (3, n, m)), ints(rng, (3, n, m)), ints(rng, (3 * m, 2 * m))
    for got, want in zip(combine(L, S, AS, Cm), combine_ref(S, AS, Cm)):
        assert np.array_equal(got, want)


@pytest.mark.parametrize("m", [5, 17, 48, 64])
def test_combine_real_data_within_bound(L, m):
    rng = np.random.default_rng(200 + m)
    n, nb = 1025, 3
    S = rng.standard_normal((nb, n, m)) * 10.0 ** rng.uniform(-4, 4, (nb, 1, m))
    AS = rng.standard_normal((nb, n, m))
    Cm = rng.standard_normal((nb * m, 2 * m))
    X, AX, P, AP = combine(L, S, AS, Cm)
    Sc, ASc = np.concatenate(list(S), axis=1), np.concatenate(list(AS), axis=1)
    Cp = Cm[:, m:].copy()
    Cp[:m] = 0.0
    N = nb * m + 1
    for got, A, Cc in ((X, Sc, Cm[:, :m]), (AX, ASc, Cm[:, :m]), (P, Sc, Cp), (AP, ASc, Cp)):
        assert np.all(np.abs(got - A @ Cc) <= 2 * gamma(N) * (np.abs(A) @ np.abs(Cc)))


def test_combine_done_leaves_outputs(L):
    rng = np.random.default_rng(8)
    n, m, nb = 1025, 22, 3
    S, AS, Cm = rng.standard_normal((nb, n, m)), rng.standard_normal((nb, n, m)), rng.standard_normal((nb * m, 2 * m))
    outs = [sentinel((n, m)) for _ in range(4)]
    for make_p in (True, False):
        for got, o in zip(combine(L, S, AS, Cm, make_p=make_p, done=1, outs=outs), outs):
            assert got.tobytes() == o.tobytes()


def test_combine_deterministic(L):
    rng = np.random.default_rng(9)
    n, m, nb = 2049, 64, 3
    S, AS, Cm = rng.standard_normal((nb, n, m)), rng.standard_normal((nb, n, m)), rng.standard_normal((nb * m, 2 * m))
    for a, b in zip(combine(L, S, AS, Cm), combine(L, S, AS, Cm)):
        assert a.tobytes() == b.tobytes()


# ---- residual: R = AX - diag(mass) X diag(lam), res_c = sqrt(sum r^2 / mass) / |lam_c|, the preconditioner's input ---------------------------

RES_MS = [1, 3, 5, 7, 12, 48, 63, 64]


def exact_residual_data(rng, n, m):
    """integers and powers of two: R, r^2 / mass and every partial sum are exact"""
    X, AX = ints(rng, (n, m)), ints(rng, (n, m))
    mass = 2.0 ** rng.integers(-2, 3, n)
    lam = ints(rng, m, 1, 8) * rng.choice([-1.0, 1.0], m)
    return X, AX, mass, lam


@pytest.mark.parametrize("m", RES_MS)
def test_residual_exact(L, m):
    rng = np.random.default_rng(300 + m)
    for n in sorted(set([m, 31, 33, 1023, 1025, 2049])):
        X, AX, mass, lam = exact_residual_data(rng, n, m)
        R = AX - (mass[:, None] * X) * lam[None, :]
        s = np.sum(R * R / mass[:, None], axis=0)              # exact: integers and their quarters, far below 2^53
        want_res = np.sqrt(s) / np.abs(lam)
        b0, u0, b32, u32, res = residual(L, X, AX, mass, lam)
        assert np.array_equal(b0, R) and np.all(u0 == 0.0) and not np.signbit(u0).any()
        assert np.array_equal(res, want_res), (n, res, want_res)
        outs = [sentinel((n, m)), sentinel((n, m)), sentinel((n, m), np.float32), sentinel((n, m), np.float32), sentinel(m)]
        b0f, u0f, b32, u32, res32 = residual(L, X, AX, mass, lam, f32=True, outs=outs)
        assert b0f.tobytes() == outs[0].tobytes() and u0f.tobytes() == outs[1].tobytes()      # f32: the fp64 input is left alone
        assert np.array_equal(b32, R.astype(np.float32)) and np.all(u32 == 0.0) and not np.signbit(u32).any()
        assert np.array_equal(res32, want_res)


def test_residual_exact_past_the_chunk_cap(L):
    rng = np.random.default_rng(11)
    n, m = BIG_N, 3
    X, AX, mass, lam = exact_residual_data(rng, n, m)
    R = AX - (mass[:, None] * X) * lam[None, :]
    b0, u0, b32, u32, res = residual(L, X, AX, mass, lam)
    assert np.array_equal(b0, R)
    assert np.array_equal(res, np.sqrt(np.sum(R * R / mass[:, None], axis=0)) / np.abs(lam))


@pytest.mark.parametrize("m", RES_MS)
def test_residual_real_data_bitwise_and_within_bound(L, m):
    rng = np.random.default_rng(400 + m)
    n = 2049
    X = rng.standard_normal((n, m))
    AX = rng.standard_normal((n, m)) * 10.0 ** rng.uniform(-3, 3, (1, m))
    mass = 10.0 ** rng.uniform(-8, 3, n)
    lam = rng.uniform(0.1, 10.0, m) * rng.choice([-1.0, 1.0], m)
    R = AX - (mass[:, None] * X) * lam[None, :]
    b0, u0, b32, u32, res = residual(L, X, AX, mass, lam)
    assert np.array_equal(b0, R)
    t = R * R / mass[:, None]
    # every term carries two roundings, the sum any order's gamma_n; sqrt halves the relative error, sqrt and / add one rounding each
    s_ref = np.sum(t, axis=0)
    rel = np.abs(res - np.sqrt(s_ref) / np.abs(lam)) / (np.sqrt(s_ref) / np.abs(lam))
    assert np.all(rel <= (gamma(n + 2) + 4 * 2.0 ** -53) * 1.01), rel.max()
    _, _, b32, _, _ = residual(L, X, AX, mass, lam, f32=True)
    assert np.array_equal(b32, R.astype(np.float32))


def test_residual_float_overflow_and_subnormals(L):
    """(float) R as numpy's astype gives it: beyond float's range -> +-inf, in float's subnormal range -> the subnormal, below it -> +-0"""
    n, m = 64, 5
    vals = np.array([1e39, -1e39, 3.5e38, 3.4028235677973366e38, 1e-39, -1e-39, 1.4e-45, 7e-46, 1e-46, -1e-300, 1.1754942e-38, 1.0, 0.0, -0.0])
    AX = np.resize(vals, (n, m)).astype(np.float64)
    X = np.zeros((n, m))
    mass, lam = np.ones(n), np.ones(m)
    _, _, b32, u32, _ = residual(L, X, AX, mass, lam, f32=True)
    with np.errstate(over="ignore"):
        want = AX.astype(np.float32)
    assert b32.tobytes() == want.tobytes()
    assert (np.abs(want) == np.inf).any() and ((want != 0) & (np.abs(want) < np.finfo(np.float32).tiny)).any()


def test_residual_done_leaves_outputs(L):
    rng = np.random.default_rng(12)
    n, m = 1025, 7
    X, AX, mass, lam = exact_residual_data(rng, n, m)
    outs = [sentinel((n, m)), sentinel((n, m)), sentinel((n, m), np.float32), sentinel((n, m), np.float32), sentinel(m)]
    for f32 in (False, True):
        for got, o in zip(residual(L, X, AX, mass, lam, f32=f32, done=1, outs=outs), outs):
            assert got.tobytes() == o.tobytes()


def test_residual_deterministic(L):
    rng = np.random.default_rng(13)
    n, m = BIG_N, 7
    X, AX = rng.standard_normal((n, m)), rng.standard_normal((n, m))
    mass, lam = 10.0 ** rng.uniform(-8, 3, n), rng.uniform(0.1, 10.0, m)
    a, b = residual(L, X, AX, mass, lam), residual(L, X, AX, mass, lam)
    assert a[4].tobytes() == b[4].tobytes() and a[0].tobytes() == b[0].tobytes()
