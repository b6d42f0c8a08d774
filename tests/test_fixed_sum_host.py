"""CPU: the fixed-order reduction under every energy, stopping test and CFL rate (csrc/smg_fixed_sum_device.hip: launch_fixed_sum,
launch_fixed_max) -- the numpy restatement pd_np.fixed_sum that every GPU test trusts, held to a second restatement written the other way
round: plain Python scalar loops that follow the two kernels lane by lane (one accumulator per lane, the halving tree entry by entry, the
shuffle tree lane by lane), so pd_np.fixed_sum does not certify itself.  Also the chunk-count formula against the constants of the .hip
file, and the refusals of the test hook smg_debug_fixed_reduce without a GPU.  tests/test_gpu_fixed_sum.py holds the device to the same
lengths."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import pd_np as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, NO_DEVICE = -1, -2
EPS = N.EPS
# every length at which the two kernels take another path: around a wave, around a block, the last lengths with one chunk, two unequal chunks
# (rows per chunk 1 025, then 1 024 rows), three chunks with a short last one, 64 and 65 chunks (the final kernel's second pass), 1 024 chunks
# of 2 048, and the capped range where rows per chunk stops being 2 048: 2 049 (last chunk 1 026 rows) and one that is no multiple of 256
LENGTHS = [1, 2, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4097, 131072, 131073, 2097152, 2097153, 3000001]


def hip_constants():
    """(threads per block, rows per thread that size a chunk, the cap on chunks) read from the .hip file"""
    txt = open(os.path.join(ROOT, "surface_multigrid_code_amd", "csrc", "smg_fixed_sum_device.hip")).read()
    threads = int(re.search(r"constexpr int SUM_THREADS = (\d+);", txt).group(1))
    cap = int(re.search(r"constexpr int SUM_MAX_GROUPS = (\d+);", txt).group(1))
    per_thread = int(re.search(r"\(long\)SUM_THREADS \* (\d+) - 1\) / \(\(long\)SUM_THREADS \* (\d+)\)", txt).group(1))
    return threads, per_thread, cap


def groups_formula(n):
    threads, per_thread, cap = hip_constants()
    want = (n + threads * per_thread - 1) // (threads * per_thread)
    return max(1, min(want, cap))


def sum_terms(n, seed=0):
    """standard_normal x 10^uniform(-8, 8): mixed signs and sixteen decades, so another order of summation gives other bits"""
    rng = np.random.default_rng([seed, n])
    return rng.standard_normal(n) * 10.0 ** rng.uniform(-8, 8, n)


def _fmax(a, b):
    """fmax: a NaN loses against a number (equal values: either)"""
    if a != a:
        return b
    if b != b:
        return a
    return a if a >= b else b


def fixed_reduce_loops(term, maximum=False):
    """k_fixed_sum_part and k_fixed_sum_final in Python scalars, lane by lane; returns (the result, the chunk results)"""
    t = np.asarray(term, dtype=np.float64).tolist()
    n = len(t)
    threads, _, _ = hip_constants()
    comb = _fmax if maximum else (lambda a, b: a + b)
    ident = -math.inf if maximum else 0.0
    groups = groups_formula(n)
    rpc = (n + groups - 1) // groups
    part = []
    for g in range(groups):                                        # one block per chunk
        r0 = g * rpc
        r1 = min(n, r0 + rpc)
        red = []
        for lane in range(threads):                                # for (r = r0 + lane; r < r1; r += SUM_THREADS)
            acc = ident
            for x in t[r0 + lane:r1:threads]:
                acc = comb(acc, x)
            red.append(acc)
        half = threads // 2
        while half > 0:                                            # the halving tree in shared memory
            for lane in range(half):
                red[lane] = comb(red[lane], red[lane + half])
            half >>= 1
        part.append(red[0])
    v = []
    for lane in range(64):                                         # one wave: for (g = lane; g < groups; g += 64)
        acc = ident
        for x in part[lane::64]:
            acc = comb(acc, x)
        v.append(acc)
    o = 32
    while o > 0:                                                   # __shfl_down(v, o, 64): a lane whose partner is past the wave reads itself
        v = [comb(v[lane], v[lane + o] if lane + o < 64 else v[lane]) for lane in range(64)]
        o >>= 1
    return v[0], part


def bits(x):
    return np.float64(x).view(np.uint64)


def test_groups_formula():
    threads, per_thread, cap = hip_constants()
    assert (threads, per_thread, cap) == (256, 8, 1024)
    q = threads * per_thread
    edges = [1, 2, q - 1, q, q + 1, 2 * q, 2 * q + 1, 64 * q, 64 * q + 1, cap * q - 1, cap * q, cap * q + 1, 2 ** 31 - 1]
    for n in sorted(set(LENGTHS + edges)):
        assert N.fixed_sum_groups(n) == groups_formula(n), n
    for n, g in ((2048, 1), (2049, 2), (4097, 3), (131072, 64), (131073, 65), (2097152, 1024), (2097153, 1024), (3000001, 1024)):
        assert N.fixed_sum_groups(n) == g
    # no chunk is ever empty: with c chunks and q = ceil(n / c) rows each, the last chunk starts below n
    for n in LENGTHS:
        c = groups_formula(n)
        assert (c - 1) * ((n + c - 1) // c) < n


@pytest.mark.parametrize("n", LENGTHS)
def test_restatement_against_the_kernel_text_in_scalar_loops(n):
    t = sum_terms(n)
    got = N.fixed_sum(t)
    want, part = fixed_reduce_loops(t)
    assert len(part) == N.fixed_sum_groups(n)
    assert bits(got) == bits(want), (n, got, want)
    bound = 2 * n * EPS * math.fsum(np.abs(t))
    print("n = %d: |fixed_sum - fsum| = %.3e (bound %.3e)" % (n, abs(got - math.fsum(t)), bound))
    assert abs(got - math.fsum(t)) <= bound
    if 64 <= n <= 131073:                                           # the order matters on these terms: the plain left-to-right sum has other bits
        assert any(bits(N.fixed_sum(sum_terms(n, s))) != bits(float(np.cumsum(sum_terms(n, s))[-1])) for s in range(4))


@pytest.mark.parametrize("n", [1, 2, 65, 257, 2049, 4097, 131073])
def test_scalar_loops_of_the_maximum(n):
    """the same loops with fmax and the identity -inf: the maximum of negative data, a NaN loses against a number, n NaNs give -inf"""
    rng = np.random.default_rng(n)
    t = -rng.uniform(1.0, 2.0, n) * 10.0 ** rng.uniform(-8, 8, n)
    assert fixed_reduce_loops(t, True)[0] == np.max(t) < 0.0
    t[rng.random(n) < 0.3] = np.nan
    t[rng.integers(n)] = -3.0
    assert fixed_reduce_loops(t, True)[0] == np.nanmax(t)
    assert fixed_reduce_loops(np.full(n, np.nan), True)[0] == -math.inf


def _call(L, op, n, term, out, groups=True, bad=True):
    dp = C.POINTER(C.c_double)
    g, b = C.c_int(-1), C.c_int(-1)
    return L.smg_debug_fixed_reduce(op, n, None if term is None else term.ctypes.data_as(dp), None if out is None else out.ctypes.data_as(dp),
                                    C.byref(g) if groups else None, C.byref(b) if bad else None)


def test_hook_refusals(smg_mod):
    L = smg_mod._lib.load()
    assert hasattr(L, "smg_debug_fixed_reduce")
    t, out = np.ones(5), np.zeros(1)
    for op in (-1, 2):
        assert _call(L, op, 5, t, out) == INVALID                                       # unknown op
    for op in (0, 1):
        assert _call(L, op, 0, t, out) == INVALID and _call(L, op, -4, t, out) == INVALID   # n <= 0
        assert _call(L, op, 5, None, out) == INVALID and _call(L, op, 5, t, None) == INVALID
        assert b"smg_debug_fixed_reduce" in L.smg_last_error()
    assert out[0] == 0.0
    if L.smg_device_count() == 0:
        for op in (0, 1):
            assert _call(L, op, 5, t, out) == NO_DEVICE
            assert _call(L, op, 5, t, out, groups=False, bad=False) == NO_DEVICE          # the two counters are optional
        assert "no CPU fallback" in L.smg_last_error().decode()
