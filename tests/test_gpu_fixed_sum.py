"""GPU (-m gpu): launch_fixed_sum / launch_fixed_max (csrc/smg_fixed_sum_device.hip) at lengths of the test's choosing, through
smg_debug_fixed_reduce (kernel_hooks.fixed_reduce: the chunk scratch holds exactly the launched chunk count, the result one double, both
between guards).

The sum is held bit for bit to pd_np.fixed_sum, which tests/test_fixed_sum_host.py holds to the kernel text in scalar loops; the maximum to
numpy.max on negative data with the largest entry where a chunk, a stride or a lane could drop it, and to the documented rule that a NaN
loses against a number."""
import numpy as np
import pytest

import kernel_hooks as K
import pd_np as N
from test_fixed_sum_host import LENGTHS, bits, sum_terms
from test_gpu_parity import smg  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n", LENGTHS)
def test_sum_is_the_restatement_bit_for_bit(smg, n):
    L = smg._lib.load()
    t = sum_terms(n)
    want = N.fixed_sum(t)
    got, groups = K.fixed_reduce(L, "SUM", t)
    print("n = %d: %d chunks of %d rows, sum %.17g, restatement %.17g" % (n, groups, (n + groups - 1) // groups, got, want))
    assert groups == N.fixed_sum_groups(n)
    assert bits(got) == bits(want), (got, want)
    again, _ = K.fixed_reduce(L, "SUM", t)
    assert bits(again) == bits(got)


def max_positions(n):
    """where the largest entry is placed: the first and the last entry, the last row of chunk 0 and the first of chunk 1 (rows per chunk is
    no multiple of 256 once it is not 2 048: the chunk's last, partial stride), the last row of the short last chunk, and chunks past the
    final kernel's first pass (64, the last one)"""
    g = N.fixed_sum_groups(n)
    rpc = (n + g - 1) // g
    pos = {0, n - 1, min(rpc, n) - 1, min(rpc, n - 1), (g - 1) * rpc, n // 2}
    if g > 64:
        pos |= {64 * rpc, min(64 * rpc + rpc - 1, n - 1), min((g - 1) * rpc + 255, n - 1)}
    return sorted(pos)


@pytest.mark.parametrize("n", LENGTHS)
def test_max_of_negative_data(smg, n):
    """every entry is negative -- a tree that starts from 0 returns 0 -- and the largest sits in turn at each place of max_positions"""
    L = smg._lib.load()
    rng = np.random.default_rng([1, n])
    base = -rng.uniform(1.0, 2.0, n) * 10.0 ** rng.uniform(-8, 8, n)
    got, groups = K.fixed_reduce(L, "MAX", base)
    assert groups == N.fixed_sum_groups(n)
    assert bits(got) == bits(np.max(base)) and got < 0.0
    for p in max_positions(n):
        t = base.copy()
        t[p] = -1.25e-9                                                             # above every other entry (those are <= -1e-8)
        got, _ = K.fixed_reduce(L, "MAX", t)
        assert bits(got) == bits(np.max(t)) and got == -1.25e-9, (n, p, got)
    again, _ = K.fixed_reduce(L, "MAX", t)
    assert bits(again) == bits(got)


@pytest.mark.parametrize("n", LENGTHS)
def test_max_lets_a_nan_lose_against_a_number(smg, n):
    L = smg._lib.load()
    rng = np.random.default_rng([2, n])
    t = -rng.uniform(1.0, 2.0, n) * 10.0 ** rng.uniform(-8, 8, n)
    nan = rng.random(n) < 0.3
    nan[:min(n, 300):7] = True                                                      # lanes whose first term is a NaN, and one whole ...
    if n > 4096:
        nan[2048:4096] = True                                                       # ... stretch longer than a chunk
    nan[rng.integers(n)] = False
    t[nan] = np.nan
    got, _ = K.fixed_reduce(L, "MAX", t)
    assert bits(got) == bits(np.nanmax(t)) and got < 0.0                             # the numbers' maximum
    for p in sorted({0, n - 1, int(np.nonzero(~nan)[0][0])}):
        u = t.copy()
        u[p] = np.inf
        assert K.fixed_reduce(L, "MAX", u)[0] == np.inf                             # +inf wins
    assert K.fixed_reduce(L, "MAX", np.full(n, -np.inf))[0] == -np.inf              # all -inf
    assert K.fixed_reduce(L, "MAX", np.full(n, np.nan))[0] == -np.inf               # all NaN: the identity
