"""The radix-4 pass kernels with the first-layer step twiddles applied by their producer (L1_UNIFORM in
csrc/ntt_kernels4.hip.h), bit for bit against the C oracle, at the boundaries of the predicate.

The predicate holds for a pass of radix 2^S with 2^LT columns per tile when the pass reads the wide form (a middle or
last pass), has a second radix-4 step (S >= 4) and a wave's 64 >> LT values of u fit an aligned block of
U/4 = 2^(S-4): S + LT >= 10.  Every multi-pass tile has 2^10 .. 2^12 elements, so every middle and last pass the plan
dispatches takes the new path, and no first or single pass does.  Sizes: 3 .. 10 single passes (none takes it; 3, 5, 9
end in a radix-2 step; 2^10 is the one shape that meets the wave condition and fails only the role), 11 and 12 two passes
of unequal / small radix (11: S = 6, then S = 5 with a radix-2 last step on the new path), 16 and 18 (S = 8, 8 and 9, 9:
radix-2 last step on the new path), 20 the two <10, 1> passes of the headline (first: old path, last: new); ntt_max_radix
6 gives three passes -- a middle one -- at 2^16 and 2^18, ntt_tile_log 12 and 10 the <10, 2> and <10, 0> tiles at 2^20,
ntt_tile_log 10 with ntt_max_radix 6 the smallest tiles (S + LT = 10, the edge of the wave condition)."""
import ctypes as C

import numpy as np
import pytest

from oracle import bigint_oracle as B
from oracle.cpu_oracle import COSET, INVERSE, ints_to_limbs

ALL_FLAGS = [0, INVERSE, COSET, INVERSE | COSET]
SIZES = [3, 4, 5, 6, 8, 9, 10, 11, 12, 16, 18, 20]
KINDS = ["zero", "delta_first", "delta_last", "all_r_minus_1", "random", "ragged", "batch_of_2", "round_trip"]
# (log_n, ntt_tile_log, ntt_max_radix): plans the defaults do not reach
OPTION_PLANS = [(16, 0, 6), (18, 0, 6), (20, 12, 10), (20, 10, 10), (12, 10, 6)]


def l1_uniform(S, LT, in_wide=True):
    return in_wide and S >= 4 and (64 >> LT) <= ((1 << S) >> 4)


def _plan(log_n, tile_log=0, max_radix=0):
    from plonk_prototype_amd import _lib
    out = (C.c_uint32 * 20)()
    assert _lib.load().pm_test_ntt_plan(log_n, 1, tile_log, max_radix, 4, 0, out) == 0
    v = list(out)
    return [(v[1 + 4 * i], v[2 + 4 * i]) for i in range(v[0])]


def test_the_sizes_cover_the_predicate():
    """CPU: what the plan dispatches for the sizes below (the library's pure-host plan hook)."""
    import plonk_prototype_amd as pa
    plans = {k: _plan(k) for k in SIZES}
    for k in SIZES:
        assert [s for s, _ in plans[k]] == pa.ntt_plan(k)
    assert all(len(plans[k]) == 1 and plans[k][0][1] == 0 for k in SIZES if k <= 10)
    assert not l1_uniform(*plans[9][0]) and l1_uniform(*plans[10][0])           # the wave condition: just below, just above
    assert not any(l1_uniform(*plans[k][0]) for k in SIZES if k < 10)
    assert not any(l1_uniform(*plans[k][0], in_wide=False) for k in SIZES)      # no first or single pass takes the path
    assert all(l1_uniform(S, LT) for k in SIZES if k > 10 for S, LT in plans[k][1:])    # every later pass does
    assert plans[20] == [(10, 1), (10, 1)]                                     # the headline: <10, 1> first and last
    assert [s for s, _ in plans[11]] == [6, 5] and [s for s, _ in plans[18]] == [9, 9]      # radix-2 last steps
    assert {s % 2 for k in (3, 5, 9) for s, _ in plans[k]} == {1}
    assert len(_plan(16, 0, 6)) == 3 and len(_plan(18, 0, 6)) == 3             # a middle pass at a small size
    assert all(l1_uniform(S, LT) for S, LT in _plan(16, 0, 6)[1:] + _plan(18, 0, 6)[1:])
    assert _plan(20, 12, 10) == [(10, 2), (10, 2)] and _plan(20, 10, 10) == [(10, 0), (10, 0)]
    assert all(S + LT == 10 and l1_uniform(S, LT) for S, LT in _plan(12, 10, 6))    # the smallest tile: the predicate's edge


def _element(oracle, v):
    return oracle.fr_to_mont(ints_to_limbs([v], 4))


def _input(oracle, kind, k):
    n = 1 << k
    a = np.zeros((n, 4), np.uint64)
    if kind == "delta_first":
        a[0] = _element(oracle, 1)[0]
    elif kind == "delta_last":
        a[n - 1] = _element(oracle, 1)[0]
    elif kind == "all_r_minus_1":
        a[:] = _element(oracle, B.R_MOD - 1)[0]
    elif kind != "zero":
        a = oracle.fr_sample(0x4C31 + k, n)
    return a


def _check_kind(ctx, oracle, k, kind):
    n = 1 << k
    a = _input(oracle, kind, k)
    if kind == "ragged":                                      # in_len < n: zero padding is part of the transform
        for in_len in sorted({1, n // 4 + 1, n - 1}):
            for flags in (0, COSET):
                assert np.array_equal(ctx.fr_ntt(a[:in_len], k, flags), oracle.fr_ntt(a[:in_len], k, flags, 8)), (k, in_len, flags)
    elif kind == "batch_of_2":
        two = np.stack([a, oracle.fr_sample(0xB2 + k, n)])
        for flags in ALL_FLAGS:
            got = ctx.fr_ntt_batch(two, k, flags)
            for b in range(2):
                assert np.array_equal(got[b], oracle.fr_ntt(two[b], k, flags, 8)), (k, flags, b)
    elif kind == "round_trip":
        f = ctx.fr_ntt(a, k, 0)
        assert np.array_equal(f, oracle.fr_ntt(a, k, 0, 8))
        assert np.array_equal(ctx.fr_ntt(f, k, INVERSE), a)
        cf = ctx.fr_ntt(a, k, COSET)
        assert np.array_equal(ctx.fr_ntt(cf, k, INVERSE | COSET), a)
    else:
        for flags in ALL_FLAGS:
            assert np.array_equal(ctx.fr_ntt(a, k, flags), oracle.fr_ntt(a, k, flags, 8)), (k, kind, flags)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("k", SIZES)
def test_default_plans(ctx, oracle, k, kind):
    _check_kind(ctx, oracle, k, kind)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["all_r_minus_1", "random", "ragged", "batch_of_2", "round_trip"])
@pytest.mark.parametrize("k,tile,maxr", OPTION_PLANS)
def test_option_plans(ctx, oracle, k, tile, maxr, kind):
    """three passes (a middle one) at 2^16 and 2^18, the <10, 2> and <10, 0> tiles, the smallest tile"""
    ctx.set_option("ntt_tile_log", tile)
    ctx.set_option("ntt_max_radix", maxr)
    try:
        _check_kind(ctx, oracle, k, kind)
    finally:
        ctx.set_option("ntt_tile_log", 0)
        ctx.set_option("ntt_max_radix", 10)
