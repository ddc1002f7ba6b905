"""The radix-4 pass kernels with plane-major exchanges and consumer-side first-layer twiddles (csrc/ntt_kernels4.hip.h:
the first and single passes of even S), bit for bit against the C oracle.

Single passes: 2^4 is the smallest shape with an exchange (and, alone, too small for a wave-uniform step 1: it takes the
per-lane twiddles on the new exchange); 2^6, 2^8 and 2^10 are the first shapes with exchanges 1, 2 and 3, 2^10 the first
single pass whose step-1 digit is a wave's; 2^5 and 2^9 end in a radix-2 step and keep the Stockham exchange.  Multi-pass
(the first pass on the new exchange, handing its u-fast output to middle and last passes on the Stockham one):
2^12 with radix at most 2^6 in tiles of 2^10 and 2^11 (the <6, 4> kernels, the edge of the wave condition, and <6, 5>),
2^16 in tiles of 2^10 and 2^11 (the <8, 2> kernels of the 2^24 transform and <8, 3>), 2^16 with radix at most 2^6 (a
middle pass), 2^20 with the <10, 1> kernels of the headline and with the <10, 0> and <10, 2> tiles: every shape of even
S the library instantiates.  The reference of an input is computed once and shared."""
import numpy as np
import pytest

from oracle import bigint_oracle as B
from oracle.cpu_oracle import COSET, INVERSE, ints_to_limbs

ALL_FLAGS = [0, INVERSE, COSET, INVERSE | COSET]
SINGLE = [4, 5, 6, 8, 9, 10]
# (log_n, ntt_tile_log, ntt_max_radix)
MULTI = [(12, 10, 6), (12, 11, 6), (16, 0, 10), (16, 11, 10), (16, 0, 6), (20, 0, 10), (20, 10, 10), (20, 12, 10)]
KINDS = ["zero", "delta_first", "delta_last", "all_r_minus_1", "random", "ragged", "batch_of_2", "round_trip"]

_REF = {}


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
        a = oracle.fr_sample(0x706D + k, n)
    return a


def _ref(oracle, key, a, k, flags):
    """the oracle's transform of the input named by key, computed once for all plans of a size"""
    key = (k, flags) + key
    if key not in _REF:
        _REF[key] = oracle.fr_ntt(a, k, flags, 8)
        _REF[key].setflags(write=False)
    return _REF[key]


def _check_kind(ctx, oracle, k, kind):
    n = 1 << k
    a = _input(oracle, "random" if kind in ("ragged", "batch_of_2", "round_trip") else kind, k)
    if kind == "ragged":                                      # in_len < n: zero padding is part of the transform
        for in_len in sorted({1, n // 4 + 1, n - 1}):
            for flags in (0, COSET):
                assert np.array_equal(ctx.fr_ntt(a[:in_len], k, flags), _ref(oracle, ("ragged", in_len), a[:in_len], k, flags)), (k, in_len, flags)
    elif kind == "batch_of_2":
        two = np.stack([a, oracle.fr_sample(0xB2 + k, n)])
        for flags in ALL_FLAGS:
            got = ctx.fr_ntt_batch(two, k, flags)
            assert np.array_equal(got[0], _ref(oracle, ("random",), two[0], k, flags)), (k, flags, 0)
            assert np.array_equal(got[1], _ref(oracle, ("second",), two[1], k, flags)), (k, flags, 1)
    elif kind == "round_trip":
        f = ctx.fr_ntt(a, k, 0)
        assert np.array_equal(f, _ref(oracle, ("random",), a, k, 0))
        assert np.array_equal(ctx.fr_ntt(f, k, INVERSE), a)
        cf = ctx.fr_ntt(a, k, COSET)
        assert np.array_equal(ctx.fr_ntt(cf, k, INVERSE | COSET), a)
    else:
        for flags in ALL_FLAGS:
            assert np.array_equal(ctx.fr_ntt(a, k, flags), _ref(oracle, (kind,), a, k, flags)), (k, kind, flags)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("k", SINGLE)
def test_single_passes(ctx, oracle, k, kind):
    _check_kind(ctx, oracle, k, kind)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("k,tile,maxr", MULTI)
def test_multi_pass_plans(ctx, oracle, k, tile, maxr, kind):
    ctx.set_option("ntt_tile_log", tile)
    ctx.set_option("ntt_max_radix", maxr)
    try:
        _check_kind(ctx, oracle, k, kind)
    finally:
        ctx.set_option("ntt_tile_log", 0)
        ctx.set_option("ntt_max_radix", 10)


def test_the_plans_reach_the_kernels_named_above():
    """CPU: what the plan dispatches (the library's pure-host plan hook)"""
    import ctypes as C

    from plonk_prototype_amd import _lib

    def plan(log_n, tile_log=0, max_radix=0):
        out = (C.c_uint32 * 20)()
        assert _lib.load().pm_test_ntt_plan(log_n, 1, tile_log, max_radix, 4, 0, out) == 0
        v = list(out)
        return [(v[1 + 4 * i], v[2 + 4 * i]) for i in range(v[0])]

    assert [plan(k) for k in SINGLE] == [[(k, 0)] for k in SINGLE]
    assert plan(12, 10, 6) == [(6, 4), (6, 4)] and plan(12, 11, 6) == [(6, 5), (6, 5)]
    assert plan(16) == [(8, 2), (8, 2)] and plan(16, 11, 10) == [(8, 3), (8, 3)] and plan(24) == [(8, 2)] * 3
    assert len(plan(16, 0, 6)) == 3 and plan(16, 0, 6)[0] == (6, 4)
    assert plan(20) == [(10, 1), (10, 1)] and plan(20, 10, 10) == [(10, 0), (10, 0)] and plan(20, 12, 10) == [(10, 2), (10, 2)]
