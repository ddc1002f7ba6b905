"""Inter-pass twiddles applied by the producing pass (option ntt_tw_producer, csrc/ntt_kernels4.hip.h: PASS_TW_OUT /
PASS_TW_APPLIED), bit for bit against the C oracle and against the same call with ntt_tw_producer = 0.

The producers are the first passes of radix 2^10 (step4_tw_producer), so the cases that run the new code are PRODUCERS:
2^19 (10 + 9: the consumer ends in a radix-2 step) and 2^20 (10 + 10) with the default tiles, the <10, 1> kernels of the
headline, and 2^20 in tiles of 2^10 and 2^12 elements, the <10, 0> and <10, 2> kernels.  SHAPES are the smallest multi-pass
transforms of each kind -- 2^11 (6 + 5), 2^12 (6 + 6), 2^16 (8 + 8, the kernels of the 2^24 transform) and 2^15 in three
passes (ntt_max_radix = 6, the smallest the option takes, gives 5 + 5 + 5).  For them the option selects nothing and every
pass multiplies its own inputs; the cases stay, so that a shape that becomes a producer is covered the day it does.

Every case runs forward, inverse (n^-1 is in the last pass's table, so its producer applies it), coset, coset-inverse,
in_len < n and a batch of three with strides longer than the vectors, with ntt_xcd 1 and 0, each with the option on and
off.  The reference of an input is computed once and shared by all cases of its size."""
import numpy as np
import pytest

from oracle.cpu_oracle import COSET, INVERSE

ALL_FLAGS = [0, INVERSE, COSET, INVERSE | COSET]
# (log_n, ntt_max_radix, ntt_tile_log)
SHAPES = [(11, 10, 0), (12, 10, 0), (16, 10, 0), (15, 6, 0)]
PRODUCERS = [(19, 10, 0), (20, 10, 0), (20, 10, 10), (20, 10, 12)]

_REF = {}


def _ref(oracle, name, a, k, flags):
    key = (name, k, flags, a.shape[0])
    if key not in _REF:
        _REF[key] = oracle.fr_ntt(a, k, flags, 8)
        _REF[key].setflags(write=False)
    return _REF[key]


def _both(ctx, call):
    """the result of call() with the producer-side products and with the consumer-side ones"""
    ctx.set_option("ntt_tw_producer", 1)
    on = call()
    ctx.set_option("ntt_tw_producer", 0)
    try:
        off = call()
    finally:
        ctx.set_option("ntt_tw_producer", 1)
    return on, off


def _batch_dev(ctx, vecs, in_len, k, flags, pad_in, pad_out):
    """three vectors in one call through the device ABI, strides in_len + pad_in and n + pad_out"""
    import torch
    n = 1 << k
    src = np.zeros((len(vecs), in_len + pad_in, 4), np.uint64)
    for i, v in enumerate(vecs):
        src[i, :in_len] = v[:in_len]
    d_in = torch.from_numpy(src.view(np.int64)).cuda()
    d_out = torch.full((len(vecs), n + pad_out, 4), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ctx.fr_ntt_dev(d_in.data_ptr(), in_len, d_out.data_ptr(), k, flags, batch=len(vecs), in_stride=in_len + pad_in,
                   out_stride=n + pad_out)
    ctx.sync()
    out = d_out.cpu().numpy().view(np.uint64)
    assert bool((out[:, n:] == np.uint64(0xFFFFFFFFFFFFFFFF)).all())             # the padding is not written
    return out[:, :n]


def _check_size(ctx, oracle, k):
    """every case with the option on and off; against the oracle all of them up to 2^16, above that a part (the whole
    vector with every flag, one in_len, two vectors of the batch): a reference of 2^20 points takes a fraction of a second"""
    n = 1 << k
    big = k > 16
    a = oracle.fr_sample(0x7477 + k, n)
    for flags in ALL_FLAGS:
        on, off = _both(ctx, lambda: ctx.fr_ntt(a, k, flags))
        assert np.array_equal(on, off), (k, flags)
        assert np.array_equal(on, _ref(oracle, "a", a, k, flags)), (k, flags)
    for in_len in (1, n // 4 + 1, n - 1):                                         # zero padding is part of the transform
        for flags in (0, COSET):
            on, off = _both(ctx, lambda: ctx.fr_ntt(a[:in_len], k, flags))
            assert np.array_equal(on, off), (k, in_len, flags)
            if not big or in_len == n // 4 + 1:
                assert np.array_equal(on, _ref(oracle, "a", a[:in_len], k, flags)), (k, in_len, flags)
    vecs = [a, oracle.fr_sample(0xB3 + k, n), oracle.fr_sample(0xB4 + k, n)]
    for flags in ALL_FLAGS:
        on, off = _both(ctx, lambda: _batch_dev(ctx, vecs, n, k, flags, 3, 5))
        assert np.array_equal(on, off), (k, flags)
        for i, name in enumerate("abc"):
            if not big or i == 0 or (i == 1 and flags in (0, INVERSE | COSET)):
                assert np.array_equal(on[i], _ref(oracle, name, vecs[i], k, flags)), (k, flags, i)
    in_len = n // 2 + 3
    on, off = _both(ctx, lambda: _batch_dev(ctx, vecs, in_len, k, COSET, 7, 1))
    assert np.array_equal(on, off), k
    for i, name in enumerate("abc"):
        if not big or i == 2:
            assert np.array_equal(on[i], _ref(oracle, name, vecs[i][:in_len], k, COSET)), (k, i)


@pytest.mark.gpu
@pytest.mark.parametrize("xcd", [1, 0])
@pytest.mark.parametrize("k,maxr,tile", SHAPES + PRODUCERS)
def test_producer_side_twiddles(ctx, oracle, k, maxr, tile, xcd):
    ctx.set_option("ntt_max_radix", maxr)
    ctx.set_option("ntt_tile_log", tile)
    ctx.set_option("ntt_xcd", xcd)
    try:
        _check_size(ctx, oracle, k)
    finally:
        ctx.set_option("ntt_max_radix", 10)
        ctx.set_option("ntt_tile_log", 0)
        ctx.set_option("ntt_xcd", 1)
        ctx.set_option("ntt_tw_producer", 1)


def test_the_plans_named_above():
    """CPU: what the plan dispatches (the library's pure-host plan hook)"""
    import ctypes as C

    from plonk_prototype_amd import _lib

    def plan(log_n, max_radix=0):
        out = (C.c_uint32 * 20)()
        assert _lib.load().pm_test_ntt_plan(log_n, 1, 0, max_radix, 4, 0, out) == 0
        v = list(out)
        return [v[1 + 4 * i] for i in range(v[0])]

    assert plan(11) == [6, 5] and plan(12) == [6, 6] and plan(16) == [8, 8] and plan(19) == [10, 9] and plan(20) == [10, 10]
    assert plan(15, 6) == [5, 5, 5]
