"""Fixed-shape kernels of the plain 2^20 transform (csrc/ntt_kernels4.hip.h: ntt_pass4_fixed_kernel, option ntt_fixed_shape).
The two <10, 1> passes of a plain 2^20 transform take kernels with the geometry and the flags compiled in; every other launch
keeps the generic kernel.  The option is 1 by default (the first pass, which measured faster), 2 takes the last pass's
fixed kernel too, 0 none.  A fixed kernel computes what the generic one computes, instruction for instruction in the arithmetic,
so with the option at 2, 1 and 0 a call must give the same bytes, and those of the CPU oracle; pm_test_ntt_last_variants says
which kernels the call's passes took.

    plain forward, inverse, round trip                         2: fixed, fixed; 1: fixed, generic; 0: generic, generic
    a batch of two; two strided vectors in place (device)      the same: the batch only moves the uniform base
    in_len 2^18, coset forward / inverse, ntt_tw_producer 0,
    ntt_step_prio 0, 2^19, 2^21                                generic, whatever the option says
    edge inputs through the fixed kernels                      zeros, all r - 1, one 1 at index 0 / n - 1; the exit's vote
                                                               (fe_reduce_canon_pack) without a voter, with every lane voting
                                                               and with a few lanes voting

2^20 is the smallest size that reaches these kernels.  The oracle's transforms are computed once each and shared."""
import ctypes as C

import numpy as np
import pytest

from oracle import bigint_oracle as B
from oracle.cpu_oracle import COSET, INVERSE, ints_to_limbs

K = 20
N = 1 << K
GENERIC, FIXED = 1, 2
SEED = 0x46495853

_cache = {}


def _once(key, make):
    if key not in _cache:
        v = make()
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
        _cache[key] = v
    return _cache[key]


def _sample(oracle, tag, n=N):
    return _once(("in", tag, n), lambda: oracle.fr_sample(SEED + tag, n))


def _ref(oracle, key, a, k, flags):
    return _once(("ref", key, k, flags), lambda: oracle.fr_ntt(a, k, flags))


def _variants(ctx):
    out = (C.c_uint32 * 4)()
    ctx._check(ctx._lib.pm_test_ntt_last_variants(ctx._h, out))
    return list(out)


def _with(ctx, options, call):
    """call() under the options, which go back to the library's defaults"""
    defaults = {"ntt_fixed_shape": 1, "ntt_tw_producer": 1, "ntt_step_prio": 1}
    for key, v in options.items():
        ctx.set_option(key, v)
    try:
        out = call()
        return out, _variants(ctx)
    finally:
        for key in options:
            ctx.set_option(key, defaults[key])


def _both_paths(ctx, call, fixed, passes=2, options=None):
    """the call with ntt_fixed_shape 2, 1 and 0: same bytes, and the kernels its passes took -- with `fixed` both fixed
    kernels under 2 and the first pass's under 1, without it the generic ones whatever the option says"""
    got2, v2 = _with(ctx, {**(options or {}), "ntt_fixed_shape": 2}, call)
    got1, v1 = _with(ctx, {**(options or {}), "ntt_fixed_shape": 1}, call)
    got0, v0 = _with(ctx, {**(options or {}), "ntt_fixed_shape": 0}, call)
    generic = [GENERIC] * passes + [0] * (4 - passes)
    assert v2 == ([FIXED, FIXED, 0, 0] if fixed else generic), v2
    assert v1 == ([FIXED, GENERIC, 0, 0] if fixed else generic), v1
    assert v0 == generic, v0
    assert np.array_equal(got2, got0) and np.array_equal(got1, got0)
    return got2


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [0, INVERSE])
def test_plain_transforms(ctx, oracle, flags):
    a = _sample(oracle, 0)
    got = _both_paths(ctx, lambda: ctx.fr_ntt(a, K, flags), True)
    assert np.array_equal(got, _ref(oracle, "a", a, K, flags))


@pytest.mark.gpu
def test_round_trip(ctx, oracle):
    a = _sample(oracle, 0)
    got = _both_paths(ctx, lambda: ctx.fr_ntt(ctx.fr_ntt(a, K, 0), K, INVERSE), True)
    assert np.array_equal(got, a)


@pytest.mark.gpu
def test_batch_of_two(ctx, oracle):
    a = np.stack([_sample(oracle, 0), _sample(oracle, 1)])
    got = _both_paths(ctx, lambda: ctx.fr_ntt_batch(a, K, 0), True)
    assert np.array_equal(got[0], _ref(oracle, "a", a[0], K, 0))
    assert np.array_equal(got[1], _ref(oracle, "b", a[1], K, 0))


@pytest.mark.gpu
def test_two_strided_vectors_in_place_on_the_device(ctx, oracle):
    """pm_fr_ntt_dev: batch 2, in_stride = out_stride = n + 3 elements, input and output the same buffer; the elements
    between and behind the vectors stay as they were"""
    import torch

    stride = N + 3
    host = np.full((2 * stride, 4), 0xA5A5A5A5A5A5A5A5, np.uint64)
    host[:N] = _sample(oracle, 0)
    host[stride:stride + N] = _sample(oracle, 1)

    def call():
        buf = torch.from_numpy(host.view(np.int64).copy()).cuda()
        torch.cuda.synchronize()
        ctx.fr_ntt_dev(buf.data_ptr(), N, buf.data_ptr(), K, 0, batch=2, in_stride=stride, out_stride=stride)
        ctx.sync()
        return buf.cpu().numpy().view(np.uint64)

    got = _both_paths(ctx, call, True)
    assert np.array_equal(got[:N], _ref(oracle, "a", host[:N], K, 0))
    assert np.array_equal(got[stride:stride + N], _ref(oracle, "b", host[stride:stride + N], K, 0))
    assert np.array_equal(got[N:stride], host[N:stride]) and np.array_equal(got[stride + N:], host[stride + N:])


@pytest.mark.gpu
@pytest.mark.parametrize("what", ["padding", "coset", "coset_inverse", "tw_producer_0", "step_prio_0", "2^19", "2^21"])
def test_calls_that_keep_the_generic_kernels(ctx, oracle, what):
    a = _sample(oracle, 0)
    k, passes, options = K, 2, {}
    if what == "padding":
        call, ref = (lambda: ctx.fr_ntt(a[: N >> 2], K, 0)), lambda: _ref(oracle, "a/4", a[: N >> 2], K, 0)
    elif what == "coset":
        call, ref = (lambda: ctx.fr_ntt(a, K, COSET)), lambda: _ref(oracle, "a", a, K, COSET)
    elif what == "coset_inverse":
        call, ref = (lambda: ctx.fr_ntt(a, K, INVERSE | COSET)), lambda: _ref(oracle, "a", a, K, INVERSE | COSET)
    elif what in ("tw_producer_0", "step_prio_0"):
        options = {"ntt_" + what[:-2]: 0}
        call, ref = (lambda: ctx.fr_ntt(a, K, 0)), lambda: _ref(oracle, "a", a, K, 0)
    else:
        k = int(what[2:])
        passes = 2 if k == 19 else 3
        s = a[: 1 << k] if k < K else _sample(oracle, 2, 1 << k)
        call, ref = (lambda: ctx.fr_ntt(s, k, 0)), lambda: _ref(oracle, what, s, k, 0)
    got = _both_paths(ctx, call, False, passes, options)
    assert np.array_equal(got, ref())


def _raw(value):
    """the element whose stored words are the integer `value` (below r)"""
    return ints_to_limbs([value], 4)[0]


def _edge_input(oracle, what):
    one = oracle.fr_to_mont(ints_to_limbs([1], 4))[0]
    a = np.zeros((N, 4), np.uint64)
    if what == "all_r_minus_1":
        a[:] = _raw(B.R_MOD - 1)            # the largest canonical words in every place
    elif what == "one_at_0":
        a[0] = one
    elif what == "one_at_n_minus_1":
        a[N - 1] = one
    elif what == "every_lane_votes":
        a[0] = _raw(B.R_MOD - 1)            # a delta: every output is the words r - 1, the top limb of r in every lane
    elif what == "a_few_lanes_vote":
        # outputs chosen, the input is their inverse transform: the words r - 1 at the ends, beside each other in one wave's
        # stores and alone in others, uniform elements (top limb below r's but for 4e-8 of them) everywhere else
        y = _sample(oracle, 3).copy()
        for i in (0, 1, 2, 1023, 1024, 4097, N // 2, N - 2, N - 1):
            y[i] = _raw(B.R_MOD - 1)
        a = oracle.fr_ntt(y, K, INVERSE)
    return a


@pytest.mark.gpu
@pytest.mark.parametrize("what", ["zeros", "all_r_minus_1", "one_at_0", "one_at_n_minus_1", "every_lane_votes", "a_few_lanes_vote"])
def test_edge_inputs_through_the_fixed_kernels(ctx, oracle, what):
    a = _edge_input(oracle, what)
    got = _both_paths(ctx, lambda: ctx.fr_ntt(a, K, 0), True)
    assert np.array_equal(got, oracle.fr_ntt(a, K, 0))
    if what == "zeros":
        assert not got.any()                                         # no lane has the top limb of r: no voter
    if what == "every_lane_votes":
        assert (got == _raw(B.R_MOD - 1)).all()
    if what == "a_few_lanes_vote":
        assert np.array_equal(got[N - 1], _raw(B.R_MOD - 1)) and np.array_equal(got[4097], _raw(B.R_MOD - 1))


@pytest.mark.gpu
def test_values_outside_the_set_are_refused(ctx):
    import plonk_prototype_amd as pa
    from plonk_prototype_amd import _lib

    for v in (-1, 3, 1 << 20):
        with pytest.raises(pa.Error) as e:
            ctx.set_option("ntt_fixed_shape", v)
        assert e.value.code == _lib.PM_ERR_BAD_ARG, v
    ctx.set_option("ntt_fixed_shape", 1)
