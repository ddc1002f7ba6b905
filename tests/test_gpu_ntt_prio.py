"""Wave priorities by step in the radix-4 pass kernels (option ntt_step_prio, csrc/ntt_kernels4.hip.h: PASS_STEP_PRIO).
A priority changes which wave a SIMD serves first and nothing a wave computes, so every accepted value
of the option must give the words that 0 gives, on every kernel the flag reaches:

    2^20 forward and inverse, ntt_tw_producer 1 and 0    (10, 10)   <10, 1> first and last, on both twiddle paths
    2^19 forward                                         (10, 9)    the odd-S last pass with its radix-2 step
    2^21 forward                                         (7, 7, 7)  a middle pass
    2^16 forward and inverse                             (8, 8)     <8, 2>
    coset 2^16 -> 2^18 and its inverse                              PASS_PRE_COSET / PASS_POST_COSET with the flag
    a batch of two at 2^16                                          blockIdx.y

The flag reaches the passes of radix 2^10 (step4_has_prio: the radix-2^8 shapes measured slower with it); the other cases stay, so
that a shape is covered the day it takes the flag.  And 2^11 and 2^12, the smallest two-pass plans, against the C oracle; iNTT(NTT(a)) = a at 2^20; a value outside the accepted
set is refused.  The result with 0 is computed once per case and every other value is compared with it."""
import numpy as np
import pytest

from oracle.cpu_oracle import COSET, INVERSE

OFF = 0
DEFAULT = 1                       # the library's own value: the shared context goes back to it
ACCEPTED = [0, 1]                 # what pm_set_option takes for "ntt_step_prio"
REFUSED = [-1, 2, 3, 4, 1 << 20]    # 2 and 3 were variants with an exchange boost: measured, not kept


def _with(ctx, value, call):
    ctx.set_option("ntt_step_prio", value)
    try:
        return call()
    finally:
        ctx.set_option("ntt_step_prio", DEFAULT)


def _same_for_every_value(ctx, call, what):
    ref = _with(ctx, OFF, call)
    for v in ACCEPTED:
        if v != OFF:
            assert np.array_equal(_with(ctx, v, call), ref), (what, v)
    return ref


@pytest.mark.gpu
@pytest.mark.parametrize("producer", [1, 0])
@pytest.mark.parametrize("flags", [0, INVERSE])
def test_headline_passes(ctx, oracle, producer, flags):
    a = oracle.fr_sample(0x5052494F + 20, 1 << 20)
    ctx.set_option("ntt_tw_producer", producer)
    try:
        _same_for_every_value(ctx, lambda: ctx.fr_ntt(a, 20, flags), (20, flags, producer))
    finally:
        ctx.set_option("ntt_tw_producer", 1)


@pytest.mark.gpu
@pytest.mark.parametrize("k,flags", [(19, 0), (21, 0), (16, 0), (16, INVERSE)])
def test_other_plans(ctx, oracle, k, flags):
    a = oracle.fr_sample(0x5052494F + k, 1 << k)
    _same_for_every_value(ctx, lambda: ctx.fr_ntt(a, k, flags), (k, flags))


@pytest.mark.gpu
def test_coset_extension_and_back(ctx, oracle):
    """2^16 coefficients evaluated on the coset of the 2^18 domain, and those evaluations taken back"""
    a = oracle.fr_sample(0x5052494F + 18, 1 << 16)
    ev = _same_for_every_value(ctx, lambda: ctx.fr_ntt(a, 18, COSET), "coset")
    back = _same_for_every_value(ctx, lambda: ctx.fr_ntt(ev, 18, INVERSE | COSET), "coset inverse")
    assert np.array_equal(back[: 1 << 16], a) and not back[1 << 16:].any()


@pytest.mark.gpu
def test_batch_of_two(ctx, oracle):
    k = 16
    a = np.stack([oracle.fr_sample(0xB0 + i, 1 << k) for i in range(2)])
    out = _same_for_every_value(ctx, lambda: ctx.fr_ntt_batch(a, k, 0), "batch")
    assert np.array_equal(out[1], ctx.fr_ntt(a[1], k, 0))


@pytest.mark.gpu
@pytest.mark.parametrize("k", [11, 12])
def test_smallest_two_pass_plans_against_the_oracle(ctx, oracle, k):
    a = oracle.fr_sample(0x5052494F + k, 1 << k)
    for flags in (0, INVERSE):
        ref = oracle.fr_ntt(a, k, flags)
        for v in ACCEPTED:
            assert np.array_equal(_with(ctx, v, lambda: ctx.fr_ntt(a, k, flags)), ref), (k, flags, v)


@pytest.mark.gpu
def test_round_trip(ctx, oracle):
    a = oracle.fr_sample(0x5052494F, 1 << 20)
    for v in ACCEPTED:
        assert np.array_equal(_with(ctx, v, lambda: ctx.fr_ntt(ctx.fr_ntt(a, 20, 0), 20, INVERSE)), a), v


@pytest.mark.gpu
def test_values_outside_the_set_are_refused(ctx, oracle):
    import plonk_prototype_amd as pa
    from plonk_prototype_amd import _lib

    a = oracle.fr_sample(0x5052494F + 12, 1 << 12)
    before = ctx.fr_ntt(a, 12, 0)
    for v in REFUSED:
        with pytest.raises(pa.Error) as e:
            ctx.set_option("ntt_step_prio", v)
        assert e.value.code == _lib.PM_ERR_BAD_ARG, v
        assert np.array_equal(ctx.fr_ntt(a, 12, 0), before), v     # the context still works, and as before
    for v in ACCEPTED:
        ctx.set_option("ntt_step_prio", v)
    ctx.set_option("ntt_step_prio", DEFAULT)


def test_the_plans_named_above():
    """CPU: the passes of the cases (the library's pure-host plan hook)"""
    import ctypes as C

    from plonk_prototype_amd import _lib

    def plan(log_n):
        out = (C.c_uint32 * 20)()
        assert _lib.load().pm_test_ntt_plan(log_n, 1, 0, 0, 4, 0, out) == 0
        v = list(out)
        return [v[1 + 4 * i] for i in range(v[0])]

    assert plan(20) == [10, 10] and plan(19) == [10, 9] and plan(21) == [7, 7, 7] and plan(16) == [8, 8]
    assert plan(11) == [6, 5] and plan(12) == [6, 6]
