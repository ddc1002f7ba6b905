"""The transforms whose passes take the lazy split products (csrc/ntt_kernels4.hip.h, step4_lazy_form: the <10, 1> shapes)
and the ones beside them that must not notice, bit for bit against the CPU oracle: 2^10 (the single pass), 2^12 and 2^16
(two passes of smaller radix), 2^20 (the only size that runs <10, 1> first and last); forward, inverse and both coset
transforms; random data, every element r - 1, zeros, a delta; the producer-side inter-pass product and the wave
priorities each on and off; and, at 2^20, the other tile shapes the tunables select for radix 2^10.  A lazy product leaves
values up to 37 r where the parent left 2 r: an input that drives every limb high (r - 1) or leaves most of them zero (a
delta) is where a bound that does not hold would show."""
import itertools

import numpy as np
import pytest

from oracle import bigint_oracle as B
from oracle.cpu_oracle import COSET, INVERSE, ints_to_limbs

pytestmark = pytest.mark.gpu
ALL_FLAGS = [0, INVERSE, COSET, INVERSE | COSET]
OPTIONS = list(itertools.product((0, 1), (0, 1)))        # (ntt_tw_producer, ntt_step_prio)
_EXPECTED = {}


def _input(oracle, kind, k):
    n = 1 << k
    if kind == "random":
        return oracle.fr_sample(0x1A27 + k, n)
    if kind == "r-1":
        return np.repeat(oracle.fr_to_mont(ints_to_limbs([B.R_MOD - 1], 4)), n, axis=0)
    a = np.zeros((n, 4), np.uint64)
    if kind == "delta":
        a[n // 3] = oracle.fr_to_mont(ints_to_limbs([1], 4))[0]
    return a


def _expected(oracle, kind, k, flags):
    """one oracle transform per (input, size, kind of transform), shared by every option setting"""
    key = (kind, k, flags)
    if key not in _EXPECTED:
        want = oracle.fr_ntt(_input(oracle, kind, k), k, flags, 8)
        want.setflags(write=False)
        _EXPECTED[key] = want
    return _EXPECTED[key]


def _with_options(ctx, producer, prio, tile=0):
    ctx.set_option("ntt_tw_producer", producer)
    ctx.set_option("ntt_step_prio", prio)
    ctx.set_option("ntt_tile_log", tile)


@pytest.fixture
def restore(ctx):
    yield
    _with_options(ctx, 1, 1, 0)


@pytest.mark.parametrize("k", [10, 12, 16])
def test_small_sizes_every_input_and_option(ctx, oracle, restore, k):
    for kind in ("random", "r-1", "zero", "delta"):
        a = _input(oracle, kind, k)
        for producer, prio in OPTIONS:
            _with_options(ctx, producer, prio)
            for flags in ALL_FLAGS:
                assert np.array_equal(ctx.fr_ntt(a, k, flags), _expected(oracle, kind, k, flags)), (k, kind, flags, producer, prio)


@pytest.mark.parametrize("kind,flag_set", [("random", ALL_FLAGS), ("r-1", [0, INVERSE | COSET]), ("delta", [INVERSE, COSET])],
                         ids=["random", "r-1", "delta"])
def test_2_20_first_and_last_pass_lazy(ctx, oracle, restore, kind, flag_set):
    k = 20
    a = _input(oracle, kind, k)
    for producer, prio in OPTIONS:
        _with_options(ctx, producer, prio)
        for flags in flag_set:
            assert np.array_equal(ctx.fr_ntt(a, k, flags), _expected(oracle, kind, k, flags)), (kind, flags, producer, prio)


@pytest.mark.parametrize("tile", [10, 11, 12])
def test_2_20_tile_shapes_of_radix_1024(ctx, oracle, restore, tile):
    """tile 2^11 is <10, 1>, the lazy shape; 2^10 and 2^12 select <10, 0> and <10, 2>, which keep the (1, <2) products"""
    k = 20
    a = _input(oracle, "random", k)
    for producer in (0, 1):
        _with_options(ctx, producer, 1, tile)
        for flags in ALL_FLAGS:
            assert np.array_equal(ctx.fr_ntt(a, k, flags), _expected(oracle, "random", k, flags)), (tile, flags, producer)


def test_zero_stays_zero_at_2_20(ctx, restore):
    a = np.zeros((1 << 20, 4), np.uint64)
    for flags in (0, INVERSE | COSET):
        assert not ctx.fr_ntt(a, 20, flags).any()
