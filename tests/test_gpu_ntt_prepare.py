"""pm_domain_prepare builds every table the transforms of its size need: on a fresh context, after the call, plain and coset
transforms in both directions, a zero-padded one and a batch of two leave the number of cached NTT tables where it was,
and give the CPU oracle's bytes.  The mirror: on a context that was never prepared a plain 2^20 transform builds exactly
the tables its resolved plan names (tests/test_ntt_launches.py counts them on the host)."""
import ctypes as C

import numpy as np
import pytest

from oracle.cpu_oracle import COSET, INVERSE
from test_ntt_launches import DEFAULTS, launches, table_count, tables

pytestmark = pytest.mark.gpu


def _count(ctx):
    n = C.c_size_t(0)
    ctx._check(ctx._lib.pm_test_ntt_table_count(ctx._h, C.byref(n)))
    return n.value


@pytest.fixture()
def fresh():
    import plonk_prototype_amd as pa
    c = pa.Context(0)
    yield c
    c.close()


# 2^11: the smallest two-pass plan [6, 5]; 2^15: [8, 7]; 2^20: [10, 10], the only size with fixed variants and a producer pass
@pytest.mark.parametrize("k", [11, 15, 20])
def test_prepared_transforms_build_no_table(fresh, oracle, k):
    ctx, n = fresh, 1 << k
    assert _count(ctx) == 0
    ctx._check(ctx._lib.pm_domain_prepare(ctx._h, k))
    prepared = _count(ctx)
    assert prepared > 0
    a = oracle.fr_sample(0x50524550 + k, n)
    want = {f: oracle.fr_ntt(a, k, f, 8) for f in (0, INVERSE, COSET, INVERSE | COSET)}
    for f, exp in want.items():
        assert np.array_equal(ctx.fr_ntt(a, k, f), exp), (k, f)
        assert _count(ctx) == prepared, (k, f)
    assert np.array_equal(ctx.fr_ntt(a[:n // 2], k, 0), oracle.fr_ntt(a[:n // 2], k, 0, 8))   # zero-padded
    assert _count(ctx) == prepared, (k, "in_len = n / 2")
    # a batch of two in one launch per pass (not the pipelined vector-by-vector path): ifft of (a, fft(a)) = (ifft(a), a)
    ctx.set_option("ntt_pipeline", 0)
    got = ctx.fr_ntt_batch(np.stack([a, want[0]]), k, INVERSE)
    assert np.array_equal(got[0], want[INVERSE]) and np.array_equal(got[1], a)
    assert _count(ctx) == prepared, (k, "batch of two")


def test_unprepared_plain_transform_builds_what_its_plan_names(fresh, oracle):
    ctx, k = fresh, 20
    a = oracle.fr_sample(0x50524551, 1 << k)
    assert _count(ctx) == 0
    got = ctx.fr_ntt(a, k, 0)
    named = tables(k, 0, *launches(ctx._lib, k, 1, 0, 1 << k, DEFAULTS))
    assert _count(ctx) == table_count(named) == 5    # the domain's two, one step table, the G = 3 lazy table, one inter-pass table
    assert np.array_equal(got, oracle.fr_ntt(a, k, 0, 8))
