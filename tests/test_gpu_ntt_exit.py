"""The fused exit of the radix-4 last and single passes (fe_reduce_canon_pack, csrc/fields.hip.h) on the device.

The exit alone, through pm_test_field_raw_op (op 24, fe_reduce_canon_pack on raw limbs): the cases of
tests/test_ntt_exit_model.py, word for word against the model.  A block of the hook is one wave and cases 64 k .. 64 k + 63
share its vote, so the cases are ordered: first whole waves in which no lane votes (the fast path), then the rest, where
voters and non-voters sit side by side (the slow path, for lanes with r >= m, with top(r) = top(m) and r < m, and with a
small r).

Whole transforms against the C oracle at the smallest sizes that reach each path -- single pass 2^4, 2^8 and 2^10; two
passes 2^11 (6 + 5: the last step is a radix-2 step), 2^12 (6 + 6) and 2^16 (8 + 8); the headline 2^20 (10 + 10) -- with
three inputs: all zero (the lazy outputs are multiples of r, the weak reduction leaves r itself and every wave votes and
subtracts), a delta at index 0 scaled so that every output word is r - 1 (every lane votes, none subtracts), and seeded
random elements (with every flag up to 2^12: the inverse of a single pass and the coset transforms end in a product and keep
fe_canon_pack)."""
import random

import numpy as np
import pytest

from oracle import fe_model as F
from oracle.cpu_oracle import COSET, INVERSE, ints_to_limbs
from test_ntt_exit_model import exit_cases, exit_model, packed

pytestmark = pytest.mark.gpu

FR = F.FR
REDUCE_CANON_PACK = 24                          # enum RawOp, csrc/test_hooks.hip
SIZES = [4, 8, 10, 11, 12, 16, 20]
_REF = {}


def _ref(oracle, name, a, k, flags):
    key = (name, k, flags)
    if key not in _REF:
        _REF[key] = oracle.fr_ntt(a, k, flags, 8)
        _REF[key].setflags(write=False)
    return _REF[key]


def test_exit_on_raw_limbs(ctx):
    cases = exit_cases()
    mine = [exit_model(x)[1] for x in cases]
    quiet = [x for x, m in zip(cases, mine) if not m]
    assert len(quiet) >= 128 and any(mine)
    n_quiet = len(quiet) // 64 * 64                                  # whole waves without a voter
    # the tail: voters among non-voters in one wave
    tail = quiet[64:] + [x for x, m in zip(cases, mine) if m]
    random.Random(24).shuffle(tail)
    ordered = quiet[:n_quiet] + tail
    got = ctx.field_raw_op(0, REDUCE_CANON_PACK, np.array(ordered, dtype=np.uint64).astype(np.uint32)[:, None, :], 1)
    F.VIOLATIONS.clear()
    for x, g in zip(ordered, got.tolist()):
        want = packed(F.value_of(FR, x) % FR.mod)
        assert g[0][:8] == want and g[0][8] == 0
        assert exit_model(x, vote=True)[0] == want
    assert F.VIOLATIONS == []


def _inputs(oracle, k, flags):
    """(name, vector) -- zero, the delta whose transform is r - 1 in every word, random"""
    n = 1 << k
    zero = np.zeros((n, 4), np.uint64)
    delta = np.zeros((n, 4), np.uint64)
    # the stored words are linear in the input words: an inverse transform divides them by n
    v = (FR.mod - 1) * (n if flags & INVERSE else 1) % FR.mod
    delta[0] = ints_to_limbs([v], 4)[0]
    return [("zero", zero), ("delta", delta), ("random", oracle.fr_sample(0x45584954 + k, n))]


@pytest.mark.parametrize("k", SIZES)
def test_transforms(ctx, oracle, k):
    n = 1 << k
    top = np.uint64(FR.mod >> 192)
    for flags in (0, INVERSE):
        for name, a in _inputs(oracle, k, flags):
            got = ctx.fr_ntt(a, k, flags)
            assert np.array_equal(got, _ref(oracle, name, a, k, flags)), (k, flags, name)
            if name == "zero":
                assert not got.any()
            if name == "delta":                                      # every output r - 1: top(r) in its top limb, no subtraction
                assert bool((got[:, 3] == top).all()) and bool((got == got[0]).all()), (k, flags)
    if k <= 12:
        a = oracle.fr_sample(0x45584954 + k, n)
        for flags in (COSET, INVERSE | COSET):
            assert np.array_equal(ctx.fr_ntt(a, k, flags), _ref(oracle, "random", a, k, flags)), (k, flags)
