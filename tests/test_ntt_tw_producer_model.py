"""The inter-pass twiddles of the radix-4 pass kernels, applied by the pass that produces the element (PASS_TW_OUT /
PASS_TW_APPLIED in csrc/ntt_kernels4.hip.h), walked through the limb-exact model of oracle/fe_model.py -- no GPU, no
library.

The producer's last step is a radix-4 step (only shapes of even S are producers): it holds its outputs in dft4's output
class (B < 5, V < 40) and multiplies each by a table entry in canonical limbs (fe_mul, the data as the first factor).  The consumer's step 0 then hands what it loads to dft4 as it
is: four products, a0 included.  Checked here: the worst members of every class involved leave VIOLATIONS empty (no
precondition broken, no 32- or 64-bit wrap, every annotated intermediate inside its class), the product is of the class
(1, <2) and has the right value, and a 16-point transform of two passes, the first multiplying by the second's table in
element order, equals the direct DFT (forward, and inverse with n^-1 in the table)."""
import random

import pytest

from oracle import bigint_oracle as B
from oracle import fe_model as F

FR = F.FR


def _mont(v):
    return v * FR.RADIX % FR.mod


def _canonical_entries(seed):
    """table entries: canonical limbs of w (or of w / n for the last pass of an inverse transform) in Montgomery form"""
    rng = random.Random(seed)
    vals = [0, 1, FR.mod - 1, _mont(1), _mont(pow(1 << 20, -1, FR.mod)), (1 << 29 * 8) - 1]
    vals += [_mont(pow(B.Domain(1 << 20).group_gen, rng.randrange(1 << 20), FR.mod)) for _ in range(6)]
    vals += [rng.randrange(FR.mod) for _ in range(6)]
    out = [F.limbs_of(FR, v) for v in vals]
    out.append([FR.MASK] * 8 + [(FR.mod >> (29 * 8)) - 1])  # every low limb at its maximum: a value below r
    for l in out:
        assert F.in_class(FR, l, 1, 1) and F.value_of(FR, l) < FR.mod
    return out


@pytest.fixture(autouse=True)
def _clean():
    del F.VIOLATIONS[:]
    yield
    del F.VIOLATIONS[:]


@pytest.mark.parametrize("seed", [0, 1])
def test_producer_product_is_the_class_the_consumer_hands_dft4(seed):
    data = F.class_members(FR, 5, 40, False, n_random=40, seed=seed)
    walked = 0
    for x in data:
        assert all(v < 6 << 29 for v in x) and F.value_of(FR, x) < 68 * FR.mod      # fe_mul's first-factor limits
        for w in _canonical_entries(seed):
            p = F.fe_mul(FR, x, w)
            assert F.in_class(FR, p, 1, 2)
            assert F.value_of(FR, p) % FR.mod == F.value_of(FR, x) * F.value_of(FR, w) * FR.RINV % FR.mod
            walked += 1
    assert walked and F.VIOLATIONS == []


@pytest.mark.parametrize("seed", [0, 1])
def test_dft4_takes_four_producer_products(seed):
    """the consumer's step 0: a0..a3 as loaded, products of the producing pass -- the extremes of (1, <2) and products
    of the worst data by the worst entries"""
    w4 = F.limbs_of(FR, _mont(B.Domain(4).group_gen_inv if seed else B.Domain(4).group_gen))
    worst = F.class_members(FR, 5, 40)[:3]
    pool = F.class_members(FR, 1, 2, False, n_random=12, seed=seed)
    pool += [F.fe_mul(FR, x, w) for x in worst for w in _canonical_entries(seed)[:7]]
    for i in range(len(pool)):
        a = [pool[(i + 5 * j) % len(pool)] for j in range(4)]
        F.dft4(a[0], a[1], a[2], a[3], w4)
    top = max(pool, key=lambda l: F.value_of(FR, l))
    F.dft4(top, top, top, top, w4)
    assert F.VIOLATIONS == []


@pytest.mark.parametrize("inverse", [0, 1])
def test_two_passes_with_the_producer_product_are_the_16_point_dft(inverse):
    """N = 16 as two radix-4 passes: pass 0 stores X[t] of column j at element 4 j + t, pass 1 reads element
    idx = j + 4 row times w16^(j row) (times 1/16 for the inverse).  Pass 0 multiplies element idx by entry idx of
    pass 1's table before it stores; pass 1 feeds dft4 what it loads."""
    rng = random.Random(0x7477 + inverse)
    d16 = B.Domain(16)
    w16 = d16.group_gen_inv if inverse else d16.group_gen
    w4 = F.limbs_of(FR, _mont(pow(w16, 4, FR.mod)))
    scale = pow(16, -1, FR.mod) if inverse else 1
    # pass 1's table in element order: column j = idx & 3 (k = j: Ns = 4), row = idx >> 2
    table = [F.limbs_of(FR, _mont(pow(w16, (idx & 3) * (idx >> 2), FR.mod) * scale % FR.mod)) for idx in range(16)]
    for _ in range(6):
        vals = [rng.randrange(FR.mod) for _ in range(16)]
        x = [F.limbs_of(FR, _mont(v)) for v in vals]
        mid = [None] * 16           # pass 0: Ns = 1, out[j * 4 + t] = X[t] of column j
        for j in range(4):
            X = F.dft4(x[j], x[j + 4], x[j + 8], x[j + 12], w4)
            for t in range(4):
                mid[j * 4 + t] = X[t]
        produced = [F.fe_mul(FR, mid[idx], table[idx]) for idx in range(16)]       # PASS_TW_OUT, then st_wide
        out = [None] * 16
        for j in range(4):          # pass 1: Ns = 4, k = j, out[k + t * 4]
            X = F.dft4(produced[j], produced[j + 4], produced[j + 8], produced[j + 12], w4)
            for t in range(4):
                out[j + 4 * t] = F.value_of(FR, X[t]) * FR.RINV % FR.mod
        want = [sum(v * pow(w16, i * k, FR.mod) for i, v in enumerate(vals)) * scale % FR.mod for k in range(16)]
        assert out == want
    assert F.VIOLATIONS == []
