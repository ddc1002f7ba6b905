"""The first-layer step twiddles of the radix-4 pass kernels, applied by their producer (L1_UNIFORM in
csrc/ntt_kernels4.hip.h), walked through the limb-exact model of oracle/fe_model.py -- no GPU, no library.

Step 0 hands its dft4 outputs (B < 5, V < 40) to the LDS as: X[0] through fe_reduce_weak, X[t] (t = 1..3) through
fe_mul_split<1, 2> by w16^(t m), m = 0..3 the wave's (the waves with m = 0 multiply by 1; the reduced form is walked
for them as well, it is the narrower class).  Step 1 feeds what it reads to dft4 as it is.  Checked here: the worst
members of every class involved leave VIOLATIONS empty (no precondition broken, no 32- or 64-bit wrap, every annotated
intermediate inside its class) for every mix of reduced and multiplied inputs, and a 16-point transform built from the
two layers in the kernel's own slot order equals the direct DFT."""
import itertools
import random

import pytest

from oracle import bigint_oracle as B
from oracle import fe_model as F

FR = F.FR
HEAD_EXPONENTS = (4, 1, 2, 3, 6, 9, 0)     # block 0 is w4 = w16^4


def _w16(inverse):
    d = B.Domain(16)
    return d.group_gen_inv if inverse else d.group_gen


def _mont(v):
    return v * FR.RADIX % FR.mod


def _rows(inverse, e):
    return F.rows_of(_mont(pow(_w16(inverse), e, FR.mod)), 1, 2)


def _step0_out(x, inverse, t, m):
    """what step 0 stores for its dft4 output X[t]: the weak reduction of X[0], the product by w16^(t m) of the others"""
    return F.fe_reduce_weak(FR, x) if t == 0 else F.fe_mul_split(x, _rows(inverse, t * m), 1, 2)


@pytest.fixture(autouse=True)
def _clean():
    del F.VIOLATIONS[:]
    yield
    del F.VIOLATIONS[:]


def test_exponent_set_is_the_head():
    assert {t * m for t in (1, 2, 3) for m in (0, 1, 2, 3)} | {4} == set(HEAD_EXPONENTS)


@pytest.mark.parametrize("inverse", [0, 1])
def test_step0_outputs_stay_in_the_classes_dft4_takes(inverse):
    members = F.class_members(FR, 5, 40, False, n_random=40, seed=inverse)      # dft4's documented output class
    for x in members:
        weak = F.fe_reduce_weak(FR, x)
        assert F.in_class(FR, weak, 1, 2) and F.value_of(FR, weak) < FR.mod + (FR.mod >> 16)
        assert F.in_class(FR, weak, 1, 24, True)                                  # a0's class
        for e in HEAD_EXPONENTS:
            p = F.fe_mul_split(x, _rows(inverse, e), 1, 2)
            assert F.in_class(FR, p, 1, 2)
            assert F.value_of(FR, p) % FR.mod == F.value_of(FR, x) * pow(_w16(inverse), e, FR.mod) % FR.mod
    assert F.VIOLATIONS == []


@pytest.mark.parametrize("inverse", [0, 1])
def test_dft4_takes_every_mix_of_reduced_and_multiplied_inputs(inverse):
    """a0 is a reduced X[0] (k' = 0) or X[t] times 1 (k' = t, from an m = 0 wave); a1..a3 are all reduced (k' = 0) or all
    products (k' != 0) in the kernel -- every mix is walked, a0 in both forms.  The worst members: the largest value and
    the most redundant limbs of each class."""
    w4 = F.limbs_of(FR, _mont(pow(_w16(inverse), 4, FR.mod)))
    src = F.class_members(FR, 5, 40, False, n_random=6, seed=7 + inverse)
    weak = [F.fe_reduce_weak(FR, x) for x in src]
    prod = {e: [F.fe_mul_split(x, _rows(inverse, e), 1, 2) for x in src] for e in (0, 1, 2, 3, 6, 9)}
    # the classes' own extremes as well: (1, <2) for a product, (1, < 1 + 2^-16) for a weak reduction
    prod_extreme = F.class_members(FR, 1, 2)
    weak_extreme = [F.limbs_of(FR, FR.mod + (FR.mod >> 16) - 1), F.limbs_of(FR, FR.mod), F.limbs_of(FR, 0)]
    walked = 0
    for kinds in itertools.product("wp", repeat=3):
        pools = [weak + weak_extreme + prod[0] + prod_extreme]
        pools += [(weak + weak_extreme) if k == "w" else (prod[3] + prod[9] + prod_extreme) for k in kinds]
        n = max(len(p) for p in pools)
        for i in range(n):
            a = [p[(i + 3 * j) % len(p)] for j, p in enumerate(pools)]
            F.dft4(a[0], a[1], a[2], a[3], w4)
            walked += 1
        worst = [max(p, key=lambda l: F.value_of(FR, l)) for p in pools]
        F.dft4(worst[0], worst[1], worst[2], worst[3], w4)
    assert walked and F.VIOLATIONS == []


@pytest.mark.parametrize("inverse", [0, 1])
def test_two_layers_in_slot_order_are_the_16_point_dft(inverse):
    """R = 16, U = 4: thread u of step 0 holds rows u + 4 m', writes X[t] to slot 4 u + t with the factor w16^(t m),
    m = u >> (log2 U - 2) = u; thread u' of step 1 reads slots u' + 4 m and its X[t] is row u' + 4 t of the result."""
    rng = random.Random(0x4C31 + inverse)
    w16 = _w16(inverse)
    w4 = F.limbs_of(FR, _mont(pow(w16, 4, FR.mod)))
    rinv = FR.RINV
    for _ in range(8):
        vals = [rng.randrange(FR.mod) for _ in range(16)]
        x = [F.limbs_of(FR, _mont(v)) for v in vals]
        slots = [None] * 16
        for u in range(4):
            X = F.dft4(x[u], x[u + 4], x[u + 8], x[u + 12], w4)
            m = u
            for t in range(4):
                slots[4 * u + t] = _step0_out(X[t], inverse, t, m)
        out = [None] * 16
        for u in range(4):
            X = F.dft4(slots[u], slots[u + 4], slots[u + 8], slots[u + 12], w4)
            for t in range(4):
                out[u + 4 * t] = F.value_of(FR, X[t]) * rinv % FR.mod
        want = [sum(v * pow(w16, j * k, FR.mod) for j, v in enumerate(vals)) % FR.mod for k in range(16)]
        assert out == want
    assert F.VIOLATIONS == []
