"""Big-integer model of fe_mul_split (csrc/fields.hip.h), the "data x split constant" product of the radix-4 NTT
steps -- no GPU, no library.  The model walks the 64-bit column accumulator exactly as the device routine does
(same products per column, the digit q = -acc, the 2^W - 1 that stands in for q * m_0, the shift) for the two splits
the kernels use: step twiddles (groups of 5 limbs, 6 digits) and w4 (groups of 1 limb, 2 digits).  Checked for the
worst operands the routine's comment admits and for 10^4 random ones: no column reaches 2^64, the result limbs are
< 2^29 with value < 2r, and the result is x * w / R mod r -- what fe_mul returns for the same operands."""
import random

import pytest

from oracle.fe_model import MASK, M, N, R_MOD, RADIX, W, limbs, mul_split, rows_of, value   # noqa: F401  (the model lives there)

BX = 6                          # data limbs < BX * 2^W: the bound fe_mul_split states (the kernels stay below 5)
SPLITS = [(5, 6), (1, 2)]       # (G, D): step twiddles, w4
MACS = {(5, 6): 129, (1, 2): 97}


def check(x, rows, G, D):
    r, peak, macs = mul_split(x, rows, G, D)
    assert macs == MACS[(G, D)]
    assert peak < 1 << 64, f"column overflow: {peak:#x}"
    assert all(v < 1 << W for v in r), r
    t = sum(value(x[j * G:(j + 1) * G]) * value(rows[j]) for j in range(len(rows)))
    assert value(r) < 2 * R_MOD
    assert value(r) * (1 << (W * D)) >= t and value(r) < t // (1 << (W * D)) + R_MOD + 1
    assert (value(r) << (W * D)) % R_MOD == t % R_MOD
    return r


@pytest.mark.parametrize("G,D", SPLITS)
def test_worst_case_operands(G, D):
    top = [BX * (1 << W) - 1] * N
    groups = (N + G - 1) // G
    check(top, [limbs(R_MOD - 1)] * groups, G, D)              # constant rows at r - 1
    check(top, [[MASK] * N] * groups, G, D)                    # every constant limb at its maximum: the column bound
    w = R_MOD - 1
    r = check(top, rows_of(w, G, D), G, D)
    assert value(r) % R_MOD == value(top) * w * pow(RADIX, -1, R_MOD) % R_MOD


@pytest.mark.parametrize("G,D", SPLITS)
def test_random_operands(G, D):
    rng = random.Random(0x4E5454 + G)
    rinv = pow(RADIX, -1, R_MOD)
    for it in range(10000):
        if it % 3 == 0:      # canonical data, as loaded
            x = limbs(rng.randrange(R_MOD))
        elif it % 3 == 1:    # lazily reduced data, as the butterflies hand it over
            x = [rng.randrange(BX << W) for _ in range(N)]
        else:                # limbs near the bound
            x = [(BX << W) - 1 - rng.randrange(1 << 8) for _ in range(N)]
        w = rng.randrange(R_MOD)
        r = check(x, rows_of(w, G, D), G, D)
        assert value(r) % R_MOD == value(x) * w * rinv % R_MOD

