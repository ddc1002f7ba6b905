"""Big-integer model of fe_mul_split (csrc/fields.hip.h), the "data x split constant" product of the radix-4 NTT
steps -- no GPU, no library.  The model walks the 64-bit column accumulator exactly as the device routine does
(same products per column, the digit q = -acc, the 2^W - 1 that stands in for q * m_0, the shift) for the two splits
the kernels use: step twiddles (groups of 5 limbs, 6 digits) and w4 (groups of 1 limb, 2 digits).  Checked for the
worst operands the routine's comment admits and for 10^4 random ones: no column reaches 2^64, the result limbs are
< 2^29 with value < 2r, and the result is x * w / R mod r -- what fe_mul returns for the same operands."""
import random

import pytest

R_MOD = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
W, N = 29, 9
MASK = (1 << W) - 1
M = [(R_MOD >> (W * i)) & MASK for i in range(N)]
RADIX = 1 << (W * N)            # the device Montgomery radix R = 2^261
BX = 6                          # data limbs < BX * 2^W: the bound fe_mul_split states (the kernels stay below 5)
SPLITS = [(5, 6), (1, 2)]       # (G, D): step twiddles, w4
MACS = {(5, 6): 129, (1, 2): 97}


def limbs(v):
    return [(v >> (W * i)) & MASK for i in range(N)]


def value(l):
    return sum(x << (W * i) for i, x in enumerate(l))


def rows_of(w_mont, G, D):
    """row_j = w * 2^(W (jG + D - N)) mod r, canonical limbs (what step4_tw_kernel stores)"""
    groups = (N + G - 1) // G
    out = []
    for j in range(groups):
        e = W * (j * G + D - N)
        f = pow(2, e, R_MOD) if e >= 0 else pow(pow(2, -e, R_MOD), -1, R_MOD)
        out.append(limbs(w_mont * f % R_MOD))
    return out


def mul_split(x, rows, G, D):
    """The device routine, limb for limb.  Returns (result limbs, largest column value seen, products issued)."""
    assert M[0] == 1
    acc, peak, macs = 0, 0, 0
    q, r = [0] * D, [0] * N
    for k in range(D + N - 1):
        for i in range(N):
            b = k - i % G
            if 0 <= b < N:
                acc += x[i] * rows[i // G][b]
                macs += 1
                peak = max(peak, acc)
        for i in range(D):
            l = k - i
            if 1 <= l < N:
                acc += q[i] * M[l]
                macs += 1
                peak = max(peak, acc)
        if k < D:
            q[k] = (-acc) & MASK
            assert (acc + q[k]) >> W == (acc + MASK) >> W     # the carry does not wait for q
            acc += MASK
            peak = max(peak, acc)
        else:
            r[k - D] = acc & MASK
        acc >>= W
    r[N - 1] = acc
    return r, peak, macs


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

