"""The integers the binary GCD of csrc/field_inv.hip.h is made to iterate on, shared by the model test (test_fe_inv_model.py)
and the device tests (test_gpu_field_inv.py).  A plain module, not a conftest.

A case is y itself, 0 <= y < m: what fe_inv_int receives as canonical limbs, with no Montgomery factor put on it by the test.
Random y finish in 12 - 14 (Fr) / 19 - 21 (Fp) of the 18 / 28 rounds and take the sign repair about once in 200 inversions, so
the lists are built from the shapes that reach the rest (figures: the model, oracle/fe_model.py, over these lists):
  * small numbers, 2^k, 2^k - 1, m - k, m - 2^k, (m +- 1) / 2: every round count from 9 (Fr) / 14 (Fp) up to ROUNDS, the exact
    path from its first possible round on, and most of the sign repairs of the a row;
  * c 2^(W i) + d at every limb position: single non-zero limbs, and borrows that run through all limbs below;
  * c 2^k and m - c 2^k for small odd c and the 24 largest k: the integers whose LAST round still changes v.  With 2^k
    the b row is final from the first swap on (b = 1 from there), and the round that turns a = b = 1 into a = 0 never
    touches v, so a loop one round short gets every case above right; with c >= 3 there is a swap in round ROUNDS;
  * m / 3, 2 m / 3;
  * k R' mod m and k R mod m (R' = 2^(W N) the device radix, R = 2^(32 NS) the ABI one), k = 1 .. 128: the integers the GCD
    sees when a test hands a small x over in a Montgomery form.  This family is where the b row is repaired in Fp: about one k in
    four, against none of 3,000 random y, none of m - k, and 10 of 2,656 values next to m / 2^k (the search behind that: every
    list here, (m >> k) + d for k < 381 and |d| <= 3, and seeded random y, 7,500 model inversions in all).  So the list
    reaches the Fp b-row repair by itself and no searched-for values are hard-coded;
  * 200 seeded random values.
"""
import functools
import random

from oracle import fe_model as M

FIELDS = [M.FR, M.FP]
FIELD_ID = {"fr": 0, "fp": 1}

# one y per field that needs every round, the last one changing v (asserted in test_fe_inv_model.py); members of cases()
FULL_ROUND = {"fr": 3 << 239, "fp": 3 << 376}


@functools.lru_cache(maxsize=None)
def cases(f):
    """the integers y, in a fixed order, without repetitions; 0 comes first"""
    m, W, N = f.mod, f.W, f.N
    bits = m.bit_length()
    ys = list(range(64)) + [1 << k for k in range(bits)] + [(1 << k) - 1 for k in range(bits)]
    ys += [m - k for k in range(1, 64)] + [m - (1 << k) for k in range(bits)] + [(m - 1) // 2, (m + 1) // 2]
    ys += [c * (1 << (W * i)) + d for i in range(N) for c in (1, 2, 3, (1 << W) - 1) for d in (-1, 0, 1)]
    late = [c << k for c in (3, 5, 7, 9, 11, 13, 15) for k in range(bits - 24, bits)]
    ys += late + [m - y for y in late]
    ys += [m // 3, 2 * m // 3]
    ys += [k * f.RADIX % m for k in range(1, 129)] + [(k << (32 * f.NS)) % m for k in range(1, 129)]
    rng = random.Random(0x1A5E + W)
    ys += [rng.randrange(m) for _ in range(200)]
    return tuple(dict.fromkeys(y for y in ys if 0 <= y < m))


@functools.lru_cache(maxsize=None)
def walk(f):
    """The model over cases(f), once per process: ([(y, result limbs of fe_inv_int, trace)], violations recorded on the way).
    M.VIOLATIONS is left as it was."""
    kept = list(M.VIOLATIONS)
    M.VIOLATIONS.clear()
    out = []
    for y in cases(f):
        trace = {}
        r = M.fe_inv_int(f, M.limbs_of(f, y), trace)
        out.append((y, tuple(r), trace))
    violations = list(M.VIOLATIONS)
    M.VIOLATIONS[:] = kept
    return tuple(out), violations


def redundant(f, v):
    """v in the most redundant limbs fe_canon_limbs admits: limbs up to 2^32 - 2^(32-W) - 1"""
    return M.most_redundant(f, v, 0, top=M.canon_limb_max(f))


@functools.lru_cache(maxsize=None)
def canon_cases(f):
    """Members of fe_canon_limbs' operand class (value < 2 m, limbs < 2^32 - 2^(32-W)): the worst and edge members and 200
    seeded random ones of (7+, <2), which lies inside it; every low limb AT the limit with the top limb as large as 2 m
    allows; and 0, 1, m - 1, m, m + 1, 2 m - 1 in canonical limbs and in the most redundant limbs of the class."""
    m, top = f.mod, M.canon_limb_max(f)
    out = [tuple(l) for l in M.class_members(f, 7, 2, True, n_random=200, seed=29)]
    low = [top] * (f.N - 1)
    out.append(tuple(low + [(2 * m - 1 - M.value_of(f, low)) >> (f.W * (f.N - 1))]))
    for v in (0, 1, m - 1, m, m + 1, 2 * m - 1):
        out += [tuple(M.limbs_of(f, v)), tuple(redundant(f, v))]
    assert all(max(l) <= top and M.value_of(f, l) < 2 * m for l in out)
    return tuple(out)
