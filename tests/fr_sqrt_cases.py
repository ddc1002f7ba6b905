"""Inputs that reach every table entry and every search digit of the windowed square root (csrc/fr_sqrt.hip.h, DESIGN.md
section 7.2p), with expectations that owe nothing to it, and the kernel's algorithm restated in Python integers to PROVE that
the inputs reach what they are meant to reach.

The root works on a residue b of the subgroup of order 2^32: b = a^t for the plain root, b = (u v)^(-t) for the ratio root of
the decoder, t = (r - 1) / 2^32.  Its logarithm k (b = g^k) is found in four 8-bit windows against 256 keys; after window i < 3
b takes entry k_i of table i, and the root then takes entry (byte i of k >> 1) of table i, i = 0 .. 3.  So what an input reads
is a function of k alone -- ``seen_plain`` / ``seen_ratio`` -- and t = -1 mod 2^32: c^(2^32) g^m is met as k = -m mod 2^32.

  plain set   a = c^(2^32) g^m for chosen logarithms and random c: the roots are +-c^(2^31) g^(m / 2) BY CONSTRUCTION, a
              non-square when m is odd.  No Tonelli-Shanks goes into the expectation.
  ratio set   seeded y, kept greedily while they add a (window, digit) pair; both sign bits; the expectation is
              ``jubjub_codec_model.decode``.
  restatement ``windowed_finish`` and its two front ends over ``Tables``: which keys matched, which entries were read.  It
              defines no expectation; the tests use it for coverage and to show that a wrong entry or key changes an output.

Plain Python integers throughout; nothing here touches the library's arithmetic.  Every set is built once a process."""
import functools
import os
import random
import sys
from collections import namedtuple

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jubjub_codec_model as CM  # noqa: E402

R, D, G = CM.R, CM.D, CM.ROOT_OF_UNITY
T = (R - 1) >> 32                                  # odd, and -1 mod 2^32
WINDOWS, BITS, ENTRIES = 4, 8, 256
MASK = ENTRIES - 1
H = pow(G, 1 << 24, R)                             # of order 256
G_INV = pow(G, -1, R)
EXP_PLAIN = (T - 1) // 2                           # FR_SQRT_EXP_PLAIN
EXP_RATIO = (R - 1) - (T + 1) // 2                 # FR_SQRT_EXP_RATIO
_H_LOG = {pow(H, j, R): j for j in range(ENTRIES)}
# the logarithms the search is meant to meet at its edges: zero windows, all-ones windows, carries across every boundary
EDGE_LOGS = ([0, 1, 2, 1 << 31, (1 << 32) - 1, (1 << 32) - 2] + [MASK << (BITS * i) for i in range(WINDOWS)]
             + [(1 << (BITS * i)) + d for i in range(1, WINDOWS) for d in (-2, -1, 0, 1)]
             + [(1 << 32) - (1 << (BITS * i)) for i in range(1, WINDOWS)])
SEED = 2026
RATIO_CAP = 8192


def digit(k: int, i: int) -> int:
    return (k >> (BITS * i)) & MASK


# ------------------------------------------------------------------------------------------ the logarithm an input is met as
def subgroup_log(b: int):
    """k with b = g^k by Pohlig-Hellman, four windows over h = g^(2^24) with a dict of h^j; None outside the subgroup"""
    k = 0
    for i in range(WINDOWS):
        ki = _H_LOG.get(pow(b, 1 << (BITS * (WINDOWS - 1 - i)), R))
        if ki is None:
            return None
        k |= ki << (BITS * i)
        b = b * pow(G_INV, ki << (BITS * i), R) % R
    return k if b == 1 else None


def seen_plain(a: int):
    """k with a^t = g^k: what the search of the plain root meets; None for 0"""
    return subgroup_log(pow(a, T, R))


def ratio_operands(y: int):
    y2 = y * y % R
    return (y2 - 1) % R, (1 + D * y2) % R


def seen_ratio(y: int):
    """k with (u v)^(-t) = g^k, u = y^2 - 1, v = 1 + d y^2: what the search of the decoder meets; None when u = 0"""
    u, v = ratio_operands(y)
    return subgroup_log(pow(u * v % R, R - 1 - T, R))


# ------------------------------------------------------------------------------------------ the plain set
Plain = namedtuple("Plain", "a root flag k odd")   # k: the logarithm the search meets, None for a = 0; odd: of constructed()


def constructed(c: int, m: int):
    """a = c^(2^32) g^m -> (a, even root, flag, the parity of c^(2^31) g^(m / 2)); a non-square for odd m"""
    a = pow(c, 1 << 32, R) * pow(G, m, R) % R
    if m & 1:
        return a, 0, 0, None
    x = pow(c, 1 << 31, R) * pow(G, m >> 1, R) % R
    return a, (R - x if x & 1 else x), 1, x & 1


def plain_logs(seed: int = SEED):
    """the logarithms the plain set is met as, in order: (a) every digit of every window alone and among random windows, (b)
    the same for the digits of k >> 1 on even k, (c) odd k for every odd digit of window 0 and a sample of the other windows,
    (d) every order 2^j, (e) the edges"""
    rng = random.Random(seed)

    def among(i, j, bits=32):                      # random below 2^bits with digit j in window i
        return (rng.getrandbits(bits) & ~(MASK << (BITS * i))) | (j << (BITS * i))

    ks = []
    for i in range(WINDOWS):
        for j in range(ENTRIES):
            ks += [j << (BITS * i), among(i, j)]
    for i in range(WINDOWS):
        for j in range(ENTRIES // 2 if i == WINDOWS - 1 else ENTRIES):   # k >> 1 is below 2^31
            ks += [(j << (BITS * i)) << 1, among(i, j, 31) << 1]
    for j in range(1, ENTRIES, 2):
        ks += [j, among(0, j)]
    for i in range(1, WINDOWS):
        ks += [among(i, j) | 1 for j in (0, 1, 2, 0x7f, 0x80, 0x81, 0xfe, 0xff)] + [among(i, rng.randrange(ENTRIES)) | 1 for _ in range(8)]
    for j in range(33):                            # g^k of order 2^j: the trip counts of the host form's loop
        ks += [(odd << (32 - j)) & 0xffffffff for odd in (1, rng.getrandbits(32) | 1)]
    return ks + EDGE_LOGS


@functools.lru_cache(maxsize=None)
def plain_set(seed: int = SEED):
    """tuple of Plain: 0, 1, 4 and r - 1, then c^(2^32) g^(-k) for the k of ``plain_logs`` and random c; a count that is no
    multiple of 64, and roots of both parities before the even one is taken"""
    rng = random.Random(seed + 1)
    one, minus_one = constructed(1, 0), constructed(1, 1 << 31)
    out = [Plain(0, 0, 1, None, 0), Plain(*one[:3], 0, one[3]), Plain(4, 2, 1, seen_plain(4), 0),
           Plain(*minus_one[:3], 1 << 31, minus_one[3])]
    assert one[0] == 1 and minus_one[0] == R - 1
    logs = plain_logs(seed)
    if (len(out) + len(logs)) % 64 == 0:
        logs.append(rng.getrandbits(32))
    for k in logs:
        a, root, flag, odd = constructed(rng.randrange(1, R), -k % (1 << 32))
        out.append(Plain(a, root, flag, k, odd))
    assert len(out) % 64 != 0
    return tuple(out)


# ------------------------------------------------------------------------------------------ the ratio set
def search_pairs():
    return {(i, j) for i in range(WINDOWS) for j in range(ENTRIES)}


def correction_pairs():
    """the digits of k >> 1 < 2^31: the upper half of table 3 is out of reach"""
    return {(i, j) for i in range(WINDOWS) for j in range(ENTRIES) if (i, j) < (WINDOWS - 1, ENTRIES // 2)}


@functools.lru_cache(maxsize=None)
def ratio_ys(seed: int = SEED):
    """(the kept y, the count drawn): y = 1, r - 1 (x = 0) and 0 first, then seeded y, each kept only when it adds a pair: a
    (window, digit) of the search on any y; a (window, digit) of the correction, or a digit matched in any window, on a square
    radicand -- a wrong key or entry shows only in the output of a square"""
    rng = random.Random(seed)
    need = {("search",) + p for p in search_pairs()} | {("correct",) + p for p in correction_pairs()}
    need |= {("square", j) for j in range(ENTRIES)}
    kept, drawn = [1, R - 1, 0], 0
    while need and drawn < RATIO_CAP:
        y = rng.randrange(R)
        drawn += 1
        k = seen_ratio(y)
        if k is None:
            continue
        adds = {("search", i, digit(k, i)) for i in range(WINDOWS)}
        if k & 1 == 0:
            adds |= {("correct", i, digit(k >> 1, i)) for i in range(WINDOWS)} | {("square", digit(k, i)) for i in range(WINDOWS)}
        if adds & need:
            need -= adds
            kept.append(y)
    assert not need, (drawn, len(need))
    return tuple(kept), drawn


@functools.lru_cache(maxsize=None)
def ratio_set(seed: int = SEED):
    """tuple of 32-byte encodings: every kept y with both sign bits, then one y that is not below r (an odd count)"""
    ys, _ = ratio_ys(seed)
    return tuple(CM.y_bytes(y, sign) for y in ys for sign in (0, 1)) + (CM.y_bytes(R, 1),)


@functools.lru_cache(maxsize=None)
def ratio_expected(check_subgroup: bool, seed: int = SEED):
    """tuple of (point, status) of ``jubjub_codec_model.decode``"""
    return tuple(CM.decode(data, check_subgroup) for data in ratio_set(seed))


# ------------------------------------------------------------------------------------------ the kernel's algorithm, restated
class Tables:
    """tab[i][j] = g^(-j 2^(8 i)) and keys[j] = h^j: what sqrt_table_host() builds, as integers.  The device compares limb 0 of
    the canonical value in its own form; the integers stand for it (the build refuses keys that coincide)."""

    def __init__(self, tab=None, keys=None):
        self.tab = tab if tab is not None else [[pow(G_INV, j << (BITS * i), R) for j in range(ENTRIES)] for i in range(WINDOWS)]
        self.keys = keys if keys is not None else [pow(H, j, R) for j in range(ENTRIES)]
        self.index = {key: j for j, key in enumerate(self.keys)}   # the highest j wins, as in the kernel's ascending loop

    def with_entry(self, i: int, j: int, value: int) -> "Tables":
        tab = list(self.tab)
        tab[i] = list(tab[i])
        tab[i][j] = value
        return Tables(tab, self.keys)

    def with_key(self, j: int, value: int) -> "Tables":
        keys = list(self.keys)
        keys[j] = value
        return Tables(self.tab, keys)


@functools.lru_cache(maxsize=None)
def tables() -> Tables:
    return Tables()


class Trace:
    """what one root read: (window, digit) of the keys that matched, (table, entry) divided out of b, (table, entry) multiplied
    into the root, whether the radicand was a non-zero square -- only then does the root reach the output -- and whether the
    root was negated to make it even"""

    def __init__(self):
        self.keys, self.divide, self.correct, self.live, self.negated = set(), set(), set(), False, False


def windowed_finish(x: int, b: int, zero: bool, t: Tables, trace: Trace = None):
    """fr_sqrt_log and fr_sqrt_finish: (even root, flag) from x and b with x^2 = (the radicand) b"""
    trace = trace or Trace()
    k, found = 0, True
    for i in range(WINDOWS):
        ki = t.index.get(pow(b, 1 << (BITS * (WINDOWS - 1 - i)), R))
        if ki is None:
            found, ki = False, 0                   # 256 & 255
        else:
            trace.keys.add((i, ki))
        k |= ki << (BITS * i)
        if i + 1 < WINDOWS:
            trace.divide.add((i, ki))
            b = b * t.tab[i][ki] % R
    square = zero or (found and k & 1 == 0)
    trace.live = square and not zero
    for i in range(WINDOWS):
        j = digit(k >> 1, i)
        trace.correct.add((i, j))
        x = x * t.tab[i][j] % R
    trace.negated = bool(x & 1)
    if trace.negated:
        x = R - x
    return (x, 1) if square else (0, 0)


def plain_front(a: int):
    """fr_sqrt_dev up to the logarithm: (x, b, zero)"""
    w = pow(a, EXP_PLAIN, R)
    x = a * w % R
    return x, x * w % R, a == 0


def ratio_front(u: int, v: int):
    """fr_sqrt_ratio_dev up to the logarithm: one exponentiation on u v, no inversion"""
    a = u * v % R
    w = pow(a, EXP_RATIO, R)
    return u * w % R, a * w % R * w % R, a == 0


def decode_front(data: bytes):
    """jubjub_decode_kernel up to the logarithm: (sign, y, below, (x, b, zero)); a y that is not below r is worked on as zero"""
    v = int.from_bytes(data, "little")
    sign, y = v >> 255, v & ((1 << 255) - 1)
    below = y < R
    return sign, y, below, ratio_front(*ratio_operands(y if below else 0))


def decode_finish(front, t: Tables, trace: Trace = None):
    """the rest of jubjub_decode_kernel: (point, status) without the subgroup flag"""
    sign, y, below, xb = front
    x, square = windowed_finish(*xb, t, trace)
    if (x & 1) != sign:
        x = (R - x) % R
    status = CM.BAD_RANGE if not below else CM.BAD_NOT_ON_CURVE if not square else CM.BAD_SIGN if x == 0 and sign else CM.OK
    return ((x, y), status) if status == CM.OK else ((0, 0), status)


@functools.lru_cache(maxsize=None)
def plain_fronts():
    return tuple(plain_front(c.a) for c in plain_set())


@functools.lru_cache(maxsize=None)
def ratio_fronts():
    return tuple(decode_front(data) for data in ratio_set())


def _traced(finish, fronts):
    outs, traces = [], []
    for f in fronts:
        traces.append(Trace())
        outs.append(finish(f, tables(), traces[-1]))
    return tuple(outs), tuple(traces)


@functools.lru_cache(maxsize=None)
def plain_traced():
    """(outputs, traces) of the restatement over the plain set, on the true tables"""
    return _traced(lambda f, t, tr: windowed_finish(*f, t, tr), plain_fronts())


@functools.lru_cache(maxsize=None)
def ratio_traced():
    return _traced(decode_finish, ratio_fronts())
