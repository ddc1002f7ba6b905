"""Big-integer model of the native Schnorr signatures (include/plonk_mi355x.h, pm_schnorr_*): u G + c PK = R with
c = H(R.x, R.y, m) cut to 250 bits, on top of jubjub_model (double-and-add) and poseidon_model (the sponge).  The reference of
tests/test_schnorr_host.py and tests/test_gpu_schnorr.py, with the inputs the two share.  Plain Python integers throughout;
nothing here touches the library's arithmetic."""
import os
import random
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jubjub_model as J  # noqa: E402
import poseidon_model as PM  # noqa: E402

R, Q = J.R, J.Q
M = J.M
MASK = (1 << 250) - 1
OK, U_RANGE, R_POINT, PK_POINT, EQUATION = 0, 1, 2, 3, 4
ORDER_2 = (0, R - 1)
# (rounds, full rounds, matrices, seed): a small permutation with a matrix per round, dusk-hades' shape with one matrix
SHAPES = {"5_2_per_round": (5, 2, 5, 0x5C01), "67_8_one_matrix": (67, 8, 1, 0x5C02)}


class Hades:
    """the constants of one shape, as integers and in the order of the C interface"""

    def __init__(self, name, capacity=0):
        self.rounds, self.full, n_mds, seed = SHAPES[name]
        self.ark, self.mds = PM.constants(self.rounds, n_mds, seed)
        self.flat_ark, self.flat_mds, self.n_mds = PM.flat(self.ark, self.mds)
        self.capacity = capacity

    def hash(self, msg):
        return PM.sponge(list(msg), self.ark, self.mds, self.rounds, self.full, self.capacity)


def challenge(h: Hades, r_point, m):
    """-> (c, the untruncated hash)"""
    full = h.hash([r_point[0], r_point[1], m])
    return full & MASK, full


def sign(h: Hades, g, sk, k, m):
    """-> (u, R.x, R.y)"""
    rp = J.mul(g, k)
    c, _ = challenge(h, rp, m)
    return ((k - c * sk) % Q, rp[0], rp[1])


def _point_fault(p):
    return not (0 <= p[0] < R and 0 <= p[1] < R) or not J.on_curve(p)


def reason(h: Hades, g, pk, m, sig):
    """the lowest reason that applies; u and the coordinates are the integers in memory, whatever their size"""
    u, rp = sig[0], (sig[1], sig[2])
    if not 0 <= u < Q:
        return U_RANGE
    if _point_fault(rp):
        return R_POINT
    if _point_fault(pk):
        return PK_POINT
    c, _ = challenge(h, rp, m)
    return OK if J.add(J.mul(g, u), J.mul(pk, c)) == rp else EQUATION


# ------------------------------------------------------------------------------------------ the inputs the tests share
_CACHE = {}


def case(name, count):
    """`count` (sk, k, m) with their public keys and the model's signatures: the edge scalars of jubjub_model as sk and, shifted
    by seven places, as k, then random ones.  -> dict(h, sk, k, m, pk, sig, full) computed once per (shape, count)"""
    if (name, count) not in _CACHE:
        h = Hades(name)
        edge = J.edge_scalars()
        rng = random.Random(len(name) * 1000 + count)
        sk = (edge + [rng.randrange(R) for _ in range(count)])[:count]
        k = ([edge[(i + 7) % len(edge)] for i in range(len(edge))] + [rng.randrange(R) for _ in range(count)])[:count]
        m = [0, R - 1] + [rng.randrange(R) for _ in range(count)]
        m = m[:count]
        pk = [J.mul(J.GENERATOR, s) for s in sk]
        sig = [sign(h, J.GENERATOR, a, b, c) for a, b, c in zip(sk, k, m)]
        full = [challenge(h, (s[1], s[2]), c)[1] for s, c in zip(sig, m)]
        _CACHE[name, count] = dict(h=h, sk=sk, k=k, m=m, pk=pk, sig=sig, full=full)
    return _CACHE[name, count]


def corruptions(h: Hades, pk, m, sig):
    """one valid (pk, m, sig) -> [(label, pk', m', sig', the model's reason)], all as integers that fit 256 bits.  A coordinate
    + r is given as an integer >= r: the caller writes it to memory as it is (tests: raw_point / raw_sig)."""
    u, rx, ry = sig
    off = (pk[0], (pk[1] + 1) % R)
    assert not J.on_curve(off) and not J.on_curve((rx, (ry + 1) % R))
    out = [("u + l", pk, m, (u + Q, rx, ry)),
           ("R.y + 1", pk, m, (u, rx, (ry + 1) % R)),
           ("PK off the curve", off, m, sig),
           ("m + 1", pk, (m + 1) % R, sig),
           ("R and PK bad", off, m, (u, rx, (ry + 1) % R)),
           ("R.x + r", pk, m, (u, rx + R, ry)),
           ("PK.y + r", (pk[0], pk[1] + R), m, sig)]
    return [(lab, p, mm, s, reason(h, J.GENERATOR, p, mm, s)) for lab, p, mm, s in out]


# ------------------------------------------------------------------------------------------ arithmetic modulo the order
def scalar_cases():
    """(a, b, c): a and b over the multiples of l and their neighbours up to r - 1 and 200 random values, c over 0, 1, 2^250 - 1
    and random values below 2^250"""
    rng = random.Random(0x5CA1)
    edge = [0, 1, Q - 1, Q, Q + 1, 2 * Q - 1, 8 * Q - 1, 8 * Q, R - 1]
    assert 8 * Q == R - 1 or 8 * Q < R
    vals = edge + [rng.randrange(R) for _ in range(200)]
    cs = [0, 1, (1 << 250) - 1] + [rng.getrandbits(250) for _ in range(5)]
    cases = [(a, b, c) for a in edge for b in edge for c in cs[:3]]
    cases += [(a, rng.choice(vals), rng.choice(cs)) for a in vals] + [(rng.choice(vals), b, rng.choice(cs)) for b in vals]
    random.Random(1).shuffle(cases)                          # a wave of 64 holds edge and random cases side by side
    return cases


def scalar_arrays(cases):
    return tuple(np.stack([canon_words(t[j]) for t in cases]) for j in range(3))


def scalar_expect(cases, op):
    if op == 0:
        return [a % Q for a, _, _ in cases]
    if op == 1:
        return [(a - b * c) % Q for a, b, c in cases]
    return [int(a < Q) for a, _, _ in cases]


# ------------------------------------------------------------------------------------------ memory forms
def canon_words(v: int) -> np.ndarray:
    return np.frombuffer(int(v).to_bytes(32, "little"), dtype=np.uint64).copy()


def mont_words(v: int) -> np.ndarray:
    """the Montgomery element of v mod r; for v >= r the element of v - r PLUS r as an integer: the same residue, not canonical"""
    w = int.from_bytes(M.to_limbs([v % R])[0].tobytes(), "little")
    if v >= R:
        w += R
        assert w < 1 << 256, "this residue has no second representative below 2^256"
    return canon_words(w)


def sig_words(sig, montgomery: bool) -> np.ndarray:
    """(u, R.x, R.y) -> [3, 4]: u in the scalar form asked for (as the integer it is, even when >= l), coordinates Montgomery"""
    u = sig[0]
    uw = (mont_words(u) if u < R else canon_words(u)) if montgomery else canon_words(u)
    return np.stack([uw, mont_words(sig[1]), mont_words(sig[2])])


def point_words(p) -> np.ndarray:
    return np.stack([mont_words(p[0]), mont_words(p[1])])


def scalar_words(vals, montgomery: bool) -> np.ndarray:
    return M.to_limbs(list(vals)) if montgomery else np.stack([canon_words(v) for v in vals])
