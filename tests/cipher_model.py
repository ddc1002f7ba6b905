"""Big-integer model of the Poseidon cipher on JubJub keys (include/plonk_mi355x.h, pm_poseidon_cipher_*): the scheme of the
header in Python integers, over the constants of schnorr_model.Hades, the permutation of hades_model and the affine law of
jubjub_model.mul_affine.  The reference of tests/test_cipher_host.py and tests/test_gpu_cipher.py, with the inputs the two
share.  Plain Python integers throughout; nothing here touches the library's arithmetic."""
import os
import random
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jubjub_model as J  # noqa: E402
import schnorr_model as S  # noqa: E402

R, Q = J.R, J.Q
HM = S.PM.HM
SHAPES = S.SHAPES
DOMAIN = 1 << 32
MAX_LEN = 4
OK, POINT, RANGE, TAG = 0, 1, 2, 3
ORDER_2 = (0, R - 1)


def permute(h, state):
    return HM.hades_model(list(state), h.ark, h.mds, h.rounds, h.full)


def point_fault(p):
    return not (0 <= p[0] < R and 0 <= p[1] < R) or not J.on_curve(p)


def encrypt(h, secret, nonce, msg, L):   # noqa: N803
    """-> the L + 1 cipher words; a message shorter than L is padded with zeros"""
    m = list(msg) + [0] * (L - len(msg))
    assert 1 <= L <= MAX_LEN and len(m) == L
    s = permute(h, [DOMAIN, L, secret[0], secret[1], nonce])
    c = []
    for i in range(L):
        s[1 + i] = (s[1 + i] + m[i]) % R
        c.append(s[1 + i])
    s = permute(h, s)
    return c + [s[1]]


def decrypt(h, secret, nonce, cipher, L, tested=None):   # noqa: N803
    """-> (the L message words, status), the lowest status that applies; every argument is the integer in memory, whatever its
    size.  `tested` is the point the curve test judges: the secret, or a scan's ephemeral key."""
    assert len(cipher) == L + 1
    zero = [0] * L
    if point_fault(secret if tested is None else tested):
        return zero, POINT
    if not 0 <= nonce < R or any(not 0 <= c < R for c in cipher):
        return zero, RANGE
    s = permute(h, [DOMAIN, L, secret[0], secret[1], nonce])
    m = []
    for i in range(L):
        m.append((cipher[i] - s[1 + i]) % R)
        s[1 + i] = cipher[i]
    s = permute(h, s)
    return (m, OK) if s[1] == cipher[L] else (zero, TAG)


_MUL = {}


def mul(p, s):
    """jubjub_model.mul_affine, remembered: the law applied literally"""
    if (p, s) not in _MUL:
        _MUL[p, s] = J.mul_affine(p, s)
    return _MUL[p, s]


def scan(h, vk, eph, nonce, cipher, L):   # noqa: N803
    """one note under the viewing key -> (message, status)"""
    if point_fault(eph):
        return [0] * L, POINT
    return decrypt(h, mul(eph, vk), nonce, cipher, L, tested=eph)


# ------------------------------------------------------------------------------------------ the inputs the tests share
SPECIAL_KEYS = (1, 8, 9, R - 1, int("7f" + "9" * 10 + "0", 16))   # the last: a zero low digit, then a run of carries
_CACHE = {}


def case(shape, count):
    """`count` notes, a seeded 40 in 130 of them (the same share of any count) addressed to vk[0] and the rest to vk[1] and
    vk[2]: dict(h, vk, pk, owner, e, eph, secret, nonce, msg) with four message words a note, computed once per (shape, count).
    The points do not depend on the shape and are shared between the shapes."""
    if (shape, count) not in _CACHE:
        if ("points", count) not in _CACHE:
            rng = random.Random(0xC1F0 + count)
            vk = [rng.randrange(1, R) for _ in range(3)]
            pk = [mul(J.GENERATOR, k) for k in vk]
            own = set(rng.sample(range(count), max(1, count * 40 // 130)))
            owner = [0 if i in own else 1 + rng.randrange(2) for i in range(count)]
            edge = [1, 2, Q - 1, Q + 1, R - 1]
            e = (edge + [rng.randrange(1, R) for _ in range(count)])[:count]
            eph = [mul(J.GENERATOR, x) for x in e]
            secret = [mul(pk[o], x) for o, x in zip(owner, e)]
            nonce = ([0, R - 1] + [rng.randrange(R) for _ in range(count)])[:count]
            msg = [[rng.randrange(R) for _ in range(MAX_LEN)] for _ in range(count)]
            msg[0], msg[-1] = [0] * MAX_LEN, [R - 1] * MAX_LEN
            _CACHE["points", count] = dict(vk=vk, pk=pk, owner=owner, e=e, eph=eph, secret=secret, nonce=nonce, msg=msg)
        _CACHE[shape, count] = dict(_CACHE["points", count], h=S.Hades(shape))
    return _CACHE[shape, count]


def ciphers(cs, shape, L):   # noqa: N803
    """the model's cipher of every note of a case at capacity L, computed once"""
    key = ("ciphers", shape, len(cs["e"]), L)
    if key not in _CACHE:
        _CACHE[key] = [encrypt(cs["h"], s, k, m[:L], L) for s, k, m in zip(cs["secret"], cs["nonce"], cs["msg"])]
    return _CACHE[key]


def corruptions(h, L, point, nonce, cipher, secret=None):   # noqa: N803
    """one valid note -> [(label, point', nonce', cipher', message, status)] with every status code, the model's verdict on each,
    all as integers that fit 256 bits.  `point` is what the curve test judges: the secret (then `secret` is None) or a scan's
    ephemeral key, whose secret is given.  A value + r is an integer >= r: the caller writes it to memory as it is."""
    x, y = point
    off = (x, (y + 1) % R)
    assert not J.on_curve(off)
    bump = lambda c, j, d: c[:j] + [c[j] + d] + c[j + 1:]   # noqa: E731
    out = [("as it is", point, nonce, cipher),
           ("off the curve", off, nonce, cipher),
           ("x + r", (x + R, y), nonce, cipher),
           ("y + r", (x, y + R), nonce, cipher),
           ("nonce + r", point, nonce + R, cipher),
           ("word 0 + r", point, nonce, bump(cipher, 0, R)),
           ("tag + r", point, nonce, bump(cipher, L, R)),
           ("tag + 1", point, nonce, bump(cipher, L, 1 if cipher[L] < R - 1 else -1)),
           ("word 0 + 1", point, nonce, bump(cipher, 0, 1 if cipher[0] < R - 1 else -1)),
           ("nonce + 1", point, (nonce + 1) % R, cipher),
           ("off the curve and tampered", off, nonce, bump(cipher, L, R)),
           ("out of range and tampered", point, nonce + R, bump(cipher, L, 1 if cipher[L] < R - 1 else -1))]
    res = []
    for lab, p, k, c in out:
        sec = p if secret is None else secret
        m, st = decrypt(h, sec, k, c, L, tested=p)
        res.append((lab, p, k, c, m, st))
    assert sorted({r[5] for r in res}) == [OK, POINT, RANGE, TAG]
    return res


# ------------------------------------------------------------------------------------------ memory forms
mont_words = S.mont_words
canon_words = S.canon_words
point_words = S.point_words


def pack_words(rows) -> np.ndarray:
    """[[v, ...], ...] -> [n, k, 4]: each integer as its Montgomery element, v >= r as that of v - r plus r (not canonical)"""
    return np.stack([np.stack([mont_words(v) for v in row]) for row in rows])


def pack_points(points) -> np.ndarray:
    return np.stack([point_words(p) for p in points])


def key_words(vk, montgomery: bool) -> np.ndarray:
    return S.scalar_words([vk], montgomery)[0]
