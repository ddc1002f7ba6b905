"""Big-integer models of the JubJub MSM and of the batch Schnorr check (include/plonk_mi355x.h, pm_jubjub_msm_* and
pm_schnorr_verify_batch_dev) on top of jubjub_model (double-and-add) and schnorr_model: the plain sum of the products, no windows
and no buckets, and the random linear combination W = a G + sum b_i PK_i - sum z_i R_i literally.  Plain Python integers
throughout; nothing here touches the library's arithmetic."""
import os
import random
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jubjub_model as J  # noqa: E402
import schnorr_model as S  # noqa: E402

R, Q = J.R, J.Q
WINDOW_BITS = tuple(range(4, 17))      # what the option "jubjub_msm_window_bits" may force


def _proj(p):
    return (p[0], p[1], 1)


def _affine(acc):
    zi = pow(acc[2], -1, R)
    return acc[0] * zi % R, acc[1] * zi % R


def psum(points):
    """the sum of affine points: the projective law of jubjub_model, one inversion"""
    acc = (0, 1, 1)
    for p in points:
        acc = J._padd(acc, _proj(p))
    return _affine(acc)


def msm(points, scalars):
    """sum s_i P_i, every s_i the integer it is"""
    assert len(points) == len(scalars)
    return psum([J.mul(p, s) for p, s in zip(points, scalars)])


def neg(p):
    return ((R - p[0]) % R, p[1])


def batch_sum(h, g, pks, msgs, sigs, weights):
    """W of the batch check.  An entry that fails a structural test (u >= l, R or PK not a canonical curve point) contributes the
    identity, as the device call has it."""
    a, terms = 0, []
    for pk, m, sig, z in zip(pks, msgs, sigs, weights):
        u, rp = sig[0], (sig[1], sig[2])
        if not 0 <= u < Q or S._point_fault(rp) or S._point_fault(pk):
            continue
        c, _ = S.challenge(h, rp, m)
        a = (a + z * u) % Q
        terms.append(J.mul(pk, z * c % Q))
        terms.append(J.mul(neg(rp), z))
    return psum([J.mul(g, a)] + terms)


def cofactored_ok(w):
    return J.mul(w, 8) == J.IDENTITY


def structural(h, g, pks, msgs, sigs):
    """(reason, index) of the lowest structurally bad entry, or None"""
    for i, (pk, sig) in enumerate(zip(pks, sigs)):
        if not 0 <= sig[0] < Q:
            return S.U_RANGE, i
        if S._point_fault((sig[1], sig[2])):
            return S.R_POINT, i
        if S._point_fault(pk):
            return S.PK_POINT, i
    return None


def digits(k: int, c: int):
    """the signed c-bit windows of the integer 0 <= k < 2^256, ceil(257 / c) of them, as the recoding is documented"""
    out, carry = [], 0
    for w in range((257 + c - 1) // c):
        v = ((k >> (c * w)) & ((1 << c) - 1)) + carry
        carry = 1 if v > (1 << (c - 1)) else 0
        out.append(v - (carry << c))
    assert carry == 0
    return out


# ------------------------------------------------------------------------------------------ the inputs the tests share
_CACHE = {}


def edge_case(n: int):
    """n points and scalars: the edge points of jubjub_model (the identity, (0, -1), (i, 0), a point of order != l) cycled with
    random ones, a duplicate and a pair P, -P among them; the edge scalars first, then random ones -> (points, scalars, the sum)"""
    if n not in _CACHE:
        rng = random.Random(0x4D534D + n)
        edge_p, edge_s = J.edge_points(), J.edge_scalars()
        pts = [edge_p[i % len(edge_p)] if i % 3 != 2 else J.M.curve_point(rng.randrange(R)) for i in range(n)]
        if n >= 3:
            pts[2] = pts[0]                                  # a duplicate
        if n >= 63:
            pts[40] = neg(pts[41])                           # P, -P
        # rotated, so that the big scalars do not all meet the identity and the points of small order
        sc = [edge_s[(i * 7 + 3) % len(edge_s)] if i < 2 * len(edge_s) else rng.randrange(R) for i in range(n)]
        if n >= 63:
            sc[40] = sc[41]                                  # ... and with one scalar they cancel
        _CACHE[n] = (pts, sc, msm(pts, sc))
    return _CACHE[n]
