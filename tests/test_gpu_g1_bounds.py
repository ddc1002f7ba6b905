"""The XYZZ group law of csrc/ec.hip.h AT THE BOUNDS OF ITS POINT CLASS, through pm_test_g1_raw_op (raw limbs in and out).

A point in registers or memory obeys X (1+, <10), Y (1+, <5), ZZ, ZZZ (1, <2); "every routine both accepts and produces" it.
Whole MSMs on random data never come near those limits, so here curve points are lifted to XYZZ with a random z and then pushed
to the edge of the class: X = x ZZ + k p for k up to 9, Y = y ZZZ + k p for k up to 4, ZZ / ZZZ also >= p.  Expected values are
affine sums / multiples from the oracle (oracle.g1_add, oracle.g1_mul) after converting the device output with x = X / ZZ,
y = Y / ZZZ in Python integers; the output limbs are also compared with the big-integer model (oracle/fe_model.py), which
checks every annotated intermediate of ec.hip.h against its (B, V) comment on the way.  Exact integer equality throughout.

What a pass means: the formulas, the exceptional-case detection and the bound bookkeeping of the shared inline routines hold
at the class limits on this device.  It does NOT check the code generated for the production kernels that inline them."""
import random

import numpy as np
import pytest

from oracle import bigint_oracle as B
from oracle import fe_model as M
from oracle.cpu_oracle import ints_to_limbs, limbs_to_ints

pytestmark = pytest.mark.gpu

P = B.P_MOD
F = M.FP
RP = F.RADIX % P
DOUBLE_AFFINE, DOUBLE, MADD, ADD, MUL_SMALL, HALF_DOUBLE, HALF_ADD = range(7)
INF = M.xyzz_identity()


@pytest.fixture(autouse=True)
def clean_log():
    M.VIOLATIONS.clear()
    yield
    M.VIOLATIONS.clear()


@pytest.fixture(scope="module")
def points(oracle):
    """three dozen curve points as affine integer pairs"""
    xy = oracle.g1_bases_arith(ints_to_limbs([0x1234567], 4)[0], ints_to_limbs([0xabcdef123456789], 4)[0], 36)
    v = limbs_to_ints(oracle.fp_from_mont(xy.reshape(-1, 6)))
    return [(v[2 * i], v[2 * i + 1]) for i in range(36)]


class Ref:
    """affine sums and multiples from the C oracle, on integer pairs (None = the identity)"""

    def __init__(self, oracle):
        self.o = oracle

    def _mont(self, pt):
        return self.o.fp_to_mont(ints_to_limbs(list(pt), 6)).reshape(12)

    def _ints(self, xy):
        return tuple(limbs_to_ints(self.o.fp_from_mont(xy.reshape(2, 6))))

    def mul(self, pt, k):
        if pt is None or k == 0:
            return None
        return self._ints(self.o.g1_mul(self._mont(pt), ints_to_limbs([k], 4)[0]))

    def add(self, a, b):
        if a is None or b is None:
            return b if a is None else a
        if a[0] == b[0]:
            return self.mul(a, 2) if a[1] == b[1] else None
        return self._ints(self.o.g1_add(self._mont(a), self._mont(b)))


@pytest.fixture(scope="module")
def ref(oracle):
    return Ref(oracle)


def neg(pt):
    return (pt[0], P - pt[1])


def lift(pt, rng, kx=None, ky=None):
    """affine -> XYZZ in the device Montgomery form at a random place of the class: random z, ZZ / ZZZ sometimes >= p, X = x ZZ + kx p
    (kx <= 9), Y = y ZZZ + ky p (ky <= 4), in the most redundant limb form the class (1+) allows or normalised"""
    if pt is None:
        return INF
    z = rng.randrange(1, P)
    zz, zzz = z * z % P, z * z * z % P
    kx = rng.randrange(10) if kx is None else kx
    ky = rng.randrange(5) if ky is None else ky
    form = (lambda v: M.most_redundant(F, v, 1, True)) if rng.random() < 0.7 else (lambda v: M.limbs_of(F, v))
    up = lambda v: v + P if rng.random() < 0.5 else v              # noqa: E731  (1, <2) members >= p
    r = (form(pt[0] * zz * RP % P + kx * P), form(pt[1] * zzz * RP % P + ky * P), M.limbs_of(F, up(zz * RP % P)),
         M.limbs_of(F, up(zzz * RP % P)), False)
    assert M.point_in_class(r)
    return r


def affine_operand(pt, ky):
    """the madd operand at its class x2 (<=1, <1), y2 (<=3, <3): y2 = y + ky p, unnormalised"""
    return (M.limbs_of(F, pt[0] * RP % P), M.most_redundant(F, pt[1] * RP % P + ky * P, 3), F.M[:], F.M[:], False)


def pack(pts):
    out = np.zeros((len(pts), 57), np.uint32)
    for i, p in enumerate(pts):
        out[i, :56] = np.array(p[0] + p[1] + p[2] + p[3], dtype=np.uint64).astype(np.uint32)
        out[i, 56] = 1 if p[4] else 0
    return out


def unpack(arr):
    rows = arr.tolist()
    return [(r[0:14], r[14:28], r[28:42], r[42:56], bool(r[56])) for r in rows]


def check(got, want, model=None):
    """in the class the header promises; the expected affine point; ZZ^3 = ZZZ^2; and the model's limbs"""
    assert M.point_in_class(got)
    assert M.to_affine(got) == want
    if got[4]:
        assert not any(got[0] + got[1] + got[2] + got[3])
    else:
        zz, zzz = M.value_of(F, got[2]), M.value_of(F, got[3])
        assert (zz ** 3 * F.RINV - zzz ** 2) % P == 0               # device Montgomery form: (zz / R')^3 = (zzz / R')^2
    if model is not None:
        assert got[4] == model[4] and (got[4] or [list(c) for c in model[:4]] == [list(c) for c in got[:4]])


def test_double(ctx, ref, points):
    rng = random.Random(1)
    ins = [lift(pt, rng, kx, ky) for pt in points for kx, ky in ((9, 4), (0, 0), (None, None))] + [INF]
    want = [ref.mul(pt, 2) for pt in points for _ in range(3)] + [None]
    for a, w, g in zip(ins, want, unpack(ctx.g1_raw_op(DOUBLE, pack(ins)))):
        check(g, w, M.xyzz_double(a))
    fin = ins[:-1]
    for a, w, g in zip(fin, want, unpack(ctx.g1_raw_op(DOUBLE_AFFINE, pack(fin)))):
        m = M.xyzz_double_affine(a[0], a[1])                        # 2 (X, Y) read as an affine point: not on the curve, the class still holds
        assert M.point_in_class(g) and [list(c) for c in m[:4]] == [list(c) for c in g[:4]] and not g[4]
    aff = [(M.most_redundant(F, pt[0] * RP % P + kx * P, 1, True), M.most_redundant(F, pt[1] * RP % P + ky * P, 1, True), F.M[:], F.M[:], False)
           for pt in points for kx, ky in ((9, 4), (0, 0), (3, 1))]
    for a, w, g in zip(aff, want, unpack(ctx.g1_raw_op(DOUBLE_AFFINE, pack(aff)))):
        check(g, w, M.xyzz_double_affine(a[0], a[1]))
    assert not M.VIOLATIONS, sorted(set(M.VIOLATIONS))[:3]


def _pairs(points, rng, n):
    """(a, b, expected-operands): ordinary sums and every exceptional case, the two representations of P differing in z and k"""
    out = []
    for i in range(n):
        p, q = points[i % len(points)], points[(7 * i + 3) % len(points)]
        kind = i % 8
        if kind == 0:
            q = p                                                    # P + P: U2 - U1 is a non-zero multiple of p
        elif kind == 1:
            q = neg(p)                                               # P + (-P)
        elif kind == 2:
            q = None                                                 # P + inf
        elif kind == 3:
            p = None                                                 # inf + P
        elif kind == 4 and i % 16 == 4:
            p = q = None                                             # inf + inf
        out.append((p, q))
    return out


def test_add(ctx, ref, points):
    rng = random.Random(2)
    pq = _pairs(points, rng, 400)
    a = [lift(p, rng, 9 if i % 3 == 0 else None, 4 if i % 3 == 0 else None) for i, (p, _) in enumerate(pq)]
    b = [lift(q, rng, 9 if i % 5 == 0 else None, 4 if i % 5 == 0 else None) for i, (_, q) in enumerate(pq)]
    got = unpack(ctx.g1_raw_op(ADD, pack(a), pack(b)))
    for (p, q), x, y, g in zip(pq, a, b, got):
        check(g, ref.add(p, q), M.xyzz_add(x, y))
    assert sum(g[4] for g in got) >= 20
    assert not M.VIOLATIONS, sorted(set(M.VIOLATIONS))[:3]


def test_madd(ctx, ref, points):
    rng = random.Random(3)
    pq = [(p, q) for p, q in _pairs(points, rng, 400) if q is not None]
    a = [lift(p, rng, 9 if i % 3 == 0 else None, 4 if i % 3 == 0 else None) for i, (p, _) in enumerate(pq)]
    b = [affine_operand(q, (2, 0, 1)[i % 3] if q[1] + 2 * P < 3 * P else 0) for i, (_, q) in enumerate(pq)]
    got = unpack(ctx.g1_raw_op(MADD, pack(a), pack(b)))
    for (p, q), x, y, g in zip(pq, a, b, got):
        check(g, ref.add(p, q), M.xyzz_madd(x, y[0], y[1]))
    assert sum(g[4] for g in got) >= 10
    assert not M.VIOLATIONS, sorted(set(M.VIOLATIONS))[:3]


def test_mul_small(ctx, ref, points):
    rng = random.Random(4)
    ks = list(range(18)) + [31, 32, 255, 1000, 65537]
    ins = [lift(points[i % len(points)], rng, 9 if i % 2 else None, 4 if i % 2 else None) for i in range(len(ks))] + [INF]
    ks.append(5)
    b = np.zeros((len(ks), 57), np.uint32)
    b[:, 0] = ks
    for i, (a, k, g) in enumerate(zip(ins, ks, unpack(ctx.g1_raw_op(MUL_SMALL, pack(ins), b)))):
        check(g, None if a[4] else ref.mul(points[i % len(points)], k), M.xyzz_mul_small(a, k) if k < 40 else None)
    assert not M.VIOLATIONS, sorted(set(M.VIOLATIONS))[:3]


def test_half_routines_under_divergence(ctx, ref, points):
    """Whole waves, one point per lane pair, neighbouring pairs on different branches in one launch (ordinary addition, doubling,
    cancellation, an infinite operand on either side): fp_pair_swap (DPP) runs under divergence.  The results are those of
    xyzz_add / xyzz_double on the same inputs -- from the device and from the oracle -- after conversion to affine."""
    rng = random.Random(5)
    pq = _pairs(points, rng, 192)                                    # 192 pairs = 6 waves of 32 pairs, the branch changes from pair to pair
    a = [lift(p, rng, 9 if i % 3 == 0 else None, 4 if i % 3 == 0 else None) for i, (p, _) in enumerate(pq)]
    b = [lift(q, rng, 9 if i % 5 == 0 else None, 4 if i % 5 == 0 else None) for i, (_, q) in enumerate(pq)]
    half = unpack(ctx.g1_raw_op(HALF_ADD, pack(a), pack(b)))
    full = unpack(ctx.g1_raw_op(ADD, pack(a), pack(b)))
    for (p, q), h, g in zip(pq, half, full):
        check(h, ref.add(p, q))
        assert M.to_affine(h) == M.to_affine(g)
    ins = [lift(p if i % 4 else None, rng, 9 if i % 3 == 0 else None, 4 if i % 3 == 0 else None) for i, (p, _) in enumerate(pq)]
    ins = [INF if x[4] else x for x in ins]
    half = unpack(ctx.g1_raw_op(HALF_DOUBLE, pack(ins)))
    full = unpack(ctx.g1_raw_op(DOUBLE, pack(ins)))
    for i, ((p, _), x, h, g) in enumerate(zip(pq, ins, half, full)):
        check(h, None if x[4] else ref.mul(p, 2))
        assert M.to_affine(h) == M.to_affine(g)
        assert h[4] or (h[0], h[2], h[3]) == (g[0], g[2], g[3])     # X3, ZZ3, ZZZ3 come from the same products: the same limbs


def test_closure(ctx, ref, points):
    """every routine accepts what every routine produces: outputs fed back as inputs for a few rounds, starting from the class
    maximum (not a curve point: the bound bookkeeping does not care) and from curve points at the class edge"""
    rng = random.Random(6)
    top = (M.all_max(F, 1, 10, True), M.all_max(F, 1, 5, True), M.all_max(F, 1, 2), M.all_max(F, 1, 2), False)
    pts = points[:15]
    a = [top] + [lift(p, rng, 9, 4) for p in pts]
    b = [top] + [lift(p, rng, 9, 4) for p in pts[::-1]]
    x2 = [(M.all_max(F, 1, 1), M.all_max(F, 3, 3), F.M[:], F.M[:], False)] + [affine_operand(p, 0 if p[1] + 2 * P >= 3 * P else 2) for p in pts[3:] + pts[:3]]
    want_a, want_b = [None] + pts, [None] + pts[::-1]
    aff = [None] + pts[3:] + pts[:3]
    for _ in range(3):
        a = unpack(ctx.g1_raw_op(ADD, pack(a), pack(b)))
        want_a = [ref.add(p, q) for p, q in zip(want_a, want_b)]
        b = unpack(ctx.g1_raw_op(DOUBLE, pack(b)))
        want_b = [ref.mul(q, 2) for q in want_b]
        a = unpack(ctx.g1_raw_op(MADD, pack(a), pack(x2)))
        want_a = [ref.add(p, q) for p, q in zip(want_a, aff)]
        b = unpack(ctx.g1_raw_op(HALF_ADD, pack(b), pack(a)))
        want_b = [ref.add(q, p) for p, q in zip(want_a, want_b)]
        for i, (x, y) in enumerate(zip(a, b)):
            assert M.point_in_class(x) and M.point_in_class(y)
            if i:
                assert M.to_affine(x) == want_a[i] and M.to_affine(y) == want_b[i]
