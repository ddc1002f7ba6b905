"""The limb-exact CPU model of the device field arithmetic, butterflies and group law (oracle/fe_model.py) -- no GPU, no
library.  Three claims: every modelled routine computes what plain integers say; a walk of dft8 / dft4 / ec.hip.h with the
worst members of the classes their call sites document wraps no 32- or 64-bit intermediate, breaks no documented
precondition and leaves no annotated class; and the detector does fire when a bound is exceeded on purpose.
Every comparison is exact integer equality."""
import itertools
import random

import pytest

from oracle import bigint_oracle as B
from oracle import fe_model as M

FIELDS = [M.FR, M.FP]
SUB_K = {"fr": (2, 3, 5, 9), "fp": (2, 3, 5, 6, 8, 11)}


@pytest.fixture(autouse=True)
def clean_log():
    M.VIOLATIONS.clear()
    yield
    M.VIOLATIONS.clear()


def val(f, l):
    return M.value_of(f, l)


def worst(f, Bl, V, plus=False, n_random=0):
    return M.class_members(f, Bl, V, plus, n_random, seed=7)


# ---------------------------------------------------------------------------- the generator itself
@pytest.mark.parametrize("f", FIELDS, ids=repr)
def test_class_generator(f):
    for Bl, V, plus in ((1, 1, False), (1, 2, False), (1, 10, True), (4, 13, False), (3, 6, False), (5, 40, False)):
        mem = M.class_members(f, Bl, V, plus, 50, seed=1)
        lim = Bl * (1 << f.W) + (f.SLACK if plus else 0)
        assert all(l == lim - 1 for l in mem[0][:-1])                # every limb at its maximum ...
        assert val(f, mem[0]) < V * f.mod <= val(f, mem[0]) + (1 << (f.W * (f.N - 1)))   # ... the top as large as V m allows
        assert val(f, mem[1]) == V * f.mod - 1 == val(f, mem[2])
        if Bl > 1:
            assert mem[1] != mem[2] and max(mem[1][:-1]) >= 1 << f.W   # the redundant form really is redundant
        for i in range(f.N - 1):                                     # ... and maximally so: no limb can take another 2^W
            assert mem[1][i + 1] == 0 or mem[1][i] + (1 << f.W) >= lim
        vals = {val(f, l) for l in mem}
        assert {0, 1, f.mod - 1} <= vals and ((V == 1) or {f.mod, 2 * f.mod - 1} <= vals)
        assert all(M.in_class(f, l, Bl, V, plus) for l in mem)
        assert mem == M.class_members(f, Bl, V, plus, 50, seed=1)    # seeded
    assert not M.VIOLATIONS


# ---------------------------------------------------------------------------- field routines against plain integers
@pytest.mark.parametrize("f", FIELDS, ids=repr)
def test_add_sub_norm(f):
    for K in SUB_K[f.name]:
        a_s = worst(f, 4, 30, True, 20)
        # the subtrahend at the limit the routine documents: limbs 2^(W+1) - 2, value < (K - 1) m
        top = (1 << (f.W + 1)) - 2
        b_s = [l for l in worst(f, 2, K - 1, False, 20) if max(l[:-1]) <= top] + [M.most_redundant(f, (K - 1) * f.mod - 1, 2)]
        b_s = [l for l in b_s if max(l[:-1]) <= top]
        edge = [top] * (f.N - 1)
        edge.append(((K - 1) * f.mod - 1 - val(f, edge)) >> (f.W * (f.N - 1)))
        b_s.append(edge)
        for a, b in itertools.product(a_s, b_s):
            d = M.fe_sub(f, K, 1, a, b)
            assert val(f, d) == val(f, a) - val(f, b) + K * f.mod
            assert max(d) < max(a) + (1 << (f.W + 1)) + (1 << f.W) + 1
            s = M.fe_add(f, a, b)
            assert val(f, s) == val(f, a) + val(f, b)
            for x in (d, s):
                n1, n2 = M.fe_norm(f, x), M.fe_norm_full(f, x)
                assert val(f, n1) == val(f, x) == val(f, n2)
                assert max(n1[:-1]) < (1 << f.W) + f.SLACK and max(n2[:-1]) < 1 << f.W
    assert not M.VIOLATIONS, M.VIOLATIONS[:5]


def _product_operands(f):
    """(a, b) pairs of the classes the call sites multiply: the wide operand up to the stated limb bound, against a
    normalised one; and the widest pairs of ec.hip.h / dft8"""
    wide = 5 if f is M.FR else 12
    pairs = list(itertools.product(worst(f, wide, 13, True, 6), worst(f, 1, 2, True, 6)))
    if f is M.FP:
        pairs += list(itertools.product(worst(f, 3, 6, False, 3), worst(f, 4, 13, False, 3)))     # M D, R D
        pairs += list(itertools.product(worst(f, 2, 10, 2, 3), worst(f, 2, 10, 2, 3)))            # U^2
    else:
        pairs += list(itertools.product(worst(f, 4, 5, False, 3), worst(f, 1, 1, False, 3)))      # dft8: x7 w2
    return pairs


@pytest.mark.parametrize("f", FIELDS, ids=repr)
def test_products(f):
    m, ri = f.mod, f.RINV
    pairs = _product_operands(f)
    rng = random.Random(11)
    for a, b in pairs:
        r = M.fe_mul(f, a, b)
        assert val(f, r) % m == val(f, a) * val(f, b) * ri % m and max(r) < 1 << f.W
        assert val(f, r) < val(f, a) * val(f, b) // f.RADIX + m + 1
    for a, b in pairs[::3]:
        c, d = rng.choice(pairs)
        r0, r1 = M.fe_mul2(f, a, b, c, d)
        assert (r0, r1) == (M.fe_mul(f, a, b), M.fe_mul(f, c, d))
        e, g = rng.choice(pairs)
        assert M.fe_mul3(f, a, b, c, d, e, g) == [r0, r1, M.fe_mul(f, e, g)]
    squares = worst(f, 2, 10, 2, 10) + worst(f, 1, 13, True, 10) + (worst(f, 3, 6, False, 10) if f is M.FP else [])   # U, P, M
    for a in squares:
        r = M.fe_sqr(f, a)
        assert r == M.fe_mul(f, a, a) and val(f, r) % m == val(f, a) ** 2 * ri % m
        b = rng.choice(squares)
        assert M.fe_sqr2(f, a, b) == [r, M.fe_sqr(f, b)]
    for a in worst(f, 5 if f is M.FR else 12, 13, True, 10):
        for b0 in (0, 1, 32, f.MASK, rng.randrange(1 << f.W)):
            r = M.fe_mul_limb(f, a, b0)
            assert val(f, r) % m == val(f, a) * b0 * ri % m and val(f, r) < 2 * m and max(r) < 1 << f.W
            assert r == M.fe_mul(f, a, [b0] + [0] * (f.N - 1))
    assert not M.VIOLATIONS, M.VIOLATIONS[:5]


@pytest.mark.parametrize("f", FIELDS, ids=repr)
def test_mma2(f):
    """(a0 b0 + c0 d0) / R' with one reduction, at the classes of its two call sites (R D + nY1 PPP, R D + nS1 PPP) and
    at the documented limit Ba Bb + Bc Bd < 17 (Fp) / the fe_mul limit shared between the two products (Fr)"""
    m, ri = f.mod, f.RINV
    if f is M.FP:
        shapes = [((1, 8, True), (4, 13, False), (3, 6, False), (1, 2, False)),      # xyzz_madd
                  ((1, 5, True), (4, 13, False), (3, 3, False), (1, 2, False)),      # xyzz_add
                  ((3, 6, False), (4, 13, False), (4, 13, False), (1, 2, True))]     # 12 + 4 = 16 < 17
    else:
        shapes = [((1, 8, True), (3, 13, False), (2, 6, False), (1, 2, False))]      # 3 + 2 = 5 < 6
    for sa, sb, sc, sd in shapes:
        for a, b, c, d in itertools.product(*(worst(f, *s, n_random=2)[:2] + worst(f, *s, n_random=2)[-2:] for s in (sa, sb, sc, sd))):
            r0, r1 = M.fe_mma2(f, a, b, c, d, c, d)
            assert val(f, r0) % m == (val(f, a) * val(f, b) + val(f, c) * val(f, d)) * ri % m
            assert max(r0) < 1 << f.W and r1 == M.fe_mul(f, c, d)
    assert not M.VIOLATIONS, M.VIOLATIONS[:5]


@pytest.mark.parametrize("f", FIELDS, ids=repr)
def test_reduce_weak(f):
    """any limbs < 2^32 with value < 2^(W N): same residue, normalised, value < m + m / 2^16 (Fr), m + m / 2^5 (Fp)"""
    rng = random.Random(5)
    cases = worst(f, 6, 40, False, 50) + worst(f, 4, 5, True, 20) + worst(f, 1, 2, False, 10)
    for it in range(300):                                            # limbs up to 2^32 - 1, value up to 2^(W N) - 1
        l = [M.M32 - (rng.randrange(1 << rng.randrange(1, 32)) if it % 2 else 0) for _ in range(f.N - 1)]
        room = (f.RADIX - 1 - val(f, l)) >> (f.W * (f.N - 1))
        l.append(room if it % 3 else rng.randint(0, room))
        cases.append(l)
    for x in cases:
        r = M.fe_reduce_weak(f, x)
        assert val(f, r) % f.mod == val(f, x) % f.mod and max(r) < 1 << f.W
        assert val(f, r) < f.mod + (f.mod >> (16 if f is M.FR else 5))
    assert not M.VIOLATIONS, M.VIOLATIONS[:5]


@pytest.mark.parametrize("f", FIELDS, ids=repr)
def test_boundary_and_constants(f):
    m = f.mod
    sat = lambda v: [(v >> (32 * j)) & M.M32 for j in range(f.NS)]   # noqa: E731
    for x in [0, 1, 2, m - 1, m - 2, (m - 1) // 2, (1 << 200) % m] + [random.Random(3).randrange(m) for _ in range(50)]:
        assert M.fe_unpack(f, sat(x)) == M.limbs_of(f, x)
        assert M.fe_pack_raw(f, M.limbs_of(f, x)) == sat(x)
        forms = [M.limbs_of(f, x), M.most_redundant(f, x, 4), M.limbs_of(f, x + m), M.most_redundant(f, x + m, 4, True)]
        for l in forms:
            assert M.fe_canon_pack(f, l) == sat(x)
    for v in (m, 2 * m - 1):
        for l in (M.limbs_of(f, v), M.most_redundant(f, v, 2), M.most_redundant(f, v, 7, True)):
            assert M.fe_canon_pack(f, l) == sat(v % m)
    for e in (0, 1, f.W, f.W * f.N, 2 * f.W * f.N - 32 * f.NS, 2 * f.W * f.N):
        assert M.fe_pow2(f, e) == M.limbs_of(f, pow(2, e, m))
    assert val(f, M.fe_one(f)) == f.RADIX % m
    for K in SUB_K[f.name]:
        assert val(f, M.sub_bias(f, K, 1)) == K * m and val(f, M.k_mod(f, K)) == K * m
    assert val(f, M.rbar(f)) == f.RADIX - m
    assert not M.VIOLATIONS, M.VIOLATIONS[:5]


def test_mul_split_through_the_recorder():
    rng = random.Random(9)
    for G, D in ((5, 6), (1, 2)):
        for x in worst(M.FR, 5, 40, False, 20) + [[(6 << 29) - 1] * 9]:
            w = rng.randrange(B.R_MOD)
            r = M.fe_mul_split(x, M.rows_of(w, G, D), G, D)
            assert val(M.FR, r) % B.R_MOD == val(M.FR, x) * w * M.FR.RINV % B.R_MOD
    assert not M.VIOLATIONS, M.VIOLATIONS[:5]


# ---------------------------------------------------------------------------- butterflies
W8 = pow(B.ROOT_OF_UNITY, 1 << 29, B.R_MOD)                          # a primitive 8th root of unity


def _tw(k):
    return M.limbs_of(M.FR, pow(W8, k, B.R_MOD) * M.FR.RADIX % B.R_MOD)      # Montgomery form, canonical limbs


def _dft_inputs(n, n_random):
    """worst members first: x0 of (1+, <24), the others of (1, <2), in every combination of the two worst forms"""
    x0s = worst(M.FR, 1, 24, True, n_random)
    ps = worst(M.FR, 1, 2, False, n_random)
    out = [[a] + [p] * (n - 1) for a in x0s[:3] for p in ps[:3]]
    rng = random.Random(21)
    out += [[rng.choice(x0s)] + [rng.choice(ps) for _ in range(n - 1)] for _ in range(40)]
    return out


def test_dft8_walk():
    r = B.R_MOD
    for x in _dft_inputs(8, 10):
        y = M.dft8(x, _tw(1), _tw(2), _tw(3))
        v = [val(M.FR, l) for l in x]
        for p in range(8):
            j = int(f"{p:03b}"[::-1], 2)
            assert val(M.FR, y[p]) % r == sum(v[n] * pow(W8, j * n, r) for n in range(8)) % r, p
            assert M.in_class(M.FR, y[p], 5, 40)
    assert not M.VIOLATIONS, sorted(set(M.VIOLATIONS))[:5]


def test_dft4_walk():
    r, w4 = B.R_MOD, pow(W8, 2, B.R_MOD)
    for x in _dft_inputs(4, 10):
        y = M.dft4(*x, _tw(2))
        v = [val(M.FR, l) for l in x]
        for j in range(4):
            assert val(M.FR, y[j]) % r == sum(v[n] * pow(w4, j * n, r) for n in range(4)) % r, j
            assert M.in_class(M.FR, y[j], 5, 40)
    assert not M.VIOLATIONS, sorted(set(M.VIOLATIONS))[:5]


# ---------------------------------------------------------------------------- group law
P_MOD = B.P_MOD
RP = M.FP.RADIX % P_MOD


def lift(P, z, kx=0, ky=0, redundant=False):
    """affine P -> XYZZ in the device Montgomery form with ZZ = z^2, ZZZ = z^3, X = x ZZ + kx p, Y = y ZZZ + ky p"""
    x, y = P
    zz, zzz = z * z % P_MOD, z * z * z % P_MOD
    form = (lambda v, plus: M.most_redundant(M.FP, v, 1, plus)) if redundant else (lambda v, plus: M.limbs_of(M.FP, v))
    return (form(x * zz * RP % P_MOD + kx * P_MOD, True), form(y * zzz * RP % P_MOD + ky * P_MOD, True),
            M.limbs_of(M.FP, zz * RP % P_MOD), M.limbs_of(M.FP, zzz * RP % P_MOD), False)


def affine_operand(P, ky=0):
    return M.limbs_of(M.FP, P[0] * RP % P_MOD), M.most_redundant(M.FP, P[1] * RP % P_MOD + ky * P_MOD, 3)


POINTS = [B.g1_mul(k, B.G1_GEN) for k in (1, 2, 3, 5, 0x1234567, B.R_MOD - 1)]


def check_point(got, want):
    assert M.point_in_class(got)
    assert M.to_affine(got) == want
    if not got[4]:
        zz, zzz = val(M.FP, got[2]), val(M.FP, got[3])
        assert (zz ** 3 * M.FP.RINV - zzz ** 2) % P_MOD == 0         # ZZ^3 = ZZZ^2 in Montgomery form: zz^3 / R'^2 = zzz^2 / R'


def test_group_law_against_affine_addition():
    rng = random.Random(33)
    for P in POINTS:
        for Q in POINTS:
            for _ in range(2):
                a = lift(P, rng.randrange(1, P_MOD), rng.randrange(10), rng.randrange(5), rng.random() < 0.5)
                b = lift(Q, rng.randrange(1, P_MOD), rng.randrange(10), rng.randrange(5), rng.random() < 0.5)
                if not (M.point_in_class(a) and M.point_in_class(b)):
                    continue
                check_point(M.xyzz_add(a, b), B.g1_add(P, Q))
                check_point(M.xyzz_add(a, lift(B.g1_neg(Q), 7, 3, 2)), B.g1_add(P, B.g1_neg(Q)))
                check_point(M.xyzz_madd(a, *affine_operand(Q, rng.randrange(3))), B.g1_add(P, Q))
                check_point(M.xyzz_madd(a, *affine_operand(B.g1_neg(Q), 2 if B.g1_neg(Q)[1] < P_MOD // 2 else 0)),
                            B.g1_add(P, B.g1_neg(Q)))
        a = lift(P, rng.randrange(1, P_MOD), 8, 3, True)
        check_point(M.xyzz_double(a), B.g1_add(P, P))
        check_point(M.xyzz_mul_small(a, 11), B.g1_mul(11, P))
        inf = M.xyzz_identity()
        check_point(M.xyzz_add(a, inf), P)
        check_point(M.xyzz_add(inf, a), P)
        check_point(M.xyzz_add(inf, inf), None)
        check_point(M.xyzz_double(inf), None)
        check_point(M.xyzz_madd(inf, *affine_operand(P, 2)), P)
    assert not M.VIOLATIONS, sorted(set(M.VIOLATIONS))[:5]


def test_double_affine_against_affine_doubling():
    for P in POINTS:
        for kx, ky in ((0, 0), (9, 4), (5, 2)):
            x = M.most_redundant(M.FP, P[0] * RP % P_MOD + kx * P_MOD, 1, True)
            y = M.most_redundant(M.FP, P[1] * RP % P_MOD + ky * P_MOD, 1, True)
            check_point(M.xyzz_double_affine(x, y), B.g1_add(P, P))
    assert not M.VIOLATIONS, sorted(set(M.VIOLATIONS))[:5]


def test_group_law_walk_at_the_class_bounds():
    """The bound bookkeeping does not need curve points: every coordinate at the two worst members of its class, in every
    combination, through every routine; each annotated intermediate is checked against its (B, V) comment by the model."""
    f = M.FP
    Xs, Ys, Zs = worst(f, 1, 10, True)[:2], worst(f, 1, 5, True)[:2], worst(f, 1, 2)[:2]
    pts = [(X, Y, ZZ, ZZZ, False) for X, Y, ZZ, ZZZ in itertools.product(Xs, Ys, Zs, Zs)]
    x2s, y2s = worst(f, 1, 1)[:2], worst(f, 3, 3)[:2]
    for a in pts:
        assert M.point_in_class(M.xyzz_double(a))
        assert M.point_in_class(M.xyzz_double_affine(a[0], a[1]))
        for x2, y2 in itertools.product(x2s, y2s):
            assert M.point_in_class(M.xyzz_madd(a, x2, y2))
    for a, b in itertools.product(pts, pts[::3]):
        assert M.point_in_class(M.xyzz_add(a, b))
    assert not M.VIOLATIONS, sorted(set(M.VIOLATIONS))[:5]


def test_group_law_closure():
    """every routine accepts what every routine produces: worst outputs fed back for a few rounds stay in the class"""
    f = M.FP
    a = (M.all_max(f, 1, 10, True), M.all_max(f, 1, 5, True), M.all_max(f, 1, 2), M.all_max(f, 1, 2), False)
    b = lift(POINTS[3], 5, 9, 4, True)
    x2, y2 = M.all_max(f, 1, 1), M.all_max(f, 3, 3)
    for _ in range(4):
        a = M.xyzz_add(a, b)
        b = M.xyzz_double(b)
        a = M.xyzz_madd(a, x2, y2)
        b = M.xyzz_add(b, a)
        assert M.point_in_class(a) and M.point_in_class(b)
    assert not M.VIOLATIONS, sorted(set(M.VIOLATIONS))[:5]


@pytest.mark.parametrize("V", [1, 2, 5, 13])
def test_is_zero(V):
    f = M.FP
    assert M.fp_is_zero_product(M.fe_zero(f)) and M.fp_is_zero_product(M.limbs_of(f, P_MOD))
    for v in (P_MOD - 1, P_MOD + 1, 2 * P_MOD - 1, 1):
        assert not M.fp_is_zero_product(M.limbs_of(f, v))
    mem = worst(f, 1, V, True, 20) + [M.most_redundant(f, k * P_MOD, 1, True) for k in range(V)]
    mem += [M.limbs_of(f, k * P_MOD + d) for k in range(V) for d in (-1, 1) if 0 <= k * P_MOD + d < V * P_MOD]
    for l in mem:
        assert M.fp_is_zero_lazy(l) == (val(f, l) % P_MOD == 0)
    assert not M.VIOLATIONS


# ---------------------------------------------------------------------------- the detector fires
def test_negative_control_fe_mul_column_overflow():
    a = [7 * (1 << 29) - 1] * 9
    M.fe_mul(M.FR, a, a)
    assert any("u64 wrap" in v for v in M.VIOLATIONS) and any("precondition" in v for v in M.VIOLATIONS)


def test_negative_control_fe_sub_limb():
    a = M.limbs_of(M.FR, 5)
    b = M.limbs_of(M.FR, 7)
    b[3] = 1 << 30
    M.fe_sub(M.FR, 3, 1, a, b)
    assert any("fe_sub<3,1> precondition" in v for v in M.VIOLATIONS)
    M.VIOLATIONS.clear()
    b[3] = 1 << 31                                                   # past the bias itself: the device limb would wrap
    M.fe_sub(M.FR, 3, 1, a, b)
    assert any("goes negative" in v for v in M.VIOLATIONS)
    M.VIOLATIONS.clear()
    b[3] = (1 << 30) - 2                                             # the limit itself is fine
    M.fe_sub(M.FR, 3, 1, a, b)
    assert not M.VIOLATIONS


def test_negative_control_classes():
    """a value one multiple of m above its class, and a limb one above, are both reported"""
    f = M.FP
    P = POINTS[2]
    a = lift(P, 3, 10, 0)                                            # X = x ZZ + 10 p: outside (1+, <10)
    M.xyzz_double(a)
    assert any("double in X" in v for v in M.VIOLATIONS)
    M.VIOLATIONS.clear()
    x = M.limbs_of(M.FR, 5)
    x[2] = 1 << 29                                                   # a product operand must have limbs < 2^29
    M.dft8([M.limbs_of(M.FR, 1)] + [x] * 7, _tw(1), _tw(2), _tw(3))
    assert any("dft8 in x1" in v for v in M.VIOLATIONS)
    M.VIOLATIONS.clear()
    M.fe_reduce_weak(M.FR, M.limbs_of(M.FR, M.FR.RADIX))
    M.fe_canon_pack(f, M.limbs_of(f, 2 * P_MOD))
    assert len(M.VIOLATIONS) >= 2
