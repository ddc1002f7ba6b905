"""The device field routines, the zero tests of ec.hip.h and the dft8 / dft4 butterflies AT THEIR OPERAND BOUNDS.

pm_test_field_raw_op runs the shared inline routines of csrc/fields.hip.h, csrc/ec.hip.h and csrc/ntt_kernels.hip.h on raw
limbs -- no unpacking, no reduction, no canonical packing -- so the operands are the worst members of the classes the call
sites document (every limb at the top of its class, a value one below V m in its most redundant form, the canonical edges)
and seeded random members, and the result limbs are compared with the big-integer model (oracle/fe_model.py) limb for limb,
then, independently of the model, with plain integer arithmetic and with the result class the routine documents.  Every
comparison is exact integer equality.

What a pass means: the arithmetic and the bound bookkeeping of the shared routines are right on this device.  It does NOT
check the code the compiler generates for a production kernel that inlines them (another instance, other registers, other
scheduling); the end-to-end NTT / MSM parity tests do that."""
import itertools
import random

import numpy as np
import pytest

from oracle import bigint_oracle as B
from oracle import fe_model as M

pytestmark = pytest.mark.gpu

FIELD_ID = {"fr": 0, "fp": 1}
FIELDS = [M.FR, M.FP]
SUB_K = {"fr": (2, 3, 5, 9), "fp": (2, 3, 5, 6, 8, 11)}
(ADD, NORM, NORM_FULL, MUL, SQR, MUL_LIMB, MUL2, MUL3, MMA2, SQR2, REDUCE_WEAK, UNPACK, CANON_PACK, POW2, SPLIT_5_6, SPLIT_1_2,
 ZERO_PRODUCT, ZERO_LAZY, DFT8, DFT4, CANON_LIMBS, INV_INT, INV_DEV) = range(23)   # 20 - 22: tests/test_gpu_field_inv.py
SUB = 32


def val(f, l):
    return M.value_of(f, l)


def run(ctx, f, op, cases, n_out):
    """cases: [case][element][limb] -> [case][element][limb] from the device, one launch"""
    x = np.array(cases, dtype=np.uint64)
    assert x.ndim == 3 and x.shape[2] == f.N and int(x.max()) <= M.M32
    return ctx.field_raw_op(FIELD_ID[f.name], op, x.astype(np.uint32), n_out).tolist()


def members(f, classes, n_random, seed):
    """Operand tuples for a routine whose operands have the given (B, V, plus) classes: the two worst members of every class
    in every combination, every worst / edge member of each class at least once against the others', and n_random seeded
    random tuples."""
    mem = [M.class_members(f, *c, n_random=n_random, seed=seed + 17 * i) for i, c in enumerate(classes)]
    fixed = [m[:len(m) - n_random] for m in mem]
    out = list(itertools.product(*[m[:2] for m in fixed]))
    for i in range(max(len(m) for m in fixed)):
        out.append(tuple(m[i % len(m)] for m in fixed))
        for j in range(len(fixed)):
            for w in (0, 1):
                out.append(tuple(m[i % len(m)] if k == j else m[w] for k, m in enumerate(fixed)))
    out += list(zip(*[m[len(m) - n_random:] for m in mem]))
    return [list(t) for t in out]


@pytest.fixture(autouse=True)
def clean_log():
    M.VIOLATIONS.clear()
    yield
    M.VIOLATIONS.clear()


# ---------------------------------------------------------------------------- sums, differences, carries
@pytest.mark.parametrize("f", FIELDS, ids=repr)
def test_add_norm(ctx, f):
    cases = members(f, [(4, 30, True), (2, 8, False)], 1500, 1) + members(f, [(1, 10, True), (1, 10, True)], 500, 2)
    got = run(ctx, f, ADD, cases, 1)
    sums = []
    for (a, b), (g,) in zip(cases, got):
        assert g == M.fe_add(f, a, b) and val(f, g) == val(f, a) + val(f, b)
        sums.append([g])
    # any limbs the carry steps admit: up to 2^32 - 1 less the carry that comes in (< 2^(32 - W))
    wide = [[[M.M32 - f.SLACK - (i % 7)] * f.N] for i in range(16)] + [[[M.M32 - f.SLACK] * (f.N - 1) + [5]]]
    for op, fn, lim in ((NORM, M.fe_norm, (1 << f.W) + f.SLACK), (NORM_FULL, M.fe_norm_full, 1 << f.W)):
        cs = sums + wide
        for (a,), (g,) in zip(cs, run(ctx, f, op, cs, 1)):
            assert g == fn(f, a) and val(f, g) == val(f, a) and max(g[:-1]) < lim
    assert not M.VIOLATIONS, M.VIOLATIONS[:3]


def _sub_cases(f, K, n_random):
    """minuend up to (4+, <30); subtrahend up to the limit fe_sub<K,1> documents: limbs 2^(W+1) - 2, value < (K - 1) m"""
    top = (1 << (f.W + 1)) - 2
    edge = [top] * (f.N - 1)
    edge.append(((K - 1) * f.mod - 1 - val(f, edge)) >> (f.W * (f.N - 1)))
    at_top = [top] * (f.N - 1) + [M.sub_bias(f, K, 1)[-1]]            # ... and the top limb at ITS limit, top(K m) - 2
    cm = M.class_members(f, 2, K - 1, False, n_random, seed=K)
    fixed_b = [edge, at_top, M.most_redundant(f, (K - 1) * f.mod - 1, 2)] + cm[:len(cm) - n_random]
    fixed_b = [l for l in fixed_b if max(l[:-1]) <= top]
    rand_b = [l for l in cm[len(cm) - n_random:] if max(l[:-1]) <= top]
    a_s = M.class_members(f, 4, 30, True, n_random, seed=K + 50)
    out = [[a, b] for a in a_s[:len(a_s) - n_random] for b in fixed_b]
    out += [[a, b] for a, b in zip(a_s[len(a_s) - n_random:], rand_b)]
    return out


@pytest.mark.parametrize("f,K", [(f, K) for f in FIELDS for K in SUB_K[f.name]], ids=lambda v: repr(v))
def test_sub(ctx, f, K):
    cases = _sub_cases(f, K, 1500)
    got = run(ctx, f, SUB + K, cases, 1)
    for (a, b), (g,) in zip(cases, got):
        assert g == M.fe_sub(f, K, 1, a, b)
        assert val(f, g) == val(f, a) - val(f, b) + K * f.mod        # no limb wrapped: the integer identity holds exactly
        assert max(g) < max(a) + (1 << (f.W + 1)) + (1 << f.W)
    assert not M.VIOLATIONS, M.VIOLATIONS[:3]


def test_sub_rejects_what_the_library_does_not_instantiate(ctx):
    from plonk_prototype_amd import _lib
    x = np.zeros((1, 2, 9), np.uint32)
    out = np.zeros((1, 1, 9), np.uint32)
    for field, op in ((0, SUB + 4), (0, SUB + 11), (1, SUB + 9), (0, ZERO_LAZY), (1, DFT8), (1, SPLIT_5_6), (0, INV_DEV + 1), (1, 31), (2, ADD)):
        rc = ctx._lib.pm_test_field_raw_op(ctx._h, field, op, x.ctypes.data_as(_lib.u32p), out.ctypes.data_as(_lib.u32p), 1)
        assert rc == _lib.PM_ERR_BAD_ARG, (field, op)


# ---------------------------------------------------------------------------- products
# operand classes of the call sites, per field.  Fr: data up to (5+, .) against a canonical or (1, <2) twiddle (the bound fe_mul
# states is limbs < 6 * 2^29), values with Va Vb <= 70 < R' / r, so that the product is < 2r; Fp: the pairs ec.hip.h multiplies, and the stated limit (< 13 * 2^28 against a normalised one).
PAIRS = {
    "fr": [((5, 40, True), (1, 1, False)), ((4, 5, False), (1, 2, False)), ((1, 2, False), (1, 2, False)), ((5, 35, True), (1, 2, True))],
    "fp": [((1, 10, True), (1, 2, False)), ((3, 6, False), (4, 13, False)), ((2, 10, 2), (1, 2, False)), ((1, 13, True), (1, 2, False)),
           ((3, 3, False), (1, 2, False)), ((12, 13, True), (1, 2, True))],
}
SQUARES = {"fr": [(2, 8, 2), (1, 8, True), (1, 2, False)], "fp": [(2, 10, 2), (3, 6, False), (1, 13, True), (1, 10, True)]}


def _pairs(f, n_random, seed):
    out = []
    for i, cls in enumerate(PAIRS[f.name]):
        out += members(f, list(cls), n_random // len(PAIRS[f.name]), seed + i)
    return out


def _check_product(f, r, total):
    """the class every product routine documents: limbs < 2^W, value < 2m, == total / R' (mod m); and tighter, < total / R' + m"""
    assert max(r) < 1 << f.W and val(f, r) < 2 * f.mod
    assert val(f, r) % f.mod == total * f.RINV % f.mod and val(f, r) * f.RADIX < total + f.mod * f.RADIX


@pytest.mark.parametrize("f", FIELDS, ids=repr)
def test_mul(ctx, f):
    cases = _pairs(f, 2000, 100)
    for (a, b), (g,) in zip(cases, run(ctx, f, MUL, cases, 1)):
        assert g == M.fe_mul(f, a, b)
        _check_product(f, g, val(f, a) * val(f, b))
    assert not M.VIOLATIONS, M.VIOLATIONS[:3]


@pytest.mark.parametrize("f", FIELDS, ids=repr)
def test_sqr_sqr2(ctx, f):
    cases = [c for i, cls in enumerate(SQUARES[f.name]) for c in members(f, [cls], 500, 200 + i)]
    for (a,), (g,) in zip(cases, run(ctx, f, SQR, cases, 1)):
        assert g == M.fe_sqr(f, a)
        _check_product(f, g, val(f, a) ** 2)
    two = [[a[0], b[0]] for a, b in zip(cases, cases[7:] + cases[:7])]
    for (a, b), g in zip(two, run(ctx, f, SQR2, two, 2)):
        assert g == M.fe_sqr2(f, a, b)
        _check_product(f, g[0], val(f, a) ** 2)
        _check_product(f, g[1], val(f, b) ** 2)
    assert not M.VIOLATIONS, M.VIOLATIONS[:3]


@pytest.mark.parametrize("f", FIELDS, ids=repr)
def test_mul_limb(ctx, f):
    rng = random.Random(31)
    wide = (5, 40, True) if f is M.FR else (12, 13, True)
    data = [c[0] for c in members(f, [wide], 1200, 300)] + [c[0] for c in members(f, [(1, 2, False)], 300, 301)]
    b0s = [0, 1, 32, f.MASK, f.MASK - 1, 1 << (f.W - 1)]
    cases = [[a, [b0s[i % 6] if i < 60 else rng.randrange(1 << f.W)] + [0] * (f.N - 1)] for i, a in enumerate(data)]
    for (a, b), (g,) in zip(cases, run(ctx, f, MUL_LIMB, cases, 1)):
        assert g == M.fe_mul_limb(f, a, b[0])
        _check_product(f, g, val(f, a) * b[0])
    assert not M.VIOLATIONS, M.VIOLATIONS[:3]


@pytest.mark.parametrize("f", FIELDS, ids=repr)
def test_mul2_mul3(ctx, f):
    p = _pairs(f, 900, 400)
    two = [a + b for a, b in zip(p, p[11:] + p[:11])]
    for c, g in zip(two, run(ctx, f, MUL2, two, 2)):
        assert g == M.fe_mul2(f, *c)
        _check_product(f, g[0], val(f, c[0]) * val(f, c[1]))
        _check_product(f, g[1], val(f, c[2]) * val(f, c[3]))
    three = [a + b + c for a, b, c in zip(p, p[5:] + p[:5], p[23:] + p[:23])][::2]
    for c, g in zip(three, run(ctx, f, MUL3, three, 3)):
        assert g == M.fe_mul3(f, *c)
        for k in range(3):
            _check_product(f, g[k], val(f, c[2 * k]) * val(f, c[2 * k + 1]))
    assert not M.VIOLATIONS, M.VIOLATIONS[:3]


# fe_mma2's first chain takes two products into one column: Ba Bb + Bc Bd < 17 (Fp; Fr shares fe_mul's 6 between the two)
MMA = {
    "fp": [[(1, 8, True), (4, 13, False), (3, 6, False), (1, 2, False), (1, 2, False), (1, 2, False)],       # xyzz_madd: R D + nY1 PPP | ZZZ1 PPP
           [(1, 5, True), (4, 13, False), (3, 3, False), (1, 2, False), (1, 2, False), (1, 2, False)],       # xyzz_add:  R D + nS1 PPP | z12 PP
           [(3, 6, False), (4, 13, False), (4, 13, False), (1, 2, True), (12, 13, True), (1, 2, True)]],     # the limit: 12 + 4 = 16
    "fr": [[(1, 5, True), (3, 10, False), (2, 6, False), (1, 2, False), (5, 40, True), (1, 1, False)]],      # 3 + 2 = 5
}


@pytest.mark.parametrize("f", FIELDS, ids=repr)
def test_mma2(ctx, f):
    cases = [c for i, cls in enumerate(MMA[f.name]) for c in members(f, cls, 900 // len(MMA[f.name]), 500 + i)]
    for c, g in zip(cases, run(ctx, f, MMA2, cases, 2)):
        assert g == M.fe_mma2(f, *c)
        a0, b0, c0, d0, a1, b1 = (val(f, x) for x in c)
        _check_product(f, g[0], a0 * b0 + c0 * d0)
        _check_product(f, g[1], a1 * b1)
    assert not M.VIOLATIONS, M.VIOLATIONS[:3]


@pytest.mark.parametrize("G,D,op", [(5, 6, SPLIT_5_6), (1, 2, SPLIT_1_2)])
def test_mul_split(ctx, G, D, op):
    """the model of tests/test_fe_mul_split_model.py against the device: data up to the stated bound (limbs < 6 * 2^29), rows
    canonical (as stored) and with every limb at 2^29 - 1 (the column bound)"""
    f, rng = M.FR, random.Random(41)
    data = [c[0] for c in members(f, [(5, 40, True)], 1500, 600)] + [[(6 << 29) - 1] * 9, [(6 << 29) - 1 - i for i in range(9)]]
    groups = (9 + G - 1) // G
    cases, ws = [], []
    for i, x in enumerate(data):
        w = (B.R_MOD - 1, 0, 1)[i] if i < 3 else rng.randrange(B.R_MOD)
        rows = M.rows_of(w, G, D) if i % 50 != 49 else [[f.MASK] * 9] * groups
        cases.append([x] + rows)
        ws.append(w if i % 50 != 49 else None)
    for c, w, (g,) in zip(cases, ws, run(ctx, f, op, cases, 1)):
        assert g == M.fe_mul_split(c[0], c[1:], G, D)
        assert max(g) < 1 << 29 and val(f, g) < 2 * B.R_MOD
        t = sum(val(f, c[0][j * G:(j + 1) * G]) * val(f, c[1 + j]) for j in range(groups))
        assert (val(f, g) << (29 * D)) % B.R_MOD == t % B.R_MOD
        if w is not None:
            assert val(f, g) % B.R_MOD == val(f, c[0]) * w * f.RINV % B.R_MOD        # what fe_mul returns for the same operands
    assert not M.VIOLATIONS, M.VIOLATIONS[:3]


# ---------------------------------------------------------------------------- cheap reduction, boundary, constants
@pytest.mark.parametrize("f", FIELDS, ids=repr)
def test_reduce_weak(ctx, f):
    """classes of its call sites ((<6, <40) butterfly outputs, sums and differences of products) and anything the routine
    admits: limbs < 2^32, value < 2^(W N)"""
    rng = random.Random(5)
    cases = members(f, [(6, 40, False)], 1500, 700) + members(f, [(4, 5, True)], 300, 701) + members(f, [(1, 2, False)], 100, 702)
    for it in range(300):
        l = [M.M32 - (rng.randrange(1 << rng.randrange(1, 32)) if it % 2 else 0) for _ in range(f.N - 1)]
        room = (f.RADIX - 1 - val(f, l)) >> (f.W * (f.N - 1))
        cases.append([l + [room if it % 3 else rng.randint(0, room)]])
    for (x,), (g,) in zip(cases, run(ctx, f, REDUCE_WEAK, cases, 1)):
        assert g == M.fe_reduce_weak(f, x)
        assert val(f, g) % f.mod == val(f, x) % f.mod and max(g) < 1 << f.W
        assert val(f, g) < f.mod + (f.mod >> (16 if f is M.FR else 5))
    assert not M.VIOLATIONS, M.VIOLATIONS[:3]


@pytest.mark.parametrize("f", FIELDS, ids=repr)
def test_unpack_canon_pack_pow2(ctx, f):
    m, rng = f.mod, random.Random(3)
    sat = lambda v: [(v >> (32 * j)) & M.M32 for j in range(f.NS)]   # noqa: E731
    pad = [0] * (f.N - f.NS)
    xs = [0, 1, 2, m - 1, m - 2, (m - 1) // 2, (1 << 200) % m, (1 << (f.W * (f.N - 1))) - 1] + [rng.randrange(m) for _ in range(500)]
    for x, (g,) in zip(xs, run(ctx, f, UNPACK, [[sat(x) + pad] for x in xs], 1)):
        assert g == M.limbs_of(f, x) == M.fe_unpack(f, sat(x))
    # x, x + m (< 2m), m itself and 2m - 1, normalised and unnormalised: the canonical limbs of x mod m
    cases, want = [], []
    for x in xs + [m, 2 * m - 1]:
        forms = [M.limbs_of(f, x), M.most_redundant(f, x, 4), M.most_redundant(f, x, 7, True), M.most_redundant(f, x, 1, True)]
        if x < m:
            forms += [M.limbs_of(f, x + m), M.most_redundant(f, x + m, 4, True), M.most_redundant(f, x + m, 7, True)]
        for l in forms:
            cases.append([l])
            want.append(sat(x % m) + pad)
    for (a,), w, (g,) in zip(cases, want, run(ctx, f, CANON_PACK, cases, 1)):
        assert g == w and g[:f.NS] == M.fe_canon_pack(f, a)
    exps = (f.W * f.N, 2 * f.W * f.N - 32 * f.NS, 64 * f.NS + f.W * f.N)
    for e, (g,) in zip(exps, run(ctx, f, POW2, [[[i] + [0] * (f.N - 1)] for i in range(3)], 1)):
        assert g == M.limbs_of(f, pow(2, e, m)) == M.fe_pow2(f, e)
    assert not M.VIOLATIONS, M.VIOLATIONS[:3]


# ---------------------------------------------------------------------------- zero tests of ec.hip.h
def test_fp_is_zero_product(ctx):
    f, p = M.FP, B.P_MOD
    cases = [([0] * 14, 1), (M.limbs_of(f, p), 1), (M.limbs_of(f, p - 1), 0), (M.limbs_of(f, p + 1), 0), (M.limbs_of(f, 2 * p - 1), 0),
             (M.limbs_of(f, 1), 0), (M.limbs_of(f, 1 << 364), 0)]
    for i in range(14):                                              # one limb off the limbs of 0 and of p, at every position
        for base in ([0] * 14, M.limbs_of(f, p)):
            l = list(base)
            l[i] ^= 1 << (i % 28)
            cases.append((l, 0))
    cases += [(c[0], int(val(f, c[0]) in (0, p))) for c in members(f, [(1, 2, False)], 500, 800)]
    got = run(ctx, f, ZERO_PRODUCT, [[l] for l, _ in cases], 1)
    for (l, want), (g,) in zip(cases, got):
        assert g[0] == want == int(M.fp_is_zero_product(l)) and not any(g[1:]), l


def test_fp_is_zero_lazy(ctx):
    """agrees with value % p == 0 over class members up to V = 13, non-zero multiples of p in redundant limb forms included"""
    f, p = M.FP, B.P_MOD
    cases = []
    for V in (1, 2, 5, 8, 10, 13):
        for Bl, plus in ((1, True), (4, False)):
            cases += [c[0] for c in members(f, [(Bl, V, plus)], 100, 900 + V)]
            for k in range(V):
                cases += [M.limbs_of(f, k * p), M.most_redundant(f, k * p, Bl, plus)]
                cases += [M.most_redundant(f, k * p + d, Bl, plus) for d in (-1, 1) if 0 <= k * p + d < V * p]
    got = run(ctx, f, ZERO_LAZY, [[l] for l in cases], 1)
    n_zero = 0
    for l, (g,) in zip(cases, got):
        want = int(val(f, l) % p == 0)
        n_zero += want
        assert g[0] == want == int(M.fp_is_zero_lazy(l)), (val(f, l) // p, val(f, l) % p)
    assert n_zero >= 100
    assert not M.VIOLATIONS, M.VIOLATIONS[:3]


# ---------------------------------------------------------------------------- butterflies
W8 = pow(B.ROOT_OF_UNITY, 1 << 29, B.R_MOD)                          # a primitive 8th root of unity


def _tw(k, redundant=False):
    """w8^k in the device Montgomery form; canonical limbs, or (1, <2) as a product leaves it"""
    v = pow(W8, k, B.R_MOD) * M.FR.RADIX % B.R_MOD
    return M.limbs_of(M.FR, v + B.R_MOD if redundant and v + B.R_MOD < 1 << 261 else v)


def _dft_cases(n, n_random):
    """x0 of (1+, <24) untwiddled, the others (1, <2) products: the two worst members in every combination (all others equal),
    every edge member, random members"""
    x0s = M.class_members(M.FR, 1, 24, True, n_random, seed=61)
    ps = M.class_members(M.FR, 1, 2, False, n_random, seed=62)
    rng = random.Random(63)
    out = [[a] + [p] * (n - 1) for a in x0s[:len(x0s) - n_random] for p in ps[:len(ps) - n_random]]
    out += [[x0s[i % 2]] + [ps[(i >> (j + 1)) & 1] for j in range(n - 1)] for i in range(1 << n)]
    out += [[rng.choice(x0s)] + [rng.choice(ps) for _ in range(n - 1)] for _ in range(n_random)]
    return out


def test_dft8(ctx):
    f, r = M.FR, B.R_MOD
    cases = [x + [_tw(1, i % 2), _tw(2, i % 3 == 1), _tw(3, i % 2)] for i, x in enumerate(_dft_cases(8, 500))]
    for c, g in zip(cases, run(ctx, f, DFT8, cases, 8)):
        assert g == M.dft8(c[:8], *c[8:])
        v = [val(f, l) for l in c[:8]]
        for p in range(8):
            j = int(f"{p:03b}"[::-1], 2)                             # x[p] = X[bitrev3(p)]
            assert val(f, g[p]) % r == sum(v[n] * pow(W8, j * n, r) for n in range(8)) % r
            assert M.in_class(f, g[p], 5, 40)
    assert not M.VIOLATIONS, sorted(set(M.VIOLATIONS))[:3]


def test_dft4(ctx):
    f, r, w4 = M.FR, B.R_MOD, pow(W8, 2, B.R_MOD)
    cases = [x + [_tw(2, i % 2)] for i, x in enumerate(_dft_cases(4, 1500))]
    for c, g in zip(cases, run(ctx, f, DFT4, cases, 4)):
        assert g == M.dft4(*c)
        v = [val(f, l) for l in c[:4]]
        for j in range(4):
            assert val(f, g[j]) % r == sum(v[n] * pow(w4, j * n, r) for n in range(4)) % r
            assert M.in_class(f, g[j], 5, 40)
    assert not M.VIOLATIONS, sorted(set(M.VIOLATIONS))[:3]
