"""The plane-major exchanges of the radix-4 first and single pass kernels of even S (csrc/ntt_kernels4.hip.h; the passes
that read the wide form keep the Stockham exchange, as those of odd S do), on the CPU: the index maps through the
library's pure-host hook pm_test_ntt_exchange_map (the constexpr functions the kernels index with), a model of the LDS
banks, and the consumer-side step-1 products through the limb-exact model of oracle/fe_model.py.

Map: thread tau of step s owns the Stockham butterfly g_s(tau), writes X[t] to plane t at its own place and reads, at the
next step, the four elements that hold the logical positions u'' + m U.  Banks (per wave64 instruction, lanes in fixed
groups, one LDS cycle per group when no two distinct addresses of a group share a bank): a 16-byte store is served in 8
groups of 8 consecutive lanes over 32 banks of 4 bytes, a 16-byte load in the four 16-lane sets below over 64 banks, a
4-byte access in two groups of 32 lanes over 32 banks.  Limbs 0-7 of an element live in two arrays of 16 bytes per
element, limb 8 in an array of 4 bytes per element; all three start at multiples of 256 bytes."""
import ctypes as C
import functools
import random

import pytest

from oracle import bigint_oracle as B
from oracle import fe_model as F

FR = F.FR
NONE = 0xFFFFFFFF
# every (S, LT) of even S >= 4 the library instantiates: single passes (in wave order), then the multi-pass tiles (a first pass
# writes u-fast); both orders are walked for all of them
SHAPES = [(4, 0), (6, 0), (8, 0), (10, 0), (6, 5), (6, 4), (8, 3), (8, 2), (10, 1), (10, 2)]
STAYS = [(2, 0), (3, 0), (5, 0), (7, 0), (9, 0), (5, 6), (7, 4), (9, 2), (9, 1)]      # single-step and radix-2-tailed passes

_HALF = [list(range(0, 4)) + list(range(12, 16)) + list(range(20, 28)), list(range(4, 12)) + list(range(16, 20)) + list(range(28, 32))]
READ_B128 = _HALF + [[l + 32 for l in g] for g in _HALF]
WRITE_B128 = [list(range(8 * i, 8 * i + 8)) for i in range(8)]
B32 = [list(range(32)), list(range(32, 64))]


@functools.lru_cache(maxsize=None)
def _maps(S, LT, ufast):
    """[step][tid] -> (butterfly, column, writes, reads, digit, uniform)"""
    from plonk_prototype_amd import _lib
    lib = _lib.load()
    out = (C.c_uint32 * 12)()
    steps = []
    for s in range(S // 2):
        rows = []
        for tid in range(1 << (S - 2 + LT)):
            assert lib.pm_test_ntt_exchange_map(S, LT, ufast, s, tid, out) == 0
            v = list(out)
            rows.append((v[0], v[1], tuple(v[2:6]), tuple(v[6:10]), v[10], v[11]))
        steps.append(rows)
    return steps


def _cases():
    return [(S, LT, uf) for S, LT in SHAPES for uf in (0, 1)]


def test_the_other_shapes_keep_the_stockham_exchange():
    from plonk_prototype_amd import _lib
    out = (C.c_uint32 * 12)()
    for S, LT in STAYS:
        assert _lib.load().pm_test_ntt_exchange_map(S, LT, 0, 0, 0, out) == _lib.PM_ERR_BAD_ARG
    assert _lib.load().pm_test_ntt_exchange_map(10, 1, 0, 5, 0, out) == _lib.PM_ERR_BAD_ARG      # no such step
    assert _lib.load().pm_test_ntt_exchange_map(10, 1, 0, 0, 512, out) == _lib.PM_ERR_BAD_ARG    # no such thread


@pytest.mark.parametrize("S,LT,ufast", _cases())
def test_every_read_returns_the_stockham_element(S, LT, ufast):
    R, T, U = 1 << S, 1 << LT, 1 << (S - 2)
    steps = _maps(S, LT, ufast)
    last = S // 2 - 1
    for s, rows in enumerate(steps):
        nsp = 1 << (2 * s)
        for tid, (u, c, wr, rd, digit, _) in enumerate(rows):
            assert digit == u & (nsp - 1)
            assert (wr == (NONE,) * 4) == (s == last) and (rd == (NONE,) * 4) == (s == 0)
            if s in (0, last):                                   # the HBM side: the thread order of the Stockham kernel
                tau, col = (tid % U, tid // U) if (ufast and s == last) else (tid >> LT, tid & (T - 1))
                assert (u, c) == (tau, col)
        assert sorted((u, c) for u, c, *_ in rows) == [(u, c) for u in range(U) for c in range(T)]
        if s == last:
            break
        tile = {}
        for u, c, wr, _, digit, _ in rows:
            for t in range(4):
                assert wr[t] not in tile and wr[t] < R * T
                tile[wr[t]] = (c, 4 * (u - digit) + digit + t * nsp)          # Stockham's position of X[t]
        assert len(tile) == R * T                                               # a bijection onto the tile
        for u, c, _, rd, _, _ in steps[s + 1]:
            for m in range(4):
                assert tile[rd[m]] == (c, u + m * U)


@pytest.mark.parametrize("S,LT,ufast", _cases())
def test_step1_digit_is_the_waves(S, LT, ufast):
    steps = _maps(S, LT, ufast)
    uniform = (64 >> LT) <= ((1 << S) >> 4) and not (ufast and S == 4)
    assert all(r[5] == (1 if uniform and s == 1 else 0) for s, rows in enumerate(steps) for r in rows)
    if uniform:
        digits = [r[4] for r in steps[1]]
        for w0 in range(0, len(digits), 64):
            assert len(set(digits[w0:w0 + 64])) == 1
        assert set(digits) == {0, 1, 2, 3}


def test_the_headline_first_pass_has_a_uniform_step1():
    assert all(_maps(10, 1, uf)[1][0][5] == 1 for uf in (0, 1))
    # the distinct step-s digits of a wave: 1, 2, 8, 32
    rows = _maps(10, 1, 0)
    assert [max(len({r[4] for r in rows[s][w0:w0 + 64]}) for w0 in range(0, 512, 64)) for s in (1, 2, 3, 4)] == [1, 2, 8, 32]


def _ways(elems, groups, banks, dwords):
    """the worst number of distinct dwords on one bank within one lane group; elems[lane] = element index"""
    worst = 1
    for g in groups:
        seen = {}
        for lane in g:
            if lane < len(elems):
                for d in range(dwords):
                    a = elems[lane] * dwords + d
                    seen.setdefault(a % banks, set()).add(a)
        worst = max([worst] + [len(v) for v in seen.values()])
    return worst


@pytest.mark.parametrize("S,LT,ufast", _cases())
def test_bank_conflicts(S, LT, ufast):
    """writes conflict-free in every exchange, reads conflict-free after exchanges 0 and 1 and at most 2-way after 2 and 3"""
    steps = _maps(S, LT, ufast)
    for x in range(S // 2 - 1):
        w128 = w32 = r128 = r32 = 1
        for w0 in range(0, len(steps[x]), 64):
            for i in range(4):
                wr = [r[2][i] for r in steps[x][w0:w0 + 64]]
                rd = [r[3][i] for r in steps[x + 1][w0:w0 + 64]]
                w128 = max(w128, _ways(wr, WRITE_B128, 32, 4))
                w32 = max(w32, _ways(wr, B32, 32, 1))
                r128 = max(r128, _ways(rd, READ_B128, 64, 4))
                r32 = max(r32, _ways(rd, B32, 32, 1))
        assert (w128, w32) == (1, 1), (x, w128, w32)
        assert max(r128, r32) <= (1 if x < 2 else 2), (x, r128, r32)
        assert r128 == 1, (x, r128)              # what the rule reaches: only the 4-byte reads of a u-fast last step pair up


# ---- the consumer-side step 1 through the limb model --------------------------------------------------------------------
def _w16(inverse):
    d = B.Domain(16)
    return d.group_gen_inv if inverse else d.group_gen


def _mont(v):
    return v * FR.RADIX % FR.mod


def _rows(inverse, e):
    return F.rows_of(_mont(pow(_w16(inverse), e, FR.mod)), 1, 2)


def _step1_in(x, inverse, m, kp):
    """what step 1 feeds dft4 from its input m: the weak reduction of input 0, the product by w16^(k' m) of the others"""
    return F.fe_reduce_weak(FR, x) if m == 0 else F.fe_mul_split(x, _rows(inverse, kp * m), 1, 2)


@pytest.fixture()
def clean():
    del F.VIOLATIONS[:]
    yield
    del F.VIOLATIONS[:]


def test_exponents_are_the_heads():
    assert {kp * m for kp in range(4) for m in (1, 2, 3)} | {4} == {4, 1, 2, 3, 6, 9, 0}
    # the nibble table of w16_rows: exponent -> head block, block -> exponent (step4_head_exp); 4 is block 0
    block = {e: (0x5004003216 >> (4 * e)) & 15 for e in (0, 1, 2, 3, 4, 6, 9)}
    assert block == {4: 0, 1: 1, 2: 2, 3: 3, 6: 4, 9: 5, 0: 6}


@pytest.mark.parametrize("inverse", [0, 1])
def test_step1_products_at_the_class_limits(clean, inverse):
    """step 0 leaves (B < 5, V < 40) in the LDS; step 1 takes input 0 to (1, < 1 + 2^-16), the others to (1, < 2), and
    dft4 takes every digit's four inputs, the worst members of the classes together"""
    w4 = F.limbs_of(FR, _mont(pow(_w16(inverse), 4, FR.mod)))
    src = F.class_members(FR, 5, 40, False, n_random=12, seed=0x706D + inverse)
    worst = max(src, key=lambda l: F.value_of(FR, l))
    for kp in range(4):
        ins = [[_step1_in(x, inverse, m, kp) for x in src] for m in range(4)]
        for x, w in zip(src, ins[0]):
            assert F.in_class(FR, w, 1, 2) and F.value_of(FR, w) < FR.mod + (FR.mod >> 16)
        for m in (1, 2, 3):
            for x, p in zip(src, ins[m]):
                assert F.in_class(FR, p, 1, 2)
                assert F.value_of(FR, p) % FR.mod == F.value_of(FR, x) * pow(_w16(inverse), kp * m, FR.mod) % FR.mod
        n = len(src)
        for i in range(n):
            F.dft4(ins[0][i], ins[1][(i + 3) % n], ins[2][(i + 6) % n], ins[3][(i + 9) % n], w4)
        F.dft4(*[_step1_in(worst, inverse, m, kp) for m in range(4)], w4)
        ext = F.class_members(FR, 1, 2)                           # the product class's own extremes
        big = max(ext, key=lambda l: F.value_of(FR, l))
        F.dft4(F.limbs_of(FR, FR.mod + (FR.mod >> 16) - 1), big, big, big, w4)
    assert F.VIOLATIONS == []


@pytest.mark.parametrize("inverse", [0, 1])
def test_two_layers_in_plane_order_are_the_16_point_dft(clean, inverse):
    """S = 4: four threads, one exchange, in the kernel's own element order (the hook's maps)"""
    rng = random.Random(0x706D + inverse)
    w16 = _w16(inverse)
    w4 = F.limbs_of(FR, _mont(pow(w16, 4, FR.mod)))
    step0, step1 = _maps(4, 0, 0)
    for _ in range(8):
        vals = [rng.randrange(FR.mod) for _ in range(16)]
        x = [F.limbs_of(FR, _mont(v)) for v in vals]
        tile = [None] * 16
        for u, _, wr, _, _, _ in step0:
            X = F.dft4(x[u], x[u + 4], x[u + 8], x[u + 12], w4)
            for t in range(4):
                tile[wr[t]] = X[t]
        out = [None] * 16
        for u, _, _, rd, kp, _ in step1:
            X = F.dft4(*[_step1_in(tile[rd[m]], inverse, m, kp) for m in range(4)], w4)
            for t in range(4):
                out[u + 4 * t] = F.value_of(FR, X[t]) * FR.RINV % FR.mod
        want = [sum(v * pow(w16, j * k, FR.mod) for j, v in enumerate(vals)) % FR.mod for k in range(16)]
        assert out == want
    assert F.VIOLATIONS == []
