"""Per-point G1 scalar multiplication (pm_g1_scalar_mul_dev), its GLV split, and its two consumers: the flagged Lagrange
conversion (pm_g1_bases_lagrange_ex) and CommitKey.update.

Expected values come from the oracles only -- oracle.g1_mul of the C restatement, bigint_oracle.g1_mul for curve points
outside the subgroup, Python's divmod for the split -- and every comparison is exact equality of limbs or bytes.  The two
modes are the signed 4-bit window ladder over the whole scalar (no flag: any curve point) and the same ladder over the two
128-bit halves k = k1 + k2 z^2 with the endomorphism (PM_G1_POINTS_IN_SUBGROUP: subgroup points only)."""
import ctypes as C
import json
import os
import random

import numpy as np
import pytest

from oracle import bigint_oracle as B
from oracle.cpu_oracle import ints_to_limbs
from conftest import ROOT
from test_glv_split_host import R, Z2, split_cases

pytestmark = pytest.mark.gpu

W = 4                                   # the window of csrc/ec_mul.hip.h
MONT, CANON = 0, 1
u64p = C.POINTER(C.c_uint64)
FIXED = [0, 1, 2, Z2 - 1, Z2, Z2 + 1, 2 * Z2 - 1, 2 * Z2, R - 2, R - 1, (Z2 - 1) * Z2 - 1, 2**128 - 1, 2**128, 2**254]
# window boundaries: the lowest, a middle one, the top window of a 128-bit half (j = 31), the carry digit above it (32, 33)
# and the top window of the 255-bit integer (j = 63; 2^(4 x 63) + 1 < r)
WINDOWS = [2**(W * j) + d for j in (1, 2, 16, 31, 32, 33, 62, 63) for d in (-1, 0, 1)]
EDGE = FIXED + list(range(3, 41)) + WINDOWS


def scalars_in(oracle, ks, form):
    limbs = ints_to_limbs(ks, 4) if ks else np.zeros((0, 4), np.uint64)
    return oracle.fr_to_mont(limbs) if form == MONT and ks else limbs


def scalar_mul(ctx, points, scalars, form, flag, alias=True):
    """pm_g1_scalar_mul_dev on host arrays -> [n, 12]; alias: write the results over the points"""
    import plonk_prototype_amd as pa
    n = points.shape[0]
    d_p = pa.DeviceVector.from_host(ctx, points.reshape(-1, 4))
    d_s = pa.DeviceVector.from_host(ctx, scalars)
    d_o = d_p if alias else pa.DeviceVector(ctx, 3 * n)
    try:
        ctx.g1_scalar_mul_dev(d_p.ptr, d_s.ptr, n, d_o.ptr, form, subgroup_points=flag)
        return d_o.to_host().reshape(n, 12)
    finally:
        d_p.free()
        d_s.free()
        if not alias:
            d_o.free()


@pytest.fixture(scope="module")
def points36(oracle):
    return oracle.g1_bases_arith(ints_to_limbs([0x1234567], 4)[0], ints_to_limbs([0xabcdef123456789], 4)[0], 36)


@pytest.fixture(scope="module")
def edge_batch(oracle, points36):
    """every one of the 36 points times every edge scalar: (points, scalars as integers, expected), computed once"""
    ks = [k for _ in range(36) for k in EDGE]
    pts = np.repeat(points36, len(EDGE), axis=0)
    klimbs = ints_to_limbs(ks, 4)
    exp = np.stack([oracle.g1_mul(p, k) for p, k in zip(pts, klimbs)])
    return pts, ks, exp


@pytest.fixture(scope="module")
def random_batch(oracle, points36):
    """1000 seeded random scalars on the 36 points in turn, with the expected products"""
    rng = random.Random(0x53434D)
    ks = [rng.randrange(R) for _ in range(1000)]
    pts = points36[np.arange(1000) % 36]
    exp = np.stack([oracle.g1_mul(p, k) for p, k in zip(pts, ints_to_limbs(ks, 4))])
    return pts, ks, exp


@pytest.mark.parametrize("form", [MONT, CANON])
def test_split_on_the_device(ctx, oracle, form):
    ks = split_cases()
    sc = np.ascontiguousarray(scalars_in(oracle, ks, form))
    out = np.zeros((len(ks), 4), np.uint64)
    ctx._check(ctx._lib.pm_test_glv_split(ctx._h, sc.ctypes.data_as(u64p), len(ks), form, out.ctypes.data_as(u64p)))
    for k, o in zip(ks, out):
        assert (int(o[2]) | int(o[3]) << 64, int(o[0]) | int(o[1]) << 64) == divmod(k, Z2), hex(k)


@pytest.mark.parametrize("form", [MONT, CANON])
@pytest.mark.parametrize("flag", [False, True])
def test_edge_scalars_on_36_points(ctx, oracle, edge_batch, flag, form):
    pts, ks, exp = edge_batch
    got = scalar_mul(ctx, pts, scalars_in(oracle, ks, form), form, flag)
    bad = np.nonzero((got != exp).any(axis=1))[0]
    assert bad.size == 0, [(int(i) // len(EDGE), hex(ks[i])) for i in bad[:8]]
    zero = [i for i, k in enumerate(ks) if k == 0]
    assert zero and not got[zero].any()                      # a zero scalar: (0, 0)


@pytest.mark.parametrize("flag", [False, True])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 127, 128, 129, 1000])
def test_sizes_across_wave_and_block_boundaries(ctx, oracle, random_batch, n, flag):
    pts, ks, exp = random_batch
    got = scalar_mul(ctx, pts[:n].copy(), scalars_in(oracle, ks[:n], MONT), MONT, flag)
    assert got.shape == (n, 12) and np.array_equal(got, exp[:n])


@pytest.mark.parametrize("flag", [False, True])
def test_identities_aliasing_and_repeatability(ctx, oracle, random_batch, flag):
    pts, ks, exp = (a[:200].copy() if isinstance(a, np.ndarray) else list(a[:200]) for a in random_batch)
    for i in range(200):
        if i % 7 == 3:
            pts[i] = 0                                       # an identity point
            exp[i] = 0
        if i % 5 == 1:
            ks[i] = 0                                        # a zero scalar
            exp[i] = 0
    sc = scalars_in(oracle, ks, MONT)
    out_of_place = scalar_mul(ctx, pts, sc, MONT, flag, alias=False)
    assert np.array_equal(out_of_place, exp)
    assert not out_of_place[[i for i in range(200) if i % 7 == 3 or i % 5 == 1]].any()
    in_place = scalar_mul(ctx, pts, sc, MONT, flag, alias=True)
    assert in_place.tobytes() == out_of_place.tobytes()
    assert scalar_mul(ctx, pts, sc, MONT, flag, alias=False).tobytes() == out_of_place.tobytes()


def test_any_curve_point_in_the_plain_mode(ctx, oracle):
    """Curve points OUTSIDE the subgroup -- (0, +-2) of order 3, G + (0, 2), the small-x points -- through the unflagged
    ladder.  The order-3 point drives it through P + P = -P, P - P and identity table entries at almost every step: the
    test of the exceptional paths of xyzz_add / xyzz_double inside the ladder."""
    with open(os.path.join(ROOT, "tests", "golden", "g1_encoding.json")) as f:
        vecs = [v for v in json.load(f)["vectors"] if v["in_subgroup"] is False]
    assert len(vecs) >= 12 and any(v["name"] == "order3" for v in vecs)
    affine = [(int(v["x"], 16), int(v["y"], 16)) for v in vecs]
    ks = list(range(41)) + FIXED + WINDOWS
    pts_int, k_all = [p for p in affine for _ in ks], ks * len(affine)
    pts = oracle.fp_to_mont(ints_to_limbs([c for p in pts_int for c in p], 6)).reshape(-1, 12)
    exp = np.zeros_like(pts)
    for i, (p, k) in enumerate(zip(pts_int, k_all)):
        q = B.g1_mul(k, p)
        if q is not None:
            exp[i] = oracle.fp_to_mont(ints_to_limbs(list(q), 6)).reshape(12)
    for form in (MONT, CANON):
        got = scalar_mul(ctx, pts, scalars_in(oracle, k_all, form), form, False)
        bad = np.nonzero((got != exp).any(axis=1))[0]
        assert bad.size == 0, [(vecs[int(i) // len(ks)]["name"], hex(k_all[i])) for i in bad[:8]]


TAU = 0x1f2e3d4c5b6a79880123456789abcdef0fedcba987654321aabbccddeeff0011 % R
DELTA = 0x2b7e151628aed2a6abf7158809cf4f3c762e7160f38b4da56a784d9045190cfe % R


def fr_mont(oracle, v):
    return oracle.fr_to_mont(ints_to_limbs([v], 4))[0]


def test_lagrange_with_the_subgroup_flag_gives_the_same_bytes(ctx, oracle):
    import plonk_prototype_amd as pa
    ck = pa.CommitKey.setup(2**10 - 1, fr_mont(oracle, TAU), ctx)
    for log_n in (0, 1, 2, 3, 6, 7, 10):                     # 6 | 7: the last stage with wave-uniform twiddles
        plain = ck.lagrange(log_n).points()
        flagged = ck.lagrange(log_n, subgroup_points=True).points()
        assert flagged.shape == (1 << log_n, 12) and flagged.tobytes() == plain.tobytes(), log_n


def test_update_turns_powers_of_tau_into_powers_of_tau_delta(ctx, oracle):
    import plonk_prototype_amd as pa
    ck = pa.CommitKey.setup(299, fr_mont(oracle, TAU), ctx)               # 300 points: not a multiple of 128
    want = pa.CommitKey.setup(299, fr_mont(oracle, TAU * DELTA % R), ctx).to_bytes()
    for flag in (False, True):
        new = ck.update(fr_mont(oracle, DELTA), subgroup_points=flag)
        assert new.max_degree() == 299 and new.to_bytes() == want, flag
    assert ck.update(fr_mont(oracle, 1)).to_bytes() == ck.to_bytes()
    assert ck.update(fr_mont(oracle, 1), subgroup_points=True).to_bytes() == ck.to_bytes()


def test_errors_leave_the_context_usable(ctx, oracle, points36, random_batch):
    import plonk_prototype_amd as pa
    from plonk_prototype_amd import _lib
    lib, h = ctx._lib, ctx._h
    v = pa.DeviceVector(ctx, 3 * 4)
    s = pa.DeviceVector(ctx, 4)
    try:
        assert lib.pm_g1_scalar_mul_dev(h, None, s._p, 4, 0, 0, v._p, None) == _lib.PM_ERR_BAD_ARG
        assert lib.pm_g1_scalar_mul_dev(h, v._p, None, 4, 0, 0, v._p, None) == _lib.PM_ERR_BAD_ARG
        assert lib.pm_g1_scalar_mul_dev(h, v._p, s._p, 4, 0, 0, None, None) == _lib.PM_ERR_BAD_ARG
        assert lib.pm_g1_scalar_mul_dev(h, v._p, s._p, 4, 0, 2, v._p, None) == _lib.PM_ERR_BAD_ARG      # flag bit 2
        assert lib.pm_g1_scalar_mul_dev(h, v._p, s._p, 4, 7, 0, v._p, None) == _lib.PM_ERR_BAD_ARG      # scalar form 7
        assert lib.pm_g1_scalar_mul_dev(h, None, None, 0, 0, 1, None, None) == _lib.PM_OK               # n == 0
        ck = pa.CommitKey(points36[:8], ctx)
        assert lib.pm_g1_bases_lagrange_ex(h, ck._bases._h, 4, 1, v._p, None) == _lib.PM_ERR_LENGTH     # 16 > 8 points
        assert lib.pm_g1_bases_lagrange_ex(h, ck._bases._h, 1, 2, v._p, None) == _lib.PM_ERR_BAD_ARG
        assert lib.pm_g1_bases_lagrange_ex(h, None, 1, 1, v._p, None) == _lib.PM_ERR_BAD_ARG
        assert lib.pm_g1_bases_to_dev(h, None, v._p, None) == _lib.PM_ERR_BAD_ARG
    finally:
        v.free()
        s.free()
    pts, ks, exp = random_batch
    assert np.array_equal(pa.g1_scalar_mul(pts[:5], scalars_in(oracle, ks[:5], MONT), True, ctx), exp[:5])
