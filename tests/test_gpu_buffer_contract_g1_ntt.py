"""The memory AROUND a call's buffers, group B: the transforms and the G1 calls.  The method is that of
tests/test_gpu_buffer_contract.py: every buffer is a region of one guard arena (tests/guard_arena.py), the arena is downloaded
once, the bands and the read-only inputs must be untouched and the outputs equal the oracle bit for bit.  Strided batches are
ONE region each: the padding between two vectors is 0xA5 like a band and has to come back as 0xA5."""
import ctypes as C
import json
import os
import random
import sys

import numpy as np
import pytest

from oracle import bigint_oracle as B
from oracle.cpu_oracle import ints_to_limbs

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guard_arena as G  # noqa: E402

pytestmark = pytest.mark.gpu
R = B.R_MOD
HERE = os.path.dirname(os.path.abspath(__file__))
_CACHE = {}


# ---------------------------------------------------------------------------------- pm_fr_ntt_dev
def _strided(vecs, stride):
    """the vectors at a stride longer than they are, as ONE region that ends with the last vector: [elements, 4] with the
    padding between two vectors filled with 0xA5"""
    batch, length = len(vecs), vecs[0].shape[0]
    out = np.full(((batch - 1) * stride + length, 4), np.uint64(int.from_bytes(bytes([G.FILL]) * 8, "little")))
    for b, v in enumerate(vecs):
        out[b * stride:b * stride + length] = v
    return out


@pytest.mark.parametrize("flags", [0, 1, 2, 3])
@pytest.mark.parametrize("k", [4, 10, 11, 12])
def test_ntt_strided_batch(ctx, oracle, k, flags):
    """k = 4: one pass; 10: one pass at the full radix; 11: 6 + 5; 12: 6 + 6.  Batch 3 out of place with in_stride = in_len + 3
    and out_stride = n + 5 (the bands in front of the first and behind the last vector, the padding between them), and the
    in-place batch ("d_in == d_out allowed") with in_stride == out_stride == n + 5, for in_len == n and in_len == n / 2 + 3:
    the elements of a vector from in_len on count as zero, whatever bytes they hold."""
    n, batch = 1 << k, 3
    full = [oracle.fr_sample(1000 * k + 10 * flags + b, n) for b in range(batch)]
    for in_len in (n, n // 2 + 3):
        vecs = [v[:in_len] for v in full]
        want = _strided([oracle.fr_ntt(v, k, flags) for v in vecs], n + 5)
        # out of place
        with G.GuardArena.of(ctx, src=_strided(vecs, in_len + 3), dst=32 * want.shape[0]) as ar:
            ctx.fr_ntt_dev(ar.addr("src"), in_len, ar.addr("dst"), k, flags, batch=batch, in_stride=in_len + 3, out_stride=n + 5)
            got = G.as_u64(ar.check()["dst"], -1, 4)
            assert np.array_equal(got, want), (k, flags, in_len, "out of place")
        # in place: a vector's tail [in_len, n) holds 0xA5, not zeros
        image = _strided([np.concatenate([v, np.full((n - in_len, 4), want[n, 0])]) for v in vecs], n + 5)
        assert image.shape == want.shape and (image[n:n + 5] == want[n:n + 5]).all()
        with G.GuardArena.of(ctx, io=image) as ar:
            ctx.fr_ntt_dev(ar.addr("io"), in_len, ar.addr("io"), k, flags, batch=batch, in_stride=n + 5, out_stride=n + 5)
            got = G.as_u64(ar.check(written={"io"})["io"], -1, 4)
            assert np.array_equal(got, want), (k, flags, in_len, "in place")


# ---------------------------------------------------------------------------------- G1: the shared case
NMAX = 300


def _g1_case(oracle):
    """NMAX points, scalars (integers) and products, once: an identity point and a zero scalar among the first 63, and again
    as the LAST entry of every size under test"""
    if "g1" not in _CACHE:
        rng = random.Random(0x4731)
        pts = oracle.g1_bases_arith(ints_to_limbs([0x1234567], 4)[0], ints_to_limbs([0xabcdef123456789], 4)[0], NMAX)
        ks = [rng.randrange(R) for _ in range(NMAX)]
        ks[3], ks[62], ks[64], ks[129] = 0, 0, R - 1, 0
        pts[5], pts[0] = 0, pts[1]
        pts[64] = 0
        klimbs = ints_to_limbs(ks, 4)
        _CACHE["g1"] = (pts, ks, klimbs, {})
    return _CACHE["g1"]


def _products(oracle, upto):
    pts, ks, klimbs, memo = _g1_case(oracle)
    for i in range(upto):
        if i not in memo:
            memo[i] = oracle.g1_mul(pts[i], klimbs[i]) if pts[i].any() and ks[i] else np.zeros(12, np.uint64)
    return np.stack([memo[i] for i in range(upto)])


@pytest.mark.parametrize("n", [1, 63, 65, 300])
def test_g1_fixed_base_mul(ctx, oracle, n):
    _, ks, klimbs, _ = _g1_case(oracle)
    base = oracle.g1_generator()
    memo = _CACHE.setdefault("fixed", {})
    for i in range(n):
        if i not in memo:
            memo[i] = oracle.g1_mul(base, klimbs[i]) if ks[i] else np.zeros(12, np.uint64)
    want = np.stack([memo[i] for i in range(n)])
    with G.GuardArena.of(ctx, sc=oracle.fr_to_mont(klimbs[:n]), out=96 * n) as ar:
        ctx._check(ctx._lib.pm_g1_fixed_base_mul_dev(ctx._h, base.ctypes.data_as(C.POINTER(C.c_uint64)), C.c_void_p(ar.addr("sc")), n, 0,
                                                     C.c_void_p(ar.addr("out")), None))
        assert np.array_equal(G.as_u64(ar.check()["out"], n, 12), want), n


@pytest.mark.parametrize("flag", [False, True], ids=("any_point", "subgroup_points"))
@pytest.mark.parametrize("n", [1, 63, 65, 130])
def test_g1_scalar_mul(ctx, oracle, n, flag):
    """out of place with the points unchanged, and "d_out_xy == d_points_xy is allowed" """
    pts, _, klimbs, _ = _g1_case(oracle)
    want = _products(oracle, n)
    sc = oracle.fr_to_mont(klimbs[:n])
    with G.GuardArena.of(ctx, pts=pts[:n].copy(), sc=sc, out=96 * n) as ar:
        ctx.g1_scalar_mul_dev(ar.addr("pts"), ar.addr("sc"), n, ar.addr("out"), subgroup_points=flag)
        assert np.array_equal(G.as_u64(ar.check()["out"], n, 12), want), (n, flag, "out of place")
    with G.GuardArena.of(ctx, pts=pts[:n].copy(), sc=sc) as ar:
        ctx.g1_scalar_mul_dev(ar.addr("pts"), ar.addr("sc"), n, ar.addr("pts"), subgroup_points=flag)
        assert np.array_equal(G.as_u64(ar.check(written={"pts"})["pts"], n, 12), want), (n, flag, "in place")


# ---------------------------------------------------------------------------------- pm_g1_bases_lagrange, pm_g1_bases_to_dev
def _to_limbs(pts):
    from plonk_prototype_amd.field import fp_to_limbs
    out = np.zeros((len(pts), 12), np.uint64)
    for i, p in enumerate(pts):
        if p is not None:
            out[i, :6], out[i, 6:] = fp_to_limbs(p[0]), fp_to_limbs(p[1])
    return out


@pytest.mark.parametrize("log_n", [0, 1, 5])
def test_g1_bases_lagrange(ctx, oracle, log_n):
    """powers P_j = d_j G with known d_j (one of them 0: an identity among the powers): the inverse NTT over G1 is then
    [e_i] G with e = the inverse NTT of d over Fr, so the expected points are oracle.fr_ntt and oracle.g1_mul composed -- exact,
    and quick where the big-integer G1 transform of tests/test_lagrange_host.py takes seconds"""
    import plonk_prototype_amd as pa
    n = 1 << log_n
    d = oracle.fr_sample(100 + log_n, n)
    if n > 2:
        d[3] = 0
    gen = oracle.g1_generator()
    times_g = lambda limbs: np.stack([oracle.g1_mul(gen, k) if k.any() else np.zeros(12, np.uint64)   # noqa: E731
                                      for k in oracle.fr_from_mont(limbs)])
    bases = pa.host.Bases(ctx, times_g(d))
    try:
        with G.GuardArena.of(ctx, out=96 * n) as ar:
            ctx._check(ctx._lib.pm_g1_bases_lagrange(ctx._h, bases._h, log_n, C.c_void_p(ar.addr("out")), None))
            assert np.array_equal(G.as_u64(ar.check()["out"], n, 12), times_g(oracle.fr_ntt(d, log_n, 1))), log_n
    finally:
        bases.free()


@pytest.mark.parametrize("n", [1, 33])
def test_g1_bases_to_dev(ctx, oracle, n):
    import plonk_prototype_amd as pa
    pts = _g1_case(oracle)[0][:n].copy()
    bases = pa.host.Bases(ctx, pts)
    try:
        with G.GuardArena.of(ctx, out=96 * n) as ar:
            ctx._check(ctx._lib.pm_g1_bases_to_dev(ctx._h, bases._h, C.c_void_p(ar.addr("out")), None))
            assert np.array_equal(G.as_u64(ar.check()["out"], n, 12), pts), n
    finally:
        bases.free()


# ---------------------------------------------------------------------------------- the 48-byte records
def _vectors():
    if "vectors" not in _CACHE:
        with open(os.path.join(HERE, "golden", "g1_encoding.json")) as f:
            vs = json.load(f)["vectors"]
        for v in vs:
            v["bytes"] = bytes.fromhex(v["hex"])
            v["point"] = None if v["x"] is None else (int(v["x"], 16), int(v["y"], 16))
        _CACHE["vectors"] = vs
    return _CACHE["vectors"]


def _good_batch(n):
    """subgroup points of both signs with identities mixed in (the batches of tests/test_gpu_g1_codec.py)"""
    vs = _vectors()
    sub = [v for v in vs if v["name"].startswith("subgroup_") or v["name"] in ("generator", "generator_neg")]
    ident = next(v for v in vs if v["name"] == "identity")
    good = []
    for i, v in enumerate(sub):
        good.append(v)
        if i % 7 == 3:
            good.append(ident)
    return [good[(5 * i + 1) % len(good)] for i in range(n)]


def _bytes_of(batch):
    return np.frombuffer(b"".join(v["bytes"] for v in batch), np.uint8).copy()


@pytest.mark.parametrize("n", [1, 63, 65])
def test_g1_compress(ctx, n):
    """n x 48 bytes: for odd n the output ends 16 bytes off a 32-byte boundary, and the band begins at the very next byte"""
    batch = _good_batch(n)
    with G.GuardArena.of(ctx, xy=_to_limbs([v["point"] for v in batch]), out=48 * n) as ar:
        ctx.g1_compress_dev(ar.addr("xy"), n, ar.addr("out"))
        assert ar.check()["out"].tobytes() == _bytes_of(batch).tobytes(), n


@pytest.mark.parametrize("n", [1, 63, 65])
def test_g1_decompress(ctx, n):
    """"The output is always written in full; a rejected point comes back as (0, 0)" -- and nothing more is written: a clean
    batch, then the same batch with its LAST point replaced by a curve point outside the subgroup"""
    import plonk_prototype_amd as pa
    batch = _good_batch(n)
    want = _to_limbs([v["point"] for v in batch])
    with G.GuardArena.of(ctx, data=_bytes_of(batch), out=96 * n) as ar:
        ctx.g1_decompress_dev(ar.addr("data"), n, ar.addr("out"))
        assert np.array_equal(G.as_u64(ar.check()["out"], n, 12), want), n
    bad = next(v for v in _vectors() if v["name"] == "order3")
    assert bad["curve_reason"] == 0 and not bad["in_subgroup"]
    batch[n - 1] = bad
    want[n - 1] = 0
    with G.GuardArena.of(ctx, data=_bytes_of(batch), out=96 * n) as ar:
        with pytest.raises(pa.Error) as e:
            ctx.g1_decompress_dev(ar.addr("data"), n, ar.addr("out"))
        assert (e.value.code, e.value.bad_index, e.value.bad_reason) == (pa._lib.PM_ERR_POINT, n - 1, pa._lib.G1_BAD_NOT_IN_SUBGROUP)
        assert np.array_equal(G.as_u64(ar.check()["out"], n, 12), want), (n, "rejected")
        # without the subgroup check the same bytes decode
    want[n - 1] = _to_limbs([bad["point"]])[0]
    with G.GuardArena.of(ctx, data=_bytes_of(batch), out=96 * n) as ar:
        ctx.g1_decompress_dev(ar.addr("data"), n, ar.addr("out"), check_subgroup=False)
        assert np.array_equal(G.as_u64(ar.check()["out"], n, 12), want), (n, "unchecked")


@pytest.mark.parametrize("n", [1, 63, 65])
def test_g1_check_reads_only(ctx, n):
    """"Reads only": whatever the verdict, no byte of the arena changes"""
    import plonk_prototype_amd as pa
    batch = _good_batch(n)
    with G.GuardArena.of(ctx, xy=_to_limbs([v["point"] for v in batch])) as ar:
        ctx.g1_check_dev(ar.addr("xy"), n)
        assert ar.check() == {}
    batch[n - 1] = next(v for v in _vectors() if v["name"] == "order3")
    with G.GuardArena.of(ctx, xy=_to_limbs([v["point"] for v in batch])) as ar:
        with pytest.raises(pa.Error) as e:
            ctx.g1_check_dev(ar.addr("xy"), n)
        assert (e.value.code, e.value.bad_index, e.value.bad_reason) == (pa._lib.PM_ERR_POINT, n - 1, pa._lib.G1_BAD_NOT_IN_SUBGROUP)
        assert ar.check() == {}
        ctx.g1_check_dev(ar.addr("xy"), n, subgroup=False)
        assert ar.check() == {}
