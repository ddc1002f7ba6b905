"""The JubJub wire format on the device against the big-integer model of tests/jubjub_codec_model.py,
byte for byte: the square root in Fr with the even root, decoding with every kind of refusal at the ends of two waves, encoding,
the strided forms inside a guard arena, and the two consumers -- PoseidonCipher.scan_bytes and Schnorr.verify_bytes -- against
the calls they stand for on the model-decoded points."""
import ctypes as C
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fr_sqrt_cases as F  # noqa: E402
import gadget_model as M  # noqa: E402
import jubjub_codec_model as CM  # noqa: E402
import jubjub_model as J  # noqa: E402
import schnorr_model as S  # noqa: E402
from guard_arena import FILL, GuardArena  # noqa: E402

pytestmark = pytest.mark.gpu
R = CM.R
SIZES = (1, 2, 63, 64, 65, 130)
NMAX = max(SIZES)
SENTINEL = 0x7777777777777777
_CACHE = {}


def _enc(rows) -> np.ndarray:
    return np.frombuffer(b"".join(rows), dtype=np.uint8).reshape(-1, 32).copy()


def _canon(v: int) -> np.ndarray:
    return np.frombuffer(v.to_bytes(32, "little"), dtype=np.uint64).copy()


def sqrt_case():
    """NMAX inputs, the edge ones first: (limbs, the model's roots as limbs, the model's flags)"""
    if "sqrt" not in _CACHE:
        vals = CM.sqrt_inputs(NMAX)
        want = [CM.sqrt_even(a) for a in vals]
        _CACHE["sqrt"] = (M.to_limbs(vals), M.to_limbs([w[0] for w in want]), np.array([w[1] for w in want], np.uint32))
    return _CACHE["sqrt"]


def decode_case():
    """NMAX encodings: the edge points, multiples of the generator and random points, with every kind of refusal at known
    positions -- 0, the ends of the first wave, a position in the second wave and the last one.  -> (bytes [n, 32], and per flag
    the model's points as limbs and its statuses)"""
    if "decode" not in _CACHE:
        rng = random.Random(31)
        pts = J.edge_points() + [J.mul(J.GENERATOR, rng.randrange(1, J.Q)) for _ in range(40)]
        pts += CM.random_points(NMAX - len(pts), seed=32)
        rows = [CM.encode(p) for p in pts]
        put = {0: CM.y_bytes(R), 62: CM.y_bytes(R + 1, 1), 63: CM.y_bytes(R - 1, 1), 64: CM.y_bytes(2), 70: CM.y_bytes(1, 1),
               101: CM.y_bytes((1 << 255) - 1), 128: CM.y_bytes(4, 1), NMAX - 1: CM.y_bytes(2, 1)}
        for at, data in put.items():
            rows[at] = data
        case = {"bytes": _enc(rows), "refused": sorted(put)}
        for flag in (False, True):
            got = [CM.decode(r, flag) for r in rows]
            case[flag] = (J.to_limbs([g[0] for g in got]), np.array([g[1] for g in got], np.uint32))
        assert [int(case[False][1][at]) for at in sorted(put)] == [1, 1, 3, 2, 3, 1, 2, 2]
        assert not case[False][1][[i for i in range(NMAX) if i not in put]].any()
        assert set(case[True][1].tolist()) == {0, 1, 2, 3, 4} and (case[True][1] == 0).sum() >= 40
        _CACHE["decode"] = case
    return _CACHE["decode"]


# ---------------------------------------------------------------------------------- 1. the square root
def test_fr_sqrt_is_the_model(ctx):
    import plonk_prototype_amd as pa
    import torch
    vals, roots, flags = sqrt_case()
    edge = len(CM.sqrt_edge_inputs())
    assert 0 in flags[edge:] and 1 in flags[edge:], "both classes among the random inputs"
    for n in SIZES:
        got, sq = pa.fr_sqrt(ctx, vals[:n])                  # in place
        assert sq.tolist() == flags[:n].tolist(), (n, np.flatnonzero(sq != flags[:n])[:8])
        assert got.tobytes() == roots[:n].tobytes(), (n, np.flatnonzero((got != roots[:n]).any(axis=1))[:8])
    # out of place, with the count, on a caller's stream; then without flags and without the count
    st = torch.cuda.Stream()
    d = pa.DeviceVector.from_host(ctx, vals)
    out = pa.DeviceVector.from_host(ctx, np.full((NMAX, 4), SENTINEL, np.uint64))
    f = pa.DeviceVector.from_host(ctx, np.full(((NMAX + 7) // 8, 4), SENTINEL, np.uint64))
    try:
        count = pa.fr_sqrt_dev(ctx, d.ptr, NMAX, out.ptr, f.ptr, want_count=True, stream=st.cuda_stream)
        assert count == int(flags.sum())
        assert out.to_host().tobytes() == roots.tobytes() and d.to_host().tobytes() == vals.tobytes()
        words = f.to_host().view(np.uint32).reshape(-1)
        assert words[:NMAX].tolist() == flags.tolist() and (words[NMAX:] == 0x77777777).all()
        assert pa.fr_sqrt_dev(ctx, d.ptr, 65, out.ptr, 0) is None
        ctx.sync()
        assert out.to_host()[:65].tobytes() == roots[:65].tobytes()
    finally:
        d.free(), out.free(), f.free()
    # limbs that are not below r: flag 0 and root 0, beside good neighbours
    mixed = vals[:4].copy()
    mixed[1], mixed[2] = _canon(R), _canon((1 << 256) - 1)
    got, sq = pa.fr_sqrt(ctx, mixed)
    assert sq.tolist() == [int(flags[0]), 0, 0, int(flags[3])] and not got[1:3].any()
    assert got[[0, 3]].tobytes() == roots[[0, 3]].tobytes()
    # integers in, and the host form on the same inputs
    got, sq = pa.fr_sqrt(ctx, [4, 7, 0])
    assert sq.tolist() == [1, 0, 1] and pa.field.fr_vec_from_limbs(got) == [2, 0, 0]
    for i in (0, 3, 5, 9, 17, 40):
        root, flag = pa.fr_sqrt_host(vals[i])
        assert flag == flags[i] and root.tobytes() == roots[i].tobytes()


# ---------------------------------------------------------------------------------- 2. decoding and encoding
@pytest.mark.parametrize("flag", (False, True), ids=("plain", "subgroup"))
def test_decompress_is_the_model(ctx, flag):
    import plonk_prototype_amd as pa
    case = decode_case()
    data, (points, status) = case["bytes"], case[flag]
    for n in SIZES:
        got, st = pa.jubjub_decompress(ctx, data[:n], check_subgroup=flag)
        assert st.tolist() == status[:n].tolist(), (n, np.flatnonzero(st != status[:n])[:8])
        assert got.tobytes() == points[:n].tobytes(), (n, np.flatnonzero((got != points[:n]).any(axis=(1, 2)))[:8])
    assert not points[status != 0].any(), "a refused point is (0, 0)"
    # the count, and no status wanted
    db = pa.DeviceVector.from_host(ctx, data.view(np.uint64))
    out = pa.DeviceVector.from_host(ctx, np.full((2 * NMAX, 4), SENTINEL, np.uint64))
    try:
        assert pa.jubjub_decompress_dev(ctx, db.ptr, NMAX, out.ptr, 0, flag) == int((status == 0).sum())
        assert out.to_host().tobytes() == points.tobytes()
    finally:
        db.free(), out.free()
    # the host form agrees on a few of each kind
    for i in case["refused"] + [1, 2, 3, 4, 5, 50, 100]:
        p, s = pa.jubjub_decompress_host(data[i].tobytes(), check_subgroup=flag)
        assert s == status[i] and p.tobytes() == points[i].tobytes(), i


def test_strict_names_the_lowest_bad_index_and_compress_returns_the_bytes(ctx):
    import plonk_prototype_amd as pa
    case = decode_case()
    data, (points, status) = case["bytes"], case[False]
    with pytest.raises(ValueError, match=r"encoding 0 is refused: range"):
        pa.jubjub_decompress(ctx, data, strict=True)
    with pytest.raises(ValueError, match=r"encoding 61 is refused: range"):
        pa.jubjub_decompress(ctx, data[1:], strict=True)
    with pytest.raises(ValueError, match=r"encoding 1 is refused: not_on_curve"):
        pa.jubjub_decompress(ctx, data[[1, 64, 63]], strict=True)
    assert case[True][1][:2].tolist() == [1, 4]              # the second edge point is not in the subgroup
    with pytest.raises(ValueError, match=r"encoding 0 is refused: not_in_subgroup"):
        pa.jubjub_decompress(ctx, data[1:62], check_subgroup=True, strict=True)
    good = status == 0
    got, st = pa.jubjub_decompress(ctx, data[good], strict=True)
    assert not st.any() and got.tobytes() == points[good].tobytes()
    for n in SIZES:
        back = pa.jubjub_compress(ctx, got[:n])
        assert back.dtype == np.uint8 and back.tobytes() == data[good][:n].tobytes(), n
    assert pa.jubjub_compress(ctx, [J.GENERATOR, J.IDENTITY]).tobytes() == bytes([0x12]) + bytes(31) + bytes([1]) + bytes(31)
    assert pa.jubjub_compress(ctx, got[:0]).shape == (0, 32) and pa.jubjub_decompress(ctx, b"")[0].shape == (0, 2, 4)


# ---------------------------------------------------------------------------------- 3. strides and the memory around the buffers
@pytest.mark.parametrize("flag", (False, True), ids=("plain", "subgroup"))
def test_strided_and_packed_forms_touch_nothing_else(ctx, flag):
    import plonk_prototype_amd as pa
    case = decode_case()
    n = 65
    data, (points, status) = case["bytes"][:n], (case[flag][0][:n], case[flag][1][:n])
    # signatures: 64 bytes (u | R) -> records of 96 bytes (u, R.x, R.y); the u slots are not the call's
    sigs = np.full((n, 64), 0x3C, np.uint8)
    sigs[:, 32:] = data
    with GuardArena.of(ctx, sigs=sigs, records=96 * n, status=4 * n) as arena:
        ok = pa.jubjub_decompress_dev(ctx, arena.addr("sigs") + 32, n, arena.addr("records") + 32, arena.addr("status"), flag,
                                      in_stride=64, out_stride=96)
        got = arena.check()
        rec = got["records"].reshape(n, 96)
        assert (rec[:, :32] == FILL).all(), "the u slots between the records keep their fill bytes"
        assert rec[:, 32:].tobytes() == points.tobytes()
        assert got["status"].view(np.uint32).tolist() == status.tolist() and ok == int((status == 0).sum())
    # packed: strides of 0, and the same given explicitly
    for strides in ({}, {"in_stride": 32, "out_stride": 64}):
        with GuardArena.of(ctx, data=data, points=64 * n, status=4 * n) as arena:
            ok = pa.jubjub_decompress_dev(ctx, arena.addr("data"), n, arena.addr("points"), arena.addr("status"), flag, **strides)
            got = arena.check()
            assert got["points"].tobytes() == points.tobytes() and got["status"].view(np.uint32).tolist() == status.tolist()
            assert ok == int((status == 0).sum())
    if flag:
        return
    good = status == 0
    m = int(good.sum())
    with GuardArena.of(ctx, points=points[good], data=32 * m) as arena:
        pa.jubjub_compress_dev(ctx, arena.addr("points"), m, arena.addr("data"))
        assert arena.check()["data"].tobytes() == data[good].tobytes()
    vals, roots, flags = sqrt_case()
    with GuardArena.of(ctx, vals=vals[:n], roots=32 * n, flags=4 * n) as arena:
        assert pa.fr_sqrt_dev(ctx, arena.addr("vals"), n, arena.addr("roots"), arena.addr("flags"), want_count=True) == int(flags[:n].sum())
        got = arena.check()
        assert got["roots"].tobytes() == roots[:n].tobytes() and got["flags"].view(np.uint32).tolist() == flags[:n].tolist()


# ---------------------------------------------------------------------------------- 4. refusals of the call, n = 0
def test_refusals_and_n_zero(ctx):
    import plonk_prototype_amd as pa
    from plonk_prototype_amd import _lib
    lib, h = ctx._lib, ctx._h
    n = 4
    data = decode_case()["bytes"][1:1 + n]
    with GuardArena.of(ctx, data=np.tile(data, (1, 2)), points=96 * n, status=4 * n) as arena:
        d, p, s, ok = arena.addr("data"), arena.addr("points"), arena.addr("status"), C.c_size_t(77)
        call = lambda *a: lib.pm_jubjub_decompress_dev(h, *a)   # noqa: E731
        vp = C.c_void_p
        bad = [(vp(d), 0, n, 2, vp(p), 0, vp(s), C.byref(ok), None),          # unknown flag bits
               (vp(d), 0, n, 0x80000001, vp(p), 0, vp(s), C.byref(ok), None),
               (vp(d), 40, n, 0, vp(p), 0, vp(s), C.byref(ok), None),         # a stride that is no multiple of 16
               (vp(d), 16, n, 0, vp(p), 0, vp(s), C.byref(ok), None),         # a stride below the packed size
               (vp(d), 0, n, 0, vp(p), 48, vp(s), C.byref(ok), None),
               (vp(d), 0, n, 0, vp(p), 72, vp(s), C.byref(ok), None),
               (None, 0, n, 0, vp(p), 0, vp(s), C.byref(ok), None),           # NULL
               (vp(d), 0, n, 0, None, 0, vp(s), C.byref(ok), None),
               (vp(d + 8), 0, n, 0, vp(p), 0, vp(s), C.byref(ok), None),      # not 16-byte aligned
               (vp(d), 0, n, 0, vp(p), 0, vp(s + 2), C.byref(ok), None)]
        for args in bad:
            assert call(*args) == _lib.PM_ERR_BAD_ARG, args[1:4]
        assert lib.pm_jubjub_decompress_dev(None, vp(d), 0, n, 0, vp(p), 0, vp(s), None, None) == _lib.PM_ERR_BAD_ARG
        assert lib.pm_jubjub_compress_dev(h, None, n, vp(p), None) == _lib.PM_ERR_BAD_ARG
        assert lib.pm_jubjub_compress_dev(h, vp(p), n, None, None) == _lib.PM_ERR_BAD_ARG
        assert lib.pm_fr_sqrt_dev(h, None, n, vp(p), None, None, None) == _lib.PM_ERR_BAD_ARG
        assert lib.pm_fr_sqrt_dev(h, vp(p), n, None, None, None, None) == _lib.PM_ERR_BAD_ARG
        assert lib.pm_fr_sqrt_dev(h, vp(p), n, vp(p), vp(s + 2), None, None) == _lib.PM_ERR_BAD_ARG
        # n = 0 launches nothing
        assert call(vp(d), 0, 0, 1, vp(p), 0, vp(s), C.byref(ok), None) == _lib.PM_OK and ok.value == 0
        ok = C.c_size_t(77)
        assert lib.pm_fr_sqrt_dev(h, vp(p), 0, vp(p), vp(s), C.byref(ok), None) == _lib.PM_OK and ok.value == 0
        assert lib.pm_jubjub_compress_dev(h, vp(p), 0, vp(d), None) == _lib.PM_OK
        arena.check_unchanged()
    with pytest.raises(ValueError):
        pa.jubjub_decompress(ctx, bytes(31))
    with pytest.raises(ValueError):
        pa.jubjub_decompress(ctx, np.zeros((2, 32), np.int8))


# ---------------------------------------------------------------------------------- 5. the two consumers
@pytest.fixture(scope="module")
def handles(ctx):
    import plonk_prototype_amd as pa
    h = S.Hades("5_2_per_round")
    g = pa.JubJubBase(ctx, J.GENERATOR)
    hades = pa.Hades(ctx, M.to_limbs(h.flat_ark), M.to_limbs(h.flat_mds), h.rounds, h.full)
    yield g, hades
    g.free(), hades.free()


def test_scan_bytes_is_scan_on_the_decoded_points(ctx, handles):
    import plonk_prototype_amd as pa
    g, hades = handles
    rng = random.Random(41)
    n, L = NMAX, 2   # noqa: N806
    c = pa.PoseidonCipher(hades, L)
    vk = [rng.randrange(1, R) for _ in range(3)]
    pk = g.mul(vk)
    owner = np.array([i % 3 for i in range(n)])              # a third of the notes for vk[0]
    e = [rng.randrange(1, R) for _ in range(n)]
    nonces = M.to_limbs([rng.randrange(R) for _ in range(n)])
    msgs = M.to_limbs([rng.randrange(R) for _ in range(L * n)]).reshape(n, L, 4)
    eph, ciphers = c.encrypt_to(g, pk[owner], e, nonces, msgs)
    data = pa.jubjub_compress(ctx, eph)
    eph_int = [(a, b) for a, b in zip(*[iter(pa.field.fr_vec_from_limbs(eph.reshape(-1, 4)))] * 2)]
    assert data.tobytes() == b"".join(CM.encode(p) for p in eph_int), "the device's encoding of its own ephemeral keys"
    # four of the key's own notes: three keys that do not decode, one with the sign bit flipped
    data = data.copy()
    at, reason = {0: CM.y_bytes(R), 63: CM.y_bytes(2), 129: CM.y_bytes(1, 1)}, {0: 1, 63: 2, 129: 3}
    for i, row in at.items():
        assert owner[i] == 0
        data[i] = np.frombuffer(row, np.uint8)
    assert owner[66] == 0 and eph_int[66][0] != 0
    data[66, 31] ^= 0x80
    decoded = [CM.decode(row.tobytes()) for row in data]
    assert [d[1] for d in decoded] == [reason.get(i, 0) for i in range(n)]
    assert decoded[66][0] == (R - eph_int[66][0], eph_int[66][1])
    want_m, want_s = c.scan(vk[0], J.to_limbs([d[0] for d in decoded]), nonces, ciphers)
    got_m, got_s = c.scan_bytes(vk[0], data, nonces, ciphers)
    assert got_s.tolist() == want_s.tolist() and got_m.tobytes() == want_m.tobytes()
    exp = np.where(owner == 0, 0, 3)
    exp[list(at)] = 1                                        # PM_CIPHER_POINT
    exp[66] = 3                                              # -R: another secret, PM_CIPHER_TAG
    assert got_s.tolist() == exp.tolist()
    assert not got_m[got_s != 0].any() and got_m[got_s == 0].tobytes() == msgs[got_s == 0].tobytes()
    # with the subgroup flag the same notes open: every e G lies in the subgroup
    flag_m, flag_s = c.scan_bytes(vk[0], data, nonces, ciphers, check_subgroup=True)
    assert flag_s.tolist() == exp.tolist() and flag_m.tobytes() == got_m.tobytes()
    assert c.scan_bytes(vk[0], data[:0], nonces[:0], ciphers[:0])[1].shape == (0,)


def test_verify_bytes_gives_the_reasons_of_verify(ctx, handles):
    import plonk_prototype_amd as pa
    g, hades = handles
    rng = random.Random(43)
    n = 65
    s = pa.Schnorr(g, hades)
    sk = [rng.randrange(1, J.Q) for _ in range(n)]
    k = [rng.randrange(1, J.Q) for _ in range(n)]
    msgs = M.to_limbs([rng.randrange(R) for _ in range(n)])
    pk = s.public_keys(sk)
    sig = s.sign(sk, msgs, k)                                # integers in: a canonical u
    assert not s.verify(pk, msgs, sig, scalar_form=1).any()
    sig_bytes = s.signatures_to_bytes(sig, scalar_form=1)
    assert sig_bytes.shape == (n, 64) and sig_bytes.dtype == np.uint8
    assert sig_bytes[:, :32].tobytes() == sig[:, 0].tobytes(), "the canonical u, little-endian"
    assert sig_bytes[:, 32:].tobytes() == pa.jubjub_compress(ctx, np.ascontiguousarray(sig[:, 1:])).tobytes()
    mont = s.sign(M.to_limbs(sk), msgs, M.to_limbs(k))       # limbs in: a Montgomery u, the same bytes out
    assert s.signatures_to_bytes(mont).tobytes() == sig_bytes.tobytes()
    pk_bytes = pa.jubjub_compress(ctx, pk)
    assert s.verify_bytes(pk_bytes, msgs, sig_bytes).tolist() == [0] * n
    # a flipped sign bit in R, an R that does not decode, a public key that does not decode
    sig_bytes, pk_bytes, sig2, pk2 = sig_bytes.copy(), pk_bytes.copy(), sig.copy(), pk.copy()
    sig_bytes[3, 63] ^= 0x80
    rx = pa.field.fr_from_limbs(sig[3, 1])
    assert rx != 0
    sig2[3, 1] = pa.field.fr_to_limbs(R - rx)
    sig_bytes[40, 32:] = np.frombuffer(CM.y_bytes(2), np.uint8)
    sig2[40, 1:] = 0
    pk_bytes[64] = np.frombuffer(CM.y_bytes(R), np.uint8)
    pk2[64] = 0
    want = s.verify(pk2, msgs, sig2, scalar_form=1)
    got = s.verify_bytes(pk_bytes, msgs, sig_bytes)
    assert got.tolist() == want.tolist()
    assert [int(got[i]) for i in (3, 40, 64)] == [4, 2, 3] and int(np.count_nonzero(got)) == 3
    assert s.verify_bytes(pk_bytes[:0], msgs[:0], sig_bytes[:0]).shape == (0,)


# ---------------------------------------------------------------------------------- 6. every table entry and every search digit
def table_sqrt_case():
    """the plain set of tests/fr_sqrt_cases.py: (limbs, the CONSTRUCTED roots as limbs, flags, the count of squares)"""
    if "table_sqrt" not in _CACHE:
        cases = F.plain_set()
        flags = np.array([c.flag for c in cases], np.uint32)
        even = sum(1 for c in cases if c.k is not None and c.k % 2 == 0)
        assert int(flags.sum()) == even + 1, "the even logarithms and the zero input"
        _CACHE["table_sqrt"] = (M.to_limbs([c.a for c in cases]), M.to_limbs([c.root for c in cases]), flags, even + 1)
    return _CACHE["table_sqrt"]


def table_decode_case(flag):
    """the ratio set: (bytes [n, 32], the model's points as limbs, its statuses)"""
    if ("table_decode", flag) not in _CACHE:
        want = F.ratio_expected(flag)
        _CACHE["table_decode", flag] = (_enc(F.ratio_set()), J.to_limbs([p for p, _ in want]), np.array([s for _, s in want], np.uint32))
    return _CACHE["table_decode", flag]


def _rows(got, want):
    return np.flatnonzero((got.reshape(len(want), -1) != want.reshape(len(want), -1)).any(axis=1))[:8]


def test_fr_sqrt_reads_every_reachable_table_entry(ctx):
    """pm_fr_sqrt_dev on the whole plain set in one call -- 4239 elements whose logarithms carry every digit in every window of
    the search and of the correction (tests/test_fr_sqrt_tables.py proves it, and that a wrong entry or key changes a root of
    this set) -- against roots known by construction: out of place, again from the same bytes, and in place."""
    import plonk_prototype_amd as pa
    vals, roots, flags, squares = table_sqrt_case()
    n = len(vals)
    assert n % 64 != 0 and n > 4096
    d = pa.DeviceVector.from_host(ctx, vals)
    out = pa.DeviceVector.from_host(ctx, np.full((n, 4), SENTINEL, np.uint64))
    f = pa.DeviceVector.from_host(ctx, np.full(((n + 7) // 8, 4), SENTINEL, np.uint64))
    try:
        for again in (False, True):
            assert pa.fr_sqrt_dev(ctx, d.ptr, n, out.ptr, f.ptr, want_count=True) == squares, again
            got, words = out.to_host(), f.to_host().view(np.uint32).reshape(-1)
            assert words[:n].tolist() == flags.tolist(), (again, np.flatnonzero(words[:n] != flags)[:8])
            assert got.tobytes() == roots.tobytes(), (again, _rows(got, roots))
            assert (words[n:] == 0x77777777).all() and d.to_host().tobytes() == vals.tobytes()
        assert pa.fr_sqrt_dev(ctx, d.ptr, n, d.ptr, f.ptr, want_count=True) == squares          # in place
        got = d.to_host()
        assert got.tobytes() == roots.tobytes(), _rows(got, roots)
        assert f.to_host().view(np.uint32).reshape(-1)[:n].tolist() == flags.tolist()
    finally:
        d.free(), out.free(), f.free()


@pytest.mark.parametrize("flag", (False, True), ids=("plain", "subgroup"))
def test_decompress_reads_every_reachable_table_entry(ctx, flag):
    """pm_jubjub_decompress_dev on the whole ratio set: 764 seeded y kept out of 3985 drawn, each with both sign bits, and one
    y that is not below r: 1529 encodings.  Their radicands carry every digit in every window of the search and, on squares,
    of the correction.  Points and statuses against the model; the count; and the encoder gives the bytes back.  It is the run
    WITHOUT the flag that covers the tables: with it seven points in eight are refused as not in the subgroup whatever root was
    found, so a wrong root hides behind the refusal; that run checks the second kernel over the same records."""
    import plonk_prototype_amd as pa
    data, points, status = table_decode_case(flag)
    n = len(data)
    assert n == 2 * len(F.ratio_ys()[0]) + 1 == 1529 and F.ratio_ys()[1] == 3985
    good = status == 0
    db = pa.DeviceVector.from_host(ctx, data.view(np.uint64))
    out = pa.DeviceVector.from_host(ctx, np.full((2 * n, 4), SENTINEL, np.uint64))
    ds = pa.DeviceVector.from_host(ctx, np.full(((n + 7) // 8, 4), SENTINEL, np.uint64))
    back = pa.DeviceVector.from_host(ctx, np.full((n, 4), SENTINEL, np.uint64))
    try:
        assert pa.jubjub_decompress_dev(ctx, db.ptr, n, out.ptr, ds.ptr, flag) == int(good.sum())
        got, words = out.to_host().reshape(n, 2, 4), ds.to_host().view(np.uint32).reshape(-1)
        assert words[:n].tolist() == status.tolist(), np.flatnonzero(words[:n] != status)[:8]
        assert got.tobytes() == points.tobytes(), _rows(got, points)
        assert (words[n:] == 0x77777777).all() and not got[~good].any()
        # the decoded points, refused ones and all, through the encoder: the rows that decoded are the input bytes
        pa.jubjub_compress_dev(ctx, out.ptr, n, back.ptr)
        ctx.sync()
        again = back.to_host().view(np.uint8).reshape(n, 32)
        assert again[good].tobytes() == data[good].tobytes(), _rows(again[good], data[good])
    finally:
        db.free(), out.free(), ds.free(), back.free()


def test_fr_sqrt_slice_on_a_callers_stream_without_flags(ctx):
    """d_is_square = NULL and no count, asynchronous on a caller's stream: a slice of the plain set that starts inside a wave
    and ends inside another"""
    import plonk_prototype_amd as pa
    import torch
    vals, roots, _, _ = table_sqrt_case()
    lo, n = 37, 1000
    st = torch.cuda.Stream()
    d = pa.DeviceVector.from_host(ctx, vals)
    out = pa.DeviceVector.from_host(ctx, np.full((len(vals), 4), SENTINEL, np.uint64))
    try:
        assert pa.fr_sqrt_dev(ctx, d.ptr + 32 * lo, n, out.ptr + 32 * lo, 0, stream=st.cuda_stream) is None
        st.synchronize()
        got = out.to_host()
        assert got[lo:lo + n].tobytes() == roots[lo:lo + n].tobytes(), lo + _rows(got[lo:lo + n], roots[lo:lo + n])
        assert (got[:lo] == SENTINEL).all() and (got[lo + n:] == SENTINEL).all(), "nothing outside the slice is written"
    finally:
        d.free(), out.free()
