"""The JubJub wire format without a device: the new exports are declared, bound, exported and
documented, and the three host forms -- pm_fr_sqrt_host, pm_jubjub_compress, pm_jubjub_decompress -- agree byte for byte with
the big-integer model of tests/jubjub_codec_model.py on known encodings, on the edge points, on every kind of refusal and on
the logarithms at which a windowed square root goes wrong."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gadget_model as M  # noqa: E402
import jubjub_codec_model as CM  # noqa: E402
import jubjub_model as J  # noqa: E402

R = CM.R
EXPORTS = ("pm_fr_sqrt_dev", "pm_fr_sqrt_host", "pm_jubjub_compress", "pm_jubjub_decompress", "pm_jubjub_compress_dev",
           "pm_jubjub_decompress_dev", "pm_dev_copy_strided")
PY_NAMES = ("fr_sqrt", "fr_sqrt_dev", "fr_sqrt_host", "jubjub_compress", "jubjub_compress_dev", "jubjub_compress_host",
            "jubjub_decompress", "jubjub_decompress_dev", "jubjub_decompress_host", "JUBJUB_CODEC_REASONS")


def _limbs(v: int) -> np.ndarray:
    from plonk_prototype_amd.field import fr_to_limbs
    return fr_to_limbs(v)


def _int(limbs) -> int:
    from plonk_prototype_amd.field import fr_from_limbs
    return fr_from_limbs(limbs)


def _point(limbs):
    return _int(limbs[0]), _int(limbs[1])


def test_exports_are_declared_bound_exported_and_documented():
    import plonk_prototype_amd as pa
    from plonk_prototype_amd import _lib
    header = open(os.path.join(ROOT, "include", "plonk_mi355x.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    lib = C.CDLL(pa.LIB_PATH)
    for name in EXPORTS:
        assert re.search(r"\b%s\s*\(" % name, header), f"{name} is not declared in the header"
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
        assert "pub fn %s(" % name in doc, f"{name} is missing from INTEGRATION.md's extern block"
    for name in PY_NAMES:
        assert hasattr(pa, name), f"plonk_prototype_amd.{name} is not exported"
    assert callable(pa.PoseidonCipher.scan_bytes) and callable(pa.Schnorr.verify_bytes) and callable(pa.Schnorr.signatures_to_bytes)
    for k, name in enumerate(("OK", "BAD_RANGE", "BAD_NOT_ON_CURVE", "BAD_SIGN", "BAD_NOT_IN_SUBGROUP")):
        assert re.search(r"#define PM_JUBJUB_%s %du\b" % (name, k), header), name
        assert getattr(_lib, "JUBJUB_" + name) == k
    assert (CM.OK, CM.BAD_RANGE, CM.BAD_NOT_ON_CURVE, CM.BAD_SIGN, CM.BAD_NOT_IN_SUBGROUP) == (0, 1, 2, 3, 4)
    assert "#define PM_JUBJUB_CHECK_SUBGROUP 1u" in header and _lib.JUBJUB_CHECK_SUBGROUP == 1
    assert pa.JUBJUB_CODEC_REASONS == {1: "range", 2: "not_on_curve", 3: "sign", 4: "not_in_subgroup"}
    block = header[header.index("JubJub wire format"):header.index("#define PM_JUBJUB_CHECK_SUBGROUP")].replace("\n * ", " ")
    assert "prior knowledge" in block and "REFUSED" in block and "OFF by default" in block


def test_the_model_itself():
    """the constants the model and the library's tables rest on, and the claims the header makes about the curve"""
    import json
    with open(os.path.join(ROOT, "tests", "golden", "constants.json")) as f:
        consts = json.load(f)
    assert int(consts["root_of_unity"], 16) == CM.ROOT_OF_UNITY and int(consts["r"], 16) == R
    assert pow(CM.ROOT_OF_UNITY, 1 << 31, R) == R - 1          # of order exactly 2^32
    assert M._sqrt((-pow(CM.D, -1, R)) % R) is None             # -1 / d is a non-square: 1 + d y^2 is never zero
    assert R % 4 == 1 and CM.sqrt_even(R - 1)[1] == 1
    for y in (2, 4, 6, 7, 8):                                   # the smallest y without an x
        assert CM.decode(CM.y_bytes(y))[1] == CM.BAD_NOT_ON_CURVE
    for a in CM.sqrt_edge_inputs():
        root, square = CM.sqrt_even(a)
        assert root % 2 == 0 and (root * root % R == a if square else root == 0)
    squares = [CM.sqrt_even(a)[1] for a in CM.sqrt_edge_inputs()]
    assert squares == [1, 1, 1, 1, 0, 0] + [1] * len(CM.LOG_SQUARES) + [0] * len(CM.LOG_NON_SQUARES)


def test_known_encodings():
    import plonk_prototype_amd as pa
    i = J.SQRT_M1
    cases = [(J.IDENTITY, bytes([1]) + bytes(31)),
             ((0, R - 1), (R - 1).to_bytes(32, "little")),
             ((i, 0), bytes(31) + bytes([0x80 * (i & 1)])),
             ((R - i, 0), bytes(31) + bytes([0x80 * ((R - i) & 1)])),
             (J.GENERATOR, bytes([0x12]) + bytes(31)),
             (M.curve_point(0x14), CM.encode(M.curve_point(0x14)))]
    assert {cases[2][1][31], cases[3][1][31]} == {0x00, 0x80}   # y = 0 with the two sign bits
    assert J.GENERATOR[0] % 2 == 0
    for p, want in cases:
        assert CM.encode(p) == want
        assert pa.jubjub_compress_host(p) == want, p
        got, status = pa.jubjub_decompress_host(want)
        assert status == 0 and _point(got) == p, p


def test_round_trips_on_edge_and_random_points():
    import plonk_prototype_amd as pa
    for p in J.edge_points() + CM.random_points(12):
        data = pa.jubjub_compress_host(p)
        assert data == CM.encode(p)
        got, status = pa.jubjub_decompress_host(data)
        assert (status, _point(got)) == (0, p) == (CM.decode(data)[1], CM.decode(data)[0])
        assert pa.jubjub_compress_host(got) == data               # limbs in, the same bytes out
        flipped = bytes(data[:31]) + bytes([data[31] ^ 0x80])
        want, st = CM.decode(flipped)
        got, status = pa.jubjub_decompress_host(flipped)
        assert (status, _point(got)) == (st, want)
        if p[0]:
            assert st == 0 and want == (R - p[0], p[1])
        else:
            assert st == CM.BAD_SIGN and want == (0, 0)


def test_random_bytes_decode_as_the_model_says():
    import random
    import plonk_prototype_amd as pa
    rng = random.Random(21)
    seen = set()
    for _ in range(60):
        data = CM.y_bytes(rng.randrange(R), rng.randrange(2))
        want, st = CM.decode(data)
        got, status = pa.jubjub_decompress_host(data)
        assert (status, _point(got)) == (st, want)
        if st == 0:
            assert pa.jubjub_compress_host(got) == data           # decode-then-encode is the identity
        seen.add(st)
    assert {0, 2} <= seen


def test_refusals():
    import plonk_prototype_amd as pa
    from plonk_prototype_amd import _lib
    lib = _lib.load()
    for data, st in CM.refusals():
        got, status = pa.jubjub_decompress_host(data)
        assert status == st == CM.decode(data)[1] and not got.any(), (data.hex(), st)
    # with the flag: points of small or composite order give 4, the identity and the generator pass
    for p, st in ((M.curve_point(0x14), 4), ((0, R - 1), 4), ((J.SQRT_M1, 0), 4), (J.IDENTITY, 0), (J.GENERATOR, 0)):
        data = CM.encode(p)
        assert CM.decode(data, True)[1] == st
        got, status = pa.jubjub_decompress_host(data, check_subgroup=True)
        assert status == st and _point(got) == (p if st == 0 else (0, 0))
        assert pa.jubjub_decompress_host(data)[1] == 0            # without it they decode
    # the flag does not change the earlier reasons
    for data, st in CM.refusals():
        assert pa.jubjub_decompress_host(data, check_subgroup=True)[1] == st
    # errors of the call
    out, status, buf = np.zeros(8, np.uint64), C.c_uint32(), (C.c_uint8 * 32)()
    u64p = _lib.u64p
    assert lib.pm_jubjub_decompress(buf, 2, out.ctypes.data_as(u64p), C.byref(status)) == _lib.PM_ERR_BAD_ARG
    assert lib.pm_jubjub_decompress(None, 0, out.ctypes.data_as(u64p), C.byref(status)) == _lib.PM_ERR_BAD_ARG
    assert lib.pm_jubjub_decompress(buf, 0, None, C.byref(status)) == _lib.PM_ERR_BAD_ARG
    assert lib.pm_jubjub_decompress(buf, 0, out.ctypes.data_as(u64p), None) == _lib.PM_ERR_BAD_ARG
    off = np.stack([_limbs(1), _limbs(2)])                        # (1, 2) is off the curve
    big = np.stack([np.frombuffer(R.to_bytes(32, "little"), dtype=np.uint64), _limbs(1)])   # x = r: not below r
    for bad in (off, big):
        assert lib.pm_jubjub_compress(np.ascontiguousarray(bad).ctypes.data_as(u64p), buf) == _lib.PM_ERR_BAD_ARG
    assert lib.pm_jubjub_compress(None, buf) == _lib.PM_ERR_BAD_ARG
    good = J.to_limbs([J.GENERATOR])
    assert lib.pm_jubjub_compress(good.ctypes.data_as(u64p), None) == _lib.PM_ERR_BAD_ARG
    with pytest.raises(ValueError):
        pa.jubjub_compress_host((1, 2))


def test_fr_sqrt_host():
    import plonk_prototype_amd as pa
    from plonk_prototype_amd import _lib
    inputs = CM.sqrt_inputs(len(CM.sqrt_edge_inputs()) + 64)
    flags = []
    for a in inputs:
        root, flag = pa.fr_sqrt_host(_limbs(a))
        x = _int(root)
        want, square = CM.sqrt_even(a)
        assert flag == square and x == want, hex(a)
        assert x % 2 == 0 and (x * x % R == a if flag else x == 0)
        assert int.from_bytes(root.tobytes(), "little") < R      # canonical limbs
        flags.append(flag)
    assert 0 in flags[18:] and 1 in flags[18:]                    # both classes among the random ones
    # limbs that are not below r: flag 0 and root 0
    for v in (R, R + 1, (1 << 256) - 1):
        root, flag = pa.fr_sqrt_host(np.frombuffer(v.to_bytes(32, "little"), dtype=np.uint64).copy())
        assert flag == 0 and not root.any()
    lib = _lib.load()
    a, out, f = _limbs(4), np.zeros(4, np.uint64), C.c_uint32()
    u64p = _lib.u64p
    assert lib.pm_fr_sqrt_host(None, out.ctypes.data_as(u64p), C.byref(f)) == _lib.PM_ERR_BAD_ARG
    assert lib.pm_fr_sqrt_host(a.ctypes.data_as(u64p), None, C.byref(f)) == _lib.PM_ERR_BAD_ARG
    assert lib.pm_fr_sqrt_host(a.ctypes.data_as(u64p), out.ctypes.data_as(u64p), None) == _lib.PM_ERR_BAD_ARG
