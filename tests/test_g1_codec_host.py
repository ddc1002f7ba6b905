"""The host single-point forms pm_g1_compress / pm_g1_decompress (no GPU) against the big-int oracle and the Python
decoder, every rejection with its reason, and the byte-level contract of the compressed commit-key form in srs.py.
Vectors: tests/golden/g1_encoding.json (generator: tests/golden/make_g1_encoding.py)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from oracle import bigint_oracle as B

HERE = os.path.dirname(os.path.abspath(__file__))
P, R = B.P_MOD, B.R_MOD


@pytest.fixture(scope="module")
def vectors():
    with open(os.path.join(HERE, "golden", "g1_encoding.json")) as f:
        vs = json.load(f)["vectors"]
    for v in vs:
        v["bytes"] = bytes.fromhex(v["hex"])
        v["point"] = None if v["x"] is None else (int(v["x"], 16), int(v["y"], 16))
    return {v["name"]: v for v in vs}


def _limbs(pt):
    from plonk_prototype_amd.field import fp_to_limbs
    return np.zeros(12, np.uint64) if pt is None else np.concatenate([fp_to_limbs(pt[0]), fp_to_limbs(pt[1])])


def _decompress(data, flags):
    """-> (status, reason, xy) of the raw call"""
    import plonk_prototype_amd as pa
    lib = pa.load()
    out, reason = np.zeros(12, np.uint64), C.c_uint32(0)
    rc = lib.pm_g1_decompress((C.c_uint8 * 48).from_buffer_copy(data), flags, out.ctypes.data_as(pa._lib.u64p), C.byref(reason))
    return rc, reason.value, out


def test_fixture_is_what_its_generator_says(vectors):
    """spot checks of the committed file with the oracle: the encodings, the curve equation, [r]P for a few points"""
    def mul_plain(k, pt):
        acc = None
        for bit in bin(k)[2:]:
            acc = B.g1_add(acc, acc)
            if bit == "1":
                acc = B.g1_add(acc, pt)
        return acc
    assert len(vectors) == 99
    for v in vectors.values():
        if v["curve_reason"] == 0:
            assert B.g1_is_on_curve(v["point"]) and B.g1_compress(v["point"]) == v["bytes"], v["name"]
    for name in ("generator", "order3", "generator_plus_order3", "small_x_4", "small_x_17", "cofactor_cleared_x4", "subgroup_7"):
        assert (mul_plain(R, vectors[name]["point"]) is None) == vectors[name]["in_subgroup"], name
    assert vectors["order3"]["point"] == (0, 2) and mul_plain(R, (0, 2)) == (0, 2)
    assert [vectors[n]["hex"][:2] for n in ("order3", "order3_neg", "identity")] == ["80", "a0", "c0"]
    assert vectors["cofactor_cleared_x4"]["point"] is not None and vectors["cofactor_cleared_x4"]["in_subgroup"]


def test_generator_has_its_known_bytes(vectors, golden):
    import plonk_prototype_amd as pa
    known = golden["constants"]["g1_compressed"]
    assert known.startswith("97f1d3a7") and known.endswith("c6bb")
    assert pa.g1_compress(pa.host.G1_GENERATOR).hex() == known == vectors["generator"]["hex"]
    assert np.array_equal(pa.g1_decompress(bytes.fromhex(known)), pa.host.G1_GENERATOR)


def test_round_trip_against_both_references(vectors):
    import plonk_prototype_amd as pa
    from plonk_prototype_amd import transcript as T
    names = ["generator", "generator_neg", "identity"] + [f"subgroup_{i}" for i in range(32)]
    for name in names:
        v = vectors[name]
        xy = pa.g1_decompress(v["bytes"])
        assert np.array_equal(xy, T.g1_decompress(v["bytes"])) and np.array_equal(xy, _limbs(v["point"])), name
        assert pa.g1_compress(xy) == B.g1_compress(v["point"]) == T.g1_compress(xy) == v["bytes"], name
    a = vectors["subgroup_4"]      # both signs of one x come back as each other's negation
    pos = pa.g1_decompress(a["bytes"])
    flipped = bytearray(a["bytes"])
    flipped[0] ^= 0x20
    neg = pa.g1_decompress(bytes(flipped))
    assert np.array_equal(neg[:6], pos[:6]) and np.array_equal(neg, _limbs(B.g1_neg(a["point"])))


@pytest.mark.parametrize("name,reason", [
    ("compression_bit_clear", 1), ("compression_bit_clear_sign", 1), ("infinity_with_sign", 1),
    ("infinity_with_stray_low_bit", 1), ("infinity_with_stray_high_bit", 1), ("x_equals_p", 1), ("x_equals_p_plus_1", 1),
    ("x_all_ones", 1), ("no_root_x_1", 2), ("no_root_x_2", 2), ("no_root_x_3", 2), ("no_root_x_2_sign", 2)])
def test_malformed_and_off_curve_inputs(vectors, name, reason):
    import plonk_prototype_amd as pa
    v = vectors[name]
    assert v["curve_reason"] == reason
    for flags in (0, 1):
        rc, got, xy = _decompress(v["bytes"], flags)
        assert (rc, got) == (pa._lib.PM_ERR_POINT, reason) and not xy.any()
    with pytest.raises(pa.Error) as e:
        pa.g1_decompress(v["bytes"], check_subgroup=False)
    assert e.value.code == -9 and e.value.bad_reason == reason
    with pytest.raises(ValueError):
        pa.transcript.g1_decompress(v["bytes"])


@pytest.mark.parametrize("name", ["small_x_4", "order3", "order3_neg", "generator_plus_order3"] +
                         [f"small_x_{x}" for x in (5, 6, 8, 9, 10, 11, 12, 15, 17)])
def test_points_outside_the_subgroup(vectors, name):
    v = vectors[name]
    assert v["in_subgroup"] is False
    rc, reason, xy = _decompress(v["bytes"], 1)
    assert (rc, reason) == (-9, 3) and not xy.any()
    rc, _, xy = _decompress(v["bytes"], 0)
    assert rc == 0 and np.array_equal(xy, _limbs(v["point"]))


def test_subgroup_points_pass_the_check(vectors):
    for name in ["generator", "identity", "cofactor_cleared_x4"] + [f"subgroup_{i}" for i in range(32, 64)]:
        rc, _, xy = _decompress(vectors[name]["bytes"], 1)
        assert rc == 0 and np.array_equal(xy, _limbs(vectors[name]["point"])), name


def test_arguments():
    import plonk_prototype_amd as pa
    lib = pa.load()
    out = np.zeros(12, np.uint64)
    buf = (C.c_uint8 * 48)()
    assert lib.pm_g1_decompress(None, 0, out.ctypes.data_as(pa._lib.u64p), None) == -1
    assert lib.pm_g1_decompress(buf, 0, None, None) == -1
    assert lib.pm_g1_decompress(buf, 2, out.ctypes.data_as(pa._lib.u64p), None) == -1
    assert lib.pm_g1_decompress(buf, 0, out.ctypes.data_as(pa._lib.u64p), None) == -9      # the reason may be NULL
    assert lib.pm_g1_compress(None, buf) == -1 and lib.pm_g1_compress(out.ctypes.data_as(pa._lib.u64p), None) == -1
    with pytest.raises(ValueError):
        pa.g1_decompress(bytes(47))


def test_compressed_commit_key_round_trip(vectors):
    """srs.commit_key_to_bytes / commit_key_from_bytes without a context: the host path"""
    import plonk_prototype_amd as pa
    names = ["generator", "identity", "generator_neg"] + [f"subgroup_{i}" for i in range(8)]
    pts = np.stack([_limbs(vectors[n]["point"]) for n in names])
    data = pa.srs.commit_key_to_bytes(pts)
    assert data == b"".join(vectors[n]["bytes"] for n in names)
    assert np.array_equal(pa.srs.commit_key_from_bytes(data), pts)
    bad = data[:48 * 5] + vectors["small_x_4"]["bytes"] + data[48 * 6:]
    assert np.array_equal(pa.srs.commit_key_from_bytes(bad, check_subgroup=False)[5], _limbs(vectors["small_x_4"]["point"]))
    with pytest.raises(pa.Error) as e:
        pa.srs.commit_key_from_bytes(bad)
    assert (e.value.code, e.value.bad_index, e.value.bad_reason) == (-9, 5, 3)


def test_compressed_commit_key_lengths():
    import plonk_prototype_amd as pa
    with pytest.raises(ValueError):
        pa.srs.commit_key_from_bytes(bytes(49))
    with pytest.raises(ValueError):
        pa.srs.commit_key_from_bytes(bytes(47))
    assert pa.srs.commit_key_from_bytes(b"").shape == (0, 12)
    assert pa.srs.commit_key_to_bytes(np.zeros((0, 12), np.uint64)) == b""
    assert pa.srs.G1_COMPRESSED == 48


def test_compressed_commit_key_bytes_are_the_per_point_encodings(vectors):
    """CommitKey::to_var_bytes is the points' encodings back to back: what commit_key_from_bytes must invert, checked
    here with the host decoder point by point (the device path: tests/test_gpu_g1_codec.py)"""
    import plonk_prototype_amd as pa
    names = ["generator", "identity", "subgroup_1", "subgroup_2"]
    data = b"".join(vectors[n]["bytes"] for n in names)
    pts = np.stack([pa.g1_decompress(data[48 * i:48 * i + 48]) for i in range(len(names))])
    assert np.array_equal(pts, np.stack([_limbs(vectors[n]["point"]) for n in names]))
    assert b"".join(pa.g1_compress(p) for p in pts) == data
    # and the raw form still round-trips the same points
    assert np.array_equal(pa.srs.commit_key_from_raw_bytes(pa.srs.commit_key_to_raw_bytes(pts)), pts)
