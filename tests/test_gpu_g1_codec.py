"""Checked commit-key loading on the device: pm_g1_decompress_dev / pm_g1_compress_dev / pm_g1_check_dev and the
conveniences above them, against the big-int oracle, the Python decoder (transcript.g1_decompress) and the host
encoder -- vectors from tests/golden/g1_encoding.json (generator: tests/golden/make_g1_encoding.py)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from oracle import bigint_oracle as B
from oracle.cpu_oracle import ints_to_limbs

pytestmark = pytest.mark.gpu

P = B.P_MOD
HERE = os.path.dirname(os.path.abspath(__file__))
TAU = 0x1F3A5C7E9B2D4F60718293A4B5C6D7E8F9


@pytest.fixture(scope="module")
def vectors():
    with open(os.path.join(HERE, "golden", "g1_encoding.json")) as f:
        vs = json.load(f)["vectors"]
    for v in vs:
        v["bytes"] = bytes.fromhex(v["hex"])
        v["point"] = None if v["x"] is None else (int(v["x"], 16), int(v["y"], 16))
    return vs


def _limbs(pt):
    from plonk_prototype_amd.field import fp_to_limbs
    return np.zeros(12, np.uint64) if pt is None else np.concatenate([fp_to_limbs(pt[0]), fp_to_limbs(pt[1])])


def _dev_bytes(ctx, data):
    """bytes -> a device buffer (rounded up to whole 32-byte elements)"""
    import plonk_prototype_amd as pa
    raw = np.zeros((len(data) + 31) // 32 * 32, np.uint8)
    raw[:len(data)] = np.frombuffer(data, np.uint8)
    return pa.DeviceVector.from_host(ctx, raw.view(np.uint64).reshape(-1, 4))


def _decompress(ctx, data, subgroup):
    """-> (status, bad_index, bad_reason, out [n, 12]) of pm_g1_decompress_dev on n x 48 host bytes"""
    import plonk_prototype_amd as pa
    n = len(data) // 48
    d_in, d_out = _dev_bytes(ctx, data), pa.DeviceVector(ctx, 3 * n)
    idx, reason = C.c_uint64(0), C.c_uint32(0)
    rc = ctx._lib.pm_g1_decompress_dev(ctx._h, d_in._p, n, 1 if subgroup else 0, d_out._p, C.byref(idx), C.byref(reason), None)
    out = d_out.to_host().reshape(n, 12)
    d_in.free()
    d_out.free()
    return rc, idx.value, reason.value, out


def _compress(ctx, xy):
    import plonk_prototype_amd as pa
    xy = np.ascontiguousarray(xy, np.uint64).reshape(-1, 12)
    n = xy.shape[0]
    d_in, d_out = pa.DeviceVector.from_host(ctx, xy.reshape(-1, 4)), pa.DeviceVector(ctx, (3 * n + 1) // 2)
    ctx.g1_compress_dev(d_in.ptr, n, d_out.ptr)
    out = d_out.to_host().tobytes()[:48 * n]
    d_in.free()
    d_out.free()
    return out


def _check(ctx, xy, subgroup):
    import plonk_prototype_amd as pa
    xy = np.ascontiguousarray(xy, np.uint64).reshape(-1, 12)
    d = pa.DeviceVector.from_host(ctx, xy.reshape(-1, 4))
    idx, reason = C.c_uint64(0), C.c_uint32(0)
    rc = ctx._lib.pm_g1_check_dev(ctx._h, d._p, xy.shape[0], 1 if subgroup else 0, C.byref(idx), C.byref(reason), None)
    d.free()
    return rc, idx.value, reason.value


def _good(vectors):
    """subgroup points of both signs with identities mixed in"""
    sub = [v for v in vectors if v["name"].startswith("subgroup_") or v["name"] in ("generator", "generator_neg")]
    ident = next(v for v in vectors if v["name"] == "identity")
    out = []
    for i, v in enumerate(sub):
        out.append(v)
        if i % 7 == 3:
            out.append(ident)
    return out


def _batch(vectors, n):
    good = _good(vectors)
    return [good[(5 * i + 1) % len(good)] for i in range(n)]


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 257])
def test_round_trip(ctx, vectors, n):
    import plonk_prototype_amd as pa
    from plonk_prototype_amd import transcript as T
    batch = _batch(vectors, n)
    data = b"".join(v["bytes"] for v in batch)
    rc, _, _, xy = _decompress(ctx, data, True)
    assert rc == 0
    for i, v in enumerate(batch):
        assert np.array_equal(xy[i], T.g1_decompress(v["bytes"])), (i, v["name"])
        assert np.array_equal(xy[i], _limbs(v["point"]))
    back = _compress(ctx, xy)
    assert back == data
    for i, v in enumerate(batch):
        assert back[48 * i:48 * i + 48] == pa.g1_compress(xy[i]) == B.g1_compress(v["point"])


def test_generator_bytes_are_the_pinned_ones(ctx, golden):
    import plonk_prototype_amd as pa
    assert _compress(ctx, pa.host.G1_GENERATOR).hex() == golden["constants"]["g1_compressed"]


def _expected_reason(v, subgroup):
    return v["curve_reason"] or (3 if subgroup and not v["in_subgroup"] else 0)


@pytest.mark.parametrize("subgroup", [False, True])
def test_every_vector_alone(ctx, vectors, subgroup):
    """all 99 vectors in one batch would report only the first failure: each gets a batch of its own, in one buffer of
    single-point calls' worth -- here: one call per vector"""
    for v in vectors:
        rc, idx, reason, xy = _decompress(ctx, v["bytes"], subgroup)
        exp = _expected_reason(v, subgroup)
        assert (rc, reason if rc else 0) == (-9 if exp else 0, exp), v["name"]
        if exp:
            assert idx == 0 and not xy.any(), v["name"]
        else:
            assert np.array_equal(xy[0], _limbs(v["point"])), v["name"]


@pytest.mark.parametrize("pos", [0, 63, 64, 256])
@pytest.mark.parametrize("bad", ["compression_bit_clear", "x_equals_p", "no_root_x_2", "small_x_4", "order3", "generator_plus_order3"])
def test_one_bad_point_in_a_batch(ctx, vectors, pos, bad):
    v = next(x for x in vectors if x["name"] == bad)
    batch = _batch(vectors, 257)
    batch[pos] = v
    data = b"".join(x["bytes"] for x in batch)
    for subgroup in (False, True):
        exp = _expected_reason(v, subgroup)
        rc, idx, reason, xy = _decompress(ctx, data, subgroup)
        if not exp:
            assert rc == 0 and np.array_equal(xy[pos], _limbs(v["point"]))
            continue
        assert (rc, idx, reason) == (-9, pos, exp)
        assert not xy[pos].any()
        for i, x in enumerate(batch):
            if i != pos:
                assert np.array_equal(xy[i], _limbs(x["point"])), i


def test_lowest_index_is_reported(ctx, vectors):
    by = {v["name"]: v for v in vectors}
    batch = _batch(vectors, 257)
    batch[200], batch[70], batch[130] = by["compression_bit_clear"], by["small_x_5"], by["no_root_x_3"]
    data = b"".join(x["bytes"] for x in batch)
    rc, idx, reason, xy = _decompress(ctx, data, True)
    assert (rc, idx, reason) == (-9, 70, 3)
    assert not xy[70].any() and not xy[130].any() and not xy[200].any()
    rc, idx, reason, xy = _decompress(ctx, data, False)
    assert (rc, idx, reason) == (-9, 130, 2)
    assert np.array_equal(xy[70], _limbs(by["small_x_5"]["point"]))
    import plonk_prototype_amd as pa
    with pytest.raises(pa.Error) as e:
        pa.srs.commit_key_from_bytes(data, ctx)
    assert (e.value.code, e.value.bad_index, e.value.bad_reason) == (-9, 70, 3) and "70" in str(e.value)


def test_subgroup_verdict(ctx, vectors):
    """[r]P by the fixture's big-int double-and-add decides; no point may be misjudged either way"""
    names = {f"small_x_{x}" for x in (4, 5, 6, 8, 9, 10, 11, 12, 15, 17)} | {"order3", "order3_neg", "generator_plus_order3",
                                                                               "cofactor_cleared_x4", "identity"}
    pts = [v for v in vectors if v["name"] in names or v["name"].startswith("subgroup_")]
    assert len(pts) == 15 + 64 and sum(not v["in_subgroup"] for v in pts) == 13
    for v in pts:
        rc, _, reason = _check(ctx, _limbs(v["point"]), True)
        assert (rc == 0) == v["in_subgroup"], v["name"]
        assert rc == 0 or (rc, reason) == (-9, 3)
        assert _check(ctx, _limbs(v["point"]), False)[0] == 0
    # the same in one call each way round: all good, then with the first bad one at its place
    good = np.stack([_limbs(v["point"]) for v in pts if v["in_subgroup"]])
    assert _check(ctx, good, True)[0] == 0
    mixed = np.stack([_limbs(v["point"]) for v in pts])
    first_bad = next(i for i, v in enumerate(pts) if not v["in_subgroup"])
    assert _check(ctx, mixed, True) == (-9, first_bad, 3)


def test_check_raw_points(ctx, vectors):
    import plonk_prototype_amd as pa
    from plonk_prototype_amd.field import fp_to_limbs
    good = np.stack([_limbs(v["point"]) for v in _batch(vectors, 130)])
    assert _check(ctx, good, True)[0] == 0
    G = B.G1_GEN
    off = good.copy()
    off[65, 6:] = fp_to_limbs(G[1] + 1)
    off[65, :6] = fp_to_limbs(G[0])
    assert _check(ctx, off, True) == (-9, 65, 2) and _check(ctx, off, False) == (-9, 65, 2)
    noncanon = good.copy()
    noncanon[129, :6] = np.frombuffer(P.to_bytes(48, "little"), np.uint64)
    assert _check(ctx, noncanon, False) == (-9, 129, 1)
    noncanon[3, 6:] = np.frombuffer(((1 << 384) - 1).to_bytes(48, "little"), np.uint64)
    assert _check(ctx, noncanon, True) == (-9, 3, 1)
    outside = good.copy()
    outside[64] = _limbs(next(v for v in vectors if v["name"] == "generator_plus_order3")["point"])
    assert _check(ctx, outside, False)[0] == 0 and _check(ctx, outside, True) == (-9, 64, 3)
    # resident bases (pm_g1_bases_check) and the host mirrors
    pa.CommitKey(good, ctx).check()
    for arr, subgroup, where in ((off, False, (65, 2)), (outside, True, (64, 3))):
        with pytest.raises(pa.Error) as e:
            pa.CommitKey(arr, ctx).check(subgroup)
        assert (e.value.code, e.value.bad_index, e.value.bad_reason) == (-9,) + where
    pa.CommitKey(outside, ctx).check(subgroup=False)


def test_arguments(ctx):
    lib, h = ctx._lib, ctx._h
    import plonk_prototype_amd as pa
    d = pa.DeviceVector(ctx, 6)
    assert lib.pm_g1_decompress_dev(h, None, 0, 0, None, None, None, None) == 0
    assert lib.pm_g1_check_dev(h, None, 0, 1, None, None, None) == 0
    assert lib.pm_g1_compress_dev(h, None, 0, None, None) == 0
    assert lib.pm_g1_decompress_dev(h, None, 1, 0, d._p, None, None, None) == -1
    assert lib.pm_g1_decompress_dev(h, d._p, 1, 2, d._p, None, None, None) == -1
    assert lib.pm_g1_check_dev(h, d._p, 1, 4, None, None, None) == -1
    assert lib.pm_g1_check_dev(h, None, 1, 0, None, None, None) == -1
    assert lib.pm_g1_compress_dev(h, d._p, 1, None, None) == -1
    assert lib.pm_g1_bases_check(h, None, 0, None, None) == -1
    out = C.c_void_p()
    assert lib.pm_g1_bases_from_compressed(h, None, 1, 0, C.byref(out), None, None) == -1
    assert lib.pm_g1_bases_from_compressed(h, b"\xc0" + bytes(47), 1, 8, C.byref(out), None, None) == -1
    # verdict pointers may be NULL on a failing call
    bad = _dev_bytes(ctx, bytes(48))
    assert lib.pm_g1_decompress_dev(h, bad._p, 1, 1, d._p, None, None, None) == -9
    assert b"point 0" in lib.pm_last_error(h)


def test_commit_key_end_to_end(ctx, oracle):
    import plonk_prototype_amd as pa
    from plonk_prototype_amd import prover as PR
    n = 1 << 12
    tau = oracle.fr_to_mont(ints_to_limbs([TAU % B.R_MOD], 4))[0]
    ck = pa.CommitKey.setup(n - 1, tau, ctx, host_copy=True)
    data = ck.to_bytes()
    assert len(data) == 48 * n
    assert data == b"".join(pa.transcript.g1_compress(p) for p in ck.powers_of_g)
    assert data == pa.srs.commit_key_to_bytes(ck.powers_of_g, ctx)
    assert np.array_equal(pa.srs.commit_key_from_bytes(data, ctx), ck.powers_of_g)
    ck2 = pa.CommitKey.from_bytes(data, ctx)
    assert ck2.max_degree() == n - 1 and ck2.to_bytes() == data
    ck2.check()
    poly = oracle.fr_sample(0x6731, n)
    assert np.array_equal(ck2.commit(poly), ck.commit(poly))
    # one flipped byte: point 1234 no longer decodes to a subgroup point (x + 1 has no root, is off the subgroup, or is >= p)
    broken = bytearray(data)
    broken[48 * 1234 + 47] ^= 1
    with pytest.raises(pa.Error) as e:
        pa.CommitKey.from_bytes(bytes(broken), ctx)
    assert e.value.code == -9 and e.value.bad_index == 1234 and e.value.bad_reason in (2, 3)
    with pytest.raises(ValueError):
        pa.CommitKey.from_bytes(data[:-1], ctx)
    circuit, wit, pi = pa.synthetic.chain_circuit(n, 5)
    proofs = []
    for key in (ck, ck2):
        pk = PR.preprocess(circuit, ctx, key)
        proofs.append(PR.prove(pk, key, wit, pi).to_bytes())
    assert proofs[0] == proofs[1] and len(proofs[0]) == 1040
