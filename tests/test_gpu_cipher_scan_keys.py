"""Scanning a ledger under up to 64 viewing keys in one call on the GPU (pm_poseidon_cipher_scan_keys_dev, DESIGN.md section
7.2q): against the big-integer model of tests/cipher_model.py for sizes around a wave, three capacities, two Hades shapes, both
scalar forms and a caller's stream; against K calls of pm_poseidon_cipher_scan_dev combined as the header states, for 1, 2, 5 and
64 keys and on both of the call's paths; every status at the ends of two waves; special keys and special ephemeral points; more
notes than a capped scratch holds at once; a guard arena around the outputs; refusals and n = 0; and the wrappers."""
import ctypes as C
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cipher_model as CM  # noqa: E402
import jubjub_model as J  # noqa: E402
from guard_arena import GuardArena, as_u64, untouched  # noqa: E402
from test_gpu_cipher import Rig, _corrupted  # noqa: E402  (the rig of the single-key tests and their corrupted ledger)

pytestmark = pytest.mark.gpu
R = CM.R
SIZES = (1, 2, 63, 64, 65, 130)
NMAX = max(SIZES)
SHAPE_IDS = sorted(CM.SHAPES)
SENTINEL = 0x7777777777777777


@pytest.fixture(scope="module", params=SHAPE_IDS)
def rig(ctx, request):
    r = Rig(ctx, request.param)
    yield r
    r.free()


@pytest.fixture(scope="module")
def rig52(ctx):
    r = Rig(ctx, "5_2_per_round")
    yield r
    r.free()


def key_limbs(keys, mont):
    """integers -> what the wrapper takes: the list itself (canonical), or [K, 4] Montgomery limbs"""
    return np.stack([CM.key_words(k, True) for k in keys]) if mont else list(keys)


def scan_keys(rig, L, keys, points, nonces, ciphers, mont=False, stream=0, msgs=True, status=True, count=True):   # noqa: N803
    """scan_keys_dev on host arrays, every output in front of a sentinel -> (masks, messages or None, status or None, n_hits)"""
    pa, ctx, n = rig.pa, rig.ctx, points.shape[0]
    dp, dk, dc = (pa.DeviceVector.from_host(ctx, x.reshape(-1, 4)) for x in (points, nonces, ciphers))
    dmask = pa.DeviceVector.from_host(ctx, np.full(((n + 3) // 4, 4), SENTINEL, np.uint64))
    dm = pa.DeviceVector.from_host(ctx, np.full((L * n, 4), SENTINEL, np.uint64))
    dst = pa.DeviceVector.from_host(ctx, np.full(((n + 7) // 8, 4), SENTINEL, np.uint64))
    try:
        hits = rig.cipher(L).scan_keys_dev(key_limbs(keys, mont), dp.ptr, dk.ptr, dc.ptr, n, dmask.ptr, dm.ptr if msgs else 0,
                                           dst.ptr if status else 0, count, None, stream)
        rig._sync(stream)
        ctx.sync()
        got_mask, got_m, got_s = dmask.to_host().reshape(-1), dm.to_host(), dst.to_host().view(np.uint32).reshape(-1)
        assert (got_mask[n:] == SENTINEL).all() and (got_s[n:] == 0x77777777).all(), "written behind the n-th element"
        if not msgs:
            assert (got_m == SENTINEL).all(), "d_msgs_out = NULL and something was written"
        if not status:
            assert (got_s == 0x77777777).all(), "d_status = NULL and something was written"
        return got_mask[:n].copy(), (got_m.reshape(n, L, 4) if msgs else None), (got_s[:n].copy() if status else None), hits
    finally:
        for x in (dp, dk, dc, dmask, dm, dst):
            x.free()


def popcount(masks):
    return sum(bin(int(m)).count("1") for m in masks)


def combine(per_key, n, L):   # noqa: N803
    """[(messages, status)] of the single-key scan per key, in key order -> (masks, messages, status, hits) as the header states"""
    masks, msgs, status = np.zeros(n, np.uint64), np.zeros((n, L, 4), np.uint64), np.full(n, CM.TAG, np.uint32)
    for k in reversed(range(len(per_key))):                   # the lowest key last: its message stays
        m, st = per_key[k]
        hit = st == CM.OK
        masks[hit] |= np.uint64(1 << k)
        msgs[hit] = m[hit]
    status[masks != 0] = CM.OK
    first = per_key[0][1]
    for code in (CM.RANGE, CM.POINT):                         # they depend on the note alone: every key reports them alike
        assert all(((st == code) == (first == code)).all() for _, st in per_key)
        status[first == code] = code
    return masks, msgs, status, popcount(masks)


# ---------------------------------------------------------------------------------- 1. the model
def test_three_keys_are_the_model(rig):
    import torch
    L, cs = 2, rig.cs   # noqa: N806
    keys, owner = cs["vk"], np.array(cs["owner"])
    want_mask = np.uint64(1) << owner.astype(np.uint64)
    ciphers, want_m = rig.want(L), rig.msgs(L)
    for n in SIZES:
        masks, m, st, hits = scan_keys(rig, L, keys, rig.eph[:n], rig.nonces[:n], ciphers[:n])
        assert masks.tolist() == want_mask[:n].tolist(), (n, np.flatnonzero(masks != want_mask[:n])[:8])
        assert not st.any() and hits == n and m.tobytes() == want_m[:n].tobytes(), n
    results = []
    for mont in (False, True):
        for stream in (0, torch.cuda.Stream().cuda_stream):
            masks, m, st, hits = scan_keys(rig, L, keys, rig.eph, rig.nonces, ciphers, mont=mont, stream=stream)
            assert masks.tolist() == want_mask.tolist() and not st.any() and hits == NMAX and m.tobytes() == want_m.tobytes()
            results.append(masks.tobytes() + m.tobytes() + st.tobytes())
    assert len(set(results)) == 1


@pytest.mark.parametrize("L", (1, 4))
def test_other_capacities_are_the_model(rig, L):   # noqa: N803
    n, cs = 65, rig.cs
    want_mask = (np.uint64(1) << np.array(cs["owner"][:n], np.uint64)).tolist()
    masks, m, st, hits = scan_keys(rig, L, cs["vk"], rig.eph[:n], rig.nonces[:n], rig.want(L)[:n])
    assert masks.tolist() == want_mask and not st.any() and hits == n and m.tobytes() == rig.msgs(L)[:n].tobytes()


# ---------------------------------------------------------------------------------- 2. the present call
_SINGLE = {}


def single(rig, L, vk, points, nonces, ciphers, tag):   # noqa: N803
    """pm_poseidon_cipher_scan_dev under one key -> (messages, status), once per (ledger, key)"""
    key = (rig.shape, L, tag, vk)
    if key not in _SINGLE:
        back, status, ok = rig.open(L, points, nonces, ciphers, view_key=vk)
        assert ok == int((status == 0).sum())
        _SINGLE[key] = (back, status)
    return _SINGLE[key]


def key_list(cs, K):   # noqa: N803
    """K keys: seeded strangers, the three real keys at 0, K / 2 and K - 1 where K allows, one duplicate of vk[0] at 1"""
    rng = random.Random(0x5EED + K)
    keys = [rng.randrange(1, R) for _ in range(K)]
    keys[0] = cs["vk"][0]
    if K > 1:
        keys[K - 1] = cs["vk"][2]
    if K > 2:
        keys[K // 2] = cs["vk"][1]
    if K > 3:
        keys[1] = cs["vk"][0]
    return keys


@pytest.mark.parametrize("K", (1, 2, 5, 64))
def test_k_keys_are_k_calls_of_the_single_key_scan(rig, K):   # noqa: N803
    L, cs = 2, rig.cs   # noqa: N806
    keys, ciphers = key_list(cs, K), rig.want(L)
    per_key = [single(rig, L, vk, rig.eph, rig.nonces, ciphers, "plain") for vk in keys]
    want_mask, want_m, want_s, want_hits = combine(per_key, NMAX, L)
    assert want_hits >= 40 and (K < 5 or want_hits > (want_mask != 0).sum()), "the duplicate opens vk[0]'s notes a second time"
    masks, m, st, hits = scan_keys(rig, L, keys, rig.eph, rig.nonces, ciphers)
    assert masks.tolist() == want_mask.tolist(), np.flatnonzero(masks != want_mask)[:8]
    assert st.tolist() == want_s.tolist() and hits == want_hits and m.tobytes() == want_m.tobytes()
    if K == 1:
        back, status = per_key[0]
        assert masks.tolist() == (status == 0).astype(np.uint64).tolist()
        assert m.tobytes() == back.tobytes() and st.tobytes() == status.tobytes(), "one key: that call's bytes"


def test_both_paths_write_the_same_bytes(rig52):
    """the full window table and the ladder per key, whichever the default threshold picks for three keys"""
    L, cs, ctx = 2, rig52.cs, rig52.ctx   # noqa: N806
    keys, ciphers = key_list(cs, 5)[:3] + [0], rig52.want(L)
    got = []
    try:
        for table_min in (1, 65):
            ctx.set_option("cipher_scan_keys_table_min", table_min)
            masks, m, st, hits = scan_keys(rig52, L, keys, rig52.eph, rig52.nonces, ciphers)
            got.append((masks.tobytes() + m.tobytes() + st.tobytes(), hits))
        for bad in (-1, 66):
            with pytest.raises(Exception):
                ctx.set_option("cipher_scan_keys_table_min", bad)
    finally:
        ctx.set_option("cipher_scan_keys_table_min", 0)
    assert got[0] == got[1]
    per_key = [single(rig52, L, vk, rig52.eph, rig52.nonces, ciphers, "plain") for vk in keys]
    want_mask, want_m, want_s, want_hits = combine(per_key, NMAX, L)
    assert got[0] == (want_mask.tobytes() + want_m.tobytes() + want_s.tobytes(), want_hits)


# ---------------------------------------------------------------------------------- 3. every status
def test_every_status_at_the_ends_of_two_waves(rig):
    L, cs = 2, rig.cs   # noqa: N806
    keys = cs["vk"]
    seen = set()
    for turn in range(3):
        points, nonces, ciphers, _, verdict = _corrupted(rig, L, turn, scan=True)
        per_key = [single(rig, L, vk, points, nonces, ciphers, ("corrupted", turn)) for vk in keys]
        want_mask, want_m, want_s, want_hits = combine(per_key, NMAX, L)
        faults = (verdict == CM.POINT) | (verdict == CM.RANGE)    # the model's verdict on the note: the same whatever the keys
        assert (want_s[faults] == verdict[faults]).all() and not ((want_s == CM.POINT) | (want_s == CM.RANGE))[~faults].any()
        masks, m, st, hits = scan_keys(rig, L, keys, points, nonces, ciphers)
        assert st.tolist() == want_s.tolist(), (turn, np.flatnonzero(st != want_s))
        assert masks.tolist() == want_mask.tolist() and hits == want_hits and m.tobytes() == want_m.tobytes()
        assert not masks[faults].any() and not m[st != 0].any(), "a refused note has no bit and no message"
        for at in (0, 63, 64, 129):
            assert st[at] in (1, 2, 3)
        seen |= set(st.tolist())
    assert seen == {0, 1, 2, 3}


# ---------------------------------------------------------------------------------- 4. special keys and points
def test_special_keys_and_points(rig52):
    rig = rig52
    L, cs, h = 2, rig.cs, rig.cs["h"]   # noqa: N806
    keys = list(CM.SPECIAL_KEYS) + [0]
    vk = keys[2]                                               # the sender's recipient: 9, an odd key
    honest = cs["eph"][7]
    shifted = J.add(honest, CM.ORDER_2)                        # R + (0, -1): k R' = k R + (k mod 2) (0, -1)
    off = (honest[0], (honest[1] + 1) % R)
    notes = []                                                 # the eight notes of test_scan_special_keys_and_points, for vk
    for i in (5, 6):
        notes.append((cs["eph"][i], cs["nonce"][i], CM.mul(cs["eph"][i], vk)))
    notes.append((cs["eph"][8], cs["nonce"][8], cs["secret"][8]))
    notes.append((J.IDENTITY, cs["nonce"][9], J.IDENTITY))
    notes.append((shifted, cs["nonce"][10], CM.mul(shifted, vk)))
    notes.append((shifted, cs["nonce"][11], CM.mul(honest, vk)))
    notes.append((off, cs["nonce"][12], CM.mul(honest, vk)))
    notes.append((honest, cs["nonce"][13] + R, CM.mul(honest, vk)))
    notes.append((CM.ORDER_2, cs["nonce"][14], CM.ORDER_2))                        # the identity + (0, -1): k R = (k mod 2) (0, -1)
    notes.append((CM.ORDER_2, cs["nonce"][15], J.IDENTITY))
    msgs = [cs["msg"][i][:L] for i in range(len(notes))]
    ciphers = [CM.encrypt(h, s, k % R, m, L) for (_, k, s), m in zip(notes, msgs)]
    per_key = []
    for key in keys:                                           # the expectation: cipher_model.scan per key
        model = [CM.scan(h, key, p, k, c, L) for (p, k, _), c in zip(notes, ciphers)]
        per_key.append((CM.pack_words([m for m, _ in model]), np.array([s for _, s in model], np.uint32)))
    want_mask, want_m, want_s, want_hits = combine(per_key, len(notes), L)
    every = (1 << len(keys)) - 1
    odd = sum(1 << k for k, key in enumerate(keys) if key % 2)
    assert int(want_mask[3]) == every, "R the identity: S is the identity under every key"
    assert int(want_mask[8]) == odd and int(want_mask[9]) == every ^ odd, "R + (0, -1) splits the keys by parity"
    assert odd not in (0, every)
    assert want_mask[:8].tolist() == [4, 4, 0, every, 4, 0, 0, 0] and want_s.tolist() == [0, 0, 3, 0, 0, 3, 1, 2, 0, 0]
    masks, m, st, hits = scan_keys(rig, L, keys, CM.pack_points([p for p, _, _ in notes]), CM.pack_words([[k for _, k, _ in notes]])[0],
                                   CM.pack_words(ciphers))
    assert masks.tolist() == want_mask.tolist() and st.tolist() == want_s.tolist() and hits == want_hits
    assert m.tobytes() == want_m.tobytes()


# ---------------------------------------------------------------------------------- 5. strides
def test_a_capped_scratch_walks_n_in_strides(rig52):
    rig, ctx = rig52, rig52.ctx
    L, cs, K = 2, rig.cs, 3   # noqa: N806
    n, period = 193, 64
    stride, nbytes = C.c_size_t(), C.c_size_t()
    budget = 5                                                 # MiB: 64 notes x 74 112 bytes fit, 128 do not
    assert ctx._lib.pm_test_cipher_scan_keys_plan(256, K, L, n, budget, C.byref(stride), C.byref(nbytes)) == 0 and stride.value == 64
    tile = lambda a: np.tile(a[:period], (n // period + 1,) + (1,) * (a.ndim - 1))[:n]   # noqa: E731
    keys = [cs["vk"][1], cs["vk"][0], cs["vk"][2]]
    vk = keys[1]                                               # 64 of the model's notes, every one to vk: S_i = vk R_i
    model = [CM.encrypt(cs["h"], CM.mul(p, vk), k, m[:L], L) for p, k, m in zip(cs["eph"][:period], cs["nonce"], cs["msg"])]
    eph, nonces, ciphers, msgs = tile(rig.eph), tile(rig.nonces), tile(CM.pack_words(model)).copy(), tile(rig.msgs(L))
    lost = [5, 67, 192]
    for at in lost:                                            # its neighbour's tag
        assert not np.array_equal(ciphers[at, L], ciphers[(at + 1) % period, L])
        ciphers[at, L] = ciphers[(at + 1) % period, L]
    free = scan_keys(rig, L, keys, eph, nonces, ciphers)
    try:
        ctx.set_option("cipher_scan_keys_table_min", 1)        # the table's strides, whatever the default threshold
        ctx.set_option("cipher_scan_table_mb", budget)
        assert ctx._lib.pm_poseidon_cipher_scan_keys_work_bytes(ctx._h, K, L, n) == nbytes.value
        capped = scan_keys(rig, L, keys, eph, nonces, ciphers)
    finally:
        ctx.set_option("cipher_scan_table_mb", 0)
        ctx.set_option("cipher_scan_keys_table_min", 0)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(capped[:3], free[:3])) and capped[3] == free[3], "the bytes of no cap"
    masks, m, st, hits = capped
    assert np.flatnonzero(masks == 0).tolist() == lost and set(masks.tolist()) == {0, 2}, "exactly those three lose their bit"
    assert st[lost].tolist() == [3, 3, 3] and hits == n - 3 and not m[lost].any()
    keep = np.ones(n, bool)
    keep[lost] = False
    assert not st[keep].any() and m[keep].tobytes() == msgs[keep].tobytes()


# ---------------------------------------------------------------------------------- 6. memory
def _arena_call(rig, arena, L, keys, n, msgs=True, status=True):   # noqa: N803
    from plonk_prototype_amd import _lib
    vk = np.stack([CM.key_words(k, False) for k in keys])
    hits = C.c_size_t(77)
    rc = rig.ctx._lib.pm_poseidon_cipher_scan_keys_dev(
        rig.ctx._h, rig.hades._h, vk.ctypes.data_as(_lib.u64p), len(keys), 1, C.c_void_p(arena.addr("eph")),
        C.c_void_p(arena.addr("nonces")), C.c_void_p(arena.addr("ciphers")), L, n, C.c_void_p(arena.addr("masks")),
        C.c_void_p(arena.addr("msgs")) if msgs else None, C.c_void_p(arena.addr("status")) if status else None, C.byref(hits), None)
    return rc, hits.value


def test_outputs_in_a_guard_arena(rig52):
    rig = rig52
    L, n, cs = 2, 67, rig.cs   # noqa: N806
    keys = cs["vk"]
    want_mask = (np.uint64(1) << np.array(cs["owner"][:n], np.uint64))
    with GuardArena.of(rig.ctx, eph=rig.eph[:n], nonces=rig.nonces[:n], ciphers=rig.want(L)[:n], masks=8 * n, msgs=32 * L * n,
                       status=4 * n) as arena:
        rc, hits = _arena_call(rig, arena, L, keys, n)
        assert rc == 0 and hits == n
        first = arena.check()                                  # nothing outside 8 n, 32 L n and 4 n bytes
        assert first["masks"].view(np.uint64).tolist() == want_mask.tolist()
        assert as_u64(first["msgs"], n, L, 4).tobytes() == rig.msgs(L)[:n].tobytes() and not first["status"].view(np.uint32).any()
        rc, hits = _arena_call(rig, arena, L, keys, n)
        second = arena.check()
        assert rc == 0 and hits == n and all(first[k].tobytes() == second[k].tobytes() for k in first), "two calls, the same bytes"
    with GuardArena.of(rig.ctx, eph=rig.eph[:n], nonces=rig.nonces[:n], ciphers=rig.want(L)[:n], masks=8 * n, msgs=32 * L * n,
                       status=4 * n) as arena:
        rc, hits = _arena_call(rig, arena, L, keys, n, msgs=False, status=False)
        got = arena.check()
        assert rc == 0 and hits == n and untouched(got["msgs"]) and untouched(got["status"])
        assert got["masks"].view(np.uint64).tolist() == want_mask.tolist()


# ---------------------------------------------------------------------------------- 7. refusals, n = 0
def test_refusals_leave_every_output_byte_and_n_zero(rig52):
    from plonk_prototype_amd import _lib
    rig = rig52
    L, n, cs = 2, 5, rig.cs   # noqa: N806
    lib, c, hd, OK, BAD = rig.ctx._lib, rig.ctx._h, rig.hades._h, _lib.PM_OK, _lib.PM_ERR_BAD_ARG   # noqa: N806
    keys = np.stack([CM.key_words(k, False) for k in cs["vk"]] * 22)[:65]
    kp = lambda a: a.ctypes.data_as(_lib.u64p)   # noqa: E731
    with GuardArena.of(rig.ctx, eph=rig.eph[:n], nonces=rig.nonces[:n], ciphers=rig.want(L)[:n], masks=8 * n, msgs=32 * L * n,
                       status=4 * n) as arena:
        p = {k: arena.addr(k) for k in ("eph", "nonces", "ciphers", "masks", "msgs", "status")}
        hits = C.c_size_t(77)

        def call(view_keys=kp(keys), n_keys=3, form=1, msg_len=L, count=n, ctx=c, params=hd, **moved):
            a = {k: C.c_void_p(moved.get(k, v)) if moved.get(k, v) else None for k, v in p.items()}
            return lib.pm_poseidon_cipher_scan_keys_dev(ctx, params, view_keys, n_keys, form, a["eph"], a["nonces"], a["ciphers"], msg_len,
                                                        count, a["masks"], a["msgs"], a["status"], C.byref(hits), None)

        assert call(count=0) == OK and hits.value == 0, "n = 0: PM_OK, *n_hits = 0"
        hits.value = 77
        for n_keys in (0, 65, 0xFFFFFFFF):
            assert call(n_keys=n_keys) == BAD
        big = np.stack([CM.key_words(cs["vk"][0], False), CM.canon_words(R), CM.key_words(cs["vk"][1], False)])
        for form in (0, 1):
            assert call(view_keys=kp(big)) == BAD, "a key equal to r"
            assert call(view_keys=kp(big), form=form) == BAD
        assert call(view_keys=None) == BAD
        for form in (2, 0xFFFFFFFF):
            assert call(form=form) == BAD
        for bad_len in (0, 5):
            assert call(msg_len=bad_len) == BAD
        assert call(ctx=None) == BAD and call(params=None) == BAD
        for name in ("eph", "nonces", "ciphers", "masks"):
            assert call(**{name: 0}) == BAD, f"{name} = NULL"
        for name in ("eph", "nonces", "ciphers", "masks", "msgs"):
            assert call(**{name: p[name] + 8}) == BAD, f"{name} is not 16-byte aligned"
        assert call(status=p["status"] + 2) == BAD, "d_status is not 4-byte aligned"
        assert hits.value == 77, "a refused call leaves *n_hits"
        arena.check_unchanged()
        assert lib.pm_poseidon_cipher_scan_keys_work_bytes(c, 0, L, n) == 0 and lib.pm_poseidon_cipher_scan_keys_work_bytes(c, 3, L, 0) == 0
        # and the same arguments, accepted
        assert call() == OK and hits.value == n
        got = arena.check()
        assert got["masks"].view(np.uint64).tolist() == [1 << o for o in cs["owner"][:n]]
        assert call(status=p["status"] + 4, count=n - 1) == OK and hits.value == n - 1, "4-byte alignment is enough for d_status"
        arena.check()


# ---------------------------------------------------------------------------------- 8. the wrappers
def test_hits_and_scan_keys_bytes(rig52):
    rig, pa = rig52, rig52.pa
    L, n, cs = 2, 64, rig.cs   # noqa: N806
    keys = key_list(cs, 5)
    points = rig.eph[:n]
    enc = pa.jubjub_compress(rig.ctx, points).copy()
    bad = 17
    enc[bad] = 0xFF                                            # y >= r: it does not decode
    decoded, status = pa.jubjub_decompress(rig.ctx, enc)
    assert status[bad] != 0 and not status[np.arange(n) != bad].any() and not decoded[bad].any()
    cipher = rig.cipher(L)
    want = cipher.scan_keys(keys, decoded, rig.nonces[:n], rig.want(L)[:n])
    got = cipher.scan_keys_bytes(keys, enc, rig.nonces[:n], rig.want(L)[:n])
    assert all(a.dtype == b.dtype and a.tobytes() == b.tobytes() for a, b in zip(got, want))
    masks, m, st = got
    assert masks.dtype == np.uint64 and masks.shape == (n,) and m.shape == (n, L, 4) and st.dtype == np.uint32
    assert st[bad] == 1 and masks[bad] == 0 and not m[bad].any() and not st[np.arange(n) != bad].any()
    at = {0: [0, 1], 1: [2], 2: [4]}                           # key_list(5): vk[0] at 0 and 1, vk[1] at 2, vk[2] at 4
    pairs = [[i, k] for i in range(n) if i != bad for k in at[cs["owner"][i]]]
    assert pa.PoseidonCipher.hits(masks).tolist() == pairs
    per_key = [cipher.scan(vk, decoded, rig.nonces[:n], rig.want(L)[:n]) for vk in keys]
    want_mask, want_m, want_s, _ = combine(per_key, n, L)
    assert masks.tolist() == want_mask.tolist() and m.tobytes() == want_m.tobytes() and st.tolist() == want_s.tolist()
