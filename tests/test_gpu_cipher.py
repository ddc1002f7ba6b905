"""The Poseidon cipher on JubJub keys on the GPU against the big-integer model of tests/cipher_model.py,
byte for byte: encryption and decryption for sizes around a wave, three capacities and two Hades shapes, on the default and on a
caller's stream, and against the host forms; every status of a decryption at the ends of two waves; the scan of a ledger under
one viewing key, in both scalar forms, with special keys and special ephemeral points; more notes than the grid holds at once;
refusals and n = 0; and constants taken from a key."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cipher_model as CM  # noqa: E402
import gadget_model as M  # noqa: E402
import hades_model as HM  # noqa: E402
import jubjub_model as J  # noqa: E402

pytestmark = pytest.mark.gpu
R = CM.R
SIZES = (1, 2, 63, 64, 65, 130)
NMAX = max(SIZES)
LENS = (1, 2, 4)
SHAPE_IDS = sorted(CM.SHAPES)
SENTINEL = 0x7777777777777777


class Rig:
    """a context's handle for one shape, the shared case, and the three device calls on host arrays"""

    def __init__(self, ctx, shape, hades=None):
        import plonk_prototype_amd as pa
        self.pa, self.ctx, self.shape, self.cs = pa, ctx, shape, CM.case(shape, NMAX)
        h = self.cs["h"]
        self.own = hades is None
        self.hades = pa.Hades(ctx, M.to_limbs(h.flat_ark), M.to_limbs(h.flat_mds), h.rounds, h.full) if hades is None else hades
        self.secrets, self.eph = CM.pack_points(self.cs["secret"]), CM.pack_points(self.cs["eph"])
        self.nonces = CM.pack_words([self.cs["nonce"]])[0]

    def free(self):
        if self.own:
            self.hades.free()

    def cipher(self, L):   # noqa: N803
        return self.pa.PoseidonCipher(self.hades, L)

    def msgs(self, L):   # noqa: N803
        return CM.pack_words([m[:L] for m in self.cs["msg"]])

    def want(self, L):   # noqa: N803
        return CM.pack_words(CM.ciphers(self.cs, self.shape, L))

    def _sync(self, stream):
        if stream:
            import torch
            torch.cuda.synchronize()

    def encrypt(self, L, secrets, nonces, msgs, stream=0):   # noqa: N803
        pa, ctx, n = self.pa, self.ctx, secrets.shape[0]
        ds, dk, dm = (pa.DeviceVector.from_host(ctx, x.reshape(-1, 4)) for x in (secrets, nonces, msgs))
        out = pa.DeviceVector(ctx, (L + 1) * n)
        try:
            self.cipher(L).encrypt_dev(ds.ptr, dk.ptr, dm.ptr, n, out.ptr, stream)
            self._sync(stream)
            return out.to_host().reshape(n, L + 1, 4)
        finally:
            for x in (ds, dk, dm, out):
                x.free()

    def open(self, L, points, nonces, ciphers, view_key=None, form=None, status=True, count=True, stream=0):   # noqa: N803
        """decrypt (view_key None) or scan -> (messages, status or None, n_ok or None)"""
        pa, ctx, n = self.pa, self.ctx, points.shape[0]
        dp, dk, dc = (pa.DeviceVector.from_host(ctx, x.reshape(-1, 4)) for x in (points, nonces, ciphers))
        dm = pa.DeviceVector.from_host(ctx, np.full((L * n, 4), SENTINEL, np.uint64))
        dst = pa.DeviceVector.from_host(ctx, np.full(((n + 7) // 8, 4), SENTINEL, np.uint64))
        try:
            c = self.cipher(L)
            if view_key is None:
                ok = c.decrypt_dev(dp.ptr, dk.ptr, dc.ptr, n, dm.ptr, dst.ptr if status else 0, count, stream)
            else:
                ok = c.scan_dev(view_key, dp.ptr, dk.ptr, dc.ptr, n, dm.ptr, dst.ptr if status else 0, count, form, stream)
            self._sync(stream)
            ctx.sync()
            got = dst.to_host().view(np.uint32).reshape(-1)
            if not status:
                assert (got == 0x77777777).all(), "d_status = NULL and something was written"
            return dm.to_host().reshape(n, L, 4), (got[:n].copy() if status else None), ok
        finally:
            for x in (dp, dk, dc, dm, dst):
                x.free()


@pytest.fixture(scope="module", params=SHAPE_IDS)
def rig(ctx, request):
    r = Rig(ctx, request.param)
    yield r
    r.free()


# ---------------------------------------------------------------------------------- 1. encrypt and decrypt against the model
@pytest.mark.parametrize("L", LENS)
def test_encrypt_and_decrypt_are_the_model(rig, L):   # noqa: N803
    import torch
    want, msgs = rig.want(L), rig.msgs(L)
    for n in SIZES:
        got = rig.encrypt(L, rig.secrets[:n], rig.nonces[:n], msgs[:n])
        assert got.tobytes() == want[:n].tobytes(), (L, n, np.flatnonzero((got != want[:n]).any(axis=(1, 2)))[:8])
        back, status, ok = rig.open(L, rig.secrets[:n], rig.nonces[:n], want[:n])
        assert not status.any() and ok == n, (L, n, status)
        assert back.tobytes() == msgs[:n].tobytes(), (L, n)
    st = torch.cuda.Stream()
    assert rig.encrypt(L, rig.secrets, rig.nonces, msgs, stream=st.cuda_stream).tobytes() == want.tobytes(), "on a caller's stream"
    back, status, ok = rig.open(L, rig.secrets, rig.nonces, want, stream=st.cuda_stream)
    assert back.tobytes() == msgs.tobytes() and not status.any() and ok == NMAX
    # the host forms write the same bytes
    h, cs = rig.cs["h"], rig.cs
    for i in (0, 1, 4, 40, 129):
        host = rig.pa.poseidon_cipher_encrypt_host(h.flat_ark, h.flat_mds, cs["secret"][i], cs["nonce"][i], cs["msg"][i][:L], msg_len=L,
                                                   rounds=h.rounds, full_rounds=h.full)
        assert host.tobytes() == want[i].tobytes(), (L, i)
        m, status = rig.pa.poseidon_cipher_decrypt_host(h.flat_ark, h.flat_mds, cs["secret"][i], cs["nonce"][i], host, msg_len=L,
                                                        rounds=h.rounds, full_rounds=h.full)
        assert status == 0 and m.tobytes() == msgs[i].tobytes()


# ---------------------------------------------------------------------------------- 2. every status at the ends of two waves
def _corrupted(rig, L, turn, scan):   # noqa: N803
    """the 130 valid notes with a refusal at each of 0, 63, 64, 129 -- status 1 + (j + turn) % 3 at the j-th of them, so three turns
    put every status at every end -- and every class of cipher_model.corruptions inside the waves
    -> (points, nonces, ciphers, the model's messages, the model's status)"""
    cs, h = rig.cs, rig.cs["h"]
    base = CM.ciphers(cs, rig.shape, L)
    tested = cs["eph"] if scan else cs["secret"]
    points, nonces, ciphers = [list(p) for p in tested], list(cs["nonce"]), [list(c) for c in base]
    msgs, want = [list(m[:L]) for m in cs["msg"]], [0] * NMAX

    def classes(at):
        return CM.corruptions(h, L, tested[at], cs["nonce"][at], base[at], secret=cs["secret"][at] if scan else None)

    def place(at, entry):
        _, p, k, c, m, st = entry
        points[at], nonces[at], ciphers[at], msgs[at], want[at] = list(p), k, c, m, st

    for j, at in enumerate((0, 63, 64, 129)):
        status = 1 + (j + turn) % 3
        of_status = [e for e in classes(at) if e[5] == status]
        place(at, of_status[turn % len(of_status)])
    n_classes = len(classes(10))
    for k in range(n_classes):
        place(10 + 7 * k, classes(10 + 7 * k)[k])
    assert 10 + 7 * (n_classes - 1) < 129
    return CM.pack_points(points), CM.pack_words([nonces])[0], CM.pack_words(ciphers), CM.pack_words(msgs), np.array(want, np.uint32)


def test_decrypt_every_status_at_the_ends_of_two_waves(rig):
    L = 2   # noqa: N806
    seen = {at: set() for at in (0, 63, 64, 129)}
    for turn in range(3):
        points, nonces, ciphers, msgs, want = _corrupted(rig, L, turn, scan=False)
        for at in seen:
            seen[at].add(int(want[at]))
        back, status, ok = rig.open(L, points, nonces, ciphers)
        assert status.tolist() == want.tolist(), (turn, np.flatnonzero(status != want))
        assert ok == int((want == 0).sum())
        assert back.tobytes() == msgs.tobytes()
        assert not back[want != 0].any(), "a refused note's message is not zero"
        if turn == 0:                                        # either output alone, and neither
            b2, s2, ok2 = rig.open(L, points, nonces, ciphers, status=False)
            assert s2 is None and ok2 == ok and b2.tobytes() == msgs.tobytes()
            b3, s3, ok3 = rig.open(L, points, nonces, ciphers, count=False)
            assert ok3 is None and s3.tolist() == want.tolist() and b3.tobytes() == msgs.tobytes()
            b4, s4, ok4 = rig.open(L, points, nonces, ciphers, status=False, count=False)
            assert s4 is None and ok4 is None and b4.tobytes() == msgs.tobytes()
    assert all(s == {1, 2, 3} for s in seen.values()), seen


# ---------------------------------------------------------------------------------- 3. the scan
def test_scan_is_the_model(rig):
    import torch
    L, cs, h = 2, rig.cs, rig.cs["h"]   # noqa: N806
    vk = cs["vk"][0]
    ciphers = rig.want(L)
    model = [CM.scan(h, vk, p, k, c, L) for p, k, c in zip(cs["eph"], cs["nonce"], CM.ciphers(cs, rig.shape, L))]
    want_m, want_s = CM.pack_words([m for m, _ in model]), np.array([s for _, s in model], np.uint32)
    own = np.array([o == 0 for o in cs["owner"]])
    assert own.sum() == 40 and (want_s[own] == 0).all() and (want_s[~own] == 3).all()
    assert want_m[own].tobytes() == rig.msgs(L)[own].tobytes() and not want_m[~own].any()
    results = []
    for mont in (False, True):
        back, status, ok = rig.open(L, rig.eph, rig.nonces, ciphers, view_key=CM.key_words(vk, mont), form=0 if mont else 1)
        assert status.tolist() == want_s.tolist(), np.flatnonzero(status != want_s)
        assert ok == 40 and back.tobytes() == want_m.tobytes()
        results.append(back.tobytes() + status.tobytes())
    assert results[0] == results[1]
    for n in SIZES[:-1]:
        back, status, ok = rig.open(L, rig.eph[:n], rig.nonces[:n], ciphers[:n], view_key=vk)
        assert status.tolist() == want_s[:n].tolist() and ok == int(own[:n].sum()) and back.tobytes() == want_m[:n].tobytes(), n
    back, status, ok = rig.open(L, rig.eph, rig.nonces, ciphers, view_key=vk, stream=torch.cuda.Stream().cuda_stream)
    assert status.tolist() == want_s.tolist() and ok == 40 and back.tobytes() == want_m.tobytes(), "on a caller's stream"
    # refusals of a scan at the ends of two waves: the point test judges R, the secret is still vk R
    points, nonces, bad, msgs, want = _corrupted(rig, L, 1, scan=True)
    model = [CM.scan(h, vk, (int(p[0]), int(p[1])), k, c, L) if w == 0 else (None, w)
             for p, k, c, w in zip(cs["eph"], cs["nonce"], CM.ciphers(cs, rig.shape, L), want)]
    want = np.array([s for _, s in model], np.uint32)        # a note left as it is keeps the verdict of the scan: 0 or 3
    msgs[want != 0] = 0
    back, status, ok = rig.open(L, points, nonces, bad, view_key=vk)
    assert status.tolist() == want.tolist(), np.flatnonzero(status != want)
    assert sorted(set(want.tolist())) == [0, 1, 2, 3] and ok == int((want == 0).sum()) and back.tobytes() == msgs.tobytes()
    # the wrapper on host arrays
    m, s = rig.cipher(L).scan(vk, rig.eph, rig.nonces, ciphers)
    assert s.tolist() == want_s.tolist() and m.tobytes() == want_m.tobytes()
    m, s = rig.cipher(L).decrypt(rig.secrets, rig.nonces, ciphers)
    assert not s.any() and m.tobytes() == rig.msgs(L).tobytes()


@pytest.mark.parametrize("vk", CM.SPECIAL_KEYS, ids=["1", "8", "9", "r-1", "carries"])
def test_scan_special_keys_and_points(ctx, vk):
    rig = Rig(ctx, "5_2_per_round")
    try:
        L, cs, h = 2, rig.cs, rig.cs["h"]   # noqa: N806
        honest = cs["eph"][7]
        shifted = J.add(honest, CM.ORDER_2)                  # R + (0, -1): vk R' = vk R + (vk mod 2) (0, -1)
        assert J.on_curve(shifted) and CM.mul(shifted, vk) == J.add(CM.mul(honest, vk), CM.ORDER_2 if vk % 2 else J.IDENTITY)
        off = (honest[0], (honest[1] + 1) % R)
        notes = []                                           # (R in memory, nonce in memory, the secret the sender used)
        for i in (5, 6):
            notes.append((cs["eph"][i], cs["nonce"][i], CM.mul(cs["eph"][i], vk)))                 # to vk
        notes.append((cs["eph"][8], cs["nonce"][8], cs["secret"][8]))                              # to another key
        notes.append((J.IDENTITY, cs["nonce"][9], J.IDENTITY))                                     # R = the identity: S too
        notes.append((shifted, cs["nonce"][10], CM.mul(shifted, vk)))                              # to vk, R of order 2 l ...
        notes.append((shifted, cs["nonce"][11], CM.mul(honest, vk)))                               # ... and under vk R
        notes.append((off, cs["nonce"][12], CM.mul(honest, vk)))                                   # status 1
        notes.append((honest, cs["nonce"][13] + R, CM.mul(honest, vk)))                            # status 2
        msgs = [cs["msg"][i][:L] for i in range(len(notes))]
        ciphers = [CM.encrypt(h, s, k % R, m, L) for (_, k, s), m in zip(notes, msgs)]
        model = [CM.scan(h, vk, p, k, c, L) for (p, k, _), c in zip(notes, ciphers)]
        want = [0, 0, 3, 0, 0, 3 if vk % 2 else 0, 1, 2]
        assert [s for _, s in model] == want
        back, status, ok = rig.open(L, CM.pack_points([p for p, _, _ in notes]), CM.pack_words([[k for _, k, _ in notes]])[0],
                                    CM.pack_words(ciphers), view_key=vk)
        assert status.tolist() == want and ok == want.count(0)
        assert back.tobytes() == CM.pack_words([m for m, _ in model]).tobytes()
        assert back[0].tobytes() == CM.pack_words([msgs[0]])[0].tobytes()
    finally:
        rig.free()


def test_encrypt_to_then_scan(rig):
    L, cs, h = 2, rig.cs, rig.cs["h"]   # noqa: N806
    g = rig.pa.JubJubBase(rig.ctx, J.GENERATOR)
    try:
        n = 40
        c = rig.cipher(L)
        pks = CM.pack_points([cs["pk"][o] for o in cs["owner"][:n]])
        eph, ciphers = c.encrypt_to(g, pks, cs["e"][:n], rig.nonces[:n], rig.msgs(L)[:n])
        assert eph.tobytes() == rig.eph[:n].tobytes() and ciphers.tobytes() == rig.want(L)[:n].tobytes(), "the model's (R, c)"
        m, s = c.scan(cs["vk"][0], eph, rig.nonces[:n], ciphers)
        own = np.array([o == 0 for o in cs["owner"][:n]])
        assert own.any() and not own.all()
        assert (s[own] == 0).all() and (s[~own] == 3).all()
        assert m[own].tobytes() == rig.msgs(L)[:n][own].tobytes() and not m[~own].any()
        m, s = c.scan(M.to_limbs([cs["vk"][1]])[0], eph, rig.nonces[:n], ciphers)     # Montgomery limbs of another key
        assert [int(x) for x in s] == [0 if o == 1 else 3 for o in cs["owner"][:n]]
    finally:
        g.free()


# ---------------------------------------------------------------------------------- 4. more notes than the grid holds at once
def test_scan_walks_n_in_strides(ctx):
    rig = Rig(ctx, "5_2_per_round")
    try:
        L, cs = 2, rig.cs   # noqa: N806
        stride = C.c_size_t()
        assert ctx._lib.pm_test_cipher_stride(ctx._h, C.byref(stride)) == 0
        T = stride.value   # noqa: N806
        assert T >= 64 and T % 64 == 0
        n, period = T + 65, 64
        tile = lambda a: np.tile(a[:period], (n // period + 1,) + (1,) * (a.ndim - 1))[:n]   # noqa: E731
        vk = cs["vk"][0]                                     # 64 of the model's notes, every one to vk: S_i = vk R_i
        model = [CM.encrypt(cs["h"], CM.mul(p, vk), k, m[:L], L) for p, k, m in zip(cs["eph"][:period], cs["nonce"], cs["msg"])]
        eph, nonces, ciphers, msgs = tile(rig.eph), tile(rig.nonces), tile(CM.pack_words(model)).copy(), tile(rig.msgs(L))
        back, status, ok = rig.open(L, eph, nonces, ciphers, view_key=vk)
        assert not status.any() and ok == n
        assert back.tobytes() == msgs.tobytes(), "the device's messages against 64 of the model's, tiled"
        hits = [5, T + 3, n - 1]
        for at in hits:                                      # its neighbour's tag
            assert not np.array_equal(ciphers[at, L], ciphers[(at + 1) % period, L])
            ciphers[at, L] = ciphers[(at + 1) % period, L]
        back, status, ok = rig.open(L, eph, nonces, ciphers, view_key=vk)
        assert np.flatnonzero(status).tolist() == hits and status[hits].tolist() == [3, 3, 3]
        assert ok == n - 3 and not back[hits].any()
        keep = np.ones(n, bool)
        keep[hits] = False
        assert back[keep].tobytes() == msgs[keep].tobytes()
    finally:
        rig.free()


# ---------------------------------------------------------------------------------- 5. refusals, n = 0
def test_refusals_and_n_zero(ctx):
    import plonk_prototype_amd as pa
    from plonk_prototype_amd import _lib
    rig = Rig(ctx, "5_2_per_round")
    L, n = 2, 5   # noqa: N806
    vec = lambda a: pa.DeviceVector.from_host(ctx, a.reshape(-1, 4))   # noqa: E731
    fill = lambda k: pa.DeviceVector.from_host(ctx, np.full((k, 4), 5, np.uint64))   # noqa: E731
    ds, de, dk, dm, dc = vec(rig.secrets[:n]), vec(rig.eph[:n]), vec(rig.nonces[:n]), vec(rig.msgs(L)[:n]), vec(rig.want(L)[:n])
    out_c, out_m, dst = fill((L + 1) * n), fill(L * n), fill(1)
    try:
        lib, c, OK, BAD = ctx._lib, ctx._h, _lib.PM_OK, _lib.PM_ERR_BAD_ARG   # noqa: N806
        hd = rig.hades._h
        vp = lambda d: C.c_void_p(d.ptr)   # noqa: E731
        key = lambda v, mont=False: CM.key_words(v, mont).ctypes.data_as(_lib.u64p)   # noqa: E731
        ok = C.c_size_t(77)
        enc = lambda *a: lib.pm_poseidon_cipher_encrypt_dev(c, *a)   # noqa: E731
        dec = lambda *a: lib.pm_poseidon_cipher_decrypt_dev(c, *a)   # noqa: E731
        scan = lambda *a: lib.pm_poseidon_cipher_scan_dev(c, *a)     # noqa: E731
        vk = key(rig.cs["vk"][0])

        def untouched():
            ctx.sync()
            assert (out_c.to_host() == 5).all() and (out_m.to_host() == 5).all() and (dst.to_host() == 5).all()

        # n = 0: PM_OK, nothing launched, nothing written but *n_ok = 0
        assert enc(hd, vp(ds), vp(dk), vp(dm), L, 0, vp(out_c), None) == OK
        assert dec(hd, vp(ds), vp(dk), vp(dc), L, 0, vp(out_m), vp(dst), C.byref(ok), None) == OK and ok.value == 0
        ok.value = 77
        assert scan(hd, vk, 1, vp(de), vp(dk), vp(dc), L, 0, vp(out_m), vp(dst), C.byref(ok), None) == OK and ok.value == 0
        untouched()
        # msg_len outside 1 .. 4
        for bad_len in (0, 5):
            assert enc(hd, vp(ds), vp(dk), vp(dm), bad_len, n, vp(out_c), None) == BAD
            assert dec(hd, vp(ds), vp(dk), vp(dc), bad_len, n, vp(out_m), vp(dst), C.byref(ok), None) == BAD
            assert scan(hd, vk, 1, vp(de), vp(dk), vp(dc), bad_len, n, vp(out_m), vp(dst), C.byref(ok), None) == BAD
        # a bad scalar form, a viewing key that is not below r (in either form), no key
        for form in (2, 0xFFFFFFFF):
            assert scan(hd, vk, form, vp(de), vp(dk), vp(dc), L, n, vp(out_m), vp(dst), C.byref(ok), None) == BAD
        big = CM.canon_words(R).ctypes.data_as(_lib.u64p)
        for form in (0, 1):
            assert scan(hd, big, form, vp(de), vp(dk), vp(dc), L, n, vp(out_m), vp(dst), C.byref(ok), None) == BAD
        assert scan(hd, None, 1, vp(de), vp(dk), vp(dc), L, n, vp(out_m), vp(dst), C.byref(ok), None) == BAD
        # NULL among the required pointers, one at a time; a context alone is not enough
        assert lib.pm_poseidon_cipher_encrypt_dev(None, hd, vp(ds), vp(dk), vp(dm), L, n, vp(out_c), None) == BAD
        assert enc(None, vp(ds), vp(dk), vp(dm), L, n, vp(out_c), None) == BAD
        assert dec(None, vp(ds), vp(dk), vp(dc), L, n, vp(out_m), vp(dst), C.byref(ok), None) == BAD
        assert scan(None, vk, 1, vp(de), vp(dk), vp(dc), L, n, vp(out_m), vp(dst), C.byref(ok), None) == BAD
        for j in range(4):
            a = [vp(ds), vp(dk), vp(dm), vp(out_c)]
            a[j] = None
            assert enc(hd, a[0], a[1], a[2], L, n, a[3], None) == BAD
            a = [vp(ds), vp(dk), vp(dc), vp(out_m)]
            a[j] = None
            assert dec(hd, a[0], a[1], a[2], L, n, a[3], vp(dst), C.byref(ok), None) == BAD
            a = [vp(de), vp(dk), vp(dc), vp(out_m)]
            a[j] = None
            assert scan(hd, vk, 1, a[0], a[1], a[2], L, n, a[3], vp(dst), C.byref(ok), None) == BAD
        assert enc(hd, C.c_void_p(ds.ptr + 8), vp(dk), vp(dm), L, n, vp(out_c), None) == BAD      # not 16-byte aligned
        untouched()
        # and the same arguments, accepted
        assert enc(hd, vp(ds), vp(dk), vp(dm), L, n, vp(out_c), None) == OK
        assert dec(hd, vp(ds), vp(dk), vp(dc), L, n, vp(out_m), vp(dst), C.byref(ok), None) == OK and ok.value == n
        assert out_c.to_host().tobytes() == rig.want(L)[:n].tobytes() and out_m.to_host().tobytes() == rig.msgs(L)[:n].tobytes()
        assert scan(hd, vk, 1, vp(de), vp(dk), vp(dc), L, n, vp(out_m), vp(dst), C.byref(ok), None) == OK
        assert ok.value == sum(o == 0 for o in rig.cs["owner"][:n])
    finally:
        for x in (ds, de, dk, dm, dc, out_c, out_m, dst):
            x.free()
        rig.free()


# ---------------------------------------------------------------------------------- 6. constants taken from a key
def test_constants_from_a_key_give_the_model(ctx):
    import plonk_prototype_amd as pa
    b = HM.Builder(512)
    b.hades([b.var(True) for _ in range(5)], 5, 2, level=0)
    b.fill_arithmetic(5)
    recs = b.gadget_records()
    assert [g.kind for g in recs] == [7]
    _, rounds, full, ark, mds = b.permutations[0]
    pk = pa.preprocess(b.circuit(), ctx)
    handles = []
    try:
        pk.set_gadgets(recs)
        h_key = pa.Hades.from_key(pk, 0)
        handles.append(h_key)

        class H:   # noqa: N801
            pass
        h = H()
        h.ark, h.mds, h.rounds, h.full = ark, mds, rounds, full
        cs = CM.case("5_2_per_round", NMAX)
        n, L = 20, 2   # noqa: N806
        want = CM.pack_words([CM.encrypt(h, s, k, m[:L], L) for s, k, m in zip(cs["secret"][:n], cs["nonce"][:n], cs["msg"][:n])])
        c = pa.PoseidonCipher(h_key, L)
        secrets, nonces = CM.pack_points(cs["secret"][:n]), CM.pack_words([cs["nonce"][:n]])[0]
        msgs = CM.pack_words([m[:L] for m in cs["msg"][:n]])
        got = c.encrypt(secrets, nonces, msgs)
        assert got.tobytes() == want.tobytes()
        assert got.tobytes() != CM.pack_words(CM.ciphers(cs, "5_2_per_round", L)[:n]).tobytes(), "the key's constants are its own"
        m, s = c.scan(cs["vk"][0], CM.pack_points(cs["eph"][:n]), nonces, got)
        assert [int(x) for x in s] == [0 if o == 0 else 3 for o in cs["owner"][:n]]
        own = np.array([o == 0 for o in cs["owner"][:n]])
        assert m[own].tobytes() == msgs[own].tobytes()
    finally:
        for x in handles:
            x.free()
        pk.free()
