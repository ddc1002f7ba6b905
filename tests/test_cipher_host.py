"""The Poseidon cipher on JubJub keys without a device: the new exports are declared, bound and exported
with the argument lists of the header, and its block carries the two disclaimers; the two host forms against the big-integer
model of tests/cipher_model.py, byte for byte, for three capacities and two Hades shapes; every status of a decryption, the
lowest first, with zero messages on refusal; what the header says is refused; the wrapper's argument checks; and the recoding
of a viewing key into the signed digits the scan kernel takes."""
import ctypes as C
import os
import random
import re
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cipher_model as CM  # noqa: E402
import jubjub_model as J  # noqa: E402

R = CM.R
EXPORTS = ("pm_poseidon_cipher_encrypt_dev", "pm_poseidon_cipher_decrypt_dev", "pm_poseidon_cipher_scan_dev",
           "pm_poseidon_cipher_encrypt_host", "pm_poseidon_cipher_decrypt_host", "pm_test_cipher_stride", "pm_test_cipher_digits")
LENS = (1, 2, 4)
COUNT = 12


def _u64p(a):
    from plonk_prototype_amd._lib import u64p
    return a.ctypes.data_as(u64p) if a is not None else None


def test_exports_are_declared_bound_and_exported():
    import plonk_prototype_amd as pa
    from plonk_prototype_amd import _lib
    from plonk_prototype_amd._lib import u32p, u64p
    header = open(os.path.join(ROOT, "include", "plonk_mi355x.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    lib = C.CDLL(pa.LIB_PATH)
    vp, sz, u32 = C.c_void_p, C.c_size_t, C.c_uint32
    consts = [u32, u32, u64p, u64p, u32]                      # rounds, full_rounds, ark, mds, n_mds
    want = {
        "pm_poseidon_cipher_encrypt_dev": [vp, vp, vp, vp, vp, u32, sz, vp, vp],
        "pm_poseidon_cipher_decrypt_dev": [vp, vp, vp, vp, vp, u32, sz, vp, vp, C.POINTER(sz), vp],
        "pm_poseidon_cipher_scan_dev": [vp, vp, u64p, u32, vp, vp, vp, u32, sz, vp, vp, C.POINTER(sz), vp],
        "pm_poseidon_cipher_encrypt_host": consts + [u64p, u64p, u64p, u32, u64p],
        "pm_poseidon_cipher_decrypt_host": consts + [u64p, u64p, u64p, u32, u64p, u32p],
        "pm_test_cipher_stride": [vp, C.POINTER(sz)],
        "pm_test_cipher_digits": [u64p, u32, C.POINTER(C.c_int8)],
    }
    assert set(want) == set(EXPORTS)
    for name in EXPORTS:
        assert re.search(r"\bint %s\s*\(" % name, header), f"{name} is not declared in the header"
        assert hasattr(lib, name), f"{name} is not exported by the library"
        assert _lib.SIGNATURES[name] == (C.c_int, want[name]), f"{name} is bound with another argument list"
        assert "pub fn %s(" % name in doc, f"{name} is missing from INTEGRATION.md's extern block"
    for k, name in enumerate(("OK", "POINT", "RANGE", "TAG")):
        assert re.search(r"#define PM_CIPHER_%s %du\b" % (name, k), header), name
        assert getattr(_lib, "CIPHER_" + name) == k == getattr(CM, name)
    assert pa.CIPHER_REASONS == {1: "point", 2: "range", 3: "tag"}
    for name in ("PoseidonCipher", "poseidon_cipher_encrypt_host", "poseidon_cipher_decrypt_host", "CIPHER_REASONS", "cipher"):
        assert hasattr(pa, name), name
    block = header[header.index("Poseidon cipher on JubJub keys"):header.index("#define PM_CIPHER_OK")].replace("\n * ", " ")
    assert "NOT hardened against side channels" in block and "prior knowledge" in block


# ---------------------------------------------------------------------------------- the host forms
class Host:
    """the two host calls over one shape's constants, on the words in memory"""

    def __init__(self, h):
        from plonk_prototype_amd import _lib
        self.lib, self.h = _lib.load(), h
        self.ark, self.mds = CM.S.M.to_limbs(h.flat_ark), CM.S.M.to_limbs(h.flat_mds)

    def consts(self):
        h = self.h
        return (h.rounds, h.full, _u64p(self.ark), _u64p(self.mds), h.n_mds)

    def encrypt(self, secret, nonce, msg, L):   # noqa: N803
        out = np.zeros((L + 1, 4), np.uint64)
        rc = self.lib.pm_poseidon_cipher_encrypt_host(*self.consts(), _u64p(CM.point_words(secret)), _u64p(CM.mont_words(nonce)),
                                                      _u64p(CM.pack_words([msg])), L, _u64p(out))
        assert rc == 0, rc
        return out

    def decrypt(self, secret, nonce, cipher, L):   # noqa: N803
        out, status = np.full((L, 4), 0x5555555555555555, np.uint64), C.c_uint32(99)
        rc = self.lib.pm_poseidon_cipher_decrypt_host(*self.consts(), _u64p(CM.point_words(secret)), _u64p(CM.mont_words(nonce)),
                                                      _u64p(CM.pack_words([cipher])), L, _u64p(out), C.byref(status))
        assert rc == 0, rc
        return out, status.value


@pytest.mark.parametrize("L", LENS)
@pytest.mark.parametrize("shape", sorted(CM.SHAPES))
def test_host_forms_are_the_model(shape, L):   # noqa: N803
    cs = CM.case(shape, COUNT)
    host, h, want = Host(cs["h"]), cs["h"], CM.ciphers(cs, shape, L)
    for secret, nonce, msg, c in zip(cs["secret"], cs["nonce"], cs["msg"], want):
        got = host.encrypt(secret, nonce, msg[:L], L)
        assert got.tobytes() == CM.pack_words([c]).tobytes(), (hex(nonce), L)
        back, status = host.decrypt(secret, nonce, c, L)
        assert status == CM.OK and back.tobytes() == CM.pack_words([msg[:L]]).tobytes()
    # every status, the lowest first, zero messages on refusal
    i = COUNT - 1
    cor = CM.corruptions(h, L, cs["secret"][i], cs["nonce"][i], want[i])
    assert [(lab, st) for lab, _, _, _, _, st in cor] == [
        ("as it is", 0), ("off the curve", 1), ("x + r", 1), ("y + r", 1), ("nonce + r", 2), ("word 0 + r", 2), ("tag + r", 2),
        ("tag + 1", 3), ("word 0 + 1", 3), ("nonce + 1", 3), ("off the curve and tampered", 1), ("out of range and tampered", 2)]
    for lab, p, k, c, m, st in cor:
        back, status = host.decrypt(p, k, c, L)
        assert status == st, lab
        assert back.tobytes() == CM.pack_words([m]).tobytes(), lab
        if st:
            assert not back.any(), lab


def test_a_short_message_is_padded_with_zeros():
    import plonk_prototype_amd as pa
    cs = CM.case("5_2_per_round", COUNT)
    h, i = cs["h"], 5
    secret, nonce, msg = cs["secret"][i], cs["nonce"][i], cs["msg"][i]
    for L, k in ((2, 1), (4, 1), (4, 3)):   # noqa: N806
        want = CM.pack_words([CM.encrypt(h, secret, nonce, msg[:k], L)])[0]
        assert want.tobytes() == CM.pack_words([CM.encrypt(h, secret, nonce, msg[:k] + [0] * (L - k), L)])[0].tobytes()
        got = pa.poseidon_cipher_encrypt_host(h.flat_ark, h.flat_mds, secret, nonce, msg[:k], msg_len=L, rounds=h.rounds, full_rounds=h.full)
        assert got.tobytes() == want.tobytes(), (L, k)
        back, status = pa.poseidon_cipher_decrypt_host(h.flat_ark, h.flat_mds, secret, nonce, got, msg_len=L, rounds=h.rounds,
                                                       full_rounds=h.full)
        assert status == 0 and back.tobytes() == CM.pack_words([msg[:k] + [0] * (L - k)])[0].tobytes()
    limbs = CM.pack_words([msg[:2]])[0]
    assert pa.poseidon_cipher_encrypt_host(h.flat_ark, h.flat_mds, secret, nonce, limbs, rounds=h.rounds, full_rounds=h.full).tobytes() \
        == CM.pack_words([CM.encrypt(h, secret, nonce, msg[:2], 2)])[0].tobytes()


def test_host_refusals():
    from plonk_prototype_amd import _lib
    cs = CM.case("5_2_per_round", COUNT)
    host, h = Host(cs["h"]), cs["h"]
    lib, BAD = host.lib, _lib.PM_ERR_BAD_ARG   # noqa: N806
    L, i = 2, 3   # noqa: N806
    secret, nonce, msg = cs["secret"][i], cs["nonce"][i], cs["msg"][i][:L]
    cipher = CM.encrypt(h, secret, nonce, msg, L)
    sp, kp, mp, cp = (_u64p(a) for a in (CM.point_words(secret), CM.mont_words(nonce), CM.pack_words([msg]), CM.pack_words([cipher])))
    out, back, status = np.zeros((L + 1, 4), np.uint64), np.zeros((L, 4), np.uint64), C.c_uint32()
    enc, dec = lib.pm_poseidon_cipher_encrypt_host, lib.pm_poseidon_cipher_decrypt_host
    c0 = host.consts()
    assert enc(*c0, sp, kp, mp, L, _u64p(out)) == 0
    assert dec(*c0, sp, kp, cp, L, _u64p(back), C.byref(status)) == 0 and status.value == 0
    # msg_len 0 and 5
    for bad_len in (0, 5, 0xFFFFFFFF):
        assert enc(*c0, sp, kp, mp, bad_len, _u64p(out)) == BAD
        assert dec(*c0, sp, kp, cp, bad_len, _u64p(back), C.byref(status)) == BAD
    # encrypt: a secret off the curve or with a coordinate >= r, a nonce or a message word >= r
    big = _u64p(CM.canon_words(R))
    for bad_s in ((secret[0], (secret[1] + 1) % R), (secret[0] + R, secret[1])):
        assert enc(*c0, _u64p(CM.point_words(bad_s)), kp, mp, L, _u64p(out)) == BAD
    assert enc(*c0, sp, big, mp, L, _u64p(out)) == BAD
    assert enc(*c0, sp, kp, _u64p(CM.pack_words([[msg[0], msg[1] + R]])), L, _u64p(out)) == BAD
    # NULL, one argument at a time
    for j in (2, 3):
        c1 = list(c0)
        c1[j] = None
        assert enc(*c1, sp, kp, mp, L, _u64p(out)) == BAD
        assert dec(*c1, sp, kp, cp, L, _u64p(back), C.byref(status)) == BAD
    for j in range(3):
        a = [sp, kp, mp]
        a[j] = None
        assert enc(*c0, *a, L, _u64p(out)) == BAD
        a = [sp, kp, cp]
        a[j] = None
        assert dec(*c0, *a, L, _u64p(back), C.byref(status)) == BAD
    assert enc(*c0, sp, kp, mp, L, None) == BAD
    assert dec(*c0, sp, kp, cp, L, None, C.byref(status)) == BAD
    assert dec(*c0, sp, kp, cp, L, _u64p(back), None) == BAD
    # constants pm_hades_params_create refuses
    assert enc(h.rounds, 3, c0[2], c0[3], h.n_mds, sp, kp, mp, L, _u64p(out)) == BAD
    assert dec(h.rounds, h.full, c0[2], c0[3], 2, sp, kp, cp, L, _u64p(back), C.byref(status)) == BAD


def test_wrapper_argument_checks_need_no_device():
    import plonk_prototype_amd as pa

    class FakeHades(pa.Hades):
        def __init__(self):   # no context, no handle: every check below has to come before a device call
            self.ctx, self._h = None, None

    hd = FakeHades()
    with pytest.raises(ValueError):
        pa.PoseidonCipher(object())
    for bad in (0, 5, 2.0, None):
        with pytest.raises(ValueError):
            pa.PoseidonCipher(hd, msg_len=bad)
    c = pa.PoseidonCipher(hd)
    assert c.msg_len == 2
    pts = J.to_limbs([J.GENERATOR] * 3)
    nonces, msgs, cts = np.zeros((3, 4), np.uint64), np.zeros((3, 2, 4), np.uint64), np.zeros((3, 3, 4), np.uint64)
    bad_calls = [
        lambda: c.encrypt(pts, nonces[:2], msgs),                         # n does not match
        lambda: c.encrypt(pts[:2], nonces, msgs),
        lambda: c.encrypt(pts, nonces, msgs[:2]),
        lambda: c.encrypt(pts, nonces, np.zeros((3, 3, 4), np.uint64)),   # more words than L
        lambda: c.encrypt(pts, nonces, np.zeros((3, 2, 3), np.uint64)),   # not limbs
        lambda: c.encrypt(pts, nonces, msgs.astype(np.int64)),            # another dtype
        lambda: c.encrypt(pts, nonces.astype(np.float64), msgs),
        lambda: c.encrypt([1, 2, 3], nonces, msgs),                       # points are pairs
        lambda: c.decrypt(pts, nonces, msgs),                             # ciphers have L + 1 words, no padding
        lambda: c.decrypt(pts, nonces[:1], cts),
        lambda: c.decrypt(pts, nonces, cts.reshape(9, 4)),
        lambda: c.scan(5, pts, nonces, cts[:2]),
        lambda: c.scan(5, pts[:2], nonces, cts),
        lambda: c.scan([5, 6], pts, nonces, cts),                         # one viewing key
        lambda: c.scan(R, pts, nonces, cts),                              # not below r
        lambda: c.scan(-1, pts, nonces, cts),
        lambda: c.encrypt_to(hd, pts, [1, 2], nonces, msgs),
    ]
    for k, call in enumerate(bad_calls):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"call {k} was not refused")
    got = c.encrypt(pts[:0], nonces[:0], msgs[:0])
    assert got.shape == (0, 3, 4)
    m, st = c.decrypt(pts[:0], nonces[:0], cts[:0])
    assert m.shape == (0, 2, 4) and st.shape == (0,) and st.dtype == np.uint32
    m, st = c.scan(7, pts[:0], nonces[:0], cts[:0])
    assert m.shape == (0, 2, 4) and st.shape == (0,)


# ---------------------------------------------------------------------------------- the digits of a viewing key
def test_view_key_digits():
    from plonk_prototype_amd import _lib
    lib = _lib.load()
    rng = random.Random(0xD161)
    keys = [0, 1, 8, 9, R - 1, 1 << 252] + list(CM.SPECIAL_KEYS) + [rng.randrange(R) for _ in range(50)]
    for vk in keys:
        seen = []
        for mont in (False, True):
            d = (C.c_int8 * 64)(*([99] * 64))
            assert lib.pm_test_cipher_digits(_u64p(CM.key_words(vk, mont)), 0 if mont else 1, d) == 0
            digits = list(d)
            assert all(abs(x) <= 8 for x in digits), hex(vk)
            assert sum(x * 16 ** (63 - k) for k, x in enumerate(digits)) == vk, hex(vk)      # the top digit first
            seen.append(digits)
        assert seen[0] == seen[1]
    d = (C.c_int8 * 64)()
    assert lib.pm_test_cipher_digits(_u64p(CM.key_words(CM.SPECIAL_KEYS[-1], False)), 1, d) == 0
    low = list(d)[::-1]
    assert low[0] == 0 and low[1:12] == [-7] + [-6] * 9 + [0], "a zero low digit, then a run of carries"
    assert lib.pm_test_cipher_digits(_u64p(CM.canon_words(R)), 1, d) == _lib.PM_ERR_BAD_ARG
    assert lib.pm_test_cipher_digits(_u64p(CM.canon_words(R)), 0, d) == _lib.PM_ERR_BAD_ARG
    assert lib.pm_test_cipher_digits(_u64p(CM.canon_words(5)), 2, d) == _lib.PM_ERR_BAD_ARG
    assert lib.pm_test_cipher_digits(None, 1, d) == _lib.PM_ERR_BAD_ARG
    assert lib.pm_test_cipher_digits(_u64p(CM.canon_words(5)), 1, None) == _lib.PM_ERR_BAD_ARG
