"""Native Schnorr signatures without a device: the new exports are declared, bound and exported with the
argument lists of the header; the host's arithmetic modulo the subgroup order against Python's %; the two host forms against the
big-integer model of tests/schnorr_model.py, byte for byte, in both scalar forms and for two Hades shapes; every reason of the
verification, the lowest first; a public key with a component of order 2; and what the header says is refused."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jubjub_model as J  # noqa: E402
import schnorr_model as S  # noqa: E402

R, Q = S.R, S.Q
EXPORTS = ("pm_schnorr_sign_dev", "pm_schnorr_verify_dev", "pm_schnorr_sign_host", "pm_schnorr_verify_host",
           "pm_test_jubjub_scalar_op", "pm_test_host_jubjub_scalar_op", "pm_test_schnorr_stride")
FORMS = (("canonical", False), ("montgomery", True))


def _u64p(a):
    from plonk_prototype_amd._lib import u64p
    return a.ctypes.data_as(u64p) if a is not None else None


def test_exports_are_declared_bound_and_exported():
    import plonk_prototype_amd as pa
    from plonk_prototype_amd import _lib
    from plonk_prototype_amd._lib import u32p, u64p
    header = open(os.path.join(ROOT, "include", "plonk_mi355x.h")).read()
    lib = C.CDLL(pa.LIB_PATH)
    vp, sz, u32, i = C.c_void_p, C.c_size_t, C.c_uint32, C.c_int
    consts = [u64p, u32, u32, u64p, u64p, u32, u64p]          # g_xy, rounds, full_rounds, ark, mds, n_mds, capacity
    want = {
        "pm_schnorr_sign_dev": [vp, vp, vp, u64p, vp, vp, vp, sz, u32, vp, vp],
        "pm_schnorr_verify_dev": [vp, vp, vp, u64p, vp, vp, vp, sz, u32, vp, C.POINTER(sz), vp],
        "pm_schnorr_sign_host": consts + [u64p, u64p, u64p, u32, u64p],
        "pm_schnorr_verify_host": consts + [u64p, u64p, u64p, u32, u32p],
        "pm_test_jubjub_scalar_op": [vp, i, u64p, u64p, u64p, u64p, sz],
        "pm_test_host_jubjub_scalar_op": [i, u64p, u64p, u64p, u64p, sz],
        "pm_test_schnorr_stride": [vp, C.POINTER(sz)],
    }
    assert set(want) == set(EXPORTS)
    for name in EXPORTS:
        assert re.search(r"\bint %s\s*\(" % name, header), f"{name} is not declared in the header"
        assert hasattr(lib, name), f"{name} is not exported by the library"
        assert _lib.SIGNATURES[name] == (C.c_int, want[name]), f"{name} is bound with another argument list"
    for k, name in enumerate(("OK", "U_RANGE", "R_POINT", "PK_POINT", "EQUATION")):
        assert re.search(r"#define PM_SCHNORR_%s %du\b" % (name, k), header), name
        assert getattr(_lib, "SCHNORR_" + name) == k == getattr(S, name)
    assert pa.SCHNORR_REASONS == {1: "u_range", 2: "r_point", 3: "pk_point", 4: "equation"}
    for name in ("Schnorr", "schnorr_sign_host", "schnorr_verify_host", "SCHNORR_REASONS"):
        assert hasattr(pa, name), name
    block = header[header.index("Native Schnorr signatures"):header.index("#define PM_SCHNORR_OK")].replace("\n * ", " ")
    assert "NOT hardened against side channels" in block and "prior knowledge" in block


# ---------------------------------------------------------------------------------- arithmetic modulo l
def test_host_scalar_ops_against_python():
    from plonk_prototype_amd import _lib
    lib = _lib.load()
    cases = S.scalar_cases()
    a, b, c = S.scalar_arrays(cases)
    for op in (0, 1, 2):
        out = np.zeros_like(a)
        assert lib.pm_test_host_jubjub_scalar_op(op, _u64p(a), _u64p(b), _u64p(c), _u64p(out), len(cases)) == _lib.PM_OK
        got = [int.from_bytes(row.tobytes(), "little") for row in out]
        assert got == S.scalar_expect(cases, op), op
    out = np.zeros_like(a)
    assert lib.pm_test_host_jubjub_scalar_op(0, _u64p(a), None, None, _u64p(out), 4) == _lib.PM_OK      # b and c are not read
    assert lib.pm_test_host_jubjub_scalar_op(3, _u64p(a), _u64p(b), _u64p(c), _u64p(out), 1) == _lib.PM_ERR_BAD_ARG
    assert lib.pm_test_host_jubjub_scalar_op(1, _u64p(a), None, _u64p(c), _u64p(out), 1) == _lib.PM_ERR_BAD_ARG
    assert lib.pm_test_host_jubjub_scalar_op(0, None, None, None, _u64p(out), 1) == _lib.PM_ERR_BAD_ARG


# ---------------------------------------------------------------------------------- the host forms
class Host:
    """the two host calls over one shape's constants"""

    def __init__(self, h, g=J.GENERATOR):
        from plonk_prototype_amd import _lib
        self.lib, self.h = _lib.load(), h
        self.g = S.point_words(g)
        self.ark, self.mds, self.cap = S.M.to_limbs(h.flat_ark), S.M.to_limbs(h.flat_mds), S.mont_words(h.capacity)

    def consts(self, g=None):
        h = self.h
        return (_u64p(self.g if g is None else g), h.rounds, h.full, _u64p(self.ark), _u64p(self.mds), h.n_mds, _u64p(self.cap))

    def sign(self, sk, k, m, montgomery):
        out = np.zeros((3, 4), np.uint64)
        s, kk = S.scalar_words([sk], montgomery), S.scalar_words([k], montgomery)
        rc = self.lib.pm_schnorr_sign_host(*self.consts(), _u64p(s), _u64p(kk), _u64p(S.mont_words(m)), 0 if montgomery else 1,
                                           _u64p(out))
        assert rc == 0, rc
        return out

    def verify(self, pk, m, sig, montgomery):
        reason = C.c_uint32(99)
        rc = self.lib.pm_schnorr_verify_host(*self.consts(), _u64p(S.point_words(pk)), _u64p(S.mont_words(m)),
                                             _u64p(S.sig_words(sig, montgomery)), 0 if montgomery else 1, C.byref(reason))
        assert rc == 0, rc
        return reason.value


@pytest.mark.parametrize("shape", sorted(S.SHAPES))
def test_sign_host_is_the_model(shape):
    cs = S.case(shape, len(J.edge_scalars()))
    host = Host(cs["h"])
    assert any(f >> 250 for f in cs["full"]), "no hash of the set has a bit at 250 or above: the truncation is not exercised"
    for name, mont in FORMS:
        for sk, k, m, sig in zip(cs["sk"], cs["k"], cs["m"], cs["sig"]):
            assert host.sign(sk, k, m, mont).tobytes() == S.sig_words(sig, mont).tobytes(), (name, hex(sk), hex(k))


@pytest.mark.parametrize("shape", sorted(S.SHAPES))
def test_verify_host_reasons(shape):
    cs = S.case(shape, len(J.edge_scalars()))
    host, h = Host(cs["h"]), cs["h"]
    for name, mont in FORMS:
        for pk, m, sig in zip(cs["pk"], cs["m"], cs["sig"]):
            assert host.verify(pk, m, sig, mont) == S.OK, (name, sig)
    i = len(cs["sig"]) - 1                                   # a random (sk, k, m)
    pk, m, sig = cs["pk"][i], cs["m"][i], cs["sig"][i]
    cor = S.corruptions(h, pk, m, sig)
    assert [(lab, want) for lab, _, _, _, want in cor] == [("u + l", 1), ("R.y + 1", 2), ("PK off the curve", 3), ("m + 1", 4),
                                                            ("R and PK bad", 2), ("R.x + r", 2), ("PK.y + r", 3)]
    c, _ = S.challenge(h, (sig[1], sig[2]), m)
    assert J.add(J.mul(J.GENERATOR, sig[0] + Q), J.mul(pk, c)) == (sig[1], sig[2]), "u + l satisfies the equation"
    for name, mont in FORMS:
        for lab, p, mm, s, want in cor:
            assert host.verify(p, mm, s, mont) == want, (name, lab)


def test_verify_host_public_key_with_a_component_of_order_two():
    """PK' = PK + (0, -1): c PK' = c PK + (c mod 2) (0, -1), so the signature stays valid exactly when c is even"""
    cs = S.case("5_2_per_round", len(J.edge_scalars()))
    host, h = Host(cs["h"]), cs["h"]
    parities = set()
    for pk, m, sig in list(zip(cs["pk"], cs["m"], cs["sig"]))[-10:]:
        c, _ = S.challenge(h, (sig[1], sig[2]), m)
        shifted = J.add(pk, S.ORDER_2)
        want = S.reason(h, J.GENERATOR, shifted, m, sig)
        assert want == (S.OK if c % 2 == 0 else S.EQUATION)
        parities.add(c % 2)
        for _, mont in FORMS:
            assert host.verify(shifted, m, sig, mont) == want
    assert parities == {0, 1}


def test_host_refusals():
    from plonk_prototype_amd import _lib
    cs = S.case("5_2_per_round", len(J.edge_scalars()))
    host, h = Host(cs["h"]), cs["h"]
    lib, BAD = host.lib, _lib.PM_ERR_BAD_ARG
    sk, k = (_u64p(S.canon_words(v)) for v in (5, 7))
    msg = _u64p(S.mont_words(9))
    pk, sig = _u64p(S.point_words(cs["pk"][3])), _u64p(S.sig_words(cs["sig"][3], False))
    out, reason = np.zeros((3, 4), np.uint64), C.c_uint32()
    assert lib.pm_schnorr_sign_host(*host.consts(), sk, k, msg, 1, _u64p(out)) == 0
    assert lib.pm_schnorr_verify_host(*host.consts(), pk, _u64p(S.mont_words(cs["m"][3])), sig, 1, C.byref(reason)) == 0
    assert reason.value == 0
    odd = J.M.curve_point(0x14)
    assert J.mul(odd, Q) != J.IDENTITY
    for bad_g in (S.point_words(J.IDENTITY), S.point_words(odd), S.point_words((J.GENERATOR[0], J.GENERATOR[1] + 1))):
        assert lib.pm_schnorr_sign_host(*host.consts(bad_g), sk, k, msg, 1, _u64p(out)) == BAD
        assert lib.pm_schnorr_verify_host(*host.consts(bad_g), pk, msg, sig, 1, C.byref(reason)) == BAD
    for form in (2, 0xFFFFFFFF):                              # an unknown scalar form
        assert lib.pm_schnorr_sign_host(*host.consts(), sk, k, msg, form, _u64p(out)) == BAD
        assert lib.pm_schnorr_verify_host(*host.consts(), pk, msg, sig, form, C.byref(reason)) == BAD
    big = _u64p(S.canon_words(R))                             # a message, a key or a nonce that is not below r
    assert lib.pm_schnorr_sign_host(*host.consts(), sk, k, big, 1, _u64p(out)) == BAD
    assert lib.pm_schnorr_verify_host(*host.consts(), pk, big, sig, 1, C.byref(reason)) == BAD
    assert lib.pm_schnorr_sign_host(*host.consts(), big, k, msg, 1, _u64p(out)) == BAD
    assert lib.pm_schnorr_sign_host(*host.consts(), sk, big, msg, 1, _u64p(out)) == BAD
    # NULL, one argument at a time
    c0 = host.consts()
    for j in (0, 3, 4, 6):
        c1 = list(c0)
        c1[j] = None
        assert lib.pm_schnorr_sign_host(*c1, sk, k, msg, 1, _u64p(out)) == BAD
        assert lib.pm_schnorr_verify_host(*c1, pk, msg, sig, 1, C.byref(reason)) == BAD
    assert lib.pm_schnorr_sign_host(*c0, None, k, msg, 1, _u64p(out)) == BAD
    assert lib.pm_schnorr_sign_host(*c0, sk, None, msg, 1, _u64p(out)) == BAD
    assert lib.pm_schnorr_sign_host(*c0, sk, k, None, 1, _u64p(out)) == BAD
    assert lib.pm_schnorr_sign_host(*c0, sk, k, msg, 1, None) == BAD
    assert lib.pm_schnorr_verify_host(*c0, None, msg, sig, 1, C.byref(reason)) == BAD
    assert lib.pm_schnorr_verify_host(*c0, pk, None, sig, 1, C.byref(reason)) == BAD
    assert lib.pm_schnorr_verify_host(*c0, pk, msg, None, 1, C.byref(reason)) == BAD
    assert lib.pm_schnorr_verify_host(*c0, pk, msg, sig, 1, None) == BAD
    # constants pm_hades_params_create refuses
    assert lib.pm_schnorr_sign_host(c0[0], h.rounds, 3, c0[3], c0[4], h.n_mds, c0[6], sk, k, msg, 1, _u64p(out)) == BAD


def test_python_host_wrappers():
    import plonk_prototype_amd as pa
    cs = S.case("5_2_per_round", len(J.edge_scalars()))
    h = cs["h"]
    i = 20
    got = pa.schnorr_sign_host(J.GENERATOR, h.flat_ark, h.flat_mds, cs["sk"][i], cs["k"][i], cs["m"][i], rounds=h.rounds,
                               full_rounds=h.full)
    assert got.tobytes() == S.sig_words(cs["sig"][i], False).tobytes()
    assert pa.schnorr_verify_host(J.GENERATOR, h.flat_ark, h.flat_mds, cs["pk"][i], cs["m"][i], list(cs["sig"][i]),
                                  rounds=h.rounds, full_rounds=h.full) == 0
    assert pa.schnorr_verify_host(J.GENERATOR, h.flat_ark, h.flat_mds, cs["pk"][i], cs["m"][i] ^ 1, list(cs["sig"][i]),
                                  rounds=h.rounds, full_rounds=h.full) == 4
