"""Batch Schnorr verification on the GPU (pm_schnorr_verify_batch_dev) against the big-integer model of
tests/jubjub_msm_model.py: the sum W itself, byte for byte, for valid batches, for one bad signature at every position, for
errors that cancel under equal weights and do not under others, for the two inputs on which the cofactored check and
pm_schnorr_verify_dev are documented to differ, for every structural fault, and the refusals."""
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gadget_model as M  # noqa: E402
import jubjub_model as J  # noqa: E402
import jubjub_msm_model as MM  # noqa: E402
import schnorr_model as S  # noqa: E402

pytestmark = pytest.mark.gpu
R, Q = S.R, S.Q
SIZES = (1, 2, 5, 64, 65, 130)
NMAX = max(SIZES)
TOP = (1 << 128) - 1
IDENTITY = J.to_limbs([J.IDENTITY])[0]
ORDER_2 = J.to_limbs([S.ORDER_2])[0]


def weights_for(n, seed=1):
    rng = random.Random(seed * 1000 + n)
    return ([1, TOP, 2] + [1 + rng.randrange(TOP) for _ in range(n)])[:n]


class Rig:
    def __init__(self, ctx, shape):
        import plonk_prototype_amd as pa
        self.pa, self.ctx, self.cs = pa, ctx, S.case(shape, NMAX)
        h = self.h = self.cs["h"]
        self.g = pa.JubJubBase(ctx, J.GENERATOR)
        self.hades = pa.Hades(ctx, M.to_limbs(h.flat_ark), M.to_limbs(h.flat_mds), h.rounds, h.full)
        self.s = pa.Schnorr(self.g, self.hades)

    def free(self):
        self.g.free(), self.hades.free()

    def report(self, pks, msgs, sigs, weights, mont=True):
        """integers in, as they would lie in memory -> (result, first_bad, W limbs)"""
        p = np.stack([S.point_words(x) for x in pks])
        s = np.stack([S.sig_words(x, mont) for x in sigs])
        return self.s.verify_batch_report(p, M.to_limbs(list(msgs)), s, weights, 0 if mont else 1)

    def reasons(self, pks, msgs, sigs, mont=True):
        p = np.stack([S.point_words(x) for x in pks])
        s = np.stack([S.sig_words(x, mont) for x in sigs])
        return list(self.s.verify(p, M.to_limbs(list(msgs)), s, 0 if mont else 1))

    def model(self, pks, msgs, sigs, weights):
        return J.to_limbs([MM.batch_sum(self.h, J.GENERATOR, pks, msgs, sigs, weights)])[0]


@pytest.fixture(scope="module", params=sorted(S.SHAPES))
def rig(ctx, request):
    r = Rig(ctx, request.param)
    yield r
    r.free()


@pytest.fixture(scope="module")
def rig1(ctx):
    r = Rig(ctx, "5_2_per_round")
    yield r
    r.free()


# ---------------------------------------------------------------------------------- 1. valid batches
def test_valid_batches_sum_to_the_identity(rig):
    cs = rig.cs
    for n in SIZES:
        z = weights_for(n)
        assert 1 in z and (n < 2 or TOP in z)
        for mont in ((True, False) if n in (5, 65) else (True,)):
            res, bad, w = rig.report(cs["pk"][:n], cs["m"][:n], cs["sig"][:n], z, mont)
            assert (res, bad) == (S.OK, n), (n, mont)
            assert w.tobytes() == rig.model(cs["pk"][:n], cs["m"][:n], cs["sig"][:n], z).tobytes() == IDENTITY.tobytes(), (n, mont)
    # the Python form: its own weights, both return shapes, integer triples
    pks, msgs, sigs = np.stack([S.point_words(x) for x in cs["pk"][:65]]), M.to_limbs(cs["m"][:65]), np.stack([S.sig_words(x, True) for x in cs["sig"][:65]])
    assert rig.s.verify_batch(pks, msgs, sigs) is True
    ok, w = rig.s.verify_batch(cs["pk"][:5], cs["m"][:5], cs["sig"][:5], return_sum=True)
    assert ok is True and np.array_equal(w, IDENTITY)
    assert rig.s.verify_batch(np.zeros((0, 2, 4), np.uint64), np.zeros((0, 4), np.uint64), np.zeros((0, 3, 4), np.uint64)) is True


# ---------------------------------------------------------------------------------- 2. one bad signature, everywhere
def test_one_bad_signature_at_every_position(rig1):
    # entries 1 .. 5 of the shared case: entry 0 has sk = 0, whose signature holds for every message
    n = 5
    pk, m0, sig0 = rig1.cs["pk"][1:1 + n], rig1.cs["m"][1:1 + n], rig1.cs["sig"][1:1 + n]
    assert all(s % Q for s in rig1.cs["sk"][1:1 + n])
    z = weights_for(n, 2)
    for at in range(n):
        u, rx, ry = sig0[at]
        for label, msgs, sigs in (("u + 1", m0, sig0[:at] + [((u + 1) % Q, rx, ry)] + sig0[at + 1:]),
                                  ("m + 1", m0[:at] + [(m0[at] + 1) % R] + m0[at + 1:], sig0)):
            res, bad, w = rig1.report(pk, msgs, sigs, z)
            want = rig1.model(pk, msgs, sigs, z)
            assert (res, bad) == (S.EQUATION, n), (at, label)
            assert w.tobytes() == want.tobytes() and w.tobytes() != IDENTITY.tobytes(), (at, label)
            assert rig1.s.verify_batch(np.stack([S.point_words(x) for x in pk]), M.to_limbs(msgs),
                                       np.stack([S.sig_words(x, True) for x in sigs]), z) is False


# ---------------------------------------------------------------------------------- 3. the weights are used
def test_errors_cancel_under_equal_weights_only(rig1):
    cs, d = rig1.cs, 0x1234567
    (u0, x0, y0), (u1, x1, y1) = cs["sig"][3], cs["sig"][4]
    pks, msgs, sigs = cs["pk"][3:5], cs["m"][3:5], [((u0 + d) % Q, x0, y0), ((u1 - d) % Q, x1, y1)]
    assert rig1.reasons(pks, msgs, sigs) == [S.EQUATION, S.EQUATION]
    res, bad, w = rig1.report(pks, msgs, sigs, [1, 1])                         # (+d) G + (-d) G
    assert (res, bad) == (S.OK, 2) and w.tobytes() == IDENTITY.tobytes() == rig1.model(pks, msgs, sigs, [1, 1]).tobytes()
    res, bad, w = rig1.report(pks, msgs, sigs, [1, 2])                         # (+d) G + 2 (-d) G = -d G
    assert (res, bad) == (S.EQUATION, 2) and w.tobytes() == J.to_limbs([J.mul(J.GENERATOR, (-d) % Q)])[0].tobytes()
    assert w.tobytes() == rig1.model(pks, msgs, sigs, [1, 2]).tobytes()


# ---------------------------------------------------------------------------------- 4. where the two checks differ, as documented
def test_the_cofactored_check_accepts_small_order_components(rig1):
    cs, h = rig1.cs, rig1.h
    sk, k, m, pk = cs["sk"][7], cs["k"][7], cs["m"][7], cs["pk"][7]
    # the signer adds the point of order 2 to R and signs what it then hashes
    rp = J.add(J.mul(J.GENERATOR, k), S.ORDER_2)
    c, _ = S.challenge(h, rp, m)
    sig = ((k - c * sk) % Q, rp[0], rp[1])
    assert S.reason(h, J.GENERATOR, pk, m, sig) == S.EQUATION and rig1.reasons([pk], [m], [sig]) == [S.EQUATION]
    for z, want in ((1, ORDER_2), (TOP, ORDER_2), (2, IDENTITY)):               # W = z (u G + c PK - R) = -z T
        res, bad, w = rig1.report([pk], [m], [sig], [z])
        assert (res, bad) == (S.OK, 1) and w.tobytes() == want.tobytes() == rig1.model([pk], [m], [sig], [z]).tobytes(), z
    # a public key with a component of order 2, under an odd challenge
    i = next(i for i in range(20, NMAX) if S.challenge(h, (cs["sig"][i][1], cs["sig"][i][2]), cs["m"][i])[0] & 1)
    pk2 = J.add(cs["pk"][i], S.ORDER_2)
    assert rig1.reasons([pk2], [cs["m"][i]], [cs["sig"][i]]) == [S.EQUATION]
    res, bad, w = rig1.report([pk2], [cs["m"][i]], [cs["sig"][i]], [1])         # b = c: W = c T = T
    assert (res, bad) == (S.OK, 1) and w.tobytes() == ORDER_2.tobytes() == rig1.model([pk2], [cs["m"][i]], [cs["sig"][i]], [1]).tobytes()
    # ... inside a batch of valid ones it is accepted all the same
    pks, msgs, sigs = cs["pk"][:6] + [pk2], cs["m"][:6] + [cs["m"][i]], cs["sig"][:6] + [cs["sig"][i]]
    res, bad, w = rig1.report(pks, msgs, sigs, [3, 5, 7, 9, 11, 13, 1])
    assert (res, bad) == (S.OK, 7) and w.tobytes() == ORDER_2.tobytes()


# ---------------------------------------------------------------------------------- 5. structural faults
def test_structural_faults_name_the_lowest_reason_of_the_lowest_index(rig1):
    cs, h, n = rig1.cs, rig1.h, 9
    z = weights_for(n, 3)
    bads = S.corruptions(h, cs["pk"][4], cs["m"][4], cs["sig"][4])
    assert {b[4] for b in bads} == {S.U_RANGE, S.R_POINT, S.PK_POINT, S.EQUATION}
    for mont in (True, False):
        for label, pk, m, sig, why in bads:
            if not mont and sig[0] >= R:
                continue
            pks, msgs, sigs = cs["pk"][:n], cs["m"][:n], cs["sig"][:n]
            pks[4], msgs[4], sigs[4] = pk, m, sig
            res, bad, w = rig1.report(pks, msgs, sigs, z, mont)
            want = MM.structural(h, J.GENERATOR, pks, msgs, sigs)
            assert (res, bad) == ((why, 4) if want else (S.EQUATION, n)), (label, mont)
            assert want is None or want == (why, 4)
            assert w.tobytes() == rig1.model(pks, msgs, sigs, z).tobytes(), (label, mont)   # a bad entry goes in as the identity
    # two bad entries: the lower index wins whatever its reason; and a failing equation elsewhere does not hide a structural fault
    pks, msgs, sigs = cs["pk"][:n], cs["m"][:n], cs["sig"][:n]
    pks[6] = bads[2][1]                                                        # PK off the curve at 6
    sigs[2] = (sigs[2][0], sigs[2][1], (sigs[2][2] + 1) % R)                   # R.y + 1 at 2
    assert not J.on_curve((sigs[2][1], sigs[2][2]))
    msgs[0] = (msgs[0] + 1) % R                                                # the equation fails at 0
    assert MM.structural(h, J.GENERATOR, pks, msgs, sigs) == (S.R_POINT, 2)
    res, bad, _ = rig1.report(pks, msgs, sigs, z)
    assert (res, bad) == (S.R_POINT, 2)
    assert rig1.s.verify_batch(np.stack([S.point_words(x) for x in pks]), M.to_limbs(msgs), np.stack([S.sig_words(x, True) for x in sigs]), z) is False


# ---------------------------------------------------------------------------------- 6. refusals
def test_refusals(ctx, rig1):
    pa, cs, n = rig1.pa, rig1.cs, 5
    for at in (0, 3):
        z = weights_for(n, 4)
        z[at] = 0
        if at == 3:
            z[4] = 0
        with pytest.raises(pa.Error) as e:
            rig1.report(cs["pk"][:n], cs["m"][:n], cs["sig"][:n], z)
        assert e.value.code == -1 and f"weight {at} is zero" in str(e.value)
    with pytest.raises(ValueError):
        rig1.report(cs["pk"][:n], cs["m"][:n], cs["sig"][:n], [1 << 128] * n)
    # a base whose order is not l
    g = pa.JubJubBase(ctx, J.edge_points()[1])
    try:
        with pytest.raises(pa.Error) as e:
            pa.Schnorr(g, rig1.hades).verify_batch(cs["pk"][:n], cs["m"][:n], cs["sig"][:n])
        assert e.value.code == -1 and "order" in str(e.value)
    finally:
        g.free()
    # the sum is optional; result and first_bad are not
    dv = [pa.DeviceVector.from_host(ctx, x.reshape(-1, 4)) for x in
          (np.stack([S.point_words(x) for x in cs["pk"][:2]]), M.to_limbs(cs["m"][:2]), np.stack([S.sig_words(x, True) for x in cs["sig"][:2]]),
           np.array([[1, 0, 2, 0]], np.uint64))]
    try:
        assert rig1.s.verify_batch_dev(dv[0].ptr, dv[1].ptr, dv[2].ptr, dv[3].ptr, 2) == (S.OK, 2)
        lib, s = ctx._lib, rig1.s
        import ctypes as C
        from plonk_prototype_amd.host import _p
        assert lib.pm_schnorr_verify_batch_dev(ctx._h, s.g._h, s.hades._h, _p(s._cap), C.c_void_p(dv[0].ptr), C.c_void_p(dv[1].ptr),
                                               C.c_void_p(dv[2].ptr), C.c_void_p(dv[3].ptr), 2, 0, None, None, None, None) == -1
        res, bad = C.c_uint32(), C.c_size_t()
        assert lib.pm_schnorr_verify_batch_dev(ctx._h, s.g._h, s.hades._h, _p(s._cap), C.c_void_p(dv[0].ptr), C.c_void_p(dv[1].ptr),
                                               C.c_void_p(dv[2].ptr), None, 2, 0, None, C.byref(res), C.byref(bad), None) == -1
        assert lib.pm_schnorr_verify_batch_dev(ctx._h, s.g._h, s.hades._h, _p(s._cap), C.c_void_p(dv[0].ptr + 8), C.c_void_p(dv[1].ptr),
                                               C.c_void_p(dv[2].ptr), C.c_void_p(dv[3].ptr), 2, 0, None, C.byref(res), C.byref(bad), None) == -1
        assert lib.pm_schnorr_verify_batch_dev(ctx._h, s.g._h, s.hades._h, _p(s._cap), C.c_void_p(dv[0].ptr), C.c_void_p(dv[1].ptr),
                                               C.c_void_p(dv[2].ptr), C.c_void_p(dv[3].ptr), 2, 2, None, C.byref(res), C.byref(bad), None) == -1
    finally:
        for x in dv:
            x.free()
