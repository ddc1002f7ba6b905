"""Native Schnorr signatures on JubJub (``pm_schnorr_*``): batch signing and verification on the GPU of
the check ``u G + c PK = R`` with ``c = H(R.x, R.y, m)`` truncated to 250 bits -- the construction the ``variable_base`` gadget
exists to constrain, outside a circuit.

This is the shape of dusk-schnorr 0.7's single-key signature as remembered: prior knowledge that nothing in this repository
pins, like the sponge of :mod:`.poseidon` and ``JUBJUB_GENERATOR``.  ``H`` is the modelled sponge of ``pm_poseidon_hash_dev``.

Secret keys, nonces and the ``u`` of a signature are scalars by the conventions of :mod:`.jubjub`: Montgomery limb arrays
(``uint64``, last axis 4) or Python integers in ``[0, r)``, which go in as ``PM_SCALAR_CANONICAL``; what comes back is in the
form that went in.  Messages and coordinates are always Montgomery limbs (or integers, converted).  A signature is
``[3, 4]``: ``u``, ``R.x``, ``R.y``.

With ``JubJubBase.from_key`` and ``Hades.from_key`` the base and the constants are those of a key's own FIXED_BASE and HADES
gadgets, unchanged: a natively made signature is then the one that key's gadgets constrain.  Building the in-circuit check
itself is not part of this module.

``Schnorr.verify_batch`` checks many signatures with ONE equation, a random linear combination summed by the JubJub MSM (section
7.2m).  It is a COFACTORED check, weaker than ``verify``: see its docstring.

Signing is NOT hardened against side channels: table addresses depend on the nonce."""
from __future__ import annotations

import ctypes as C
import secrets

import numpy as np

from . import _lib
from .field import fr_vec_from_limbs, fr_vec_to_limbs
from .host import DeviceVector, _p
from .jubjub import JUBJUB_ORDER, JubJubBase, _encodings, _points, _scalars, jubjub_compress, jubjub_decompress_dev
from .poseidon import Hades, _capacity, _elements

SCHNORR_REASONS = _lib.SCHNORR_REASONS


def _signatures(x, form: int) -> np.ndarray:
    """limbs ([..., 3, 4], ``u`` in ``form``) or (u, R.x, R.y) integer triples -> [n, 3, 4]"""
    if isinstance(x, np.ndarray) and x.dtype == np.uint64:
        return np.ascontiguousarray(x).reshape(-1, 3, 4)
    flat = [int(v) for v in np.asarray(x, dtype=object).reshape(-1)]
    if len(flat) % 3:
        raise ValueError("signatures are (u, R.x, R.y) triples")
    us, fu = _scalars(flat[0::3])
    if fu != form:
        raise ValueError("integer signatures carry a canonical u")
    rs = fr_vec_to_limbs([c for k in range(len(flat) // 3) for c in flat[3 * k + 1:3 * k + 3]]).reshape(-1, 2, 4)
    return np.concatenate([us.reshape(-1, 1, 4), rs], axis=1)


def _host_args(g, ark, mds, rounds, capacity):
    gp, a, m = _points(g), _elements(ark), _elements(mds)
    if gp.shape[0] != 1 or a.shape[0] != 5 * rounds or m.shape[0] % 25:
        raise ValueError("one base point, rounds x 5 round keys and whole 5 x 5 matrices")
    return gp, a, m, _capacity(capacity)


def schnorr_sign_host(g, ark, mds, secret_key, nonce, message, capacity=0, rounds: int = 67, full_rounds: int = 8) -> np.ndarray:
    """``pm_schnorr_sign_host``: one signature on the CPU, no context -> [3, 4] (``u`` in the form of ``secret_key``)"""
    gp, a, m, cap = _host_args(g, ark, mds, rounds, capacity)
    (sk, form), (k, form_k), msg = _scalars(secret_key), _scalars(nonce), _elements(message, 1)
    if form != form_k or sk.shape[0] != 1 or k.shape[0] != 1:
        raise ValueError("one secret key and one nonce, in one form")
    out = np.zeros((3, 4), np.uint64)
    rc = _lib.load().pm_schnorr_sign_host(_p(gp), rounds, full_rounds, _p(a), _p(m), m.shape[0] // 25, _p(cap), _p(sk), _p(k), _p(msg),
                                          form, _p(out))
    if rc != _lib.PM_OK:
        raise ValueError("pm_schnorr_sign_host refused its arguments")
    return out


def schnorr_verify_host(g, ark, mds, public_key, message, signature, capacity=0, rounds: int = 67, full_rounds: int = 8,
                        scalar_form: int | None = None) -> int:
    """``pm_schnorr_verify_host``: the reason (0 = valid, else a key of ``SCHNORR_REASONS``) on the CPU, no context.  A limb
    signature carries a Montgomery ``u`` unless ``scalar_form`` says otherwise; an integer triple a canonical one."""
    gp, a, m, cap = _host_args(g, ark, mds, rounds, capacity)
    limbs = isinstance(signature, np.ndarray) and signature.dtype == np.uint64
    form = scalar_form if scalar_form is not None else (_lib.SCALAR_MONTGOMERY if limbs else _lib.SCALAR_CANONICAL)
    pk, msg, sig = _points(public_key), _elements(message, 1), _signatures(signature, form)
    if pk.shape[0] != 1 or sig.shape[0] != 1:
        raise ValueError("one public key and one signature")
    reason = C.c_uint32()
    rc = _lib.load().pm_schnorr_verify_host(_p(gp), rounds, full_rounds, _p(a), _p(m), m.shape[0] // 25, _p(cap), _p(pk), _p(msg),
                                            _p(sig), form, C.byref(reason))
    if rc != _lib.PM_OK:
        raise ValueError("pm_schnorr_verify_host refused its arguments")
    return int(reason.value)


class Schnorr:
    """Signing and verification over one base and one set of Hades constants on a context's GPU.

    ``Schnorr(g, hades, capacity=0)``: ``g`` a :class:`JubJubBase` whose point has order exactly ``JUBJUB_ORDER`` (checked by the
    library at the first call, which raises otherwise), ``hades`` a :class:`Hades`, ``capacity`` the sponge's capacity word.
    Handles from ``JubJubBase.from_key`` / ``Hades.from_key`` work unchanged (the module docstring)."""

    def __init__(self, g: JubJubBase, hades: Hades, capacity=0):
        if g.ctx is not hades.ctx:
            raise ValueError("the base and the constants belong to different contexts")
        self.ctx, self.g, self.hades, self._cap = g.ctx, g, hades, _capacity(capacity)

    def public_keys(self, secret_keys) -> np.ndarray:
        """``g.mul``: [n, 2, 4] limbs of ``sk_i G``"""
        return self.g.mul(secret_keys)

    # ------------------------------------------------------------------ device forms (addresses as integers)
    def sign_dev(self, d_secret_keys: int, d_nonces: int, d_msgs: int, n: int, d_sigs: int,
                 scalar_form: int = _lib.SCALAR_MONTGOMERY, stream: int = 0):
        """``pm_schnorr_sign_dev``: n keys, nonces and messages -> n signatures (3 elements each) at ``d_sigs``; asynchronous.
        Not hardened against side channels."""
        c = self.ctx
        c._check(c._lib.pm_schnorr_sign_dev(c._h, self.g._h, self.hades._h, _p(self._cap), C.c_void_p(d_secret_keys),
                                            C.c_void_p(d_nonces), C.c_void_p(d_msgs), n, scalar_form, C.c_void_p(d_sigs),
                                            C.c_void_p(stream)))

    def verify_dev(self, d_pks: int, d_msgs: int, d_sigs: int, n: int, d_reasons: int = 0, want_first_bad: bool = True,
                   scalar_form: int = _lib.SCALAR_MONTGOMERY, stream: int = 0):
        """``pm_schnorr_verify_dev``: n reasons (``uint32``) at ``d_reasons`` (0 = none wanted); returns the lowest failing index,
        ``n`` when all pass, or None when ``want_first_bad`` is false.  Waits for the device."""
        c = self.ctx
        bad = C.c_size_t()
        c._check(c._lib.pm_schnorr_verify_dev(c._h, self.g._h, self.hades._h, _p(self._cap), C.c_void_p(d_pks), C.c_void_p(d_msgs),
                                              C.c_void_p(d_sigs), n, scalar_form, C.c_void_p(d_reasons) if d_reasons else None,
                                              C.byref(bad) if want_first_bad else None, C.c_void_p(stream)))
        return int(bad.value) if want_first_bad else None

    def verify_batch_dev(self, d_pks: int, d_msgs: int, d_sigs: int, d_weights: int, n: int, d_sum: int = 0,
                         scalar_form: int = _lib.SCALAR_MONTGOMERY, stream: int = 0):
        """``pm_schnorr_verify_batch_dev``: one cofactored equation for n signatures under the weights at ``d_weights`` (n x 16
        bytes, ``0 < z_i < 2^128``); ``d_sum`` (0 = not wanted) receives the sum W, 2 elements.  Returns ``(result, first_bad)``:
        ``(0, n)`` accepted, ``(4, n)`` the equation fails, else the structural reason and index of the lowest bad entry.  Waits."""
        c = self.ctx
        res, bad = C.c_uint32(), C.c_size_t()
        c._check(c._lib.pm_schnorr_verify_batch_dev(c._h, self.g._h, self.hades._h, _p(self._cap), C.c_void_p(d_pks), C.c_void_p(d_msgs),
                                                    C.c_void_p(d_sigs), C.c_void_p(d_weights), n, scalar_form,
                                                    C.c_void_p(d_sum) if d_sum else None, C.byref(res), C.byref(bad), C.c_void_p(stream)))
        return int(res.value), int(bad.value)

    # ------------------------------------------------------------------ host arrays in, host arrays out
    def sign(self, secret_keys, messages, nonces=None) -> np.ndarray:
        """-> [n, 3, 4]: ``u`` (in the form of ``secret_keys``), ``R.x``, ``R.y``.  ``nonces=None`` draws them with :mod:`secrets`
        in ``[1, l)``; the library itself has no random number generator."""
        sk, form = _scalars(secret_keys)
        n = sk.shape[0]
        if nonces is None:
            ks = [1 + secrets.randbelow(JUBJUB_ORDER - 1) for _ in range(n)]
            k = (_scalars(ks)[0] if form == _lib.SCALAR_CANONICAL else fr_vec_to_limbs(ks)).reshape(-1, 4)
        else:
            k, form_k = _scalars(nonces)
            if form_k != form:
                raise ValueError("secret keys and nonces must have one form")
        msg = _elements(messages)
        if k.shape[0] != n or msg.shape[0] != n:
            raise ValueError("one nonce and one message per secret key")
        if n == 0:
            return np.zeros((0, 3, 4), np.uint64)
        ds, dk, dm = (DeviceVector.from_host(self.ctx, x) for x in (sk, k, msg))
        out = DeviceVector(self.ctx, 3 * n)
        try:
            self.sign_dev(ds.ptr, dk.ptr, dm.ptr, n, out.ptr, form)
            return out.to_host().reshape(n, 3, 4)
        finally:
            for x in (ds, dk, dm, out):
                x.free()

    def _verify(self, public_keys, messages, signatures, scalar_form, reasons: bool):
        limbs = isinstance(signatures, np.ndarray) and signatures.dtype == np.uint64
        form = scalar_form if scalar_form is not None else (_lib.SCALAR_MONTGOMERY if limbs else _lib.SCALAR_CANONICAL)
        pk, msg, sig = _points(public_keys), _elements(messages), _signatures(signatures, form)
        n = sig.shape[0]
        if pk.shape[0] != n or msg.shape[0] != n:
            raise ValueError("one public key and one message per signature")
        if n == 0:
            return np.zeros(0, np.uint32), 0, 0
        dp, dm, ds = (DeviceVector.from_host(self.ctx, x) for x in (pk, msg, sig))
        dr = DeviceVector(self.ctx, (n + 7) // 8) if reasons else None     # n uint32 in 32-byte elements
        try:
            bad = self.verify_dev(dp.ptr, dm.ptr, ds.ptr, n, dr.ptr if reasons else 0, True, form)
            got = dr.to_host().view(np.uint32).reshape(-1)[:n].copy() if reasons else None
            return got, bad, n
        finally:
            for x in (dp, dm, ds, dr):
                if x is not None:
                    x.free()

    def signatures_to_bytes(self, signatures, scalar_form: int | None = None) -> np.ndarray:
        """Signatures as a ledger stores them -> ``uint8 [n, 64]``: the canonical ``u``, little-endian, then the 32-byte encoding
        of ``R`` (:func:`~.jubjub.jubjub_compress`).  A limb array carries a Montgomery ``u`` unless ``scalar_form`` says
        otherwise; integer triples a canonical one.  Nothing is validated."""
        limbs = isinstance(signatures, np.ndarray) and signatures.dtype == np.uint64
        form = scalar_form if scalar_form is not None else (_lib.SCALAR_MONTGOMERY if limbs else _lib.SCALAR_CANONICAL)
        sig = _signatures(signatures, form)
        n = sig.shape[0]
        out = np.zeros((n, 64), np.uint8)
        if n == 0:
            return out
        u = sig[:, 0, :]
        if form == _lib.SCALAR_MONTGOMERY:
            u = _scalars(fr_vec_from_limbs(np.ascontiguousarray(u)))[0]
        out[:, :32] = np.ascontiguousarray(u).view(np.uint8).reshape(n, 32)
        out[:, 32:] = jubjub_compress(self.ctx, np.ascontiguousarray(sig[:, 1:, :]))
        return out

    def verify_bytes(self, public_key_bytes, messages, signature_bytes) -> np.ndarray:
        """:meth:`verify` for keys and signatures as a ledger stores them: ``public_key_bytes`` ``uint8 [n, 32]``,
        ``signature_bytes`` ``uint8 [n, 64]`` (:meth:`signatures_to_bytes`) -> [n] ``uint32`` reasons.  Both are uploaded as they
        are; the ``R`` halves are decoded on the device straight into the ``(u, R.x, R.y)`` records (strides of 64 and 96 bytes),
        the ``u`` halves are copied beside them and go in canonical.  A key or an ``R`` that does not decode is ``(0, 0)`` and gets
        the reason :meth:`verify` gives it (``pk_point``, ``r_point``); a ``u`` that is not below ``l`` is ``verify``'s business."""
        pkb, sgb, msg = _encodings(public_key_bytes), _encodings(signature_bytes, 64), _elements(messages)
        n = sgb.shape[0]
        if pkb.shape[0] != n or msg.shape[0] != n:
            raise ValueError("one public key and one message per signature")
        if n == 0:
            return np.zeros(0, np.uint32)
        c = self.ctx
        bufs = [DeviceVector.from_host(c, x) for x in (pkb.view(np.uint64), sgb.view(np.uint64), msg)]
        try:
            dpb, dsb, dm = bufs
            dp, ds, dr = DeviceVector(c, 2 * n), DeviceVector(c, 3 * n), DeviceVector(c, (n + 7) // 8)
            bufs += [dp, ds, dr]
            jubjub_decompress_dev(c, dpb.ptr, n, dp.ptr, want_n_ok=False)
            jubjub_decompress_dev(c, dsb.ptr + 32, n, ds.ptr + 32, in_stride=64, out_stride=96, want_n_ok=False)
            c._check(c._lib.pm_dev_copy_strided(c._h, C.c_void_p(ds.ptr), 96, C.c_void_p(dsb.ptr), 64, 32, n, None))
            self.verify_dev(dp.ptr, dm.ptr, ds.ptr, n, dr.ptr, False, _lib.SCALAR_CANONICAL)
            return dr.to_host().view(np.uint32).reshape(-1)[:n].copy()
        finally:
            for x in bufs:
                x.free()

    def verify(self, public_keys, messages, signatures, scalar_form: int | None = None) -> np.ndarray:
        """-> [n] ``uint32`` reasons: 0 = valid, else a key of ``SCHNORR_REASONS``.  A limb array of signatures carries a Montgomery
        ``u`` unless ``scalar_form`` says otherwise; integer triples a canonical one."""
        return self._verify(public_keys, messages, signatures, scalar_form, True)[0]

    def verify_all(self, public_keys, messages, signatures, scalar_form: int | None = None):
        """None when every signature is valid, else the lowest bad index"""
        _, bad, n = self._verify(public_keys, messages, signatures, scalar_form, False)
        return None if bad == n else bad

    def verify_batch_report(self, public_keys, messages, signatures, weights=None, scalar_form: int | None = None):
        """:meth:`verify_batch` with everything the call says: ``(result, first_bad, W)``, W as [2, 4] limbs"""
        limbs = isinstance(signatures, np.ndarray) and signatures.dtype == np.uint64
        form = scalar_form if scalar_form is not None else (_lib.SCALAR_MONTGOMERY if limbs else _lib.SCALAR_CANONICAL)
        pk, msg, sig = _points(public_keys), _elements(messages), _signatures(signatures, form)
        n = sig.shape[0]
        if pk.shape[0] != n or msg.shape[0] != n:
            raise ValueError("one public key and one message per signature")
        zs = [1 + secrets.randbelow((1 << 128) - 1) for _ in range(n)] if weights is None else [int(z) for z in weights]
        if len(zs) != n:
            raise ValueError("one weight per signature")
        if any(not 0 <= z < (1 << 128) for z in zs):
            raise ValueError("a weight is not in [0, 2^128)")
        out = DeviceVector(self.ctx, 2)
        bufs = [out]
        try:
            if n:
                w = np.frombuffer(b"".join(z.to_bytes(16, "little") for z in zs) + bytes(16 * (n % 2)), dtype=np.uint64).reshape(-1, 4)
                bufs += [DeviceVector.from_host(self.ctx, x) for x in (pk, msg, sig, w.copy())]
            ptrs = [b.ptr for b in bufs[1:]] if n else [0, 0, 0, 0]
            res, bad = self.verify_batch_dev(ptrs[0], ptrs[1], ptrs[2], ptrs[3], n, out.ptr, form)
            return res, bad, out.to_host().reshape(2, 4)
        finally:
            for x in bufs:
                x.free()

    def verify_batch(self, public_keys, messages, signatures, weights=None, scalar_form: int | None = None, return_sum: bool = False):
        """All n signatures by ONE equation (``pm_schnorr_verify_batch_dev``) -> ``bool``, or ``(bool, W)`` with ``return_sum``.

        ``W = a G + sum b_i PK_i - sum z_i R_i`` with ``a = sum z_i u_i mod l`` and ``b_i = z_i c_i mod l``, summed by one
        :func:`~.jubjub.jubjub_msm_dev`; accepted when ``8 W`` is the identity.  ``weights=None`` draws the ``z_i`` with
        :mod:`secrets` in ``[1, 2^128)``, as :meth:`sign` draws nonces; a zero weight raises :class:`~.host.Error` (the library refuses it).

        This is a COFACTORED check: it accepts when every signature satisfies ``8 (u G + c PK - R) = O`` (and otherwise only
        with probability ``2^-128`` over the weights).  That is weaker than :meth:`verify`, which clears no cofactor: a signature
        its signer made with ``R = k G + T``, T of small order, fails there and passes here.  Whatever ``verify`` accepts, this
        accepts.  With predictable weights an attacker can make errors cancel: pass your own only in tests.  A structurally bad
        entry (``u >= l``, R or PK off the curve) raises nothing and returns ``False``; on ``False`` call :meth:`verify` to find
        the culprit.  Worth it from about 2^18 signatures on (2.4 x at 2^20); up to 2^12 the two take the same time and in between
        :meth:`verify_all` is up to 1.4 x quicker."""
        res, _, w = self.verify_batch_report(public_keys, messages, signatures, weights, scalar_form)
        return (res == _lib.SCHNORR_OK, w) if return_sum else res == _lib.SCHNORR_OK
