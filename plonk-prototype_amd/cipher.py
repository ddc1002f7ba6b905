"""The Poseidon cipher on JubJub keys (``pm_poseidon_cipher_*``): batch encryption and decryption of
notes on the GPU, and the recipient's side of a private ledger -- :meth:`PoseidonCipher.scan`, the trial decryption of every
note under one viewing key, and :meth:`PoseidonCipher.scan_keys`, under up to 64 of them in one call (section 7.2q).

With ``P`` the Hades permutation, ``L`` the message capacity (1 .. 4) and ``S`` a JubJub point, the shared secret::

    init    = [2^32, L, S.x, S.y, nonce]
    encrypt : s = P(init); s[1 + i] += m[i], c[i] = s[1 + i] (i < L); s = P(s); c[L] = s[1]
    decrypt : s = P(init); m[i] = c[i] - s[1 + i], s[1 + i] = c[i]; s = P(s); accepted when c[L] == s[1]

A note is ``(R, nonce, c)``: the sender picks an ephemeral integer ``e``, sends ``R = e G`` and encrypts under ``S = e PK`` with
``PK = vk G`` the recipient's key; the recipient recovers ``S = vk R``.  Multipliers are exact integers below ``r``.

This is the shape of dusk-poseidon's ``PoseidonCipher`` as remembered: prior knowledge that nothing in this repository pins,
like the sponge of :mod:`.poseidon` and the signature of :mod:`.schnorr`.  It is not claimed to produce dusk-poseidon's bytes.

Elements, coordinates, nonces and cipher words are Montgomery limbs (``uint64``, last axis 4) or Python integers, converted.  A
status is 0 when the tag matches, else a key of ``CIPHER_REASONS``, the lowest that applies; the messages of a refused note come
back as zeros.

The scan is NOT hardened against side channels: table addresses depend on the viewing key."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .host import DeviceVector, _p
from .jubjub import JubJubBase, _encodings, _points, _scalars, jubjub_decompress_dev, jubjub_mul
from .poseidon import WIDTH, Hades, _elements

CIPHER_REASONS = _lib.CIPHER_REASONS
CIPHER_SCAN_MAX_KEYS = _lib.CIPHER_SCAN_MAX_KEYS


def _check_len(msg_len) -> int:
    if not isinstance(msg_len, (int, np.integer)) or not 1 <= msg_len <= _lib.CIPHER_MAX_LEN:
        raise ValueError("msg_len must be 1 .. 4")
    return int(msg_len)


def _words(x, width: int, pad: bool, what: str) -> np.ndarray:
    """limbs ``[n, k, 4]`` or integers ``[n][k]`` (``[n]`` is k = 1) -> ``[n, width, 4]``; k < width is padded with zeros when
    ``pad``, anything else raises"""
    if isinstance(x, np.ndarray) and x.dtype != np.uint64 and x.dtype != object:
        raise ValueError(f"{what}: limb arrays are uint64")
    if isinstance(x, np.ndarray) and x.dtype == np.uint64:
        if x.ndim != 3 or x.shape[2] != 4:
            raise ValueError(f"{what}: limbs have the shape [n, k, 4]")
        a = np.ascontiguousarray(x)
    else:
        obj = np.asarray(x, dtype=object)
        if obj.ndim == 1:
            obj = obj.reshape(-1, 1)
        if obj.ndim != 2:
            raise ValueError(f"{what}: integers have the shape [n] or [n][k]")
        a = _elements(obj).reshape(obj.shape[0], obj.shape[1], 4) if obj.size else np.zeros((obj.shape[0], obj.shape[1], 4), np.uint64)
    k = a.shape[1]
    if k > width or k == 0 or (k < width and not pad):
        raise ValueError(f"{what}: {k} words where {'at most ' if pad else ''}{width} are expected")
    if k < width:
        a = np.concatenate([a, np.zeros((a.shape[0], width - k, 4), np.uint64)], axis=1)
    return a


def _one(x):
    """the words of ONE note, limbs ``[k, 4]`` or k integers, as a batch of one"""
    if isinstance(x, np.ndarray) and x.dtype == np.uint64 and x.ndim == 2:
        return x[None]
    return [list(x)] if not isinstance(x, np.ndarray) else x


def _nonces(x) -> np.ndarray:
    if isinstance(x, np.ndarray) and x.dtype != np.uint64 and x.dtype != object:
        raise ValueError("nonces: limb arrays are uint64")
    return _elements(x)


def _view_keys(x):
    """1 .. 64 viewing keys, integers or ``[K, 4]`` Montgomery limbs (``[4]`` is one key) -> ([K, 4] uint64, scalar_form)"""
    if isinstance(x, np.ndarray) and x.dtype == np.uint64:
        if x.ndim not in (1, 2) or x.shape[-1] != 4:
            raise ValueError("viewing keys: limbs have the shape [K, 4]")
    elif np.asarray(x, dtype=object).ndim > 1:
        raise ValueError("viewing keys: integers have the shape [K]")
    vk, form = _scalars(x)
    if not 1 <= vk.shape[0] <= CIPHER_SCAN_MAX_KEYS:
        raise ValueError(f"1 .. {CIPHER_SCAN_MAX_KEYS} viewing keys a call")
    return vk, form


def _host_consts(ark, mds, rounds):
    a, m = _elements(ark), _elements(mds)
    if a.shape[0] != WIDTH * rounds or m.shape[0] % 25 or m.shape[0] == 0:
        raise ValueError("rounds x 5 round keys and whole 5 x 5 matrices")
    return a, m


def poseidon_cipher_encrypt_host(ark, mds, secret, nonce, message, msg_len: int = 2, rounds: int = 67, full_rounds: int = 8) -> np.ndarray:
    """``pm_poseidon_cipher_encrypt_host``: one note on the CPU, no context -> ``[msg_len + 1, 4]`` limbs.  A message shorter
    than ``msg_len`` is padded with zeros."""
    L = _check_len(msg_len)
    a, m = _host_consts(ark, mds, rounds)
    s, k = _points(secret), _nonces(nonce)
    msg = _words(_one(message), L, True, "message")
    if s.shape[0] != 1 or k.shape[0] != 1 or msg.shape[0] != 1:
        raise ValueError("one secret, one nonce and one message")
    out = np.zeros((L + 1, 4), np.uint64)
    rc = _lib.load().pm_poseidon_cipher_encrypt_host(rounds, full_rounds, _p(a), _p(m), m.shape[0] // 25, _p(s), _p(k), _p(msg), L, _p(out))
    if rc != _lib.PM_OK:
        raise ValueError("pm_poseidon_cipher_encrypt_host refused its arguments")
    return out


def poseidon_cipher_decrypt_host(ark, mds, secret, nonce, cipher, msg_len: int = 2, rounds: int = 67, full_rounds: int = 8):
    """``pm_poseidon_cipher_decrypt_host``: one note on the CPU, no context -> ``(message [msg_len, 4], status)``"""
    L = _check_len(msg_len)
    a, m = _host_consts(ark, mds, rounds)
    s, k = _points(secret), _nonces(nonce)
    c = _words(_one(cipher), L + 1, False, "cipher")
    if s.shape[0] != 1 or k.shape[0] != 1 or c.shape[0] != 1:
        raise ValueError("one secret, one nonce and one cipher")
    out, status = np.zeros((L, 4), np.uint64), C.c_uint32()
    rc = _lib.load().pm_poseidon_cipher_decrypt_host(rounds, full_rounds, _p(a), _p(m), m.shape[0] // 25, _p(s), _p(k), _p(c), L, _p(out),
                                                     C.byref(status))
    if rc != _lib.PM_OK:
        raise ValueError("pm_poseidon_cipher_decrypt_host refused its arguments")
    return out, int(status.value)


class PoseidonCipher:
    """The cipher over one set of Hades constants on a context's GPU.

    ``PoseidonCipher(hades, msg_len=2)``: ``hades`` a :class:`Hades` (``Hades.from_key`` handles work unchanged), ``msg_len`` the
    message capacity L, 1 .. 4."""

    def __init__(self, hades: Hades, msg_len: int = 2):
        if not isinstance(hades, Hades):
            raise ValueError("hades must be a Hades handle")
        self.ctx, self.hades, self.msg_len = hades.ctx, hades, _check_len(msg_len)

    # ------------------------------------------------------------------ device forms (addresses as integers)
    def encrypt_dev(self, d_secrets: int, d_nonces: int, d_msgs: int, n: int, d_ciphers: int, stream: int = 0):
        """``pm_poseidon_cipher_encrypt_dev``: n secrets (2 elements each), nonces and messages (L each) -> n ciphers (L + 1
        each) at ``d_ciphers``; asynchronous.  Secrets and messages are not validated."""
        c = self.ctx
        c._check(c._lib.pm_poseidon_cipher_encrypt_dev(c._h, self.hades._h, C.c_void_p(d_secrets), C.c_void_p(d_nonces), C.c_void_p(d_msgs),
                                                       self.msg_len, n, C.c_void_p(d_ciphers), C.c_void_p(stream)))

    def decrypt_dev(self, d_secrets: int, d_nonces: int, d_ciphers: int, n: int, d_msgs: int, d_status: int = 0,
                    want_n_ok: bool = True, stream: int = 0):
        """``pm_poseidon_cipher_decrypt_dev``: n messages (L elements each, zero where refused) at ``d_msgs`` and n ``uint32`` at
        ``d_status`` (0 = not wanted).  Returns the count of status 0 and waits for the stream, or None, asynchronous, when
        ``want_n_ok`` is false."""
        c = self.ctx
        ok = C.c_size_t()
        c._check(c._lib.pm_poseidon_cipher_decrypt_dev(c._h, self.hades._h, C.c_void_p(d_secrets), C.c_void_p(d_nonces), C.c_void_p(d_ciphers),
                                                       self.msg_len, n, C.c_void_p(d_msgs), C.c_void_p(d_status) if d_status else None,
                                                       C.byref(ok) if want_n_ok else None, C.c_void_p(stream)))
        return int(ok.value) if want_n_ok else None

    def scan_dev(self, view_key, d_ephemeral: int, d_nonces: int, d_ciphers: int, n: int, d_msgs: int, d_status: int = 0,
                 want_n_ok: bool = True, scalar_form: int | None = None, stream: int = 0):
        """``pm_poseidon_cipher_scan_dev``: as :meth:`decrypt_dev` with the secrets ``vk R_i`` computed from the ephemeral keys at
        ``d_ephemeral`` under ONE viewing key, an integer (canonical) or ``[4]`` limbs (Montgomery unless ``scalar_form`` says
        otherwise).  Waits for the device.  Not hardened against side channels."""
        vk, form = _scalars(view_key)
        if vk.shape[0] != 1:
            raise ValueError("one viewing key")
        c = self.ctx
        ok = C.c_size_t()
        c._check(c._lib.pm_poseidon_cipher_scan_dev(c._h, self.hades._h, _p(vk), form if scalar_form is None else scalar_form,
                                                    C.c_void_p(d_ephemeral), C.c_void_p(d_nonces), C.c_void_p(d_ciphers), self.msg_len, n,
                                                    C.c_void_p(d_msgs), C.c_void_p(d_status) if d_status else None,
                                                    C.byref(ok) if want_n_ok else None, C.c_void_p(stream)))
        return int(ok.value) if want_n_ok else None

    # ------------------------------------------------------------------ host arrays in, host arrays out
    def encrypt(self, secrets, nonces, messages) -> np.ndarray:
        """-> ``[n, L + 1, 4]`` limbs.  ``messages``: ``[n, k, 4]`` limbs or ``[n][k]`` integers, k <= L, padded with zeros."""
        L = self.msg_len
        s, k, m = _points(secrets), _nonces(nonces), _words(messages, L, True, "messages")
        n = s.shape[0]
        if k.shape[0] != n or m.shape[0] != n:
            raise ValueError("one nonce and one message per secret")
        if n == 0:
            return np.zeros((0, L + 1, 4), np.uint64)
        ds, dk, dm = (DeviceVector.from_host(self.ctx, x.reshape(-1, 4)) for x in (s, k, m))
        out = DeviceVector(self.ctx, (L + 1) * n)
        try:
            self.encrypt_dev(ds.ptr, dk.ptr, dm.ptr, n, out.ptr)
            return out.to_host().reshape(n, L + 1, 4)
        finally:
            for x in (ds, dk, dm, out):
                x.free()

    def _open(self, first, nonces, ciphers, call, decode=None):
        """the common half of decrypt and scan: ``first`` is [n, 2, 4], ``call(d_first, d_nonces, d_ciphers, n, d_msgs, d_status)``.
        With ``decode`` (the subgroup flag) ``first`` is ``uint8 [n, 32]`` instead: uploaded as it is and decoded on the device
        into the buffer ``call`` reads, so the points never visit the host."""
        L = self.msg_len
        k, c = _nonces(nonces), _words(ciphers, L + 1, False, "ciphers")
        n = first.shape[0]
        if k.shape[0] != n or c.shape[0] != n:
            raise ValueError("one nonce and one cipher per point")
        if n == 0:
            return np.zeros((0, L, 4), np.uint64), np.zeros(0, np.uint32)
        bufs = [DeviceVector.from_host(self.ctx, x.reshape(-1, 4)) for x in (first if decode is None else first.view(np.uint64), k, c)]
        try:
            dp, dk, dc = bufs
            if decode is not None:
                bufs.append(DeviceVector(self.ctx, 2 * n))
                jubjub_decompress_dev(self.ctx, dp.ptr, n, bufs[-1].ptr, 0, decode, want_n_ok=False)
                dp = bufs[-1]
            dm, ds = DeviceVector(self.ctx, L * n), DeviceVector(self.ctx, (n + 7) // 8)     # n uint32 in 32-byte elements
            bufs += [dm, ds]
            call(dp.ptr, dk.ptr, dc.ptr, n, dm.ptr, ds.ptr)
            return dm.to_host().reshape(n, L, 4), ds.to_host().view(np.uint32).reshape(-1)[:n].copy()
        finally:
            for x in bufs:
                x.free()

    def decrypt(self, secrets, nonces, ciphers):
        """-> ``(messages [n, L, 4], status [n] uint32)``: status 0 = the tag matches, else a key of ``CIPHER_REASONS``; the
        messages of a refused note are zero"""
        return self._open(_points(secrets), nonces, ciphers, lambda *a: self.decrypt_dev(*a, want_n_ok=False))

    def scan(self, view_key, ephemeral_keys, nonces, ciphers, scalar_form: int | None = None):
        """The notes ``(R_i, nonce_i, c_i)`` under one viewing key -> ``(messages, status)`` as :meth:`decrypt`: status 0 marks
        the key's own notes, 3 the others.  ``view_key``: an integer or ``[4]`` Montgomery limbs."""
        vk, form = _scalars(view_key)
        if vk.shape[0] != 1:
            raise ValueError("one viewing key")
        form = form if scalar_form is None else scalar_form
        return self._open(_points(ephemeral_keys), nonces, ciphers,
                          lambda *a: self.scan_dev(vk, *a, want_n_ok=False, scalar_form=form))

    def scan_bytes(self, view_key, ephemeral_bytes, nonces, ciphers, check_subgroup: bool = False, scalar_form: int | None = None):
        """:meth:`scan` for ephemeral keys as a ledger stores them, ``uint8 [n, 32]`` (:func:`~.jubjub.jubjub_compress`): the
        bytes are uploaded, decoded on the device (:func:`~.jubjub.jubjub_decompress_dev`) and handed to :meth:`scan_dev` without
        a round trip of the points.  The result is that of :meth:`scan` on the decoded points: a key that does not decode comes
        back with status 1 (``point``) and zero messages.  Nonces and cipher words stay limbs or integers."""
        vk, form = _scalars(view_key)
        if vk.shape[0] != 1:
            raise ValueError("one viewing key")
        form = form if scalar_form is None else scalar_form
        return self._open(_encodings(ephemeral_bytes), nonces, ciphers,
                          lambda *a: self.scan_dev(vk, *a, want_n_ok=False, scalar_form=form), decode=bool(check_subgroup))

    # ------------------------------------------------------------------ many viewing keys in one scan
    def scan_keys_dev(self, view_keys, d_ephemeral: int, d_nonces: int, d_ciphers: int, n: int, d_masks: int, d_msgs: int = 0,
                      d_status: int = 0, want_n_hits: bool = True, scalar_form: int | None = None, stream: int = 0):
        """``pm_poseidon_cipher_scan_keys_dev``: the n notes under 1 .. 64 viewing keys in one call.  ``d_masks`` receives n
        ``uint64``: bit k is set exactly when :meth:`scan_dev` under ``view_keys[k]`` gives note i the status 0.  ``d_msgs``
        (0 = not wanted) receives the message of the LOWEST key that opens the note, zeros where none does; ``d_status`` (0 =
        not wanted) 1 or 2 as :meth:`scan_dev` reports them, else 0 where a key opens the note, else 3.  Returns the number of
        set bits, or None when ``want_n_hits`` is false.  Waits for the device.  Not hardened against side channels."""
        vk, form = _view_keys(view_keys)
        c = self.ctx
        hits = C.c_size_t()
        c._check(c._lib.pm_poseidon_cipher_scan_keys_dev(c._h, self.hades._h, _p(vk), vk.shape[0], form if scalar_form is None else scalar_form,
                                                         C.c_void_p(d_ephemeral), C.c_void_p(d_nonces), C.c_void_p(d_ciphers),
                                                         self.msg_len, n, C.c_void_p(d_masks), C.c_void_p(d_msgs) if d_msgs else None,
                                                         C.c_void_p(d_status) if d_status else None,
                                                         C.byref(hits) if want_n_hits else None, C.c_void_p(stream)))
        return int(hits.value) if want_n_hits else None

    def _scan_keys(self, view_keys, first, nonces, ciphers, scalar_form, decode=None):
        """:meth:`_open` with the masks in front: -> (masks, messages, status)"""
        vk, form = _view_keys(view_keys)
        form = form if scalar_form is None else scalar_form
        n, masks = first.shape[0], []

        def call(dp, dk, dc, n, dm, ds):
            d_masks = DeviceVector(self.ctx, (n + 3) // 4)     # n uint64 in 32-byte elements
            try:
                self.scan_keys_dev(vk, dp, dk, dc, n, d_masks.ptr, dm, ds, want_n_hits=False, scalar_form=form)
                masks.append(d_masks.to_host().reshape(-1)[:n].copy())
            finally:
                d_masks.free()

        msgs, status = self._open(first, nonces, ciphers, call, decode)
        return (masks[0] if n else np.zeros(0, np.uint64)), msgs, status

    def scan_keys(self, view_keys, ephemeral_keys, nonces, ciphers, scalar_form: int | None = None):
        """The notes ``(R_i, nonce_i, c_i)`` under 1 .. 64 viewing keys in one call -> ``(masks [n] uint64, messages [n, L, 4],
        status [n] uint32)``: bit k of ``masks[i]`` is set exactly when :meth:`scan` under ``view_keys[k]`` gives note i the
        status 0; the message is that of the LOWEST such key -- two keys open one note only when they give the same secret, and
        then the same message -- and zero where there is none; the status is 1 or 2 where :meth:`scan` reports them (they depend
        on the note alone), else 0 where the mask is not zero, else 3.  ``view_keys``: integers or ``[K, 4]`` Montgomery limbs;
        duplicates and 0 are legal.  :meth:`hits` lists the (note, key) pairs."""
        return self._scan_keys(view_keys, _points(ephemeral_keys), nonces, ciphers, scalar_form)

    def scan_keys_bytes(self, view_keys, ephemeral_bytes, nonces, ciphers, check_subgroup: bool = False, scalar_form: int | None = None):
        """:meth:`scan_keys` for ephemeral keys as a ledger stores them, ``uint8 [n, 32]``, decoded on the device as
        :meth:`scan_bytes` does: a key that does not decode comes back with mask 0, status 1 and zero messages."""
        return self._scan_keys(view_keys, _encodings(ephemeral_bytes), nonces, ciphers, scalar_form, decode=bool(check_subgroup))

    @staticmethod
    def hits(masks) -> np.ndarray:
        """the masks of :meth:`scan_keys` -> ``[h, 2]`` ``int64`` (note, key) pairs, ascending by note, then by key"""
        m = np.ascontiguousarray(masks, dtype=np.uint64).reshape(-1)
        bits = (m[:, None] >> np.arange(64, dtype=np.uint64)[None, :]) & np.uint64(1)
        return np.argwhere(bits != 0).astype(np.int64).reshape(-1, 2)

    def encrypt_to(self, g: JubJubBase, public_keys, ephemeral_secrets, nonces, messages):
        """The sender's side, composed from ``g.mul``, :func:`~.jubjub.jubjub_mul` and :meth:`encrypt`: note i is encrypted to
        ``public_keys[i]`` under the ephemeral integer ``ephemeral_secrets[i]`` -> ``(ephemeral_keys [n, 2, 4] = e_i G, ciphers)``,
        what :meth:`scan` reads.  Neither the keys nor the secrets are validated; the ephemeral secrets are the caller's, as
        nonces are in :mod:`.schnorr`."""
        if g.ctx is not self.ctx:
            raise ValueError("the base and the constants belong to different contexts")
        pk = _points(public_keys)
        e, _ = _scalars(ephemeral_secrets)
        if pk.shape[0] != e.shape[0]:
            raise ValueError("one ephemeral secret per public key")
        if e.shape[0] == 0:
            return np.zeros((0, 2, 4), np.uint64), self.encrypt(pk, nonces, messages)
        return g.mul(ephemeral_secrets), self.encrypt(jubjub_mul(self.ctx, pk, ephemeral_secrets), nonces, messages)
