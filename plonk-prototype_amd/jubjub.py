"""Native JubJub on the GPU (``pm_jubjub_*``): scalar multiplications on the embedded curve outside a
circuit -- bulk fixed-base multiplication, two-base (Pedersen) commitments in one pass, per-point variable-base
multiplication, and the sum of many products (``jubjub_msm``, section 7.2m: a Pedersen vector commitment).

A point is affine ``(x, y)``: Montgomery limbs ``[2, 4]`` (``uint64``) or a pair of Python integers; the identity is ``(0, 1)``.
Scalars are Montgomery limb arrays (``uint64``, last axis 4: ``PM_SCALAR_MONTGOMERY``) or Python integers, which go in as
``PM_SCALAR_CANONICAL``.  The multiplier of a point is the integer ``0 <= s < r`` itself, never reduced modulo the order of
the subgroup.  With ``JubJubBase.from_key`` the base is the very point a key's FIXED_BASE gadget multiplies.  None of this is
hardened against side channels.

The wire format (section 7.2p): a point as 32 bytes, the canonical ``y`` little-endian with the least significant bit of the
canonical ``x`` in bit 255.  ``jubjub_decompress`` decodes a batch on the GPU with a status per point, ``jubjub_compress``
encodes, ``fr_sqrt`` is the square root in Fr underneath.  The shape of ``JubJubAffine::to_bytes`` / ``from_bytes`` as
remembered: prior knowledge that nothing in this repository pins; ``x = 0`` with the sign bit set is refused.

``JUBJUB_GENERATOR`` is the point with ``y = 0x12``; this repository checks that it lies on the curve and that the subgroup
order ``JUBJUB_ORDER`` takes it to the identity.  That it is dusk-jubjub's ``GENERATOR`` is prior knowledge, not something this
repository can verify.  No second generator is shipped: callers pass their own H."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .field import R_MOD, fr_vec_to_limbs
from .host import Context, DeviceVector, _p

#: The point with ``y = 0x12`` and the ``x`` below.  Checked in this repository (tests/test_jubjub_host.py): it lies on the
#: curve and the subgroup order ``JUBJUB_ORDER`` takes it to the identity.  That it is dusk-jubjub's ``GENERATOR`` is prior
#: knowledge, not something this repository can verify.  No second generator is shipped: callers pass their own H.
JUBJUB_GENERATOR = (0x3FD2814C43AC65A6F1FBF02D0FD6CCE62E3EBB21FD6C54ED4DF7B7FFEC7BEACA, 0x12)
JUBJUB_ORDER = 0x0E7DB4EA6533AFA906673B0101343B00A6682093CCC81082D0970E5ED6F72CB7


def _points(x) -> np.ndarray:
    """limbs (uint64, [..., 2, 4]) or (x, y) integer pairs -> [n, 2, 4] Montgomery limbs"""
    if isinstance(x, np.ndarray) and x.dtype == np.uint64:
        return np.ascontiguousarray(x).reshape(-1, 2, 4)
    flat = [int(v) for v in np.asarray(x, dtype=object).reshape(-1)]
    if len(flat) % 2:
        raise ValueError("points are (x, y) pairs")
    return fr_vec_to_limbs(flat).reshape(-1, 2, 4)


def _scalars(x):
    """-> ([n, 4] uint64, scalar_form): limb arrays are Montgomery elements, integers go in as they are (canonical)"""
    if isinstance(x, np.ndarray) and x.dtype == np.uint64:
        return np.ascontiguousarray(x).reshape(-1, 4), _lib.SCALAR_MONTGOMERY
    vals = [int(v) for v in np.asarray(x, dtype=object).reshape(-1)]
    if any(not 0 <= v < R_MOD for v in vals):
        raise ValueError("a scalar is not in [0, r)")
    buf = b"".join(v.to_bytes(32, "little") for v in vals)
    return np.frombuffer(buf, dtype=np.uint64).reshape(-1, 4).copy(), _lib.SCALAR_CANONICAL


def jubjub_mul_host(point, scalar) -> np.ndarray:
    """``pm_jubjub_mul_host``: ``scalar * point`` on the CPU by double-and-add, no context -> [2, 4] limbs"""
    p, (s, form) = _points(point), _scalars(scalar)
    if p.shape[0] != 1 or s.shape[0] != 1:
        raise ValueError("one point and one scalar")
    out = np.zeros((2, 4), np.uint64)
    if _lib.load().pm_jubjub_mul_host(_p(p), _p(s), form, _p(out)) != _lib.PM_OK:
        raise ValueError("pm_jubjub_mul_host refused its arguments")
    return out


def jubjub_add_host(p, q) -> np.ndarray:
    """``pm_jubjub_add_host``: ``p + q`` on the CPU, no context -> [2, 4] limbs"""
    a, b = _points(p), _points(q)
    if a.shape[0] != 1 or b.shape[0] != 1:
        raise ValueError("one point each")
    out = np.zeros((2, 4), np.uint64)
    if _lib.load().pm_jubjub_add_host(_p(a), _p(b), _p(out)) != _lib.PM_OK:
        raise ValueError("pm_jubjub_add_host refused its arguments")
    return out


class JubJubBase:
    """One point B on a context's GPU with its window table (``pm_jubjub_base``): ``.point``, ``.mul(scalars)``, ``.mul_dev``."""

    def __init__(self, ctx: Context, point):
        p = _points(point)
        if p.shape[0] != 1:
            raise ValueError("one point")
        h = C.c_void_p()
        ctx._check(ctx._lib.pm_jubjub_base_create(ctx._h, _p(p), C.byref(h)))
        self.ctx, self._h = ctx, h

    @classmethod
    def from_key(cls, pk, gadget_index: int) -> "JubJubBase":
        """``pm_jubjub_base_from_key``: the base of gadget ``gadget_index`` of ``pk``'s gadget table (kind FIXED_BASE, its table
        a doubling chain).  The result does not depend on the key afterwards."""
        ctx = pk.ctx
        h = C.c_void_p()
        ctx._check(ctx._lib.pm_jubjub_base_from_key(ctx._h, pk._h, int(gadget_index), C.byref(h)))
        self = object.__new__(cls)
        self.ctx, self._h = ctx, h
        return self

    @property
    def point(self) -> np.ndarray:
        """[2, 4] limbs"""
        out = np.zeros((2, 4), np.uint64)
        self.ctx._check(self.ctx._lib.pm_jubjub_base_point(self._h, _p(out)))
        return out

    def free(self):
        if getattr(self, "_h", None) and self.ctx._h:
            self.ctx._lib.pm_jubjub_base_free(self.ctx._h, self._h)
        self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass

    def mul_dev(self, d_scalars: int, n: int, d_out: int, scalar_form: int = _lib.SCALAR_MONTGOMERY, stream: int = 0):
        """``pm_jubjub_fixed_mul_dev``: n scalars at ``d_scalars`` -> n points (2 elements each) at ``d_out``; asynchronous"""
        c = self.ctx
        c._check(c._lib.pm_jubjub_fixed_mul_dev(c._h, self._h, C.c_void_p(d_scalars), n, scalar_form, C.c_void_p(d_out),
                                                C.c_void_p(stream)))

    def mul(self, scalars) -> np.ndarray:
        """scalars -> [n, 2, 4] limbs of ``s_i * B``"""
        s, form = _scalars(scalars)
        n = s.shape[0]
        if n == 0:
            return np.zeros((0, 2, 4), np.uint64)
        d, out = DeviceVector.from_host(self.ctx, s), DeviceVector(self.ctx, 2 * n)
        try:
            self.mul_dev(d.ptr, n, out.ptr, form)
            return out.to_host().reshape(n, 2, 4)
        finally:
            d.free(), out.free()


def jubjub_commit_dev(g: JubJubBase, h: JubJubBase, d_values: int, d_blinders: int, n: int, d_out: int,
                      scalar_form: int = _lib.SCALAR_MONTGOMERY, stream: int = 0):
    """``pm_jubjub_commit_dev``: ``out[i] = v_i G + b_i H``, n points (2 elements each) at ``d_out``; asynchronous"""
    c = g.ctx
    c._check(c._lib.pm_jubjub_commit_dev(c._h, g._h, h._h, C.c_void_p(d_values), C.c_void_p(d_blinders), n, scalar_form,
                                         C.c_void_p(d_out), C.c_void_p(stream)))


def jubjub_commit(g: JubJubBase, h: JubJubBase, values, blinders) -> np.ndarray:
    """-> [n, 2, 4] limbs of ``v_i G + b_i H``; values and blinders in the same form"""
    (v, form), (b, form_b) = _scalars(values), _scalars(blinders)
    if form != form_b or v.shape != b.shape:
        raise ValueError("values and blinders must have one form and one length")
    n = v.shape[0]
    if n == 0:
        return np.zeros((0, 2, 4), np.uint64)
    dv, db, out = DeviceVector.from_host(g.ctx, v), DeviceVector.from_host(g.ctx, b), DeviceVector(g.ctx, 2 * n)
    try:
        jubjub_commit_dev(g, h, dv.ptr, db.ptr, n, out.ptr, form)
        return out.to_host().reshape(n, 2, 4)
    finally:
        dv.free(), db.free(), out.free()


def jubjub_mul_dev(ctx: Context, d_points: int, d_scalars: int, n: int, d_out: int, scalar_form: int = _lib.SCALAR_MONTGOMERY,
                   stream: int = 0):
    """``pm_jubjub_mul_dev``: ``out[i] = s_i P_i``; ``d_out`` may be ``d_points``.  The points are not validated."""
    ctx._check(ctx._lib.pm_jubjub_mul_dev(ctx._h, C.c_void_p(d_points), C.c_void_p(d_scalars), n, scalar_form, C.c_void_p(d_out),
                                          C.c_void_p(stream)))


def jubjub_mul(ctx: Context, points, scalars) -> np.ndarray:
    """-> [n, 2, 4] limbs of ``s_i P_i``"""
    p, (s, form) = _points(points), _scalars(scalars)
    n = s.shape[0]
    if p.shape[0] != n:
        raise ValueError("one scalar per point")
    if n == 0:
        return np.zeros((0, 2, 4), np.uint64)
    dp, ds = DeviceVector.from_host(ctx, p), DeviceVector.from_host(ctx, s)
    try:
        jubjub_mul_dev(ctx, dp.ptr, ds.ptr, n, dp.ptr, form)
        return dp.to_host().reshape(n, 2, 4)
    finally:
        dp.free(), ds.free()


def jubjub_msm_dev(ctx: Context, d_points: int, d_scalars: int, n: int, d_out: int, batch: int = 1, scalar_stride: int | None = None,
                   scalar_form: int = _lib.SCALAR_MONTGOMERY, stream: int = 0):
    """``pm_jubjub_msm_dev``: ``out[b] = sum_i s[b][i] P_i`` for ``batch`` scalar vectors over the same n points, vector ``b`` at
    element ``b * scalar_stride`` (``None``: n); ``batch`` points (2 elements each) at ``d_out``.  The bucket method over signed
    windows; the points are not validated; asynchronous.  Up to about 2^15 points :func:`jubjub_mul_dev` (and a sum of its outputs)
    is as quick or up to 15 % quicker: both are bound by the latency of one 256-doubling chain.  The MSM wins from between 2^16 and
    2^18 points on, 5 x at 2^20."""
    stride = n if scalar_stride is None else scalar_stride
    ctx._check(ctx._lib.pm_jubjub_msm_dev(ctx._h, C.c_void_p(d_points), C.c_void_p(d_scalars), n, stride, batch, scalar_form,
                                          C.c_void_p(d_out), C.c_void_p(stream)))


def _scalar_rows(scalars):
    """-> ([B, n, 4] uint64, scalar_form, batched): ``[n]`` / ``[n, 4]`` is one vector, ``[B, n]`` / ``[B, n, 4]`` are B"""
    if isinstance(scalars, np.ndarray) and scalars.dtype == np.uint64:
        if scalars.ndim not in (2, 3) or scalars.shape[-1] != 4:
            raise ValueError("limb scalars are [n, 4] or [B, n, 4]")
        batched = scalars.ndim == 3
        rows = scalars.shape[0] if batched else 1
        return np.ascontiguousarray(scalars).reshape((rows,) + scalars.shape[-2:]), _lib.SCALAR_MONTGOMERY, batched
    obj = np.asarray(scalars, dtype=object)
    if obj.ndim not in (1, 2):
        raise ValueError("integer scalars are [n] or [B, n]")
    flat, form = _scalars(obj)
    return flat.reshape((1 if obj.ndim == 1 else obj.shape[0], obj.shape[-1], 4)), form, obj.ndim == 2


def jubjub_msm(ctx: Context, points, scalars) -> np.ndarray:
    """``sum_i s_i P_i`` on the GPU (``pm_jubjub_msm_dev``).  Scalars ``[n]`` (integers) or ``[n, 4]`` (limbs) -> ``[2, 4]`` limbs;
    ``[B, n]`` or ``[B, n, 4]`` -> ``[B, 2, 4]``, one sum per row over the same points.  The form is inferred as in
    :func:`jubjub_mul`.  Worth it from 2^16 to 2^18 points on; below that :func:`jubjub_mul` and a host sum is as quick."""
    p = _points(points)
    s, form, batched = _scalar_rows(scalars)
    B, n = s.shape[0], s.shape[1]
    if p.shape[0] != n:
        raise ValueError("one scalar per point in every row")
    if B == 0:
        return np.zeros((0, 2, 4), np.uint64)
    out = DeviceVector(ctx, 2 * B)
    dp = DeviceVector.from_host(ctx, p) if n else None
    ds = DeviceVector.from_host(ctx, s.reshape(-1, 4)) if n else None
    try:
        jubjub_msm_dev(ctx, dp.ptr if n else 0, ds.ptr if n else 0, n, out.ptr, B, n, form)
        got = out.to_host().reshape(B, 2, 4)
        return got if batched else got[0]
    finally:
        for x in (dp, ds, out):
            if x is not None:
                x.free()


def jubjub_msm_host(points, scalars) -> np.ndarray:
    """``pm_jubjub_msm_host``: the plain sum of double-and-add products on the CPU, no context -> [2, 4] limbs"""
    p, (s, form) = _points(points), _scalars(scalars)
    if p.shape[0] != s.shape[0]:
        raise ValueError("one scalar per point")
    out = np.zeros((2, 4), np.uint64)
    if _lib.load().pm_jubjub_msm_host(_p(p), _p(s), p.shape[0], form, _p(out)) != _lib.PM_OK:
        raise ValueError("pm_jubjub_msm_host refused its arguments")
    return out


# ------------------------------------------------------------------------------------------ the wire format (section 7.2p)
#: why ``jubjub_decompress`` refused a point: the keys are the non-zero statuses, the lowest that applies
JUBJUB_CODEC_REASONS = _lib.JUBJUB_CODEC_REASONS


def _encodings(data, width: int = 32) -> np.ndarray:
    """``bytes``, a sequence of ``bytes`` or a ``uint8`` array -> ``[n, width]`` ``uint8``"""
    if isinstance(data, (bytes, bytearray)):
        a = np.frombuffer(bytes(data), dtype=np.uint8)
    elif isinstance(data, np.ndarray):
        if data.dtype != np.uint8:
            raise ValueError("encodings are uint8")
        a = data
    else:
        a = np.frombuffer(b"".join(bytes(d) for d in data), dtype=np.uint8)
    if a.size % width:
        raise ValueError(f"encodings are {width} bytes each")
    return np.ascontiguousarray(a).reshape(-1, width)


def _field_elements(x) -> np.ndarray:
    """limbs (uint64, [..., 4]) or integers -> [n, 4] Montgomery limbs"""
    if isinstance(x, np.ndarray) and x.dtype == np.uint64:
        return np.ascontiguousarray(x).reshape(-1, 4)
    return fr_vec_to_limbs([int(v) for v in np.asarray(x, dtype=object).reshape(-1)]).reshape(-1, 4)


def _words32(v: DeviceVector, n: int) -> np.ndarray:
    """the first n ``uint32`` of a vector of 32-byte elements"""
    return v.to_host().view(np.uint32).reshape(-1)[:n].copy()


def fr_sqrt_host(value):
    """``pm_fr_sqrt_host``: one element on the CPU by the plain Tonelli-Shanks loop, no context -> ``(root [4], is_square)``"""
    a = _field_elements(value)
    if a.shape[0] != 1:
        raise ValueError("one element")
    out, flag = np.zeros(4, np.uint64), C.c_uint32()
    if _lib.load().pm_fr_sqrt_host(_p(a), _p(out), C.byref(flag)) != _lib.PM_OK:
        raise ValueError("pm_fr_sqrt_host refused its arguments")
    return out, int(flag.value)


def jubjub_compress_host(point) -> bytes:
    """``pm_jubjub_compress``: one point on the CPU, no context -> 32 bytes.  A point off the curve or a coordinate that is not
    below r raises ``ValueError``."""
    p = _points(point)
    if p.shape[0] != 1:
        raise ValueError("one point")
    out = np.zeros(32, np.uint8)
    if _lib.load().pm_jubjub_compress(_p(p), out.ctypes.data_as(C.POINTER(C.c_uint8))) != _lib.PM_OK:
        raise ValueError("pm_jubjub_compress refused its arguments")
    return out.tobytes()


def jubjub_decompress_host(data, check_subgroup: bool = False):
    """``pm_jubjub_decompress``: 32 bytes on the CPU, no context -> ``(point [2, 4], status)``; a refused point is ``(0, 0)``"""
    b = _encodings(data)
    if b.shape[0] != 1:
        raise ValueError("one encoding")
    out, status = np.zeros((2, 4), np.uint64), C.c_uint32()
    rc = _lib.load().pm_jubjub_decompress(b.ctypes.data_as(C.POINTER(C.c_uint8)), _lib.JUBJUB_CHECK_SUBGROUP if check_subgroup else 0,
                                          _p(out), C.byref(status))
    if rc != _lib.PM_OK:
        raise ValueError("pm_jubjub_decompress refused its arguments")
    return out, int(status.value)


def fr_sqrt_dev(ctx: Context, d_in: int, n: int, d_out: int, d_is_square: int = 0, want_count: bool = False, stream: int = 0):
    """``pm_fr_sqrt_dev``: n roots at ``d_out`` (may be ``d_in``) and n ``uint32`` flags at ``d_is_square`` (0 = not wanted).
    Returns the count of squares and waits for the stream, or None, asynchronous, when ``want_count`` is false."""
    cnt = C.c_size_t()
    ctx._check(ctx._lib.pm_fr_sqrt_dev(ctx._h, C.c_void_p(d_in), n, C.c_void_p(d_out), C.c_void_p(d_is_square) if d_is_square else None,
                                       C.byref(cnt) if want_count else None, C.c_void_p(stream)))
    return int(cnt.value) if want_count else None


def fr_sqrt(ctx: Context, values):
    """-> ``(roots [n, 4], is_square [n] uint32)``: the root whose canonical integer is even (0 for 0) and flag 1 for a square,
    root 0 and flag 0 for a non-square or limbs that are not below r.  ``values``: Montgomery limbs or integers."""
    a = _field_elements(values)
    n = a.shape[0]
    if n == 0:
        return np.zeros((0, 4), np.uint64), np.zeros(0, np.uint32)
    d, f = DeviceVector.from_host(ctx, a), DeviceVector(ctx, (n + 7) // 8)
    try:
        fr_sqrt_dev(ctx, d.ptr, n, d.ptr, f.ptr)
        return d.to_host(), _words32(f, n)
    finally:
        d.free(), f.free()


def jubjub_compress_dev(ctx: Context, d_points: int, n: int, d_bytes: int, stream: int = 0):
    """``pm_jubjub_compress_dev``: n points (2 elements each) -> n x 32 bytes at ``d_bytes``; asynchronous.  Not validated."""
    ctx._check(ctx._lib.pm_jubjub_compress_dev(ctx._h, C.c_void_p(d_points), n, C.c_void_p(d_bytes), C.c_void_p(stream)))


def jubjub_compress(ctx: Context, points) -> np.ndarray:
    """-> ``uint8 [n, 32]``: the canonical y, little-endian, with the parity of the canonical x in bit 255.  The points are not
    validated."""
    p = _points(points)
    n = p.shape[0]
    if n == 0:
        return np.zeros((0, 32), np.uint8)
    dp, out = DeviceVector.from_host(ctx, p), DeviceVector(ctx, n)
    try:
        jubjub_compress_dev(ctx, dp.ptr, n, out.ptr)
        return out.to_host().view(np.uint8).reshape(n, 32)
    finally:
        dp.free(), out.free()


def jubjub_decompress_dev(ctx: Context, d_bytes: int, n: int, d_out: int, d_status: int = 0, check_subgroup: bool = False,
                          in_stride: int = 0, out_stride: int = 0, want_n_ok: bool = True, stream: int = 0):
    """``pm_jubjub_decompress_dev``: record i (32 bytes) at ``d_bytes + i * in_stride`` -> point i at ``d_out + i * out_stride``
    (0 = packed: 32 and 64 bytes), n ``uint32`` at ``d_status`` (0 = not wanted).  A refused point is ``(0, 0)`` and no error.
    Returns the count of status 0 and waits for the stream, or None when ``want_n_ok`` is false.  The subgroup check is off by
    default: it costs a whole ladder a point."""
    ok = C.c_size_t()
    ctx._check(ctx._lib.pm_jubjub_decompress_dev(ctx._h, C.c_void_p(d_bytes), in_stride, n,
                                                 _lib.JUBJUB_CHECK_SUBGROUP if check_subgroup else 0, C.c_void_p(d_out), out_stride,
                                                 C.c_void_p(d_status) if d_status else None, C.byref(ok) if want_n_ok else None,
                                                 C.c_void_p(stream)))
    return int(ok.value) if want_n_ok else None


def jubjub_decompress(ctx: Context, data, check_subgroup: bool = False, strict: bool = False):
    """``data``: n x 32 bytes -> ``(points [n, 2, 4], status [n] uint32)``: status 0 = decoded, else a key of
    ``JUBJUB_CODEC_REASONS``, the lowest that applies; a refused point is ``(0, 0)``, which every later call refuses.  With
    ``strict`` a refusal raises ``ValueError`` naming the lowest bad index and its reason."""
    b = _encodings(data)
    n = b.shape[0]
    if n == 0:
        return np.zeros((0, 2, 4), np.uint64), np.zeros(0, np.uint32)
    db, out, ds = DeviceVector.from_host(ctx, b.view(np.uint64)), DeviceVector(ctx, 2 * n), DeviceVector(ctx, (n + 7) // 8)
    try:
        ok = jubjub_decompress_dev(ctx, db.ptr, n, out.ptr, ds.ptr, check_subgroup)
        status = _words32(ds, n)
        if strict and ok != n:
            bad = int(np.flatnonzero(status)[0])
            raise ValueError(f"encoding {bad} is refused: {JUBJUB_CODEC_REASONS[int(status[bad])]}")
        return out.to_host().reshape(n, 2, 4), status
    finally:
        db.free(), out.free(), ds.free()


def jubjub_check(ctx: Context, points):
    """``pm_jubjub_check_dev``: None when every point is a canonical point of the curve, else the lowest bad index.  ``points``:
    limbs, integer pairs or a :class:`DeviceVector` of 2 n elements."""
    if isinstance(points, DeviceVector):
        d, n, own = points, points.n // 2, False
    else:
        p = _points(points)
        d, n, own = DeviceVector.from_host(ctx, p), p.shape[0], True
    try:
        bad = C.c_size_t()
        ctx._check(ctx._lib.pm_jubjub_check_dev(ctx._h, C.c_void_p(d.ptr), n, C.byref(bad), None))
        return None if bad.value == n else int(bad.value)
    finally:
        if own:
            d.free()
