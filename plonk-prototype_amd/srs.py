"""Commit-key bytes: the raw (uncompressed, unchecked) form and the compressed, checked form, the on-disk form either side of the MSM
(SURVEY.md section 8f row N4).

Layout restated from dusk-plonk 0.8.2 ``CommitKey::to_raw_var_bytes`` / ``from_slice_unchecked`` and
dusk-bls12_381 0.8 ``G1Affine::to_raw_bytes`` (ref:Cargo.toml:19-20; neither crate is in the
reference tree -- UNPINNED, verified by round trip only):

    u64 little-endian   number of points n
    n x 97 bytes        x: 6 x u64 LE Montgomery limbs | y: 6 x u64 LE Montgomery limbs | infinity: 1 byte

i.e. the in-memory ``G1Affine`` without padding -- which is also this backend's affine layout (the
identity is (0, 0) here and carries infinity = 1 in the file).

The compressed form (``commit_key_to_bytes`` / ``commit_key_from_bytes``) is ``CommitKey::to_var_bytes`` / ``from_slice``:
n x 48 bytes, the zcash encoding of ``G1Affine::to_compressed``, with no length prefix.
"""
from __future__ import annotations

import numpy as np

G1_RAW = 97
G1_COMPRESSED = 48


def commit_key_to_raw_bytes(powers_of_g) -> bytes:
    p = np.ascontiguousarray(powers_of_g, dtype=np.uint64).reshape(-1, 12)
    n = p.shape[0]
    out = np.zeros((n, G1_RAW), np.uint8)
    out[:, :96] = p.view(np.uint8).reshape(n, 96)
    out[:, 96] = (~p.any(axis=1)).astype(np.uint8)
    return n.to_bytes(8, "little") + out.tobytes()


def commit_key_from_raw_bytes(data: bytes) -> np.ndarray:
    """-> powers_of_g [n, 12] Montgomery limbs.  Unchecked like upstream's ``from_slice_unchecked``
    (no on-curve / subgroup test); raises ValueError only for a malformed length."""
    if len(data) < 8:
        raise ValueError("truncated commit key")
    n = int.from_bytes(data[:8], "little")
    if len(data) != 8 + n * G1_RAW:
        raise ValueError("commit key length does not match its point count")
    raw = np.frombuffer(data, dtype=np.uint8, offset=8).reshape(n, G1_RAW)
    pts = raw[:, :96].copy().view(np.uint64).reshape(n, 12)
    pts[raw[:, 96] != 0] = 0
    return pts


def _lib_reason(reason) -> str:
    from ._lib import G1_BAD_REASONS
    return G1_BAD_REASONS.get(reason, "rejected")


def commit_key_to_bytes(points, ctx=None) -> bytes:
    """powers_of_g [n, 12] -> n x 48 bytes of compressed G1, no length prefix: dusk-plonk 0.8.2's
    ``CommitKey::to_var_bytes``.  The layout is restated from the published crate (ref:Cargo.toml:19-20), which is
    not in the reference tree: UNPINNED like the raw form -- only the 48-byte point encoding itself is pinned (the
    generator's bytes in tests/golden/constants.json).  With a context the points are encoded on the GPU
    (``pm_g1_compress_dev``); without one, point by point on the host (``pm_g1_compress``: a verifier key, a small SRS)."""
    from . import host
    p = np.ascontiguousarray(points, dtype=np.uint64).reshape(-1, 12)
    n = p.shape[0]
    if n == 0:
        return b""
    if ctx is None:
        return b"".join(host.g1_compress(q) for q in p)
    d_xy, d_out = host.DeviceVector.from_host(ctx, p.reshape(-1, 4)), host.DeviceVector(ctx, (3 * n + 1) // 2)
    try:
        ctx.g1_compress_dev(d_xy.ptr, n, d_out.ptr)
        return d_out.to_host().tobytes()[:n * G1_COMPRESSED]
    finally:
        d_xy.free()
        d_out.free()


def commit_key_from_bytes(data: bytes, ctx=None, check_subgroup: bool = True) -> np.ndarray:
    """n x 48 bytes -> powers_of_g [n, 12] Montgomery limbs: dusk-plonk 0.8.2's ``CommitKey::from_slice`` (UNPINNED,
    see ``commit_key_to_bytes``).  Every point is decoded and checked: encoding, on the curve, and with
    ``check_subgroup`` of order r; a bad point raises ``host.Error`` with PM_ERR_POINT, ``bad_index`` and ``bad_reason``.
    ValueError for a length that is not a multiple of 48.  With a context the work runs on the GPU
    (``pm_g1_decompress_dev``); without one, point by point on the host (``pm_g1_decompress``, ~0.4 ms per checked
    point).  ``host.CommitKey.from_bytes`` is the form that keeps the points on the device."""
    from . import host
    if len(data) % G1_COMPRESSED:
        raise ValueError("commit key length is not a multiple of 48")
    n = len(data) // G1_COMPRESSED
    if n == 0:
        return np.zeros((0, 12), np.uint64)
    if ctx is None:
        out = np.zeros((n, 12), np.uint64)
        for i in range(n):
            try:
                out[i] = host.g1_decompress(data[G1_COMPRESSED * i:G1_COMPRESSED * (i + 1)], check_subgroup)
            except host.Error as e:
                raise host.Error(e.code, f"commit key: point {i} {_lib_reason(e.bad_reason)}", i, e.bad_reason) from None
        return out
    raw = np.zeros(((3 * n + 1) // 2) * 32, np.uint8)
    raw[:len(data)] = np.frombuffer(data, np.uint8)
    d_in, d_xy = host.DeviceVector.from_host(ctx, raw.view(np.uint64).reshape(-1, 4)), host.DeviceVector(ctx, 3 * n)
    try:
        ctx.g1_decompress_dev(d_in.ptr, n, d_xy.ptr, check_subgroup)
        return d_xy.to_host().reshape(n, 12)
    finally:
        d_in.free()
        d_xy.free()
