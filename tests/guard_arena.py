"""A guard arena for the device entry points: every buffer of a call is carved out of ONE device allocation that is filled with
the byte 0xA5, so that whatever a kernel writes outside the bytes the header gives it -- a padded lane, one element too many, the
unused slot behind a ragged output -- lands in memory the test owns and is found by comparing bytes, not by a GPU fault.

Why 0xA5: a word of 0xA5 bytes is 0xa5a5...a5.  Read as an Fr element (r < 2^255) or an Fp element (p < 2^382) it is above the
modulus, so it is no canonical element; read as a status, a reason or an index it is 2.8e9 or 1.2e19, no value the library
produces.  A correct kernel therefore never writes it as a result, and an output region that still holds it was not written.

BAND, the guard on either side of every region: 4096 elements of 32 bytes = 131072 bytes.  It has to cover the largest unit a
kernel under test works in, so that an overrun by one whole unit still lands inside the arena:
  * csrc/poly.hip        SC_TILE = 256 threads x SC_K (8) = 2048 elements of 32 bytes: the scans, Ruffini, the batch inverse;
  * csrc/ntt*.hip        the sizes under test are 2^4 .. 2^12: one vector is at most 4096 elements, the largest tile (a
                         radix-2^10 pass) 1024 elements;
  * a workgroup of records: 256 threads x 160 bytes (a Hades state, the largest record a thread owns) = 40960 bytes; the 96-byte
    G1 points give 24576, the 48-byte compressed points 12288.
4096 x 32 is twice SC_TILE and covers all three.  Two neighbouring regions share the band between them (it is at least BAND
bytes wide); `find_damage` gives the half next to a region to that region.

The comparison (`find_damage`) is a pure function over two byte arrays and a region table -- tests/test_guard_arena_host.py runs
it without a device."""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple

import numpy as np

FILL = 0xA5
BAND_ELEMENTS = 4096                  # 2 x SC_TILE (csrc/poly.hip); = the largest NTT vector under test
BAND = BAND_ELEMENTS * 32             # bytes in front of the first region, between two regions and behind the last one


class Region(NamedTuple):
    name: str
    offset: int          # bytes from the start of the arena
    nbytes: int
    is_input: bool       # carved with data: equals its upload unless the call may write it


class Damage(NamedTuple):
    region: str
    where: str           # "front": the band in front of the region; "back": the band behind it; "inside": a region not to be written
    offset: int          # first damaged byte relative to the region's first byte (negative in front, >= nbytes behind)
    count: int           # bytes that changed in that band half / region

    def __str__(self):
        place = {"front": "in front of", "back": "behind", "inside": "inside the read-only region"}[self.where]
        return f"{self.count} byte(s) changed {place} '{self.region}', the first at offset {self.offset:+d} from its start"


def _align_up(x: int, align: int) -> int:
    return (x + align - 1) // align * align


def arena_bytes(sizes, align: int = 32) -> int:
    """The bytes an arena needs for regions of these sizes carved in this order: BAND, then each region followed by BAND (and
    the padding that aligns the next region)."""
    end = BAND
    for nbytes in sizes:
        end = _align_up(end, align) + nbytes + BAND
    return end


def find_damage(before: np.ndarray, after: np.ndarray, regions, written=()) -> list:
    """`before`: the arena as uploaded (0xA5 and the inputs), `after`: as downloaded, both uint8 of one length; `regions`: the
    table in ascending order of offset; `written`: names of the regions the call may write.  Returns every Damage: changed bytes
    in a band (the gap between two regions is split in the middle: the first half is behind the region before it, the second in
    front of the region after it) and changed bytes inside a region that is not in `written`.  Empty = the contract held."""
    assert before.dtype == np.uint8 and after.dtype == np.uint8 and before.shape == after.shape and before.ndim == 1
    written, out, total = set(written), [], before.shape[0]
    unknown = written - {r.name for r in regions}
    assert not unknown, f"no such region: {sorted(unknown)}"

    def changed(lo, hi):
        idx = np.flatnonzero(before[lo:hi] != after[lo:hi])
        return (lo + int(idx[0]), int(idx.size)) if idx.size else None

    prev_end, prev = 0, None
    for r in list(regions) + [None]:
        lo, hi = prev_end, (r.offset if r is not None else total)
        assert hi >= lo, "regions overlap or are out of order"
        # the gap [lo, hi): behind `prev`, in front of `r`
        mid = lo if prev is None else hi if r is None else (lo + hi) // 2
        if prev is not None and (c := changed(lo, mid)):
            out.append(Damage(prev.name, "back", c[0] - prev.offset, c[1]))
        if r is not None and (c := changed(mid, hi)):
            out.append(Damage(r.name, "front", c[0] - r.offset, c[1]))
        if r is None:
            break
        if r.name not in written and (c := changed(r.offset, r.offset + r.nbytes)):   # an input, or an output of a refused call
            out.append(Damage(r.name, "inside", c[0] - r.offset, c[1]))
        prev_end, prev = r.offset + r.nbytes, r
    return out


class GuardArena:
    """One device allocation of `capacity` bytes (pm_dev_alloc), all 0xA5.  `carve` hands out regions front to back; `check`
    downloads the arena once.  `GuardArena.of(ctx, name=data_or_nbytes, ...)` sizes the allocation for exactly the regions
    given and carves them in that order."""

    def __init__(self, ctx, capacity: int):
        self.ctx, self.capacity = ctx, capacity
        self.image = np.full(capacity, FILL, np.uint8)         # what the device holds before the call
        self.regions: list[Region] = []
        self._end = 0                                           # the end of the last region
        h = C.c_void_p()
        ctx._check(ctx._lib.pm_dev_alloc(ctx._h, capacity, C.byref(h)))
        self._p = h
        ctx._check(ctx._lib.pm_dev_upload(ctx._h, self._p, self.image.ctypes.data_as(C.c_void_p), capacity))

    @classmethod
    def of(cls, ctx, align: int = 32, **specs) -> "GuardArena":
        """name = a numpy array (an input, uploaded) or a number of bytes (an output, left 0xA5)."""
        size = lambda v: int(v.nbytes) if isinstance(v, np.ndarray) else int(v)   # noqa: E731
        self = cls(ctx, arena_bytes([size(v) for v in specs.values()], align))
        for name, v in specs.items():
            self.carve(size(v), v if isinstance(v, np.ndarray) else None, align, name)
        return self

    @property
    def base(self) -> int:
        return self._p.value or 0

    def carve(self, nbytes: int, data=None, align: int = 32, name: str | None = None) -> int:
        """-> the device address of a region of exactly `nbytes` bytes with at least BAND bytes of 0xA5 on both sides."""
        offset = _align_up(self._end + BAND, align)
        if offset + nbytes + BAND > self.capacity:
            raise ValueError(f"the arena of {self.capacity} bytes cannot hold another region of {nbytes}")
        name = name if name is not None else f"region{len(self.regions)}"
        assert name not in {r.name for r in self.regions}, name
        if data is not None:
            raw = np.ascontiguousarray(data).reshape(-1).view(np.uint8)
            if raw.shape[0] != nbytes:
                raise ValueError(f"'{name}': {raw.shape[0]} bytes of data for a region of {nbytes}")
            self.image[offset:offset + nbytes] = raw
            if nbytes:
                chunk = np.ascontiguousarray(self.image[offset:offset + nbytes])
                self.ctx._check(self.ctx._lib.pm_dev_upload(self.ctx._h, C.c_void_p(self.base + offset),
                                                            chunk.ctypes.data_as(C.c_void_p), nbytes))
        self.regions.append(Region(name, offset, nbytes, data is not None))
        self._end = offset + nbytes
        return self.base + offset

    def addr(self, name: str) -> int:
        return self.base + self._region(name).offset

    def _region(self, name: str) -> Region:
        return next(r for r in self.regions if r.name == name)

    def check(self, written=()) -> dict:
        """Synchronise, download the arena once, assert that every band is 0xA5 and every input outside `written` equals its
        upload; -> {name: uint8 array} of the regions in `written` and of every output region."""
        self.ctx.sync()
        after = np.empty(self.capacity, np.uint8)
        self.ctx._check(self.ctx._lib.pm_dev_download(self.ctx._h, after.ctypes.data_as(C.c_void_p), self._p, self.capacity))
        writable = set(written) | {r.name for r in self.regions if not r.is_input}
        damage = find_damage(self.image, after, self.regions, writable)
        assert not damage, "the call wrote outside its buffers: " + "; ".join(str(d) for d in damage)
        return {r.name: after[r.offset:r.offset + r.nbytes].copy() for r in self.regions if r.name in writable}

    def check_unchanged(self):
        """A refused call changes no byte: bands, inputs and outputs all as before."""
        self.ctx.sync()
        after = np.empty(self.capacity, np.uint8)
        self.ctx._check(self.ctx._lib.pm_dev_download(self.ctx._h, after.ctypes.data_as(C.c_void_p), self._p, self.capacity))
        damage = find_damage(self.image, after, self.regions)
        assert not damage, "a refused call changed the arena: " + "; ".join(str(d) for d in damage)

    def free(self):
        if getattr(self, "_p", None) and self.ctx._h:
            self.ctx._lib.pm_dev_free(self.ctx._h, self._p)
        self._p = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()


def untouched(raw: np.ndarray) -> bool:
    """an output region that was never written"""
    return bool((raw == FILL).all())


def as_u64(raw: np.ndarray, *shape) -> np.ndarray:
    """the bytes of a region as uint64 limbs of the given shape"""
    return raw.view(np.uint64).reshape(*shape)
