"""The comparison behind tests/guard_arena.py on plain numpy arrays, no device: it has to name the region, the side, the first
damaged byte and the number of changed bytes -- and it has to stay silent on an arena nobody touched."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guard_arena as G  # noqa: E402


def _arena(sizes, inputs, align=32):
    """the image and the region table `GuardArena` would build for regions of these sizes; `inputs`: which of them carry data"""
    image = np.full(G.arena_bytes(sizes, align), G.FILL, np.uint8)
    regions, end = [], 0
    rng = np.random.default_rng(5)
    for i, (nbytes, is_input) in enumerate(zip(sizes, inputs)):
        offset = G._align_up(end + G.BAND, align)
        if is_input:
            image[offset:offset + nbytes] = rng.integers(0, 256, nbytes, dtype=np.uint8)
        regions.append(G.Region(f"r{i}", offset, nbytes, is_input))
        end = offset + nbytes
    assert end + G.BAND == image.shape[0]
    return image, regions


def test_band_covers_the_units_of_the_kernels():
    """BAND is derived, not guessed: twice SC_TILE of csrc/poly.hip, read from the source"""
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "plonk-prototype_amd", "csrc", "poly.hip")).read()
    sc_k = int(re.search(r"constexpr int SC_K = (\d+);", src).group(1))
    assert re.search(r"constexpr int SC_TILE = 256 \* SC_K;", src)
    sc_tile = 256 * sc_k
    assert G.BAND_ELEMENTS >= 2 * sc_tile and G.BAND == G.BAND_ELEMENTS * 32
    assert G.BAND_ELEMENTS >= 1 << 12                 # the largest transform of the buffer-contract tests, whole
    assert G.BAND >= 256 * 160                        # a workgroup of the largest per-thread record, a Hades state


def test_layout_gives_every_region_a_band_on_both_sides():
    sizes = [32, 48 * 63, 96 * 65, 4, 0, 32 * 2047]
    image, regions = _arena(sizes, [True] * len(sizes))
    assert regions[0].offset >= G.BAND
    for a, b in zip(regions, regions[1:]):
        assert b.offset - (a.offset + a.nbytes) >= G.BAND and b.offset % 32 == 0
    assert image.shape[0] - (regions[-1].offset + regions[-1].nbytes) == G.BAND
    # 48-byte records end off a 32-byte boundary: the band begins at the very next byte
    assert (regions[1].offset + regions[1].nbytes) % 32 == 16


def test_untouched_arena_passes():
    image, regions = _arena([320, 64, 4096], [True, False, True])
    assert G.find_damage(image, image.copy(), regions) == []
    assert G.find_damage(image, image.copy(), regions, written={"r1"}) == []


def test_written_output_passes_and_is_not_an_error():
    image, regions = _arena([320, 64], [True, False])
    after = image.copy()
    after[regions[1].offset:regions[1].offset + 64] = 7
    assert G.find_damage(image, after, regions, written={"r1"}) == []
    # ... but the same bytes are damage when the call was refused and may write nothing
    assert G.find_damage(image, after, regions) == [G.Damage("r1", "inside", 0, 64)]


@pytest.mark.parametrize("which", [0, 1, 2])
def test_single_byte_in_a_front_band(which):
    image, regions = _arena([320, 48 * 5, 4096], [True, False, True])
    r = regions[which]
    for back in (1, 17, G.BAND // 2 - 1 if which else G.BAND):
        after = image.copy()
        after[r.offset - back] ^= 0xFF
        assert G.find_damage(image, after, regions, written={"r1"}) == [G.Damage(r.name, "front", -back, 1)]


@pytest.mark.parametrize("which", [0, 1, 2])
def test_single_byte_in_a_back_band(which):
    image, regions = _arena([320, 48 * 5, 4096], [True, False, True])
    r = regions[which]
    for past in (0, 31, G.BAND // 2 - 1 if which < 2 else G.BAND - 1):
        after = image.copy()
        after[r.offset + r.nbytes + past] ^= 0x01
        assert G.find_damage(image, after, regions, written={"r1"}) == [G.Damage(r.name, "back", r.nbytes + past, 1)]


def test_single_byte_in_a_read_only_input():
    image, regions = _arena([320, 64, 4096], [True, False, True])
    after = image.copy()
    after[regions[2].offset + 1234] ^= 0x80
    assert G.find_damage(image, after, regions, written={"r1"}) == [G.Damage("r2", "inside", 1234, 1)]
    # an input the call may write (an in-place form) is not damage
    assert G.find_damage(image, after, regions, written={"r1", "r2"}) == []


def test_ragged_output_slot_n_minus_1_written():
    """an output of exactly n - 1 elements: the kernel that also writes slot n - 1 is reported behind it, at offset 32 (n - 1)"""
    n = 2049
    image, regions = _arena([32 * n, 32 * (n - 1)], [True, False])
    out = regions[1]
    after = image.copy()
    after[out.offset:out.offset + out.nbytes] = 3                     # the n - 1 results
    assert G.find_damage(image, after, regions, written={"r1"}) == []
    after[out.offset + 32 * (n - 1):out.offset + 32 * n] = 0           # ... and one element too many (a zero, say)
    assert G.find_damage(image, after, regions, written={"r1"}) == [G.Damage("r1", "back", 32 * (n - 1), 32)]


def test_damage_on_both_sides_of_a_gap_and_the_count():
    image, regions = _arena([64, 64], [False, False])
    after = image.copy()
    gap_lo = regions[0].offset + 64
    after[gap_lo + 8:gap_lo + 40] = 0                                  # behind r0: 32 bytes
    after[regions[1].offset - 96:regions[1].offset - 90] = 0           # in front of r1: 6 bytes
    got = G.find_damage(image, after, regions, written={"r0", "r1"})
    assert got == [G.Damage("r0", "back", 64 + 8, 32), G.Damage("r1", "front", -96, 6)]
    text = str(got[0]) + " | " + str(got[1])
    assert "behind 'r0'" in text and "+72" in text and "32 byte(s)" in text
    assert "in front of 'r1'" in text and "-96" in text and "6 byte(s)" in text


def test_a_write_of_the_fill_byte_cannot_be_seen_and_is_no_result():
    """the limit of the method, stated: 0xA5 over 0xA5 is invisible -- which is why the fill is no value a kernel produces"""
    r_mod = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
    p_mod = int("1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaab", 16)
    assert int.from_bytes(bytes([G.FILL]) * 32, "little") >= r_mod
    assert int.from_bytes(bytes([G.FILL]) * 48, "little") >= p_mod
    assert int.from_bytes(bytes([G.FILL]) * 4, "little") > 1 << 31    # no status, reason or 32-bit index
    assert G.untouched(np.full(96, G.FILL, np.uint8)) and not G.untouched(np.zeros(96, np.uint8))
