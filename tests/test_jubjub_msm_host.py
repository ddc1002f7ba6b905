"""The JubJub MSM without a GPU: the new exports are declared, bound and documented; pm_jubjub_msm_host is
the model's sum on the edge points and edge scalars; the signed-window recoding the kernels run (compiled for the host) is an
identity on every 256-bit integer with every digit inside its bucket range; and the plan covers 256 bits and the carry, grows with
n and refuses what it documents."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gadget_model as M  # noqa: E402
import jubjub_model as J  # noqa: E402
import jubjub_msm_model as MM  # noqa: E402
import schnorr_model as S  # noqa: E402
from conftest import ROOT  # noqa: E402

R = J.R
NEW = ("pm_jubjub_msm_dev", "pm_jubjub_msm_host", "pm_schnorr_verify_batch_dev", "pm_test_jubjub_msm_plan", "pm_test_jubjub_msm_digits")
ALL_ONES = (1 << 256) - 1


@pytest.fixture(scope="module")
def lib():
    import plonk_prototype_amd as pa
    return pa.load()


def test_exports_are_declared_bound_and_documented(lib):
    import plonk_prototype_amd as pa
    from plonk_prototype_amd import _lib
    header = open(os.path.join(ROOT, "include", "plonk_mi355x.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    declared = set(re.findall(r"\b(pm_[a-z0-9_]+)\s*\(", header))
    bound = set(re.findall(r"pub fn (pm_[a-z0-9_]+)", doc))
    for name in NEW:
        assert name in declared and name in _lib.SIGNATURES and name in bound and hasattr(lib, name), name
    for name in ("jubjub_msm", "jubjub_msm_dev", "jubjub_msm_host"):
        assert callable(getattr(pa, name)), name
    assert callable(pa.Schnorr.verify_batch) and callable(pa.Schnorr.verify_batch_dev)
    assert (_lib.JUBJUB_MSM_MIN_WINDOW_BITS, _lib.JUBJUB_MSM_MAX_WINDOW_BITS) == (MM.WINDOW_BITS[0], MM.WINDOW_BITS[-1])
    # the Schnorr block documents the cofactored check and keeps the two sentences of the single check
    block = header[header.index("Native Schnorr signatures on JubJub"):header.index("pm_plonk_proof_to_bytes")]
    for phrase in ("COFACTORED", "2^-128", "NOT hardened against side channels", "prior knowledge", "predictable weights"):
        assert phrase in block, phrase


# ---------------------------------------------------------------------------------- the host sum
def test_host_msm_is_the_model():
    import plonk_prototype_amd as pa
    pts, sc = J.edge_points(), J.edge_scalars()
    # every edge point meets every edge scalar once: len(pts) rotations of the scalar list
    for rot in range(len(pts)):
        n = len(sc)
        p = [pts[(i + rot) % len(pts)] for i in range(n)]
        want = MM.msm(p, sc)
        assert np.array_equal(pa.jubjub_msm_host(p, sc), J.to_limbs([want])[0]), ("canonical", rot)
        if rot < 2:
            assert np.array_equal(pa.jubjub_msm_host(J.to_limbs(p), M.to_limbs(sc)), J.to_limbs([want])[0]), ("montgomery", rot)
    # a single product is pm_jubjub_mul_host's; no point at all is the identity
    assert np.array_equal(pa.jubjub_msm_host([pts[1]], [sc[9]]), pa.jubjub_mul_host(pts[1], sc[9]))
    assert np.array_equal(pa.jubjub_msm_host(np.zeros((0, 2, 4), np.uint64), np.zeros((0, 4), np.uint64)), J.to_limbs([J.IDENTITY])[0])


def test_host_msm_refusals(lib):
    from plonk_prototype_amd._lib import u64p
    p = lambda x: x.ctypes.data_as(u64p)   # noqa: E731
    good_p, good_s = J.to_limbs([J.GENERATOR, J.GENERATOR]), M.to_limbs([3, 5])
    out = np.zeros((2, 4), np.uint64)
    assert lib.pm_jubjub_msm_host(p(good_p), p(good_s), 2, 0, p(out)) == 0
    assert lib.pm_jubjub_msm_host(None, None, 0, 0, p(out)) == 0 and np.array_equal(out, J.to_limbs([J.IDENTITY])[0])
    assert lib.pm_jubjub_msm_host(p(good_p), p(good_s), 2, 2, p(out)) == -1            # an unknown form
    assert lib.pm_jubjub_msm_host(None, p(good_s), 2, 0, p(out)) == -1
    assert lib.pm_jubjub_msm_host(p(good_p), None, 2, 0, p(out)) == -1
    assert lib.pm_jubjub_msm_host(p(good_p), p(good_s), 2, 0, None) == -1
    off = good_p.copy()
    off[1] = S.point_words((J.GENERATOR[0], (J.GENERATOR[1] + 1) % R))                 # the second point is off the curve
    assert lib.pm_jubjub_msm_host(p(off), p(good_s), 2, 0, p(out)) == -1
    big = good_p.copy()
    big[1, 0] = S.canon_words(int.from_bytes(good_p[1, 0].tobytes(), "little") + R)    # a coordinate >= r
    assert lib.pm_jubjub_msm_host(p(big), p(good_s), 2, 0, p(out)) == -1
    bad_s = np.stack([S.canon_words(3), S.canon_words(R)])                             # a scalar >= r, either form
    for form in (0, 1):
        assert lib.pm_jubjub_msm_host(p(good_p), p(bad_s), 2, form, p(out)) == -1


# ---------------------------------------------------------------------------------- the recoding
def _digits(lib, k, c):
    from plonk_prototype_amd._lib import u64p
    words = S.canon_words(k)
    d = (C.c_int32 * 66)()
    nd = C.c_uint32()
    assert lib.pm_test_jubjub_msm_digits(words.ctypes.data_as(u64p), c, d, C.byref(nd)) == 0
    return list(d[:nd.value])


def _plan(lib, n, batch, c, rc=0):
    from plonk_prototype_amd._lib import u64p
    out = np.zeros(8, np.uint64)
    assert lib.pm_test_jubjub_msm_plan(n, batch, c, 0, out.ctypes.data_as(u64p)) == rc, (n, batch, c)
    return [int(v) for v in out]


def test_digits_are_an_identity_on_every_word(lib):
    scalars = J.edge_scalars() + [ALL_ONES, R, R + 1, 1 << 255, (1 << 255) - 1, ALL_ONES - 1, int("8" * 64, 16), int("7" * 64, 16) + (1 << 255)]
    for c in MM.WINDOW_BITS:
        windows = _plan(lib, 1, 1, c)[1]
        for k in scalars:
            d = _digits(lib, k, c)
            assert len(d) == windows, (c, hex(k))                                      # no carry out of the top window
            assert sum(v << (c * w) for w, v in enumerate(d)) == k, (c, hex(k))
            assert all(abs(v) <= 1 << (c - 1) for v in d), (c, hex(k))                 # bucket |d| - 1 < 2^(c-1)
            assert d == MM.digits(k, c), (c, hex(k))
    from plonk_prototype_amd._lib import u64p
    w = S.canon_words(5)
    d, nd = (C.c_int32 * 66)(), C.c_uint32()
    for c in (0, 3, 17, 64):
        assert lib.pm_test_jubjub_msm_digits(w.ctypes.data_as(u64p), c, d, C.byref(nd)) == -1
    assert lib.pm_test_jubjub_msm_digits(None, 8, d, C.byref(nd)) == -1


# ---------------------------------------------------------------------------------- the plan
def test_plan_covers_the_carry_grows_with_n_and_refuses(lib):
    sizes = (1, 31, 1 << 10, 1 << 16, 1 << 20, 1 << 24)
    for batch in (1, 4):
        for c in (0,) + MM.WINDOW_BITS:
            last = 0
            for n in sizes:
                if c == 0:
                    got = _plan(lib, n, batch, 0)
                else:
                    rows = batch * ((257 + c - 1) // c)
                    fits = n * rows <= 0xFFFFFFFF and n * rows // 32 + rows * (1 << (c - 1)) <= 0xFFFFFFFF
                    got = _plan(lib, n, batch, c, 0 if fits else -6)
                    if not fits:
                        assert got == [0] * 8
                        continue
                    assert got[0] == c
                cc, windows, buckets, pairs, ws, rows_got, items, seg = got
                assert cc in MM.WINDOW_BITS and windows * cc >= 257 and (windows - 1) * cc < 257   # 256 bits and the carry, no more
                assert buckets == 1 << (cc - 1) and rows_got == windows * batch and pairs == n * windows * batch
                assert items == pairs // 32 + rows_got * buckets and seg * 256 >= buckets and buckets % seg == 0
                # every array of the workspace fits: counts, cursors, two offset arrays, the pairs, a point per segment and row
                assert ws >= 16 * rows_got * buckets + 4 * pairs + 144 * (items + rows_got)
                if c:
                    assert ws > last, (n, batch, c)                                   # monotone in n at a fixed width
                    last = ws
    # the rule's width never shrinks as n grows
    widths = [_plan(lib, n, 1, 0)[0] for n in sizes]
    assert widths == sorted(widths) and widths[0] == MM.WINDOW_BITS[0]
    assert _plan(lib, 0, 1, 0)[3] == 0                                                 # n = 0 plans (and launches) nothing
    # refusals
    assert _plan(lib, 1 << 10, 0, 0, -1) == [0] * 8                                    # batch = 0
    for c in (-1, 1, 3, 17, 20):
        _plan(lib, 1 << 10, 1, c, -1)
    _plan(lib, 1 << 31, 1, 0, -6)                                                      # n > 2^31 - 1
    _plan(lib, (1 << 31) - 1, 1, 16, -6)                                               # pairs > 2^32 - 1
    _plan(lib, 1 << 10, 1 << 14, 16, -6)                                               # buckets > 2^28
    from plonk_prototype_amd._lib import u64p
    assert lib.pm_test_jubjub_msm_plan(1, 1, 0, 0, None) == -1
