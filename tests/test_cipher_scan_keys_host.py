"""Scanning a ledger under up to 64 viewing keys in one call, what needs no device: the new exports are
declared, bound and exported with the argument lists of the header; the plan of the scratch (csrc/cipher_scan_plan.h) through its
hook -- the stride, the bytes, the budget; the wrapper's refusals; and the premise of the full window table in integers: the
signed digits of a key, summed over the multiples 16^w R of a point, give vk R, also for the identity and for a point of even
order."""
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
MAX_KEYS = 64
TABLE_BYTES = 73728                                           # 64 windows x 8 entries x 144 bytes


def _u64p(a):
    from plonk_prototype_amd._lib import u64p
    return a.ctypes.data_as(u64p) if a is not None else None


def note_bytes(n_keys, L):   # noqa: N803
    return TABLE_BYTES + n_keys * (64 + 32 * L)


def tail_bytes(n_keys):
    """behind the slots: 64 bytes of digits a key, 16 for the count of hits"""
    return 64 * n_keys + 16


def plan(num_cus, n_keys, L, n, table_mb=0):   # noqa: N803
    from plonk_prototype_amd import _lib
    stride, nbytes = C.c_size_t(99), C.c_size_t(99)
    rc = _lib.load().pm_test_cipher_scan_keys_plan(num_cus, n_keys, L, n, table_mb, C.byref(stride), C.byref(nbytes))
    return rc, stride.value, nbytes.value


# ---------------------------------------------------------------------------------- 1. the exports
def test_exports_are_declared_bound_and_exported():
    import plonk_prototype_amd as pa
    from plonk_prototype_amd import _lib
    from plonk_prototype_amd._lib import u64p
    header = open(os.path.join(ROOT, "include", "plonk_mi355x.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    lib = C.CDLL(pa.LIB_PATH)
    vp, sz, u32 = C.c_void_p, C.c_size_t, C.c_uint32
    want = {
        "pm_poseidon_cipher_scan_keys_dev": (C.c_int, [vp, vp, u64p, u32, u32, vp, vp, vp, u32, sz, vp, vp, vp, C.POINTER(sz), vp]),
        "pm_poseidon_cipher_scan_keys_work_bytes": (sz, [vp, u32, u32, sz]),
        "pm_test_cipher_scan_keys_plan": (C.c_int, [u32, u32, u32, sz, C.c_long, C.POINTER(sz), C.POINTER(sz)]),
    }
    for name, sig in want.items():
        ret = "size_t" if sig[0] is sz else "int"
        assert re.search(r"\b%s %s\s*\(" % (ret, name), header), f"{name} is not declared in the header"
        assert hasattr(lib, name), f"{name} is not exported by the library"
        assert _lib.SIGNATURES[name] == sig, f"{name} is bound with another argument list"
        assert "pub fn %s(" % name in doc, f"{name} is missing from INTEGRATION.md's extern block"
    assert re.search(r"#define PM_CIPHER_SCAN_MAX_KEYS 64u\b", header)
    assert _lib.CIPHER_SCAN_MAX_KEYS == pa.CIPHER_SCAN_MAX_KEYS == MAX_KEYS
    for name in ("scan_keys", "scan_keys_dev", "scan_keys_bytes", "hits"):
        assert hasattr(pa.PoseidonCipher, name), name
    block = header[header.index("pm_poseidon_cipher_scan_keys_dev (DESIGN.md"):header.index("#define PM_CIPHER_OK")].replace("\n * ", " ")
    assert "LOWEST" in block and "side channels" in block


# ---------------------------------------------------------------------------------- 2. the plan
@pytest.mark.parametrize("num_cus", (1, 4, 256))
def test_plan_stride_and_bytes(num_cus):
    grid = num_cus * 8 * 64                                   # slot_blocks: eight workgroups of 64 a CU
    for n_keys in (1, 2, 5, 64):
        for L in (1, 2, 4):   # noqa: N806
            for n in (1, 63, 64, 65, 130, grid - 1, grid, grid + 1, 3 * grid + 7, 1 << 20):
                rc, stride, nbytes = plan(num_cus, n_keys, L, n)
                assert rc == 0
                assert stride % 64 == 0 and 64 <= stride <= grid
                assert stride == min(grid, (n + 63) // 64 * 64), "no cap: the grid, or n rounded up to whole workgroups only"
                assert nbytes == stride * note_bytes(n_keys, L) + tail_bytes(n_keys)


def test_plan_budget():
    num_cus, n_keys, L, n = 256, 16, 2, 1 << 20   # noqa: N806
    grid, per, tail = num_cus * 8 * 64, note_bytes(16, 2), tail_bytes(16)
    seen = []
    for mb in (1, 2, 4, 5, 9, 10, 64, 100, 1024, 4096, 9000, 9473, 9474, 20000):
        rc, stride, nbytes = plan(num_cus, n_keys, L, n, mb)
        assert rc == 0 and stride % 64 == 0 and 64 <= stride <= grid
        assert nbytes == stride * per + tail
        fit = ((mb << 20) - tail) // per // 64 * 64           # the largest multiple of 64 whose scratch fits
        assert stride == max(64, min(grid, fit)), mb
        if fit >= 64:
            assert nbytes <= mb << 20
            assert stride == grid or (stride + 64) * per + tail > mb << 20, "a larger stride would have fitted"
        seen.append(stride)
    assert seen == sorted(seen), "the plan is monotone in the budget"
    assert seen[0] == 64 and seen[-1] == grid and len(set(seen)) > 4
    assert plan(num_cus, n_keys, L, n, 0)[1] == grid, "0 = no cap"
    # the smallest budget gives a stride of 64, also where 64 notes do not fit it
    assert 64 * per + tail > 1 << 20
    assert plan(num_cus, n_keys, L, n, 1)[1:] == (64, 64 * per + tail)
    # n smaller than a stride is rounded up to whole workgroups only, with or without a budget
    assert plan(num_cus, n_keys, L, 130, 0)[1] == 192 and plan(num_cus, n_keys, L, 130, 4096)[1] == 192
    assert plan(num_cus, n_keys, L, 130, 10)[1] == 128
    assert plan(num_cus, n_keys, L, 1, 0)[1] == 64
    assert plan(num_cus, n_keys, L, 0, 0) == (0, 0, 0), "n = 0: nothing in flight"


def test_plan_refusals():
    from plonk_prototype_amd import _lib
    BAD = _lib.PM_ERR_BAD_ARG   # noqa: N806
    for n_keys in (0, 65, 0xFFFFFFFF):
        assert plan(256, n_keys, 2, 100) == (BAD, 0, 0)
    for L in (0, 5):   # noqa: N806
        assert plan(256, 3, L, 100) == (BAD, 0, 0)
    assert plan(256, 3, 2, 100, -1) == (BAD, 0, 0)
    lib, s = _lib.load(), C.c_size_t()
    assert lib.pm_test_cipher_scan_keys_plan(256, 3, 2, 100, 0, None, C.byref(s)) == BAD
    assert lib.pm_test_cipher_scan_keys_plan(256, 3, 2, 100, 0, C.byref(s), None) == BAD


# ---------------------------------------------------------------------------------- 3. the wrapper's refusals
def test_wrapper_refusals_need_no_device():
    import plonk_prototype_amd as pa

    class FakeHades(pa.Hades):
        def __init__(self):   # no context, no handle: every check below has to come before a device call
            self.ctx, self._h = None, None

    c = pa.PoseidonCipher(FakeHades())
    pts = J.to_limbs([J.GENERATOR] * 3)
    enc = np.zeros((3, 32), np.uint8)
    nonces, cts = np.zeros((3, 4), np.uint64), np.zeros((3, 3, 4), np.uint64)
    limbs = np.zeros((2, 4), np.uint64)
    bad_calls = [
        lambda: c.scan_keys([], pts, nonces, cts),                                  # 0 keys
        lambda: c.scan_keys(list(range(1, 66)), pts, nonces, cts),                  # 65 keys
        lambda: c.scan_keys(np.zeros((0, 4), np.uint64), pts, nonces, cts),
        lambda: c.scan_keys(np.zeros((65, 4), np.uint64), pts, nonces, cts),
        lambda: c.scan_keys(np.zeros((4, 3), np.uint64), pts, nonces, cts),         # a key of the wrong shape
        lambda: c.scan_keys(np.zeros((2, 2, 4), np.uint64), pts, nonces, cts),
        lambda: c.scan_keys([[1, 2], [3, 4]], pts, nonces, cts),
        lambda: c.scan_keys([1, R], pts, nonces, cts),                              # not below r
        lambda: c.scan_keys([1, -1], pts, nonces, cts),
        lambda: c.scan_keys([5, 6], pts, nonces[:2], cts),                          # mismatched counts
        lambda: c.scan_keys([5, 6], pts, nonces, cts[:2]),
        lambda: c.scan_keys([5, 6], pts[:2], nonces, cts),
        lambda: c.scan_keys(limbs, pts, nonces, cts[:, :2]),                        # ciphers have L + 1 words
        lambda: c.scan_keys_bytes([5, 6], enc, nonces[:2], cts),
        lambda: c.scan_keys_bytes([5, 6], enc[:, :31], nonces, cts),
        lambda: c.scan_keys_bytes([], enc, nonces, cts),
        lambda: c.scan_keys_dev([], 16, 16, 16, 3, 16),
        lambda: c.scan_keys_dev(list(range(65)), 16, 16, 16, 3, 16),
    ]
    for k, call in enumerate(bad_calls):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"call {k} was not refused")
    masks, m, st = c.scan_keys([7, 7, 0], pts[:0], nonces[:0], cts[:0])              # duplicates and 0 are legal keys
    assert masks.shape == (0,) and masks.dtype == np.uint64 and m.shape == (0, 2, 4) and st.shape == (0,) and st.dtype == np.uint32


def test_hits_lists_the_pairs_in_order():
    import plonk_prototype_amd as pa
    masks = np.array([0, 1, (1 << 63) | 4, 0, 6, 1 << 63], np.uint64)
    got = pa.PoseidonCipher.hits(masks)
    assert got.dtype == np.int64 and got.tolist() == [[1, 0], [2, 2], [2, 63], [4, 1], [4, 2], [5, 63]]
    assert pa.PoseidonCipher.hits(np.zeros(5, np.uint64)).shape == (0, 2)
    assert pa.PoseidonCipher.hits(np.zeros(0, np.uint64)).shape == (0, 2)
    assert len(pa.PoseidonCipher.hits(np.full(3, 0xFFFFFFFFFFFFFFFF, np.uint64))) == 192


# ---------------------------------------------------------------------------------- 4. the premise, in integers
def _digits(vk):
    """pm_test_cipher_digits, from the bottom up: d[w] is the digit of 16^w"""
    from plonk_prototype_amd import _lib
    d = (C.c_int8 * 64)(*([99] * 64))
    assert _lib.load().pm_test_cipher_digits(_u64p(CM.key_words(vk, False)), 1, d) == 0
    return list(d)[::-1]


def test_signed_digits_over_the_window_multiples_give_the_product():
    rng = random.Random(0x5CA9)
    keys = list(CM.SPECIAL_KEYS) + [0] + [rng.randrange(R) for _ in range(3)]
    honest = CM.case("5_2_per_round", 130)["eph"][7]
    points = [honest, J.IDENTITY, J.add(honest, CM.ORDER_2)]
    assert all(J.on_curve(p) for p in points)
    digits = {vk: _digits(vk) for vk in keys}
    for vk, d in digits.items():
        assert all(abs(x) <= 8 for x in d) and sum(x * 16 ** w for w, x in enumerate(d)) == vk, hex(vk)
    for p in points:
        base, windows = p, []                                  # 16^w P, w = 0 .. 63
        for _ in range(64):
            windows.append(base)
            for _ in range(4):
                base = J.add(base, base)
        for vk, d in digits.items():
            acc = J.IDENTITY
            for w, x in enumerate(d):
                if x:
                    e = J.mul_affine(windows[w], abs(x))         # the table's entry |d| 16^w P
                    acc = J.add(acc, e if x > 0 else ((R - e[0]) % R, e[1]))
            assert acc == CM.mul(p, vk), (hex(vk), p == J.IDENTITY)
