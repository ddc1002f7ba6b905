"""The lazy split table of the radix-4 passes (csrc/ntt_kernels4.hip.h, step4_lazy_tw_kernel), read back through
pm_test_ntt_step4_lazy_table and re-derived with oracle/bigint_oracle.py: the w4 head for fe_mul_split<1, 1>, nine rows
w4 2^(29 (j - 8)) mod r transposed into 84 words, then, for every entry of the radix-4 steps s >= 2 in the order of the
existing table, the rows w 2^(29 (j G + G - 9)) mod r of the form G, padded to a multiple of four words.  And the
existing table, read through pm_test_ntt_step4_table before and after, is what it was, word for word."""
import ctypes as C

import numpy as np
import pytest

from oracle import bigint_oracle as B

W, N = 29, 9
MASK = (1 << W) - 1
RADIX = 1 << (W * N)
HEAD = 84
OLD_HEAD_EXPONENTS = (4, 1, 2, 3, 6, 9, 0)


def _limbs(v):
    return [(v >> (W * i)) & MASK for i in range(N)]


def _shift(v, e):
    return v * (pow(2, e, B.R_MOD) if e >= 0 else pow(pow(2, -e, B.R_MOD), -1, B.R_MOD)) % B.R_MOD


def _read(ctx, fn, *args):
    from plonk_prototype_amd import _lib
    words = C.c_size_t()
    ctx._check(fn(ctx._h, *args, None, 0, C.byref(words)))
    out = np.zeros(words.value, np.uint32)
    ctx._check(fn(ctx._h, *args, out.ctypes.data_as(_lib.u32p), out.size, None))
    return out


def _w_R(inverse, S):
    d = B.Domain(1 << S)
    return d.group_gen_inv if inverse else d.group_gen


def _step_entries(S, inverse, from_step):
    """(s, w) of every entry of the steps s >= from_step, in table order"""
    wR, steps = _w_R(inverse, S), (S + 1) // 2
    for s in range(steps):
        lq = 2 if S - 2 * s >= 2 else 1
        nsp = 1 << (2 * s)
        for i in range(((1 << lq) - 1) * nsp):
            if s >= from_step:
                t, kp = i // nsp + 1, i % nsp
                yield s, lq, pow(wR, (kp * t) << (S - 2 * s - lq), B.R_MOD)


def _old_table(S, inverse):
    wR, R = _w_R(inverse, S), 1 << S
    out = []
    for e in OLD_HEAD_EXPONENTS:
        w_mont = pow(wR, e * R // 16, B.R_MOD) * RADIX % B.R_MOD if S >= 4 else None
        if w_mont is None:
            return None
        rows = [_limbs(_shift(w_mont, W * (j - 7))) for j in range(N)]
        out += [rows[j][b] for b in range(N) for j in range(N)] + [0, 0, 0]
    for _, _, w in _step_entries(S, inverse, 0):
        w_mont = w * RADIX % B.R_MOD
        out += _limbs(_shift(w_mont, -87)) + _limbs(_shift(w_mont, 58)) + [0, 0]
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("inverse", [0, 1])
@pytest.mark.parametrize("S", [4, 8, 10])
def test_lazy_table_and_the_existing_one_beside_it(ctx, inverse, S):
    old_fn, lazy_fn = ctx._lib.pm_test_ntt_step4_table, ctx._lib.pm_test_ntt_step4_lazy_table
    before = _read(ctx, old_fn, inverse, S)
    w4_mont = (_w_R(inverse, 2)) * RADIX % B.R_MOD
    for G in (3, 5, 2, 1):
        rows_n = (N + G - 1) // G
        ent_words = 4 * ((9 * rows_n + 3) // 4)
        tab = _read(ctx, lazy_fn, inverse, S, G).tolist()
        rows = [_limbs(_shift(w4_mont, W * (j - 8))) for j in range(N)]
        assert tab[:HEAD] == [rows[j][b] for b in range(N) for j in range(N)] + [0, 0, 0], (S, inverse, G)
        assert sum(rows[8][b] << (W * b) for b in range(N)) == w4_mont          # row 8 is w4 itself
        want = []
        for s, lq, w in _step_entries(S, inverse, 2):
            if lq != 2:
                continue
            w_mont = w * RADIX % B.R_MOD
            ent = [l for j in range(rows_n) for l in _limbs(_shift(w_mont, W * (j * G + G - N)))]
            want += ent + [0] * (ent_words - len(ent))
        assert len(tab) == HEAD + len(want), (S, inverse, G)
        assert tab[HEAD:] == want, (S, inverse, G)
    after = _read(ctx, old_fn, inverse, S)
    assert np.array_equal(before, after)
    assert after.tolist() == _old_table(S, inverse)


@pytest.mark.gpu
def test_lazy_hook_rejects_bad_arguments(ctx):
    from plonk_prototype_amd import _lib
    words = C.c_size_t()
    fn = ctx._lib.pm_test_ntt_step4_lazy_table
    assert fn(None, 0, 10, 3, None, 0, C.byref(words)) == _lib.PM_ERR_BAD_ARG
    assert fn(ctx._h, 2, 10, 3, None, 0, C.byref(words)) == _lib.PM_ERR_BAD_ARG
    assert fn(ctx._h, 0, 11, 3, None, 0, C.byref(words)) == _lib.PM_ERR_BAD_ARG
    assert fn(ctx._h, 0, 10, 4, None, 0, C.byref(words)) == _lib.PM_ERR_BAD_ARG
    assert fn(ctx._h, 0, 10, 3, None, 4, C.byref(words)) == _lib.PM_ERR_BAD_ARG


def test_lazy_hook_is_declared_everywhere():
    import os
    from conftest import ROOT
    from plonk_prototype_amd import _lib
    assert "pm_test_ntt_step4_lazy_table" in _lib.SIGNATURES
    for rel in (("include", "plonk_mi355x.h"), ("INTEGRATION.md",)):
        assert "pm_test_ntt_step4_lazy_table" in open(os.path.join(ROOT, *rel)).read()
