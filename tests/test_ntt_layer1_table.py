"""The head of the radix-4 step table (csrc/ntt_kernels4.hip.h, step4_tw_kernel), read back through
pm_test_ntt_step4_table and re-derived with oracle/bigint_oracle.py: seven constants of 84 words -- w4 and w16^e for
e = 1, 2, 3, 6, 9, 0, w16 = wR^(R/16) of the table's direction -- each as the nine rows w 2^(29 (j - 7)) mod r of
fe_mul_split<1, 2>, transposed; then the entries, the first layer's per-lane block still in its place."""
import ctypes as C

import numpy as np
import pytest

from oracle import bigint_oracle as B

W, N = 29, 9
MASK = (1 << W) - 1
RADIX = 1 << (W * N)                 # the device Montgomery radix
HEAD_EXPONENTS = (4, 1, 2, 3, 6, 9, 0)  # block 0 is w4 = w16^4, the last one is 1
BLOCK, ENTRY = 84, 20                # words


def _limbs(v):
    return [(v >> (W * i)) & MASK for i in range(N)]


def _shift(v, e):
    """v 2^e mod r"""
    return v * (pow(2, e, B.R_MOD) if e >= 0 else pow(pow(2, -e, B.R_MOD), -1, B.R_MOD)) % B.R_MOD


def _table(ctx, inverse, S):
    from plonk_prototype_amd import _lib
    words = C.c_size_t()
    ctx._check(ctx._lib.pm_test_ntt_step4_table(ctx._h, inverse, S, None, 0, C.byref(words)))
    out = np.zeros(words.value, np.uint32)
    ctx._check(ctx._lib.pm_test_ntt_step4_table(ctx._h, inverse, S, out.ctypes.data_as(_lib.u32p), out.size, None))
    return out


def _w_R(inverse, S):
    d = B.Domain(1 << S)
    return d.group_gen_inv if inverse else d.group_gen


@pytest.mark.gpu
@pytest.mark.parametrize("inverse", [0, 1])
@pytest.mark.parametrize("S", [4, 5, 8, 10])
def test_head_constants_and_rows(ctx, inverse, S):
    tab = _table(ctx, inverse, S)
    R = 1 << S
    wR = _w_R(inverse, S)
    for blk, e in enumerate(HEAD_EXPONENTS):
        w = pow(wR, e * R // 16, B.R_MOD)                              # w16^e of this direction
        assert pow(w, 16, B.R_MOD) == 1
        w_mont = w * RADIX % B.R_MOD
        head = tab[BLOCK * blk: BLOCK * (blk + 1)].tolist()
        for j in range(N):
            got = [head[9 * b + j] for b in range(N)]
            assert got == _limbs(_shift(w_mont, W * (j - 7))), (S, inverse, e, j)
        # row 7 is the constant itself: the limbs read as a number, out of Montgomery form, are w16^e
        const = sum(head[9 * b + 7] << (W * b) for b in range(N))
        assert const * pow(RADIX, -1, B.R_MOD) % B.R_MOD == w
        assert head[81:] == [0, 0, 0]
    assert pow(wR, 4 * R // 16, B.R_MOD) == pow(_w_R(inverse, 2), 1, B.R_MOD)    # block 0 is the w4 the kernels always used


@pytest.mark.gpu
@pytest.mark.parametrize("inverse", [0, 1])
@pytest.mark.parametrize("S", [4, 5, 10])
def test_entries_follow_the_head_and_keep_the_layer1_block(ctx, inverse, S):
    """Entry [(t - 1) Ns' + k'] of block s = wR^(k' t R / (Ns' q)): rows w 2^-87 and w 2^58.  Shapes that do not take the
    wave-uniform path still read block 1 (Ns' = 4), the per-lane first-layer twiddles."""
    tab = _table(ctx, inverse, S)
    wR = _w_R(inverse, S)
    steps = (S + 1) // 2
    lq = [2 if S - 2 * s >= 2 else 1 for s in range(steps)]
    total = sum(((1 << lq[s]) - 1) << (2 * s) for s in range(steps))
    assert tab.size == len(HEAD_EXPONENTS) * BLOCK + ENTRY * total
    off = 0
    for s in range(steps):
        nsp = 1 << (2 * s)
        cnt = ((1 << lq[s]) - 1) * nsp
        if s <= 1:                                                     # block 0 (all ones) and the first-layer block
            for i in range(cnt):
                t, kp = i // nsp + 1, i % nsp
                w = pow(wR, (kp * t) << (S - 2 * s - lq[s]), B.R_MOD)
                ent = tab[len(HEAD_EXPONENTS) * BLOCK + ENTRY * (off + i):][:ENTRY].tolist()
                w_mont = w * RADIX % B.R_MOD
                assert ent[:9] == _limbs(_shift(w_mont, -87)) and ent[9:18] == _limbs(_shift(w_mont, 58)), (S, s, i)
                assert ent[18:] == [0, 0]
        off += cnt


@pytest.mark.gpu
def test_hook_rejects_bad_arguments(ctx):
    from plonk_prototype_amd import _lib
    words = C.c_size_t()
    assert ctx._lib.pm_test_ntt_step4_table(None, 0, 10, None, 0, C.byref(words)) == _lib.PM_ERR_BAD_ARG
    assert ctx._lib.pm_test_ntt_step4_table(ctx._h, 2, 10, None, 0, C.byref(words)) == _lib.PM_ERR_BAD_ARG
    assert ctx._lib.pm_test_ntt_step4_table(ctx._h, 0, 11, None, 0, C.byref(words)) == _lib.PM_ERR_BAD_ARG
    assert ctx._lib.pm_test_ntt_step4_table(ctx._h, 0, 10, None, 4, C.byref(words)) == _lib.PM_ERR_BAD_ARG


def test_hook_is_declared_everywhere():
    """header, ctypes table and the Rust bindings of INTEGRATION.md name the hook (CPU: no context is made)"""
    import os
    from conftest import ROOT
    from plonk_prototype_amd import _lib
    assert "pm_test_ntt_step4_table" in _lib.SIGNATURES
    for rel in (("include", "plonk_mi355x.h"), ("INTEGRATION.md",)):
        assert "pm_test_ntt_step4_table" in open(os.path.join(ROOT, *rel)).read()
