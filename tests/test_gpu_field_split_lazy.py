"""The lazy split products on the device: fe_mul_split<3, 3>, <5, 5> and <1, 1> (csrc/fields.hip.h) and the fe_sub<K, 1> of
dft4s_lazy (K = 18, 34, 39), run on raw limbs through pm_test_field_raw_op and compared limb for limb with the big-integer
model (oracle/fe_model.py), one wave per 64 cases, at the limits of the classes the radix-2^10 passes hand them
(tests/test_fe_mul_split_lazy_model.py walks the same classes without a device).  Every comparison is exact."""
import random

import numpy as np
import pytest

from oracle import bigint_oracle as B
from oracle import fe_model as M

pytestmark = pytest.mark.gpu

SPLIT_3_3, SPLIT_1_1, SPLIT_5_5, SUB = 25, 26, 27, 32
# (G, op, data limb bound Bx, data value class V)
FORMS = [(3, SPLIT_3_3, 5, 60), (5, SPLIT_5_5, 5, 60), (1, SPLIT_1_1, 4, 35)]
W, N = M.W, M.N


def run(ctx, op, cases):
    x = np.array(cases, dtype=np.uint64)
    assert x.ndim == 3 and x.shape[2] == N and int(x.max()) <= M.M32
    return ctx.field_raw_op(0, op, x.astype(np.uint32), 1).tolist()


@pytest.fixture(autouse=True)
def clean_log():
    M.VIOLATIONS.clear()
    yield
    M.VIOLATIONS.clear()


@pytest.mark.parametrize("G,op,Bx,V", FORMS, ids=lambda v: str(v))
def test_lazy_split_against_the_model(ctx, G, op, Bx, V):
    f, rng = M.FR, random.Random(43 + G)
    groups = (N + G - 1) // G
    data = M.class_members(f, Bx, V, False, 1500, 700 + G) + [[(Bx << W) - 1] * N, [(Bx << W) - 1 - i for i in range(N)]]
    cases, ws = [], []
    for i, x in enumerate(data):
        w = (B.R_MOD - 1, 0, 1)[i] if i < 3 else rng.randrange(B.R_MOD)
        rows = M.rows_of(w, G, G) if i % 50 != 49 else [M.limbs(B.R_MOD - 1)] * groups      # every row at r - 1: the value bound
        cases.append([x] + rows)
        ws.append(w if i % 50 != 49 else None)
    bound = (groups * Bx * ((1 << (W - 1)) + 1) + (1 << (W - 1))) * B.R_MOD                 # 2^(W-1) times the stated value bound
    biggest = 0
    for c, w, (g,) in zip(cases, ws, run(ctx, op, cases)):
        want, peak, _ = M.mul_split(c[0], c[1:], G, G)
        assert peak < 1 << 64 and g == want
        assert max(g) < 1 << W and M.value(g) << (W - 1) < bound                           # every limb, the top one too
        t = sum(M.value(c[0][j * G:(j + 1) * G]) * M.value(c[1 + j]) for j in range(groups))
        assert (M.value(g) << (W * G)) % B.R_MOD == t % B.R_MOD
        if w is not None:
            assert M.value(g) % B.R_MOD == M.value(c[0]) * w * f.RINV % B.R_MOD              # what fe_mul returns for the same operands
        biggest = max(biggest, M.value(g))
    assert biggest > 2 * B.R_MOD


@pytest.mark.parametrize("K,Vb", [(18, 17), (34, 33), (39, 38)])
def test_the_butterfly_differences(ctx, K, Vb):
    """fe_sub<K, 1>: minuend up to (2+, <20), subtrahend a sum of two normalised elements (limbs <= 2^30 - 2) of value < (K - 1) r"""
    f = M.FR
    top = (1 << (W + 1)) - 2
    edge = [top] * (N - 1)
    edge.append((Vb * f.mod - 1 - M.value_of(f, edge)) >> (W * (N - 1)))
    cm = M.class_members(f, 2, Vb, False, 600, seed=K)
    bs = [edge, M.most_redundant(f, Vb * f.mod - 1, 2)] + [b for b in cm if max(b[:-1]) <= top]
    a_s = M.class_members(f, 2, 20, True, len(bs), seed=K + 50)
    cases = [[a_s[i % len(a_s)], b] for i, b in enumerate(bs)] + [[a_s[0], b] for b in bs[:8]] + [[a_s[1], b] for b in bs[:8]]
    for (a, b), (g,) in zip(cases, run(ctx, SUB + K, cases)):
        assert g == M.fe_sub(f, K, 1, a, b)
        assert M.value_of(f, g) == M.value_of(f, a) - M.value_of(f, b) + K * f.mod           # no limb wrapped
    assert not M.VIOLATIONS, M.VIOLATIONS[:3]


def test_unknown_forms_are_rejected(ctx):
    from plonk_prototype_amd import _lib
    x = np.zeros((1, 10, 9), np.uint32)
    out = np.zeros((1, 1, 9), np.uint32)
    for field, op in ((1, SPLIT_3_3), (1, SPLIT_1_1), (1, SPLIT_5_5), (0, 28), (1, SUB + 18), (0, SUB + 17), (0, SUB + 40)):
        rc = ctx._lib.pm_test_field_raw_op(ctx._h, field, op, x.ctypes.data_as(_lib.u32p), out.ctypes.data_as(_lib.u32p), 1)
        assert rc == _lib.PM_ERR_BAD_ARG, (field, op)
