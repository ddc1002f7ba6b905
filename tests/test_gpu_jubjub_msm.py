"""The JubJub MSM on the GPU against the big-integer sum of tests/jubjub_msm_model.py, byte for byte: the
edge points and edge scalars at sizes around a wave under every window width; degenerate scalar vectors (all zero, all one, all
equal: one bucket per window holds everything); a batch at a padded stride; more points than one workgroup holds, checked by
discrete logarithm; determinism, a caller's stream, pm_trim; and the refusals that return before any launch."""
import ctypes as C
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jubjub_model as J  # noqa: E402
import jubjub_msm_model as MM  # noqa: E402
import schnorr_model as S  # noqa: E402

pytestmark = pytest.mark.gpu
R, Q = J.R, J.Q
SIZES = (0, 1, 2, 3, 63, 64, 65, 130)
WIDTHS = (0,) + MM.WINDOW_BITS                   # 0: the rule's own choice
FORMS = (("canonical", False), ("montgomery", True))
IDENTITY = J.to_limbs([J.IDENTITY])[0]


def _form(mont):
    return 0 if mont else 1


@pytest.fixture
def width(ctx):
    """sets the option for one test and puts the rule back"""
    def force(c):
        ctx.set_option("jubjub_msm_window_bits", c)
    yield force
    ctx.set_option("jubjub_msm_window_bits", 0)


def msm_words(ctx, points, scalars, mont, batch=1, stride=None, stream=0):
    """points [n, 2, 4] limbs and scalar words [rows, 4] as they lie in memory -> [batch, 2, 4]"""
    import plonk_prototype_amd as pa
    n = points.shape[0]
    dp = pa.DeviceVector.from_host(ctx, points.reshape(-1, 4))
    ds = pa.DeviceVector.from_host(ctx, scalars.reshape(-1, 4))
    out = pa.DeviceVector.from_host(ctx, np.full((2 * batch, 4), 0x7777777777777777, np.uint64))
    try:
        pa.jubjub_msm_dev(ctx, dp.ptr, ds.ptr, n, out.ptr, batch, stride, _form(mont), stream)
        if stream:
            import torch
            torch.cuda.synchronize()
        return out.to_host().reshape(batch, 2, 4)
    finally:
        for x in (dp, ds, out):
            x.free()


def msm_ints(ctx, points, scalars, mont=False, **kw):
    return msm_words(ctx, J.to_limbs(points) if len(points) else np.zeros((0, 2, 4), np.uint64),
                     S.scalar_words(scalars, mont) if len(scalars) else np.zeros((0, 4), np.uint64), mont, **kw)[0]


# ---------------------------------------------------------------------------------- 1. the model, at the edges
@pytest.mark.parametrize("form", FORMS, ids=[f[0] for f in FORMS])
def test_edge_points_and_scalars_are_the_model(ctx, width, form):
    name, mont = form
    for n in SIZES:
        pts, sc, want = MM.edge_case(n)
        want = J.to_limbs([want])[0]
        for c in WIDTHS:
            width(c)
            got = msm_ints(ctx, pts, sc, mont)
            assert got.tobytes() == want.tobytes(), (name, n, c)
    pts, sc, _ = MM.edge_case(130)
    assert {J.IDENTITY, (0, R - 1), (J.SQRT_M1, 0), J.M.curve_point(0x14)} <= set(pts) and pts[2] == pts[0] and pts[40] == MM.neg(pts[41])
    assert {0, 1, R - 1, Q, 8 * Q} <= set(sc)


def test_the_python_form_and_the_host_form_agree(ctx):
    import plonk_prototype_amd as pa
    pts, sc, want = MM.edge_case(65)
    want = J.to_limbs([want])[0]
    assert np.array_equal(pa.jubjub_msm(ctx, pts, sc), want)                                         # [n] integers
    assert np.array_equal(pa.jubjub_msm(ctx, J.to_limbs(pts), J.M.to_limbs(sc)), want)               # [n, 4] limbs
    rows = [sc, sc[::-1], [1] * 65]
    got = pa.jubjub_msm(ctx, pts, rows)                                                              # [B, n]
    assert got.shape == (3, 2, 4) and np.array_equal(got[0], want)
    assert np.array_equal(got[1], J.to_limbs([MM.msm(pts, sc[::-1])])[0]) and np.array_equal(got[2], J.to_limbs([MM.psum(pts)])[0])
    assert np.array_equal(pa.jubjub_msm(ctx, J.to_limbs(pts), np.stack([J.M.to_limbs(r) for r in rows])), got)   # [B, n, 4]
    assert np.array_equal(pa.jubjub_msm_host(pts[:9], sc[:9]), pa.jubjub_msm(ctx, pts[:9], sc[:9]))
    assert np.array_equal(pa.jubjub_msm(ctx, [], []), IDENTITY)


# ---------------------------------------------------------------------------------- 2. degenerate scalar vectors
def test_degenerate_scalars(ctx, width):
    pts, _, _ = MM.edge_case(130)
    rng = random.Random(77)
    one_value = rng.randrange(R)
    plain = J.to_limbs([MM.psum(pts)])[0]
    skew = J.to_limbs([J.mul(MM.psum(pts), one_value)])[0]                    # s (sum P) = sum s P
    top = J.to_limbs([J.mul(pts[1], R - 1)])[0]
    for c in (0, 4, 9, 16):
        width(c)
        for mont in (False, True):
            assert np.array_equal(msm_ints(ctx, pts, [0] * 130, mont), IDENTITY), (c, mont)      # no pair at all
            assert np.array_equal(msm_ints(ctx, pts, [1] * 130, mont), plain), (c, mont)         # one bucket of one window
            assert np.array_equal(msm_ints(ctx, pts, [one_value] * 130, mont), skew), (c, mont)  # one bucket of every window
            assert np.array_equal(msm_ints(ctx, pts[1:2], [R - 1], mont), top), (c, mont)


# ---------------------------------------------------------------------------------- 3. a batch at a padded stride
def test_batch_equals_single_calls_and_ignores_the_padding(ctx, width):
    n, batch, stride = 65, 3, 70
    pts, sc, _ = MM.edge_case(n)
    rng = random.Random(3)
    rows = [sc, [rng.randrange(R) for _ in range(n)], [rng.randrange(1 << 16) for _ in range(n)]]
    p = J.to_limbs(pts)
    for mont in (False, True):
        buf = np.full((batch * stride, 4), 0xFFFFFFFFFFFFFFFF, np.uint64)     # the padding: words no scalar has
        for b, row in enumerate(rows):
            buf[b * stride:b * stride + n] = S.scalar_words(row, mont)
        for c in (0, 5, 16):
            width(c)
            got = msm_words(ctx, p, buf, mont, batch=batch, stride=stride)
            for b, row in enumerate(rows):
                single = msm_words(ctx, p, S.scalar_words(row, mont), mont)[0]
                assert got[b].tobytes() == single.tobytes(), (mont, c, b)
            other = buf.copy()
            other[n:stride] = 0x0123456789ABCDEF
            assert msm_words(ctx, p, other, mont, batch=batch, stride=stride).tobytes() == got.tobytes(), (mont, c)
    assert got[0].tobytes() == J.to_limbs([MM.edge_case(n)[2]])[0].tobytes()


# ---------------------------------------------------------------------------------- 4. beyond one workgroup
def test_many_points_by_discrete_logarithm(ctx, width):
    import plonk_prototype_amd as pa
    n = (1 << 14) + 37
    rng = random.Random(0xD106)
    ks = [rng.randrange(R) for _ in range(n)]
    g = pa.JubJubBase(ctx, J.GENERATOR)
    try:
        pts = g.mul(ks)                                                       # k_i G: held against the model by its own tests
    finally:
        g.free()
    uniform = [rng.randrange(R) for _ in range(n)]

    def witness_like():
        t = rng.random()
        return 0 if t < 0.05 else 1 if t < 0.06 else rng.randrange(1 << 16) if t < 0.96 else rng.randrange(R)
    witness = [witness_like() for _ in range(n)]
    for label, sc in (("uniform", uniform), ("witness-like", witness)):
        want = J.to_limbs([J.mul(J.GENERATOR, sum(s * k for s, k in zip(sc, ks)) % Q)])[0]
        words = S.scalar_words(sc, True)
        for c in (0, MM.WINDOW_BITS[0], MM.WINDOW_BITS[-1]):
            width(c)
            got = msm_words(ctx, pts, words, True)[0]
            assert got.tobytes() == want.tobytes(), (label, c)
    # the same bytes again, on a caller's stream, and after the workspace went back
    import torch
    again = msm_words(ctx, pts, words, True)[0]
    assert again.tobytes() == want.tobytes()
    st = torch.cuda.Stream()
    assert msm_words(ctx, pts, words, True, stream=st.cuda_stream)[0].tobytes() == want.tobytes()
    assert ctx.trim() > 0
    assert msm_words(ctx, pts, words, True)[0].tobytes() == want.tobytes()


# ---------------------------------------------------------------------------------- 5. refusals, all before any launch
def test_refusals(ctx):
    import plonk_prototype_amd as pa
    n = 8
    dp, ds, out = pa.DeviceVector(ctx, 2 * n), pa.DeviceVector(ctx, 2 * n), pa.DeviceVector(ctx, 4)

    def rc(points, scalars, n_, stride, batch, form, o):
        return ctx._lib.pm_jubjub_msm_dev(ctx._h, C.c_void_p(points), C.c_void_p(scalars), n_, stride, batch, form, C.c_void_p(o), None)
    try:
        assert rc(0, ds.ptr, n, n, 1, 0, out.ptr) == -1 and rc(dp.ptr, 0, n, n, 1, 0, out.ptr) == -1
        assert rc(dp.ptr, ds.ptr, n, n, 1, 0, 0) == -1 and rc(0, 0, 0, 0, 1, 0, 0) == -1
        for bad in ((dp.ptr + 8, ds.ptr, out.ptr), (dp.ptr, ds.ptr + 8, out.ptr), (dp.ptr, ds.ptr, out.ptr + 8)):
            assert rc(bad[0], bad[1], n, n, 1, 0, bad[2]) == -1
        assert rc(dp.ptr, ds.ptr, n, n, 0, 0, out.ptr) == -1                   # batch = 0
        assert rc(dp.ptr, ds.ptr, n, n - 1, 1, 0, out.ptr) == -1               # scalar_stride < n
        assert rc(dp.ptr, ds.ptr, n, n, 1, 2, out.ptr) == -1                   # scalar_form
        assert rc(dp.ptr, ds.ptr, n, n, 1, 0, dp.ptr) == -1                    # the output on the points
        assert rc(dp.ptr, ds.ptr, n, n, 1, 0, dp.ptr + 64 * (n - 1)) == -1
        assert rc(dp.ptr, ds.ptr, n, n, 2, 0, ds.ptr + 32 * n - 64) == -1      # ... on the scalars
        assert "overlaps" in ctx._lib.pm_last_error(ctx._h).decode()
        assert rc(dp.ptr, ds.ptr, 1 << 31, 1 << 31, 1, 0, out.ptr) == -6       # n > 2^31 - 1
        ctx.set_option("jubjub_msm_window_bits", 16)
        assert rc(dp.ptr, ds.ptr, 1 << 20, 1 << 20, 300, 0, out.ptr) == -6     # more pairs than the plan indexes: nothing runs
        ctx.set_option("jubjub_msm_window_bits", 0)
        for c in (-1, 1, 3, 17, 20):
            with pytest.raises(pa.Error) as e:
                ctx.set_option("jubjub_msm_window_bits", c)
            assert e.value.code == -1
    finally:
        ctx.set_option("jubjub_msm_window_bits", 0)
        for x in (dp, ds, out):
            x.free()
