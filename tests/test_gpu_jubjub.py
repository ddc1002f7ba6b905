"""Native JubJub on the GPU: fixed-base multiplication, commitments and variable-base multiplication
against the big-integer model of tests/jubjub_model.py, byte for byte, on the edge scalars and points, in both scalar forms, in
place, over more than one block and on a caller's stream; the point check; the native product against the rows a FIXED_BASE
gadget fills; and a commitment hashed by the native Poseidon without a host copy."""
import ctypes as C
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gadget_model as M  # noqa: E402
import jubjub_model as J  # noqa: E402
import poseidon_model as PM  # noqa: E402

pytestmark = pytest.mark.gpu
R, Q = J.R, J.Q
SIZES = (1, 2, 63, 64, 65, 130)
NMAX = max(SIZES)
ODD = M.curve_point(0x14)            # its order is not Q
_CACHE = {}


def _scalars(n=NMAX):
    """the edge scalars first, then random ones"""
    if "scalars" not in _CACHE:
        _CACHE["scalars"] = J.edge_scalars(extra=NMAX)[:NMAX]
    return _CACHE["scalars"][:n]


def _products(base):
    """the model's s_i * base for the NMAX scalars, once per base"""
    if ("prod", base) not in _CACHE:
        _CACHE["prod", base] = [J.mul(base, s) for s in _scalars()]
    return _CACHE["prod", base]


def _mont(scalars):
    return M.to_limbs(scalars)


def _same(got, want_points, what=""):
    want = J.to_limbs(want_points)
    assert got.shape == want.shape, (got.shape, want.shape)
    if got.tobytes() != want.tobytes():
        bad = np.flatnonzero((got != want).any(axis=(1, 2)))
        raise AssertionError(f"{what}: {bad.size} of {len(want_points)} points differ, first {bad[:8]}")


# ---------------------------------------------------------------------------------- 1. fixed base
@pytest.mark.parametrize("base", (J.GENERATOR, ODD), ids=("generator", "order_not_q"))
def test_fixed_base(ctx, base):
    import plonk_prototype_amd as pa
    b = pa.JubJubBase(ctx, base)
    try:
        assert b.point.tobytes() == J.to_limbs([base])[0].tobytes()
        want = _products(base)
        for n in SIZES:
            s = _scalars(n)
            _same(b.mul(s), want[:n], f"canonical, n = {n}")
            _same(b.mul(_mont(s)), want[:n], f"montgomery, n = {n}")
        assert b.mul([]).shape == (0, 2, 4)
    finally:
        b.free()


def test_base_create_refusals(ctx):
    import plonk_prototype_amd as pa
    with pytest.raises(pa.Error):
        pa.JubJubBase(ctx, (J.GENERATOR[0], J.GENERATOR[1] + 1))                # off the curve
    raw = J.to_limbs([J.IDENTITY]).copy()
    raw[0, 1] = np.frombuffer((R + int.from_bytes(raw[0, 1].tobytes(), "little")).to_bytes(32, "little"), dtype=np.uint64)
    with pytest.raises(pa.Error):
        pa.JubJubBase(ctx, raw)                                                  # (0, 1 + r): a coordinate >= r
    lib, out = ctx._lib, C.c_void_p()
    assert lib.pm_jubjub_base_create(ctx._h, None, C.byref(out)) == pa._lib.PM_ERR_BAD_ARG


# ---------------------------------------------------------------------------------- 2. commitments
def test_commit(ctx):
    import plonk_prototype_amd as pa
    g, h = pa.JubJubBase(ctx, J.GENERATOR), pa.JubJubBase(ctx, ODD)
    try:
        sc = _scalars()
        v = [0, sc[20], 0] + sc[:NMAX - 3]                       # v = 0; b = 0; both 0 -> (0, 1); then the edge scalars
        bl = [sc[21], 0, 0] + list(reversed(sc))[:NMAX - 3]
        pg, ph = dict(zip(sc, _products(J.GENERATOR))), dict(zip(sc, _products(ODD)))        # 0 is among the edge scalars
        want = [J.add(pg[x], ph[y]) for x, y in zip(v, bl)]
        assert want[2] == J.IDENTITY
        for n in SIZES:
            _same(pa.jubjub_commit(g, h, v[:n], bl[:n]), want[:n], f"canonical, n = {n}")
            _same(pa.jubjub_commit(g, h, _mont(v[:n]), _mont(bl[:n])), want[:n], f"montgomery, n = {n}")
        # ... and the two-step host route: add_host(mul_host, mul_host)
        got = pa.jubjub_commit(g, h, v[:8], bl[:8])
        for i in range(8):
            two_step = pa.jubjub_add_host(pa.jubjub_mul_host(J.GENERATOR, v[i]), pa.jubjub_mul_host(ODD, bl[i]))
            assert got[i].tobytes() == two_step.tobytes(), i
        # g is h with b = q - v: the identity through a chain that is not trivial
        vs = [s % Q for s in sc[:40]]
        got = pa.jubjub_commit(g, g, vs, [(Q - x) % R for x in vs])
        _same(got, [J.IDENTITY] * len(vs), "g is h, b = q - v")
    finally:
        g.free(), h.free()


# ---------------------------------------------------------------------------------- 3. variable base
def _var_case():
    """NMAX (point, scalar) pairs: the edge points in turn, then one point under every edge scalar"""
    if "var" not in _CACHE:
        pts, sc = J.edge_points(), _scalars()
        ps = [pts[i % len(pts)] for i in range(48)] + [ODD] * (NMAX - 48)
        ss = sc[:48] + sc[:NMAX - 48]
        _CACHE["var"] = (ps, ss, [J.mul(p, s) for p, s in zip(ps, ss)])
    return _CACHE["var"]


def test_variable_base(ctx):
    import plonk_prototype_amd as pa
    ps, ss, want = _var_case()
    for n in SIZES:
        _same(pa.jubjub_mul(ctx, ps[:n], ss[:n]), want[:n], f"canonical, in place, n = {n}")
    # Montgomery scalars, and out of place
    n = NMAX
    dp, ds, out = (pa.DeviceVector.from_host(ctx, J.to_limbs(ps)), pa.DeviceVector.from_host(ctx, _mont(ss)),
                   pa.DeviceVector(ctx, 2 * n))
    try:
        pa.jubjub_mul_dev(ctx, dp.ptr, ds.ptr, n, out.ptr)
        _same(out.to_host().reshape(n, 2, 4), want, "montgomery, out of place")
        assert dp.to_host().tobytes() == J.to_limbs(ps).tobytes()          # the points are untouched
    finally:
        dp.free(), ds.free(), out.free()


def test_variable_base_equals_fixed_base(ctx):
    import plonk_prototype_amd as pa
    sc = _scalars()
    for base in (J.GENERATOR, ODD):
        b = pa.JubJubBase(ctx, base)
        try:
            assert pa.jubjub_mul(ctx, [base] * NMAX, sc).tobytes() == b.mul(sc).tobytes()
        finally:
            b.free()


# ---------------------------------------------------------------------------------- 4. more than one block
def test_many_waves(ctx):
    """n = 2^14 with scalars and points of period 97: every lane of 256 waves against 97 results of the model"""
    import plonk_prototype_amd as pa
    n, period = 1 << 14, 97
    rng = random.Random(97)
    pts = J.edge_points(extra=2)
    sc = [rng.randrange(R) for _ in range(period)]
    bl = [rng.randrange(R) for _ in range(period)]
    ps = [pts[i % len(pts)] for i in range(period)]
    tile = lambda a: (a * (n // period + 1))[:n]   # noqa: E731
    g, h = pa.JubJubBase(ctx, J.GENERATOR), pa.JubJubBase(ctx, ODD)
    try:
        fixed = [J.mul(J.GENERATOR, s) for s in sc]
        _same(g.mul(_mont(tile(sc))), tile(fixed), "fixed base")
        commit = [J.add(f, J.mul(ODD, b)) for f, b in zip(fixed, bl)]
        _same(pa.jubjub_commit(g, h, _mont(tile(sc)), _mont(tile(bl))), tile(commit), "commit")
        var = [J.mul(p, s) for p, s in zip(ps, sc)]
        _same(pa.jubjub_mul(ctx, J.to_limbs(tile(ps)), _mont(tile(sc))), tile(var), "variable base")
    finally:
        g.free(), h.free()


def test_variable_base_walks_n_in_strides(ctx):
    """more products than the grid holds threads: the kernel's own loop takes a second round, a full wave and a ragged one, in place"""
    import plonk_prototype_amd as pa
    stride = C.c_size_t()
    assert ctx._lib.pm_test_schnorr_stride(ctx._h, C.byref(stride)) == 0     # the one grid of the calls with a slot a thread
    T = stride.value
    assert T >= 64 and T % 64 == 0
    n, period = T + 65, 64
    rng = random.Random(64)
    pts = J.edge_points(extra=2)
    ps = [pts[i % len(pts)] for i in range(period)]
    sc = [rng.randrange(R) for _ in range(period)]
    want = J.to_limbs([J.mul(p, s) for p, s in zip(ps, sc)])
    tile = lambda a: np.tile(a, (n // period + 1,) + (1,) * (a.ndim - 1))[:n]   # noqa: E731
    dp, ds = pa.DeviceVector.from_host(ctx, tile(J.to_limbs(ps))), pa.DeviceVector.from_host(ctx, tile(_mont(sc)))
    try:
        pa.jubjub_mul_dev(ctx, dp.ptr, ds.ptr, n, dp.ptr)                      # out = the points
        got = dp.to_host().reshape(n, 2, 4)
    finally:
        dp.free(), ds.free()
    if got.tobytes() != tile(want).tobytes():
        bad = np.flatnonzero((got != tile(want)).any(axis=(1, 2)))
        raise AssertionError(f"{bad.size} of {n} products differ from 64 of the model's, tiled; first {bad[:8]}, T = {T}")


# ---------------------------------------------------------------------------------- 5. the point check
def test_check(ctx):
    import plonk_prototype_amd as pa
    pts = J.edge_points()
    good = J.to_limbs([pts[i % len(pts)] for i in range(130)])
    assert pa.jubjub_check(ctx, good) is None
    bad = good.copy()
    for i in (5, 70, 129):
        bad[i] = J.to_limbs([(pts[0][0], pts[0][1] + 1 + i)])[0]
        assert not J.on_curve((pts[0][0], pts[0][1] + 1 + i))
    assert pa.jubjub_check(ctx, bad) == 5
    assert pa.jubjub_check(ctx, bad[6:]) == 64 and pa.jubjub_check(ctx, bad[71:]) == 58 and pa.jubjub_check(ctx, bad[:5]) is None
    # the identity with y = 1 + r (as a Montgomery element): on the curve modulo r, not canonical
    nc = good.copy()
    y = int.from_bytes(J.to_limbs([J.IDENTITY])[0, 1].tobytes(), "little") + R
    assert y < 1 << 256
    nc[77] = np.stack([np.zeros(4, np.uint64), np.frombuffer(y.to_bytes(32, "little"), dtype=np.uint64)])
    assert pa.jubjub_check(ctx, nc) == 77
    assert pa.jubjub_check(ctx, np.zeros((0, 2, 4), np.uint64)) is None       # n = 0
    bad_first = C.c_size_t(123)
    assert ctx._lib.pm_jubjub_check_dev(ctx._h, None, 0, C.byref(bad_first), None) == 0 and bad_first.value == 0


# ---------------------------------------------------------------------------------- 6. native equals in-circuit
def test_from_key_equals_the_filled_gadget(ctx):
    import plonk_prototype_amd as pa
    rounds = 256
    b = M.Builder(512)
    sx, sy, s, v = b.var(True), b.var(True), b.var(True), b.var(True)
    out_x, out_y = b.fixed_base(s, rounds, (sx, sy))             # gadget 0
    b.range(v, 1)                                                # gadget 1: another kind
    arith = b.fill_arithmetic(5)
    rng = random.Random(250)
    scalars = [0, 1, (1 << 250) - 1, rng.getrandbits(250), rng.getrandbits(250), rng.getrandbits(200)]
    assignments = [{sx: 0, sy: 1, s: k, v: 0x5a, **arith} for k in scalars]
    pk = pa.preprocess(b.circuit(), ctx)
    try:
        assert pk.set_gadgets(b.gadget_records()) > 0
        models = [b.model(a) for a in assignments]
        assert not any(m[2] for m in models)
        filled, reports = pk.fill_gadgets([M.to_limbs(only) for only, _, _ in models])
        assert all(r.ok for r in reports)
        base = pa.JubJubBase.from_key(pk, 0)
        assert base.point.tobytes() == J.to_limbs([M.base_table(1)[0]])[0].tobytes()
        got = base.mul(scalars)
        assert got.tobytes() == np.stack([filled[:, out_x], filled[:, out_y]], axis=1).tobytes()
        _same(got, [J.mul(M.base_table(1)[0], k) for k in scalars], "against the model")
        with pytest.raises(pa.Error):
            pa.JubJubBase.from_key(pk, 1)                        # a RANGE gadget
        with pytest.raises(pa.Error):
            pa.JubJubBase.from_key(pk, 2)                        # no such gadget
        pk.set_gadgets([])
        _same(base.mul(scalars[:2]), [J.IDENTITY, M.base_table(1)[0]], "after the key's table is gone")
        base.free()
    finally:
        pk.free()


# ---------------------------------------------------------------------------------- 7. a commitment into Poseidon, on the device
def test_commit_into_poseidon_on_the_device(ctx):
    import plonk_prototype_amd as pa
    shape = (5, 2)
    ark, mds = PM.constants(shape[0], 1, 77)
    a, m, _ = PM.flat(ark, mds)
    hades = pa.Hades(ctx, PM.to_limbs(a), PM.to_limbs(m), *shape)
    g, h = pa.JubJubBase(ctx, J.GENERATOR), pa.JubJubBase(ctx, ODD)
    n = 5
    rng = random.Random(7)
    v, bl = [rng.randrange(1 << 64) for _ in range(n)], [rng.randrange(R) for _ in range(n)]
    dv, db = pa.DeviceVector.from_host(ctx, _mont(v)), pa.DeviceVector.from_host(ctx, _mont(bl))
    points, hashes = pa.DeviceVector(ctx, 2 * n), pa.DeviceVector(ctx, n)
    try:
        pa.jubjub_commit_dev(g, h, dv.ptr, db.ptr, n, points.ptr)
        hades.hash_dev(points.ptr, 2, n, hashes.ptr, form="thread")
        commitments = [J.add(J.mul(J.GENERATOR, x), J.mul(ODD, y)) for x, y in zip(v, bl)]
        want = PM.to_limbs([PM.sponge(list(c), ark, mds, *shape) for c in commitments])
        assert hashes.to_host().tobytes() == want.tobytes()
        assert pa.jubjub_check(ctx, points) is None
    finally:
        for x in (dv, db, points, hashes, g, h, hades):
            x.free()


# ---------------------------------------------------------------------------------- 8. streams, n = 0, NULL
def test_streams_zero_and_null(ctx):
    import plonk_prototype_amd as pa
    import torch
    from plonk_prototype_amd import _lib
    n = 65
    sc, (ps, ss, _) = _scalars(n), _var_case()
    g, h = pa.JubJubBase(ctx, J.GENERATOR), pa.JubJubBase(ctx, ODD)
    ds, ds2 = pa.DeviceVector.from_host(ctx, _mont(sc)), pa.DeviceVector.from_host(ctx, _mont(ss[:n]))
    dp = pa.DeviceVector.from_host(ctx, J.to_limbs(ps[:n]))
    outs = [pa.DeviceVector(ctx, 2 * n) for _ in range(6)]
    try:
        st = torch.cuda.Stream()
        for k, stream in enumerate((0, st.cuda_stream)):
            g.mul_dev(ds.ptr, n, outs[3 * k].ptr, stream=stream)
            pa.jubjub_commit_dev(g, h, ds.ptr, ds2.ptr, n, outs[3 * k + 1].ptr, stream=stream)
            pa.jubjub_mul_dev(ctx, dp.ptr, ds2.ptr, n, outs[3 * k + 2].ptr, stream=stream)
        st.synchronize()
        ctx.sync()
        for k in range(3):
            assert outs[k].to_host().tobytes() == outs[3 + k].to_host().tobytes(), k
        _same(outs[0].to_host().reshape(n, 2, 4), _products(J.GENERATOR)[:n], "fixed base on the context's stream")
        # n = 0: PM_OK, nothing written
        before = outs[0].to_host().tobytes()
        lib, c, OK, BAD = ctx._lib, ctx._h, _lib.PM_OK, _lib.PM_ERR_BAD_ARG
        vp = lambda d: C.c_void_p(d.ptr)   # noqa: E731
        assert lib.pm_jubjub_fixed_mul_dev(c, g._h, vp(ds), 0, 0, vp(outs[0]), None) == OK
        assert lib.pm_jubjub_commit_dev(c, g._h, h._h, vp(ds), vp(ds2), 0, 0, vp(outs[0]), None) == OK
        assert lib.pm_jubjub_mul_dev(c, vp(dp), vp(ds), 0, 0, vp(outs[0]), None) == OK
        assert outs[0].to_host().tobytes() == before
        # NULL and an unknown scalar form
        assert lib.pm_jubjub_fixed_mul_dev(c, None, vp(ds), n, 0, vp(outs[0]), None) == BAD
        assert lib.pm_jubjub_fixed_mul_dev(c, g._h, None, n, 0, vp(outs[0]), None) == BAD
        assert lib.pm_jubjub_fixed_mul_dev(c, g._h, vp(ds), n, 0, None, None) == BAD
        assert lib.pm_jubjub_fixed_mul_dev(c, g._h, vp(ds), n, 2, vp(outs[0]), None) == BAD
        assert lib.pm_jubjub_commit_dev(c, g._h, None, vp(ds), vp(ds2), n, 0, vp(outs[0]), None) == BAD
        assert lib.pm_jubjub_commit_dev(c, g._h, h._h, vp(ds), None, n, 0, vp(outs[0]), None) == BAD
        assert lib.pm_jubjub_commit_dev(c, g._h, h._h, vp(ds), vp(ds2), n, 7, vp(outs[0]), None) == BAD
        assert lib.pm_jubjub_mul_dev(c, None, vp(ds), n, 0, vp(outs[0]), None) == BAD
        assert lib.pm_jubjub_mul_dev(c, vp(dp), vp(ds), n, 2, vp(outs[0]), None) == BAD
        assert lib.pm_jubjub_check_dev(c, vp(dp), n, None, None) == BAD
        assert outs[0].to_host().tobytes() == before
    finally:
        for x in [g, h, ds, ds2, dp] + outs:
            x.free()
