"""The memory AROUND a call's buffers, group A: the polynomial and round helpers (csrc/poly.hip, csrc/plonk_rounds.hip).

Every case carves its buffers out of one guard arena (tests/guard_arena.py: one allocation of 0xA5 with a band of 4096 elements
on both sides of every region), calls the entry point with raw addresses, downloads the arena once and asserts three things:
every band is untouched, every input the call may not write equals its upload, and the outputs equal the oracle bit for bit.
The in-place forms the header allows run with the output ON an input; the ragged output of Ruffini is carved at exactly n - 1
elements; the one refusal the header states ("Not in place") is asserted with its code and an unchanged arena."""
import os
import random
import sys
import types

import numpy as np
import pytest

from oracle import bigint_oracle as B
from oracle import plonk_rounds_oracle as PO
from oracle.cpu_oracle import ints_to_limbs

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guard_arena as G  # noqa: E402
import test_gpu_prover as TP  # noqa: E402   (the argument builders of the round kernels)

pytestmark = pytest.mark.gpu
R = B.R_MOD


def _edges(oracle, a, where):
    """0, 1 and r - 1 at the front or the back of a sample"""
    edge = oracle.fr_to_mont(ints_to_limbs([0, 1, R - 1], 4))
    k = min(a.shape[0], 3)
    if where == "front":
        a[:k] = edge[:k]
    else:
        a[a.shape[0] - k:] = edge[:k]
    return a


def _fr(raw, n):
    return G.as_u64(raw, n, 4)


def _mont_vec(oracle, vals):
    return oracle.fr_to_mont(ints_to_limbs([v % R for v in vals], 4))


# ---------------------------------------------------------------------------------- the arena itself, on the device
def test_the_arena_sees_a_stray_write(ctx, oracle):
    """what every case below relies on: bytes the HOST writes next to a region (pm_dev_upload: no kernel misbehaves here) are
    found by `check` and named with region, side, offset and count; an untouched arena passes, a changed input does not"""
    import ctypes as C
    a = oracle.fr_sample(1, 7)
    stray = np.zeros(32, np.uint8)

    def poke(ar, address):
        ctx._check(ctx._lib.pm_dev_upload(ctx._h, C.c_void_p(address), stray.ctypes.data_as(C.c_void_p), 32))

    with G.GuardArena.of(ctx, a=a, out=32 * 6) as ar:
        assert G.untouched(ar.check()["out"])
        ar.check_unchanged()
        poke(ar, ar.addr("out") + 32 * 6)                   # slot n - 1 of an output of n - 1 elements
        with pytest.raises(AssertionError, match=r"32 byte\(s\) changed behind 'out', the first at offset \+192 "):
            ar.check()
    with G.GuardArena.of(ctx, a=a, out=32 * 6) as ar:
        poke(ar, ar.addr("a") - 32)
        with pytest.raises(AssertionError, match=r"32 byte\(s\) changed in front of 'a', the first at offset -32 "):
            ar.check()
    with G.GuardArena.of(ctx, a=a, out=32 * 6) as ar:
        poke(ar, ar.addr("a") + 64)
        with pytest.raises(AssertionError, match=r"32 byte\(s\) changed inside the read-only region 'a', the first at offset \+64 "):
            ar.check()
        assert np.array_equal(_fr(ar.check(written={"a"})["a"], 7)[[0, 1, 3]], a[[0, 1, 3]])
    with G.GuardArena.of(ctx, a=a, out=32 * 6) as ar:
        poke(ar, ar.addr("out"))                            # an output of a REFUSED call has to stay 0xA5 too
        assert not G.untouched(ar.check()["out"])
        with pytest.raises(AssertionError, match="inside the read-only region 'out'"):
            ar.check_unchanged()


# ---------------------------------------------------------------------------------- pm_fr_vec_op_dev
VEC_LAYOUTS = ("distinct", "out_is_a", "out_is_b", "all_one", "scalar_b_out_is_a")


@pytest.mark.parametrize("layout", VEC_LAYOUTS)
@pytest.mark.parametrize("n", [1, 255, 256, 257, 5000])
def test_vec_op(ctx, oracle, n, layout):
    """"In place allowed": out on a, on b, on both; a one-element b broadcast into a"""
    a = _edges(oracle, oracle.fr_sample(1, n), "front")
    b = _edges(oracle, oracle.fr_sample(2, n), "back")
    for op in (0, 1, 2):
        if layout == "distinct":
            ar = G.GuardArena.of(ctx, a=a, b=b, out=32 * n)
            pa_, pb_, po, blen, out, want = "a", "b", "out", n, "out", oracle.fr_vec_op(op, a, b)
        elif layout == "out_is_a":
            ar = G.GuardArena.of(ctx, a=a, b=b)
            pa_, pb_, po, blen, out, want = "a", "b", "a", n, "a", oracle.fr_vec_op(op, a, b)
        elif layout == "out_is_b":
            ar = G.GuardArena.of(ctx, a=a, b=b)
            pa_, pb_, po, blen, out, want = "a", "b", "b", n, "b", oracle.fr_vec_op(op, a, b)
        elif layout == "all_one":
            ar = G.GuardArena.of(ctx, a=a)
            pa_, pb_, po, blen, out, want = "a", "a", "a", n, "a", oracle.fr_vec_op(op, a, a)
        else:
            ar = G.GuardArena.of(ctx, a=a, b=b[-1:].copy())
            pa_, pb_, po, blen, out, want = "a", "b", "a", 1, "a", oracle.fr_vec_op(op, a, b[-1:])
        with ar:
            ctx.fr_vec_op(op, ar.addr(pa_), ar.addr(pb_), blen, ar.addr(po), n)
            got = ar.check(written={out})            # every region but `out` is an unchanged input
            assert np.array_equal(_fr(got[out], n), want), (n, layout, op)


# ---------------------------------------------------------------------------------- pm_fr_prefix_product_dev
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("n", [1, 7, 2047, 2048, 2049, 4097, 70001])
def test_prefix_product(ctx, oracle, n, mode):
    """"In place allowed", under each value of the option poly_lookback: 0 = the chunked scan (one level up to 2048 elements,
    three at 70001), 1 = the library's rule and 2 = the one-pass look-back from 2049 elements on.  (The chunked scan with a
    look-back TOP level needs more than 2^20 elements: out of reach of a test of this size.)"""
    a = oracle.fr_sample(21 + n, n)
    if n == 70001:
        a[n // 2] = 0                                       # everything after a zero factor is zero
    want = oracle.fr_prefix_product(a)
    try:
        ctx.set_option("poly_lookback", mode)
        with G.GuardArena.of(ctx, a=a, out=32 * n) as ar:
            ctx.fr_prefix_product(ar.addr("a"), n, ar.addr("out"))
            assert np.array_equal(_fr(ar.check()["out"], n), want), (n, mode, "out of place")
        with G.GuardArena.of(ctx, a=a) as ar:
            ctx.fr_prefix_product(ar.addr("a"), n, ar.addr("a"))
            assert np.array_equal(_fr(ar.check(written={"a"})["a"], n), want), (n, mode, "in place")
    finally:
        ctx.set_option("poly_lookback", 1)


# ---------------------------------------------------------------------------------- pm_fr_poly_ruffini_dev
def _ruffini_points(oracle):
    return {"random": oracle.fr_sample(9, 1)[0], "zero": np.zeros(4, np.uint64),
            "one": _mont_vec(oracle, [1])[0], "minus_one": _mont_vec(oracle, [R - 1])[0]}


@pytest.mark.parametrize("n", [2, 3, 2048, 2049, 2050, 4097])
def test_ruffini_ragged_output(ctx, oracle, n):
    """n - 1 coefficients from kernels that work in tiles of 2048: the output region is EXACTLY n - 1 elements, so a write to
    slot n - 1 lands in the band behind it"""
    c = oracle.fr_sample(7 + n, n)
    for name, z in _ruffini_points(oracle).items():
        with G.GuardArena.of(ctx, c=c, out=32 * (n - 1)) as ar:
            ctx.fr_ruffini(ar.addr("c"), n, z, ar.addr("out"))
            got = ar.check()
            assert np.array_equal(_fr(got["out"], n - 1), oracle.fr_poly_ruffini(c, z)), (n, name)


@pytest.mark.parametrize("n", [2, 2049])
def test_ruffini_refuses_in_place(ctx, oracle, n):
    """"Not in place": PM_ERR_BAD_ARG, and no byte of the arena changes"""
    import plonk_prototype_amd as pa
    c = oracle.fr_sample(7 + n, n)
    for name, z in _ruffini_points(oracle).items():
        with G.GuardArena.of(ctx, c=c) as ar:
            with pytest.raises(pa.Error) as e:
                ctx.fr_ruffini(ar.addr("c"), n, z, ar.addr("c"))
            assert e.value.code == pa._lib.PM_ERR_BAD_ARG, name
            ar.check_unchanged()


# ---------------------------------------------------------------------------------- pm_fr_batch_inverse_dev
@pytest.mark.parametrize("n,quads", [(1, 0), (3, 1), (63, 0), (65, 0), (1000, 3), (5000, 7)])
def test_batch_inverse(ctx, oracle, n, quads):
    a = oracle.fr_sample(11 + n, n)
    a[:: max(1, n // 7)] = 0                                # zeros stay zero
    if n > 5:
        a[5], a[4] = _mont_vec(oracle, [1])[0], _mont_vec(oracle, [R - 1])[0]
    ctx.set_option("binv_quads", quads)
    try:
        with G.GuardArena.of(ctx, a=a) as ar:
            ctx.fr_batch_inverse(ar.addr("a"), n)
            assert np.array_equal(_fr(ar.check(written={"a"})["a"], n), oracle.fr_batch_inverse(a)), (n, quads)
    finally:
        ctx.set_option("binv_quads", 0)


# ---------------------------------------------------------------------------------- pm_fr_powers_dev, pm_fr_lincomb_dev
@pytest.mark.parametrize("n", [1, 255, 257, 4097, 70001])
def test_powers(ctx, oracle, n):
    base, scale = oracle.fr_sample(31 + n, 2)
    with G.GuardArena.of(ctx, out=32 * n) as ar:
        ctx.fr_powers(base, scale, n, ar.addr("out"))
        assert np.array_equal(_fr(ar.check()["out"], n), oracle.fr_powers(base, scale, n)), n


@pytest.mark.parametrize("n", [1, 257, 5000])
@pytest.mark.parametrize("k", [1, 2, 16])
def test_lincomb(ctx, oracle, k, n):
    vecs = [oracle.fr_sample(100 * k + j, n) for j in range(k)]
    coeffs = oracle.fr_sample(77 + k, k)
    if k > 2:
        coeffs[1], coeffs[2] = 0, _mont_vec(oracle, [R - 1])[0]
    with G.GuardArena.of(ctx, **{f"v{j}": v for j, v in enumerate(vecs)}, out=32 * n) as ar:
        ctx.fr_lincomb([ar.addr(f"v{j}") for j in range(k)], coeffs, n, ar.addr("out"))
        assert np.array_equal(_fr(ar.check()["out"], n), oracle.fr_lincomb(coeffs, vecs)), (k, n)


# ---------------------------------------------------------------------------------- pm_plonk_perm_terms_dev, pm_plonk_quotient_dev
def _handle(ar, name):
    """what the argument builders of tests/test_gpu_prover.py take for a device vector"""
    return types.SimpleNamespace(ptr=ar.addr(name))


@pytest.mark.parametrize("n", [1, 257, 300])
def test_perm_terms(ctx, oracle, n):
    import plonk_prototype_amd as pa
    rng = random.Random(n)
    wires, sigmas, roots = [TP._rand(rng, n) for _ in range(4)], [TP._rand(rng, n) for _ in range(4)], TP._rand(rng, n)
    wires[0][0], sigmas[1][0] = 0, R - 1
    beta, gamma = rng.randrange(R), rng.randrange(R)
    regions = {f"w{j}": _mont_vec(oracle, wires[j]) for j in range(4)}
    regions.update({f"s{j}": _mont_vec(oracle, sigmas[j]) for j in range(4)})
    with G.GuardArena.of(ctx, **regions, roots=_mont_vec(oracle, roots), num=32 * n, den=32 * n) as ar:
        args = TP._perm_args(pa, oracle, [_handle(ar, f"w{j}") for j in range(4)], [_handle(ar, f"s{j}") for j in range(4)],
                             _handle(ar, "roots"), beta, gamma)
        ctx.plonk_perm_terms(args, n, ar.addr("num"), ar.addr("den"))
        got = ar.check()                                  # all nine inputs unchanged
        en, ed = PO.perm_terms(wires, sigmas, roots, beta, gamma)
        assert np.array_equal(_fr(got["num"], n), _mont_vec(oracle, en))
        assert np.array_equal(_fr(got["den"], n), _mont_vec(oracle, ed))


def test_quotient_with_every_widget(ctx, oracle):
    import plonk_prototype_amd as pa
    n, widgets = 64, ("q_arith", "q_range", "q_logic", "q_fixed_group_add", "q_variable_group_add")
    rng = random.Random(n + 7 * len(widgets))
    n4 = 4 * n
    names = ["w0", "w1", "w2", "w3", "z", "q_m", "q_l", "q_r", "q_o", "q_4", "q_c", "pi", "s0", "s1", "s2", "s3", "l1"]
    v = {k: TP._rand(rng, n4) for k in names + list(widgets)}
    v["q_m"][0], v["z"][1], v["w0"][2] = 0, 1, R - 1
    x = PO.powers(B.Domain(n4).group_gen, 7, n4)
    ch = {k: rng.randrange(R) for k in PO.CHALLENGES}
    with G.GuardArena.of(ctx, **{k: _mont_vec(oracle, val) for k, val in v.items()}, x=_mont_vec(oracle, x), out=32 * n4) as ar:
        d = {k: _handle(ar, k) for k in v}
        ctx.plonk_quotient(TP._quotient_args(pa, oracle, d, _handle(ar, "x"), x, n, ch, widgets), n, ar.addr("out"))
        got = ar.check()                                  # the 23 input vectors unchanged, the 4n outputs and nothing else written
    sel = {k: v[k] for k in ("q_m", "q_l", "q_r", "q_o", "q_4", "q_c", "q_arith") + tuple(PO.WIDGET_SELECTORS)}
    exp = PO.quotient_evals(n, [v[f"w{j}"] for j in range(4)], v["z"], sel, v["pi"], [v[f"s{j}"] for j in range(4)], v["l1"], x, ch)
    assert np.array_equal(_fr(got["out"], n4), _mont_vec(oracle, exp))


# ---------------------------------------------------------------------------------- pm_fr_poly_evaluate_many_dev
@pytest.mark.parametrize("n", [1, 257, 4097])
def test_evaluate_many_reads_only(ctx, oracle, n):
    """the results go to the host: the point here is that the 16 inputs and everything around them stay as they were"""
    k = 16
    polys = [oracle.fr_sample(200 + j, n) for j in range(k)]
    pt = oracle.fr_sample(12, 1)[0]
    with G.GuardArena.of(ctx, **{f"p{j}": p for j, p in enumerate(polys)}) as ar:
        got = ctx.fr_evaluate_many([ar.addr(f"p{j}") for j in range(k)], n, pt)
        assert ar.check() == {}
    assert np.array_equal(got, np.stack([oracle.fr_poly_evaluate(p, pt) for p in polys]))


# ---------------------------------------------------------------------------------- the EvaluationDomain helpers, device forms
@pytest.mark.parametrize("log_n", [0, 1, 8, 11])
def test_domain_helpers(ctx, oracle, log_n):
    import ctypes as C
    from plonk_prototype_amd import _lib
    n = 1 << log_n
    ref, rng = B.Domain(n), random.Random(7 + log_n)
    for deg in sorted(d for d in {0, 1, n // 4, n - 1} if d < n):
        with G.GuardArena.of(ctx, out=32 * n) as ar:
            ctx._check(ctx._lib.pm_domain_vanishing_poly_over_coset_dev(ctx._h, log_n, deg, C.c_void_p(ar.addr("out")), None))
            assert np.array_equal(_fr(ar.check()["out"], n), _mont_vec(oracle, ref.compute_vanishing_poly_over_coset(deg))), deg
    for tau in (rng.randrange(R), ref.group_gen, pow(ref.group_gen, n - 1, R), 1):
        t = _mont_vec(oracle, [tau])[0]
        with G.GuardArena.of(ctx, out=32 * n) as ar:
            ctx._check(ctx._lib.pm_domain_evaluate_all_lagrange_coefficients_dev(ctx._h, log_n, t.ctypes.data_as(_lib.u64p),
                                                                                C.c_void_p(ar.addr("out")), None))
            assert np.array_equal(_fr(ar.check()["out"], n), _mont_vec(oracle, ref.evaluate_all_lagrange_coefficients(tau))), tau
