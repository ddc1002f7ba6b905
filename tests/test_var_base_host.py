"""Host-side ground for the variable-base scalar multiplication gadget: the constant is the header's,
the ``Gadget`` constructor gives the record the header describes, ``pm_plonk_gadget_rows`` counts 6 R, and the big-integer model
of tests/var_base_model.py satisfies the widget and arithmetic identities of every circuit that tests/test_gpu_var_base.py fills
on the device, equals an independent double-and-add and agrees with the fixed-base model.  No device compute here."""
import os
import random
import re
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gadget_model as M  # noqa: E402
import var_base_circuits as VC  # noqa: E402
import var_base_model as VM  # noqa: E402

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "plonk_mi355x.h")
R = VM.R


def test_constants_match_the_header():
    from plonk_prototype_amd import _lib
    text = open(HEADER).read()
    assert int(re.search(r"#define PM_PLONK_GADGET_VAR_BASE \((\d+)u\)", text).group(1)) == _lib.PLONK_GADGET_VAR_BASE == 10
    assert int(re.search(r"#define PM_PLONK_GADGET_MAX_ROUNDS (\d+)u", text).group(1)) == VM.MAX_ROUNDS == 256
    assert _lib.PLONK_CHAIN_KINDS == {10: "variable_base"}
    # no new reason: a report packs it into two bits
    assert _lib.PLONK_GADGET_REASONS == {1: "too_wide", 2: "scalar_too_long", 3: "degenerate"}


def test_constructor_and_raw():
    import plonk_prototype_amd as pa
    g = pa.Gadget.variable_base(40)
    assert (g.kind, g.first_row, g.count, g.level, g.param, g.in_vars) == (10, 40, 252, 0, 0, ())
    g = pa.Gadget.variable_base(9, rounds=5, level=3)
    assert (g.kind, g.first_row, g.count, g.level, g.param, g.in_vars) == (10, 9, 5, 3, 0, ())
    raw = g._raw()
    assert (raw.kind, raw.level, raw.first_row, raw.count, raw.param, list(raw.in_var)) == (10, 3, 9, 5, 0, [0xFFFFFFFF, 0xFFFFFFFF])
    rep = pa.GadgetReport(ok=False, failed=1, first_gadget=0, first_reason="degenerate")
    assert "(variable_base at row 9)" in str(pa.GadgetInputError({0: rep}, [g]))
    assert "(kind 8 at row 3)" in str(pa.GadgetInputError({0: rep}, [pa.Gadget(8, 3)]))


def test_gadget_rows():
    import plonk_prototype_amd as pa
    G = pa.Gadget
    for rounds in (1, 2, 5, 63, 64, 65, 129, 252, 256):
        assert G.variable_base(0, rounds).rows == 6 * rounds == VM.ROWS_PER_ROUND * rounds
    assert G.variable_base(7).rows == 1512
    assert G.variable_base(0, 0).rows == 0 and G.variable_base(0, 257).rows == 0 and G.variable_base(0, 0xFFFFFFFF).rows == 0
    # 8 and 9 are still no kinds
    assert G(8, 0, 1).rows == 0 and G(9, 0, 1).rows == 0 and G(11, 0, 1).rows == 0


def test_model_against_the_law_by_hand():
    """one round with the bit set and one without, written out"""
    rng = random.Random(7)
    p, s = M.curve_point(rng.randrange(R)), M.curve_point(rng.randrange(R))
    (r1,), reason = VM.var_base_trace([1], s, p)
    dbl = M.jubjub_add(s, s)
    assert reason is None and r1["dbl"] == dbl and r1["new"] == M.jubjub_add(dbl, p) and (r1["sx"], r1["sy"]) == p
    assert r1["d_dbl"] == s[0] * s[1] % R and r1["d_add"] == dbl[0] * p[1] % R
    (r0,), reason = VM.var_base_trace([0], s, p)
    assert reason is None and r0["new"] == dbl == r0["dbl"] and (r0["sx"], r0["sy"]) == (0, 1) and r0["d_add"] == dbl[0]
    # the select values are exact for any value of the bit; such a value is reported
    (rw,), reason = VM.var_base_trace([5], s, p)
    assert reason == VM.TOO_WIDE and rw["sx"] == 5 * p[0] % R and rw["sy"] == (5 * p[1] - 4) % R and rw["new"] is None


@pytest.mark.parametrize("rounds", [1, 5, 64, 252, 256])
def test_model_equals_an_independent_double_and_add(rounds):
    rng = random.Random(rounds)
    p, s = M.curve_point(rng.randrange(R)), M.curve_point(rng.randrange(R))
    for scalar in (0, 1, (1 << rounds) - 1, 1 << (rounds - 1), rng.randrange(1 << rounds)):
        assert VM.var_base_model(scalar, rounds, M.IDENTITY, p) == VM.double_and_add(scalar, p)
        assert VM.var_base_model(scalar, rounds, s, p) == VM.double_and_add(scalar, p, s, rounds)     # 2^R S + s P


def test_model_equals_the_fixed_base_model():
    rng = random.Random(11)
    base = M.base_table(252)
    table = [base[252 - 1 - k] for k in range(252)]
    for scalar in (rng.randrange(1 << 251), (1 << 251) - 1, 1, 0):
        pts, _, _, reason = M.fixed_base_model(scalar, 252, M.IDENTITY, table)
        assert reason is None and pts[-1] == VM.var_base_model(scalar, 252, M.IDENTITY, base[0])


def _assert_satisfied(b, models, skip=()):
    for only, full, reasons in models:
        assert not reasons
        assert [i for i in b.arithmetic_failures(full) if i not in skip] == [] and b.var_rows_failures(full) == []
        assert b.arithmetic_failures(only) != [] or b.var_rows_failures(only) != []     # the inputs alone do not satisfy the rows


def test_model_satisfies_the_circuits_of_the_gpu_tests():
    b, _, models, inputs = VC.shapes_case()
    assert len(models) == 64 and [g[3] for g in b.gadgets if g[0] == "var_base"] == list(VC.SHAPES_A)
    assert len(set(g[1] for g in b.gadgets)) == 1 and min(g[2] for g in b.gadgets if g[0] == "var_base") > 0
    _assert_satisfied(b, models[:8] + models[36:44])
    # the last (a, b) of every chain is 2^R S + s P
    for (only, full, _), (scalars, p, s) in list(zip(models, inputs))[:44:3]:
        for (r0, rounds, x, y), scalar in zip(b.chains, scalars):
            if M.on_curve(p) and M.on_curve(s):
                assert (full[x], full[y]) == VM.double_and_add(scalar, p, s, rounds)
    b, _, models, _ = VC.shapes_case(VC.SHAPES_B, 64, 47)
    assert b.n == 2048 and [g[3] for g in b.gadgets if g[0] == "var_base"] == [256]
    _assert_satisfied(b, models[::7])
    b, a, decoys = VC.refusal_case()
    only, full, reasons = b.model(a)
    assert not reasons and len(decoys) >= 30
    bad = set(b.arithmetic_failures(full)) | set(b.var_rows_failures(full))     # everything but the rows nobody fills
    assert bad and all(any(r0 <= i < r0 + 12 for r0 in decoys.values()) for i in bad)


@pytest.mark.parametrize("rounds", [5, 252])
def test_model_equals_the_composed_form(rounds):
    (b1, a1, m1), (b2, a2, m2) = VC.cross_case(rounds)
    assert [g[0] for g in b1.gadgets] == ["arith", "var_base"]
    assert [g[0] for g in b2.gadgets] == ["arith"] + ["curve_add", "arith", "curve_add"] * rounds
    assert len(set(g[1] for g in b2.gadgets)) == 2 * rounds
    assert a1 == a2 and [m[1] for m in m1] == [m[1] for m in m2] and [m[0] for m in m1] == [m[0] for m in m2]
    _assert_satisfied(b1, m1)


def test_dusk_and_fixed_base_circuits():
    b, inputs, out, pi_rows = VC.dusk_case()
    assert b.n == 2048 and [(g[0], g[1], g[3]) for g in b.gadgets] == [("bits", 0, 252), ("var_base", 1, 252)]
    a = inputs(1)
    model = b.model(a)
    _assert_satisfied(b, [model], skip=pi_rows)
    assert sorted(b.arithmetic_failures(model[1])) == sorted(pi_rows)
    s_var, px, py = b.gadgets[0][5][0], b.wires[1][b.chains[0][0] + 2], b.wires[1][b.chains[0][0] + 3]
    assert (model[1][out[0]], model[1][out[1]]) == VM.double_and_add(a[s_var], (a[px], a[py]))
    b, assignments, models, fixed, variable, scalars = VC.fixed_base_case()
    for (only, full, reasons), scalar in zip(models, scalars):
        assert not reasons and scalar < 1 << 251
        assert (full[fixed[0]], full[fixed[1]]) == (full[variable[0]], full[variable[1]]) == VM.double_and_add(scalar, M.base_table(1)[0])


def test_report_models():
    b, assignments, models = VC.report_case()
    assert [m[2] for m in models] == [{}, {0: VM.TOO_WIDE}, {0: VM.DEGENERATE}]
    # the select rows hold in all three
    for (only, full, _) in models:
        assert b.arithmetic_failures(full) == []
