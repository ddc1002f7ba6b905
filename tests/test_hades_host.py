"""Host-side ground for the HADES gadget kind: the constants are the header's, the ``Gadget``
constructor gives the record the header describes, ``pm_plonk_gadget_rows`` counts the rows of every kind, and the big-integer
model of tests/hades_model.py satisfies, row by row, the arithmetic identity of every circuit that tests/test_gpu_hades.py
fills on the device -- and equals the model of the same rows taken as an ARITH run.  No device compute here."""
import os
import random
import re
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hades_circuits as HC  # noqa: E402
import hades_model as HM  # noqa: E402

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "plonk_mi355x.h")
R = HM.R


def test_constants_match_the_header():
    from plonk_prototype_amd import _lib
    text = open(HEADER).read()
    assert int(re.search(r"#define PM_PLONK_PERMUTATION_HADES (\d+)u", text).group(1)) == _lib.PLONK_PERMUTATION_HADES == 7
    assert int(re.search(r"#define PM_PLONK_HADES_WIDTH (\d+)u", text).group(1)) == _lib.PLONK_HADES_WIDTH == HM.WIDTH == 5
    assert _lib.PLONK_PERMUTATION_KINDS == {7: "hades"}
    # the lists of the other kinds are as they were
    assert sorted(_lib.PLONK_COMPOSED_KINDS) == [4, 5, 6] and len(_lib.PLONK_GADGET_KINDS) == 4
    assert "pm_plonk_gadget_rows" in _lib.SIGNATURES


def test_constructor_and_raw():
    import plonk_prototype_amd as pa
    g = pa.Gadget.hades(40)
    assert (g.kind, g.first_row, g.count, g.level, g.param, g.in_vars) == (7, 40, 67, 0, 8, ())
    g = pa.Gadget.hades(9, rounds=5, full_rounds=2, level=3)
    assert (g.kind, g.first_row, g.count, g.level, g.param, g.in_vars) == (7, 9, 5, 3, 2, ())
    raw = g._raw()
    assert (raw.kind, raw.level, raw.first_row, raw.count, raw.param, list(raw.in_var)) == (7, 3, 9, 5, 2, [0xFFFFFFFF, 0xFFFFFFFF])
    rep = pa.GadgetReport(ok=False, failed=1, first_gadget=0, first_reason="too_wide")
    assert "(hades at row 9)" in str(pa.GadgetInputError({0: rep}, [g]))
    assert "(kind 9 at row 3)" in str(pa.GadgetInputError({0: rep}, [pa.Gadget(9, 3)]))


def test_gadget_rows_of_every_kind():
    import plonk_prototype_amd as pa
    G = pa.Gadget
    assert G.range(0, 4, 1).rows == 5 and G.logic(0, 7, 1, 2).rows == 8 and G.fixed_base(0, 256, 1).rows == 257
    assert G.curve_add(3).rows == 2 and G.curve_add(3, level=2).rows == 2
    assert G.arith(0, 1).rows == 1 and G.arith(5, 1302).rows == 1302
    assert G.bits(0, 1, 1).rows == 2 and G.bits(0, 256, 1).rows == 512
    assert G.maybe_equal(0).rows == 3
    want = {(1, 0): 18, (2, 2): 60, (5, 2): 114, (67, 8): 1302}
    for (rounds, full), rows in want.items():
        assert G.hades(0, rounds, full).rows == rows == HM.hades_rows(rounds, full)
    assert G.hades(0).rows == 1302
    assert G.hades(0, 3, 0).rows == 54 and G.hades(0, 4, 4).rows == 120
    # 0: an unknown kind, and what set_gadgets refuses without looking at the circuit
    assert G(8, 0, 1).rows == 0 and G(0xFFFFFFFF, 0, 1).rows == 0
    assert G.hades(0, 5, 3).rows == 0 and G.hades(0, 2, 4).rows == 0 and G.hades(0, 0, 0).rows == 0
    assert G.range(0, 0, 1).rows == 0 and G.logic(0, 0, 1, 2).rows == 0 and G.arith(0, 0).rows == 0 and G.bits(0, 0, 1).rows == 0
    assert G.fixed_base(0, 0, 1).rows == 0 and G.fixed_base(0, 257, 1).rows == 0 and G.bits(0, 257, 1).rows == 0
    assert pa.load().pm_plonk_gadget_rows(None) == 0
    # no 32-bit wrap: the largest counts
    assert G.arith(0, 0xFFFFFFFF).rows == 0xFFFFFFFF and G.range(0, 0xFFFFFFFF, 1).rows == 1 << 32
    assert G.hades(0, 0xFFFFFFFF, 0xFFFFFFFE).rows == 30 * 0xFFFFFFFE + 18


def test_model_against_the_definition_by_hand():
    """one partial and one full round written out, and the single-matrix form of the arguments"""
    rng = random.Random(5)
    s = [rng.randrange(R) for _ in range(5)]
    ark = [[rng.randrange(R) for _ in range(5)] for _ in range(2)]
    m = [[rng.randrange(R) for _ in range(5)] for _ in range(5)]
    keyed = [(x + k) % R for x, k in zip(s, ark[0])]
    partial = keyed[:4] + [pow(keyed[4], 5, R)]
    assert HM.hades_model(s, ark[:1], m, 1, 0) == [sum(m[i][j] * partial[j] for j in range(5)) % R for i in range(5)]
    full = [pow(x, 5, R) for x in keyed]
    one = [sum(m[i][j] * full[j] for j in range(5)) % R for i in range(5)]
    keyed2 = [pow((x + k) % R, 5, R) for x, k in zip(one, ark[1])]
    assert HM.hades_model(s, ark, m, 2, 2) == [sum(m[i][j] * keyed2[j] for j in range(5)) % R for i in range(5)]
    assert HM.hades_model(s, ark, [m, m], 2, 2) == HM.hades_model(s, ark, m, 2, 2)
    assert [HM.is_full(r, 67, 8) for r in (0, 3, 4, 62, 63, 66)] == [True, True, False, False, True, True]


def test_builder_lays_the_rows_the_header_counts():
    for rounds, full in HC.SHAPES + (HC.DUSK,):
        b = HM.Builder(2048)
        b.hades([b.var(True) for _ in range(5)], rounds, full)
        assert b.row == HM.hades_rows(rounds, full) == {(1, 0): 18, (2, 2): 60, (5, 2): 114, (4, 0): 72, (67, 8): 1302}[(rounds, full)]
        rec = b.gadget_records()
        assert len(rec) == 1 and (rec[0].kind, rec[0].count, rec[0].param, rec[0].rows) == (7, rounds, full, b.row)


def _assert_satisfied(b, models, skip=()):
    for only, full, reasons in models:
        assert not reasons
        assert [i for i in b.arithmetic_failures(full) if i not in skip] == []
        assert b.arithmetic_failures(only) != []          # the inputs alone do not satisfy the rows


def test_model_satisfies_the_circuits_of_the_gpu_tests():
    b, _, models = HC.shapes_case()
    assert len(models) == 64 and [g[0] for g in b.gadgets].count("hades") == 4 and len(set(g[1] for g in b.gadgets)) == 1
    assert min(g[2] for g in b.gadgets if g[0] == "hades") > 0
    _assert_satisfied(b, models)
    b, inputs, out, pi_row = HC.sponge_case()
    assert [(g[0], g[1]) for g in b.gadgets] == [("arith", 0), ("hades", 1), ("arith", 2), ("hades", 3)]
    assert [g[3] for g in b.gadgets if g[0] == "arith"] == [4, 3]
    model = b.model(inputs(1))
    _assert_satisfied(b, [model], skip=(pi_row,))          # that row holds with its public input, minus the hash
    assert b.arithmetic_failures(model[1]) == [pi_row] and model[1][out] != 0
    b, a, decoys = HC.refusal_case()
    bad = set(b.arithmetic_failures(b.model(a)[1]))       # everything but the rows nobody fills
    assert bad and all(any(r0 <= i < r0 + 18 for r0 in decoys.values()) for i in bad)


def test_rule_decoys_are_each_wrong_in_one_place():
    """hades_circuits.rule_decoys_case: distinct names over the parts, every decoy differs from the rows the builder lays (the
    case asserts that), the good table is satisfied by the model and never claims a decoy"""
    rows, names = HM.hades_rows(*HC.DECOY_SHAPE), []
    assert rows == 96 and HC._ROUND == (0, 30, 48, 66)
    for part in range(HC.RULE_PARTS):
        b, a, decoys = HC.rule_decoys_case(part)
        assert b.n <= 1024 and "good" in decoys and 2 <= len(decoys) <= HC.RULE_DECOYS_PER_CIRCUIT + 1
        names += [k for k in decoys if k != "good"]
        assert [(g[0], g[1], g[3], g[4]) for g in b.gadgets] == [("arith", 0, 1, 0), ("hades", 1, 1, 0), ("hades", 1, 1, 0)]
        claimed_end = max(g[2] for g in b.gadgets) + 18
        assert min(decoys.values()) >= claimed_end
        only, full, reasons = b.model(a)
        assert not reasons
        bad = set(b.arithmetic_failures(full))               # everything but the rows nobody fills
        assert bad and all(any(r0 <= i < r0 + rows for r0 in decoys.values()) for i in bad)
    assert len(set(names)) == len(names) >= 60


@pytest.mark.parametrize("shape", [(5, 2), HC.DUSK])
def test_model_equals_the_arith_form(shape):
    (b1, a1, m1), (b2, a2, m2) = HC.cross_case(*shape)
    assert [g[0] for g in b1.gadgets] == ["arith", "hades"] and [g[0] for g in b2.gadgets] == ["arith", "arith"]
    assert b2.gadgets[1][2] == b1.gadgets[1][2] and b2.gadgets[1][3] == HM.hades_rows(*shape)
    assert a1 == a2 and [m[1] for m in m1] == [m[1] for m in m2] and [m[0] for m in m1] == [m[0] for m in m2]
    _assert_satisfied(b1, m1)
    # ... and the final state is the permutation of the inputs
    r0, rounds, full, ark, mds = b1.permutations[0]
    for _, val, _ in m1:
        state = [val[b1.wires[0][r0 + j]] for j in range(5)]
        last = r0 + HM.hades_rows(rounds, full) - 10
        assert [val[b1.wires[2][last + 2 * i + 1]] for i in range(5)] == HM.hades_model(state, ark, mds, rounds, full)
