"""Host-side ground for the composed gadget kinds (ARITH, BITS, MAYBE_EQUAL): the constants are the
header's, the ``Gadget`` constructors give the records the header describes, and the big-integer model of
tests/composed_gadget_model.py satisfies, row by row, the arithmetic identity of every circuit that
tests/test_gpu_composed_gadgets.py fills on the device.  No device compute here."""
import os
import re
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import composed_gadget_circuits as CC  # noqa: E402
import composed_gadget_model as CM  # noqa: E402

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "plonk_mi355x.h")
R = CM.R


def test_constants_match_the_header():
    from plonk_prototype_amd import _lib
    text = open(HEADER).read()
    header = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define PM_PLONK_COMPOSED_(\w+) (\d+)u", text)}
    assert header == {"ARITH": 4, "BITS": 5, "MAYBE_EQUAL": 6, "MAX_BITS": 256}
    for name, value in header.items():
        assert getattr(_lib, "PLONK_COMPOSED_" + name) == value
    assert {getattr(_lib, "PLONK_COMPOSED_" + nm.upper()): nm for nm in _lib.PLONK_COMPOSED_KINDS.values()} == _lib.PLONK_COMPOSED_KINDS
    assert sorted(_lib.PLONK_COMPOSED_KINDS) == [4, 5, 6]
    assert len(_lib.PLONK_GADGET_KINDS) == 4           # the widget kinds keep their own list


def test_constructors():
    import plonk_prototype_amd as pa
    g = pa.Gadget.arith(7, 3, level=2)
    assert (g.kind, g.first_row, g.count, g.level, g.param, g.in_vars) == (4, 7, 3, 2, 0, ())
    assert list(g._raw().in_var) == [0xFFFFFFFF, 0xFFFFFFFF]
    g = pa.Gadget.bits(10, 64, 5, level=1)
    assert (g.kind, g.first_row, g.count, g.level, g.param, g.in_vars) == (5, 10, 64, 1, 0, (5,))
    raw = g._raw()
    assert (raw.kind, raw.level, raw.first_row, raw.count, raw.param, list(raw.in_var)) == (5, 1, 10, 64, 0, [5, 0xFFFFFFFF])
    g = pa.Gadget.maybe_equal(20, level=4)
    assert (g.kind, g.first_row, g.count, g.level, g.in_vars) == (6, 20, 0, 4, ())
    pair = pa.Gadget.decomposition(100, 255, 9, level=3)
    assert pair == [pa.Gadget.bits(100, 255, 9, level=3), pa.Gadget.maybe_equal(100 + 510, level=4)]
    assert pa.Gadget.decomposition(0, 1, 2) == [pa.Gadget.bits(0, 1, 2, 0), pa.Gadget.maybe_equal(2, 1)]
    # the message of a failing fill names a composed kind without an index error
    rep = pa.GadgetReport(ok=False, failed=1, first_gadget=0, first_reason="too_wide")
    for gadget, name in ((pa.Gadget.bits(3, 8, 1), "bits"), (pa.Gadget.arith(3, 1), "arith"), (pa.Gadget.maybe_equal(3), "maybe_equal"),
                         (pa.Gadget(9, 3), "kind 9")):
        assert f"({name} at row 3)" in str(pa.GadgetInputError({0: rep}, [gadget]))


def test_builder_records_follow_the_layout():
    b, _, _ = CC.refusal_case()
    recs = b.gadget_records()
    assert [g.level for g in recs] == sorted(g.level for g in recs)
    kinds = sorted((g.kind, g.level) for g in recs)
    assert kinds == [(0, 0), (4, 0), (5, 1), (6, 2)]
    bits = next(g for g in recs if g.kind == 5)
    eq = next(g for g in recs if g.kind == 6)
    assert eq.first_row == bits.first_row + 2 * bits.count       # Gadget.decomposition's pair


def _assert_satisfied(b, models, skip=()):
    for _, full, reasons in models:
        assert not reasons
        assert [i for i in b.arithmetic_failures(full) if i not in skip] == []


def test_model_satisfies_the_circuits_of_the_gpu_tests():
    for which in ("small", "full"):
        b, _, models = CC.bits_case(which)
        _assert_satisfied(b, models)
    b, assignments, models, outs = CC.maybe_equal_case()
    _assert_satisfied(b, models)
    for a, (_, full, _) in zip(assignments, models):
        for g, y in enumerate(outs):
            r0 = b.gadgets[g][2]
            x1, x2 = full[b.wires[0][r0]], full[b.wires[1][r0]]
            u, z = full[b.wires[2][r0]], full[b.wires[0][r0 + 1]]
            assert u == (x1 - x2) % R and full[y] == (1 if x1 == x2 else 0)
            assert (z * u % R == 1) if u else z == 0
    b, _, models = CC.arith_case()
    _assert_satisfied(b, models)
    for b, _, models in CC.cross_case():
        _assert_satisfied(b, models)
    same = [m[1] for m in CC.cross_case()[0][2]], [m[1] for m in CC.cross_case()[1][2]]
    assert same[0] == same[1]                                       # the two forms of one decomposition agree in the model
    b, inputs, out = CC.end_to_end_case()
    for value, want in ((CC.RANGE_MIN + 12345, 1), (CC.RANGE_MAX, 0)):
        model = b.model(inputs(value))
        _assert_satisfied(b, [model])
        assert model[1][out] == want
    # the refusal circuit: everything but the rows that are wrong on purpose
    b, a, decoys = CC.refusal_case()
    bad = set(b.arithmetic_failures(b.model(a)[1]))
    assert bad and all(any(r0 <= i < r0 + 8 for r0 in decoys.values()) for i in bad)


def test_rule_decoys_are_each_wrong_in_one_place():
    """composed_gadget_circuits.rule_decoys_case: every decoy differs from the rows its kind lays (the case asserts that), the
    good table holds two gadgets of every composed kind, is satisfied by the model and never claims a decoy"""
    b, a, decoys = CC.rule_decoys_case()
    assert b.n <= 1024 and sorted(g[0] for g in b.gadgets) == ["arith", "arith", "bits", "bits", "maybe_equal", "maybe_equal"]
    rows = {"bits": 2 * CC.DECOY_BITS, "maybe_equal": 3, "arith": 1}
    claimed_end = max(g[2] + 3 for g in b.gadgets)
    spans = [(r0, r0 + rows[kind]) for kind, table in decoys.items() for r0 in table.values()]
    assert min(lo for lo, _ in spans) >= claimed_end and len(set(spans)) == len(spans)
    assert all("good" in table for table in decoys.values())
    assert len(decoys["bits"]) >= 30 and len(decoys["maybe_equal"]) >= 25 and len(decoys["arith"]) == 5
    only, full, reasons = b.model(a)
    assert not reasons
    bad = set(b.arithmetic_failures(full))
    assert bad and all(any(lo <= i < hi for lo, hi in spans) for i in bad)


@pytest.mark.parametrize("bounds", [(CC.RANGE_MIN, CC.RANGE_MAX), (0, 1 << 64), (5, 6), (1, 1 << 31)])
def test_range_check_is_one_inside_the_bounds(bounds):
    lo, hi = bounds
    b, x, out = CC.range_check_circuit(lo, hi)
    assert sorted(set(g[1] for g in b.gadgets)) == [0, 1, 2, 3]
    for value in ((lo - 1) % R, lo, hi - 1, hi, 0, R - 1):
        _, full, reasons = b.model({x: value})
        assert not reasons
        assert full[out] == (1 if lo <= value < hi else 0), hex(value)
        assert full[out] in (0, 1)
        assert b.arithmetic_failures(full) == []


def test_bits_model_edges():
    for B in (1, 32, 33, 256):
        for v in (0, 1, R - 1, (1 << B) % R):
            for acc0 in (0, 1, R - 1):
                bits, acc = CM.bits_model(v, B, acc0)
                assert sum(bit << k for k, bit in enumerate(bits)) == v % (1 << B)
                assert acc[-1] == (acc0 + v % (1 << B)) % R
                prev = acc0
                for k in range(B):      # the accumulating row: 2^k bit + acc_(k-1) - acc_k
                    assert ((bits[k] << k) + prev - acc[k]) % R == 0 and bits[k] * bits[k] == bits[k]
                    prev = acc[k]
