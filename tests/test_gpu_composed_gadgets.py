"""Composed gadget witnesses on the GPU: arithmetic runs, bit decompositions and maybe_equal filled
on the device against the big-integer model of tests/composed_gadget_model.py -- every comparison is byte equality of the
whole [batch][num_vars] array.  The circuits come from tests/composed_gadget_circuits.py, which builds each once."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import composed_gadget_circuits as CC  # noqa: E402
import composed_gadget_model as CM  # noqa: E402
import gadget_model as M  # noqa: E402

pytestmark = pytest.mark.gpu
R = M.R


def _key(ctx, b, ck=None):
    import plonk_prototype_amd as pa
    pk = pa.preprocess(b.circuit(), ctx, ck)
    assert pk.set_gadgets(b.gadget_records()) > 0
    return pk


def _limbs(models, which):
    return [M.to_limbs(m[which]) for m in models]


def _fill_and_compare(pk, models, only=None, full=None):
    """fill the inputs-only form of every model in ONE call and compare all bytes"""
    only = _limbs(models, 0) if only is None else only
    full = _limbs(models, 1) if full is None else full
    filled, reports = pk.fill_gadgets(only)
    want = np.stack(full)
    assert filled.shape == want.shape and len(reports) == len(models)
    assert all(r.ok and r.first_gadget is None for r in reports)          # the composed kinds never report
    if filled.tobytes() != want.tobytes():
        p, v = np.argwhere((filled != want).any(axis=2))[0]
        raise AssertionError(f"proof {p}: variable {v} differs (and {int((filled != want).any(axis=2).sum()) - 1} more)")
    return filled


# ---------------------------------------------------------------------------------- 1. BITS
@pytest.mark.parametrize("which", ["small", "full"])
def test_bits(ctx, which):
    b, assignments, models = CC.bits_case(which)
    assert len(models) == 64
    pk = _key(ctx, b)
    try:
        only, full = _limbs(models, 0), _limbs(models, 1)
        filled = _fill_and_compare(pk, models, only, full)                    # batch 64
        _fill_and_compare(pk, models[20:23], only[20:23], full[20:23])        # batch 3
        one, rep = pk.fill_gadgets(only[40])                                  # batch 1
        assert rep[0].ok and one.tobytes() == filled[40].tobytes()
        if which == "small":
            pk.enable_check()
            for rep in pk.check_witnesses(variables=[filled[p] for p in (0, 8, 20, 63)]):
                assert rep.ok, rep.describe()
    finally:
        pk.free()


# ---------------------------------------------------------------------------------- 2. MAYBE_EQUAL
def test_maybe_equal_partial_wave(ctx):
    from plonk_prototype_amd.field import fr_from_limbs
    b, assignments, models, outs = CC.maybe_equal_case()
    assert len(b.gadgets) == 65 and len(set(g[1] for g in b.gadgets)) == 1
    pk = _key(ctx, b)
    try:
        filled = _fill_and_compare(pk, models)
        for g in (0, 1, 2, 3, 64):       # equal inputs give 1, others 0 -- read back from the device's own bytes
            r0 = b.gadgets[g][2]
            u = fr_from_limbs(filled[0][b.wires[2][r0]])
            z = fr_from_limbs(filled[0][b.wires[0][r0 + 1]])
            assert fr_from_limbs(filled[0][outs[g]]) == (0 if u else 1)
            assert (z * u % R == 1) if u else z == 0
        pk.enable_check()
        for rep in pk.check_witnesses(variables=[filled[p] for p in range(len(models))]):
            assert rep.ok, rep.describe()
    finally:
        pk.free()


# ---------------------------------------------------------------------------------- 3. ARITH
def test_arith_runs(ctx):
    b, assignments, models = CC.arith_case()
    assert [g[0] for g in b.gadgets] == ["arith", "arith"] and b.gadgets[0][1] == b.gadgets[1][1]
    pk = _key(ctx, b)
    try:
        filled = _fill_and_compare(pk, models)
        pk.enable_check()
        for rep in pk.check_witnesses(variables=[filled[p] for p in range(len(models))]):
            assert rep.ok, rep.describe()
        assert not pk.check_witness(variables=M.to_limbs(models[0][0])).ok       # the fill is what made the rows hold
    finally:
        pk.free()


# ---------------------------------------------------------------------------------- 4. two kernels, one computation
def test_bits_equal_the_arith_form(ctx):
    (b1, _, m1), (b2, _, m2) = CC.cross_case()
    assert [g[0] for g in b1.gadgets] == ["bits", "maybe_equal"] and [g[0] for g in b2.gadgets] == ["arith", "maybe_equal"]
    assert b2.gadgets[0][3] == 2 * b1.gadgets[0][3]
    out = []
    for b, models in ((b1, m1), (b2, m2)):
        pk = _key(ctx, b)
        try:
            out.append(_fill_and_compare(pk, models))
        finally:
            pk.free()
    assert out[0].tobytes() == out[1].tobytes()


# ---------------------------------------------------------------------------------- 5. end to end
def test_range_check_end_to_end(ctx, oracle):
    import plonk_prototype_amd as pa
    from plonk_prototype_amd.field import fr_from_limbs, fr_to_limbs
    from test_gpu_gadgets import TAU, _pairing_verifier_accepts
    b, inputs, out = CC.end_to_end_case()
    n = b.n
    recs = b.gadget_records()
    assert sorted(set(g.level for g in recs)) == [0, 1, 2, 3] and {g.kind for g in recs} == {2, 3, 4, 5, 6}
    ck = pa.CommitKey.setup(n + 9, fr_to_limbs(TAU), ctx, precompute=True)
    pk = _key(ctx, b, ck)
    try:
        pk.enable_check()
        for value, want in ((CC.RANGE_MIN + 12345, 1), (CC.RANGE_MAX, 0)):          # inside; x = max: outside
            only, full, reasons = b.model(inputs(value))
            assert not reasons and full[out] == want
            only, full = M.to_limbs(only), M.to_limbs(full)
            filled, reps = pk.fill_gadgets(only)
            assert reps[0].ok and filled.tobytes() == full.tobytes()
            assert fr_from_limbs(filled[out]) == want
            assert pk.check_witness(variables=only, fill=True).ok and not pk.check_witness(variables=only).ok
            sent = pa.prove(pk, ck, variables=only, fill=True, check=True)
            dense = pa.prove(pk, ck, variables=full)
            assert sent.native_bytes == dense.native_bytes and len(sent.native_bytes) == 1040
            _pairing_verifier_accepts(oracle, pk, sent, n, np.zeros((n, 4), np.uint64))
    finally:
        pk.free()


# ---------------------------------------------------------------------------------- 6. refusals
def test_refusals_name_the_gadget_and_keep_the_table(ctx):
    import plonk_prototype_amd as pa
    from plonk_prototype_amd import _lib
    b, a, decoys = CC.refusal_case()
    n = b.n
    pk = pa.preprocess(b.circuit(), ctx)
    lib, h = ctx._lib, ctx._h
    good = b.gadget_records()
    G = pa.Gadget
    first = good[0]
    assert first.level == 0

    def refuse(recs, index):
        raw = (_lib.Gadget * len(recs))(*[g._raw() for g in recs])
        out = C.c_size_t(12345)
        assert lib.pm_plonk_key_set_gadgets(h, pk._h, raw, len(recs), C.byref(out)) == _lib.PM_ERR_BAD_ARG
        assert f"gadget {index}:" in lib.pm_last_error(h).decode(), lib.pm_last_error(h).decode()

    try:
        assert pk.set_gadgets(good) > 0
        refuse([first, G.bits(decoys["bits_q_l"], 4, 1)], 1)                      # q_l != 2^k
        assert pk.set_gadgets([G.bits(decoys["bits_q_l"], 2, 1)]) > 0             # ... the rows before the wrong one are fine
        assert pk.set_gadgets(good) > 0
        refuse([first, G.bits(decoys["bits_wire"], 4, 1)], 1)                     # a != c on a boolean row
        refuse([first, G.bits(decoys["bits_wire"], 0, 1)], 1)                     # count 0
        refuse([first, G.bits(decoys["bits_wire"], 257, 1)], 1)                   # count 257
        refuse([first, G.bits(n - 6, 4, 1)], 1)                                   # rows leave [0, n)
        refuse([G.bits(decoys["bits_q_l"], 2, b.num_vars)], 0)                    # in_var >= num_vars
        refuse([first, G.arith(decoys["arith_q_o"], 1)], 1)                       # q_o != -1
        refuse([first, G.arith(decoys["arith_off"], 1)], 1)                       # q_arith = 0
        refuse([first, G.arith(decoys["arith_widget"], 1)], 1)                       # a widget selector
        refuse([G.arith(n - 1, 2)], 0)
        refuse([G.arith(0, 0)], 0)
        refuse([first, G.maybe_equal(decoys["maybe_equal_q_c"])], 1)              # q_c != 1 on row 1
        refuse([G.maybe_equal(n - 2)], 0)
        refuse([pa.Gadget(7, 0, 1)], 0)                                           # kind 7 is still unknown
        # the lowest offender: a device finding before a host finding after it, and the reverse
        refuse([first, G.arith(decoys["arith_off"], 1), G.bits(0, 257, 1)], 1)
        refuse([first, G.bits(0, 257, 1), G.arith(decoys["arith_off"], 1)], 1)
        # after all that the key still has the table it was given, and fills correctly
        model = b.model(a)
        got, reps = pk.fill_gadgets(M.to_limbs(model[0]))
        assert reps[0].ok and got.tobytes() == M.to_limbs(model[1]).tobytes()
    finally:
        pk.free()


def test_every_set_time_rule_refuses_its_decoy(ctx):
    """composed_gadget_circuits.rule_decoys_case: every field the set-time check looks at, wrong in that one place only"""
    import plonk_prototype_amd as pa
    b, a, decoys = CC.rule_decoys_case()
    pk = pa.preprocess(b.circuit(), ctx)
    good = b.gadget_records()
    assert [g.kind for g in good] == [4, 4, 5, 5, 6, 6] and good[-1].level == 2
    G = pa.Gadget
    make = {"bits": lambda r0: G.bits(r0, CC.DECOY_BITS, 1, level=2), "maybe_equal": lambda r0: G.maybe_equal(r0, level=2),
            "arith": lambda r0: G.arith(r0, 1, level=2)}
    why = "a row it claims is not the arithmetic row its kind lays out (selectors, coefficients or wire variables)"
    try:
        added = pk.set_gadgets(good)
        assert added > 0
        for kind, table in decoys.items():
            assert len(table) >= 5
            assert pk.set_gadgets(good + [make[kind](table["good"])]) > added      # an untouched one is fine
            assert pk.set_gadgets(good) == added
            for name, r0 in table.items():
                if name == "good":
                    continue
                with pytest.raises(pa.Error) as e:
                    pk.set_gadgets(good + [make[kind](r0)])
                assert str(e.value).endswith(f"gadget {len(good)}: {why}"), (kind, name, str(e.value))
        # after all that the key still has the table it was given: the second gadget of every kind fills from its own offset
        model = b.model(a)
        got, reps = pk.fill_gadgets(M.to_limbs(model[0]))
        assert reps[0].ok and got.tobytes() == M.to_limbs(model[1]).tobytes()
    finally:
        pk.free()


# ---------------------------------------------------------------------------------- 7. tables of the widget kinds are as before
# pm_plonk_key_set_gadgets' added_bytes for the table of test_gpu_gadgets._small_circuit (a fixed-base of 8 rounds, a range, a
# logic and a curve addition), as the commit before the composed kinds reports it on an MI355X
SMALL_CIRCUIT_ADDED_BYTES = 1664


def test_widget_tables_hold_what_they_held(ctx):
    import plonk_prototype_amd as pa
    from test_gpu_gadgets import _small_circuit
    b, inputs, _ = _small_circuit()
    pk = pa.preprocess(b.circuit(), ctx)
    try:
        assert pk.set_gadgets(b.gadget_records()) == SMALL_CIRCUIT_ADDED_BYTES
        only, full, _ = b.model(inputs(4))
        got, reps = pk.fill_gadgets(M.to_limbs(only))
        assert reps[0].ok and got.tobytes() == M.to_limbs(full).tobytes()
    finally:
        pk.free()
