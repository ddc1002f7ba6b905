"""The variable-base scalar multiplication gadget on the GPU: the six rows of every round filled by one
wave per gadget and proof, against the big-integer model of tests/var_base_model.py and against the composed form (CURVE_ADD,
ARITH, CURVE_ADD on 2 R levels) on the same rows -- every comparison is byte equality of the whole [batch][num_vars] array.  The
circuits come from tests/var_base_circuits.py, which builds each once."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import var_base_circuits as VC  # noqa: E402
import var_base_model as VM  # noqa: E402

pytestmark = pytest.mark.gpu
R = VM.R
RECORD_BYTES = 32          # what pm_plonk_key_set_gadgets keeps for a gadget of the kind (include/plonk_mi355x.h): its record


def _key(ctx, b, ck=None):
    import plonk_prototype_amd as pa
    pk = pa.preprocess(b.circuit(), ctx, ck)
    assert pk.set_gadgets(b.gadget_records()) > 0
    return pk


def _limbs(models, which):
    return [VM.to_limbs(m[which]) for m in models]


def _fill_and_compare(pk, only, full):
    """fill the inputs-only assignments in ONE call and compare all bytes with the model's"""
    filled, reports = pk.fill_gadgets(only)
    want = np.stack(full)
    assert filled.shape == want.shape and len(reports) == len(full)
    assert all(r.ok and r.first_gadget is None for r in reports)
    if filled.tobytes() != want.tobytes():
        p, v = np.argwhere((filled != want).any(axis=2))[0]
        raise AssertionError(f"proof {p}: variable {v} differs (and {int((filled != want).any(axis=2).sum()) - 1} more)")
    return filled


# ---------------------------------------------------------------------------------- 1. the shapes
@pytest.mark.parametrize("case", [(VC.SHAPES_A, 64, 41), (VC.SHAPES_B, 64, 47)], ids=["1_to_252", "256"])
def test_shapes_in_one_level(ctx, case):
    b, assignments, models, _ = VC.shapes_case(*case)
    assert [g[3] for g in b.gadgets if g[0] == "var_base"] == list(case[0]) and b.n <= 4096
    pk = _key(ctx, b)
    try:
        only, full = _limbs(models, 0), _limbs(models, 1)
        filled = _fill_and_compare(pk, only, full)                            # the whole batch
        _fill_and_compare(pk, only[1:4], full[1:4])                           # batch 3
        one, rep = pk.fill_gadgets(only[19])                                  # batch 1
        assert rep[0].ok and one.tobytes() == filled[19].tobytes()
        pk.enable_check()
        for rep in pk.check_witnesses(variables=[filled[p] for p in (0, 14, 28, 39)]):
            assert rep.ok, rep.describe()
        assert not pk.check_witness(variables=only[39]).ok                    # the fill is what made the rows hold
    finally:
        pk.free()


# ---------------------------------------------------------------------------------- 2. two kernels, one computation
@pytest.mark.parametrize("rounds", [5, 252])
def test_equals_the_composed_form(ctx, rounds):
    (b1, _, m1), (b2, _, m2) = VC.cross_case(rounds)
    r1, r2 = b1.gadget_records(), b2.gadget_records()
    assert [g.kind for g in r1] == [4, 10] and sorted(set(g.kind for g in r2)) == [3, 4] and len(r2) == 1 + 3 * rounds
    assert r1[1].rows == 6 * rounds and max(g.level for g in r2) == 2 * rounds - 1
    only = _limbs(m1, 0)
    pk = _key(ctx, b1)                    # one key: the rows are the same, only the claim differs
    try:
        as_chain, reps = pk.fill_gadgets(only)
        assert all(r.ok for r in reps)
        assert pk.set_gadgets(r2) > 0
        as_composed, reps = pk.fill_gadgets(only)
        assert all(r.ok for r in reps)
        assert as_chain.tobytes() == as_composed.tobytes()
        assert as_chain.tobytes() == np.stack(_limbs(m1, 1)).tobytes()
    finally:
        pk.free()


# ---------------------------------------------------------------------------------- 3. against FIXED_BASE
def test_ends_where_the_fixed_base_gadget_ends(ctx):
    b, assignments, models, fixed, variable, scalars = VC.fixed_base_case()
    assert [(g[0], g[1]) for g in b.gadgets] == [("fixed_base", 0), ("bits", 0), ("var_base", 1)]
    pk = _key(ctx, b)
    try:
        filled = _fill_and_compare(pk, _limbs(models, 0), _limbs(models, 1))
        for p in range(len(models)):
            assert filled[p][fixed[0]].tobytes() == filled[p][variable[0]].tobytes()
            assert filled[p][fixed[1]].tobytes() == filled[p][variable[1]].tobytes()
            assert filled[p][variable[0]].any()
    finally:
        pk.free()


# ---------------------------------------------------------------------------------- 4. dusk's shape, end to end
def test_dusk_shape_end_to_end(ctx, oracle):
    import plonk_prototype_amd as pa
    from plonk_prototype_amd.field import fr_to_limbs
    from test_gpu_gadgets import TAU, _pairing_verifier_accepts
    b, inputs, out, pi_rows = VC.dusk_case()
    n = b.n
    recs = b.gadget_records()
    assert [(g.kind, g.level, g.count) for g in recs] == [(5, 0, 252), (10, 1, 252)]
    ck = pa.CommitKey.setup(n + 9, fr_to_limbs(TAU), ctx, precompute=True)
    pk = _key(ctx, b, ck)
    try:
        pk.enable_check()
        only, full, pubs = [], [], []
        for seed in (1, 2, 3):
            o, f, reasons = b.model(inputs(seed))
            assert not reasons and f[out[0]] != 0
            pi = [0] * n
            for row, var in zip(pi_rows, out):
                pi[row] = (-f[var]) % R                                    # the rows are a + PI = 0
            only.append(VM.to_limbs(o)), full.append(VM.to_limbs(f)), pubs.append(VM.to_limbs(pi))
        sent = pa.prove(pk, ck, variables=only[0], public_inputs=pubs[0], fill=True, check=True)
        dense = pa.prove(pk, ck, variables=full[0], public_inputs=pubs[0])
        assert sent.native_bytes == dense.native_bytes and len(sent.native_bytes) == 1040
        assert pk.check_witness(variables=only[0], public_inputs=pubs[0], fill=True).ok
        assert not pk.check_witness(variables=only[0], public_inputs=pubs[0]).ok
        assert not pk.check_witness(variables=only[0], public_inputs=pubs[1], fill=True).ok       # another point
        _pairing_verifier_accepts(oracle, pk, sent, n, pubs[0])
        got = pa.prove_batch(pk, ck, variables=only, public_inputs=pubs, fill=True, check=True)
        singles = [pa.prove(pk, ck, variables=f, public_inputs=p) for f, p in zip(full, pubs)]
        assert [g.native_bytes for g in got] == [s.native_bytes for s in singles] and got[0].native_bytes == sent.native_bytes
    finally:
        pk.free()


# ---------------------------------------------------------------------------------- 5. reports
def test_reports(ctx):
    import plonk_prototype_amd as pa
    from plonk_prototype_amd.field import fr_to_limbs
    from test_gpu_gadgets import TAU
    b, assignments, models = VC.report_case()
    assert [m[2] for m in models] == [{}, {0: VM.TOO_WIDE}, {0: VM.DEGENERATE}]
    ck = pa.CommitKey.setup(b.n + 9, fr_to_limbs(TAU), ctx, precompute=True)
    pk = _key(ctx, b, ck)
    try:
        only, full = _limbs(models, 0), _limbs(models, 1)
        filled, reports = pk.fill_gadgets(only)
        assert reports[0].ok and filled[0].tobytes() == full[0].tobytes()
        assert (reports[1].ok, reports[1].failed, reports[1].first_gadget, reports[1].first_reason) == (False, 1, 0, "too_wide")
        assert (reports[2].ok, reports[2].failed, reports[2].first_gadget, reports[2].first_reason) == (False, 1, 0, "degenerate")
        sel = b.select_vars()
        for p in (1, 2):                                                    # the select rows are exact all the same
            assert filled[p][sel].tobytes() == full[p][sel].tobytes()
        again, _ = pk.fill_gadgets(only)                                    # ... and the rest is deterministic
        assert again.tobytes() == filled.tobytes()
        for p, reason in ((1, "too_wide"), (2, "degenerate")):
            with pytest.raises(pa.GadgetInputError) as e:
                pa.prove(pk, ck, variables=only[p], fill=True)
            assert "gadget 0" in str(e.value) and "variable_base" in str(e.value) and reason in str(e.value)
        with pytest.raises(pa.GadgetInputError) as e:
            pa.prove_batch(pk, ck, variables=only, fill=True)
        assert set(e.value.reports) == {1, 2}
    finally:
        pk.free()


# ---------------------------------------------------------------------------------- 6. refusals
def test_refusals_name_the_gadget_and_keep_the_table(ctx):
    import plonk_prototype_amd as pa
    from plonk_prototype_amd import _lib
    b, a, decoys = VC.refusal_case()
    n = b.n
    pk = pa.preprocess(b.circuit(), ctx)
    lib, h = ctx._lib, ctx._h
    good = b.gadget_records()
    V = pa.Gadget.variable_base
    first = good[0]
    assert first.level == 0 and [g.kind for g in good] == [4, 10]
    K = VC.DECOY_ROUNDS

    def refuse(recs, index):
        raw = (_lib.Gadget * len(recs))(*[g._raw() for g in recs])
        out = C.c_size_t(12345)
        assert lib.pm_plonk_key_set_gadgets(h, pk._h, raw, len(recs), C.byref(out)) == _lib.PM_ERR_BAD_ARG
        assert f"gadget {index}:" in lib.pm_last_error(h).decode(), lib.pm_last_error(h).decode()

    try:
        assert pk.set_gadgets(good) > 0
        assert pk.set_gadgets([first, V(decoys["good"], K, level=1)]) > 0        # an untouched multiplication is fine
        assert pk.set_gadgets([first, V(decoys["good"], 1, level=1)]) > 0        # ... and so is its first round alone
        assert pk.set_gadgets(good) > 0
        for name, r0 in decoys.items():                                          # one decoy per set-time test
            if name != "good":
                refuse([first, V(r0, K, level=1)], 1)
        refuse([V(decoys["good"] + 1, 1)], 0)                                    # rows that are no round
        refuse([first, V(decoys["good"], 0, level=1)], 1)                        # count 0
        refuse([first, V(decoys["good"], 257, level=1)], 1)                      # above PM_PLONK_GADGET_MAX_ROUNDS
        refuse([first, pa.Gadget(10, decoys["good"], K, 1, 1)], 1)               # param != 0
        refuse([first, V(n - 6 * K + 1, K, level=1)], 1)                         # rows leave [0, n)
        refuse([V(n, 1)], 0)
        refuse([first, pa.Gadget(8, decoys["good"], K, 1)], 1)                   # 8 and 9 are no kinds
        refuse([first, pa.Gadget(9, decoys["good"], K, 1)], 1)
        # the lowest offender: a device finding before a host finding after it, and the reverse
        refuse([first, V(decoys["x_q_m"], K, level=1), V(decoys["good"], 257, level=1)], 1)
        refuse([first, V(decoys["good"], 257, level=1), V(decoys["x_q_m"], K, level=1)], 1)
        # after all that the key still has the table it was given, and fills correctly
        model = b.model(a)
        got, reps = pk.fill_gadgets(VM.to_limbs(model[0]))
        assert reps[0].ok and got.tobytes() == VM.to_limbs(model[1]).tobytes()
    finally:
        pk.free()


# ---------------------------------------------------------------------------------- 7. what a table holds
def test_added_bytes(ctx):
    import plonk_prototype_amd as pa
    from test_gpu_composed_gadgets import SMALL_CIRCUIT_ADDED_BYTES
    from test_gpu_gadgets import _small_circuit
    b, _, _ = _small_circuit()
    pk = pa.preprocess(b.circuit(), ctx)
    try:
        assert pk.set_gadgets(b.gadget_records()) == SMALL_CIRCUIT_ADDED_BYTES      # no gadget of the kind: what it was
    finally:
        pk.free()
    (b, _, _), _ = VC.cross_case(252)
    glue, chain = b.gadget_records()
    pk = pa.preprocess(b.circuit(), ctx)
    try:
        without = pk.set_gadgets([glue])
        assert pk.set_gadgets([glue, chain]) == without + RECORD_BYTES              # the fill reads the key's wire map
        assert pk.set_gadgets([glue]) == without
    finally:
        pk.free()
