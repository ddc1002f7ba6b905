"""The HADES gadget on the GPU: the rows of a Hades permutation filled by one wave per gadget and
proof, against the big-integer model of tests/hades_model.py and against the ARITH kernel on the same rows -- every comparison
is byte equality of the whole [batch][num_vars] array.  The circuits come from tests/hades_circuits.py, which builds each once."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hades_circuits as HC  # noqa: E402
import hades_model as HM  # noqa: E402

pytestmark = pytest.mark.gpu
R = HM.R
# what pm_plonk_key_set_gadgets keeps for a round (include/plonk_mi355x.h): 30 coefficients and 30 ids; and for a record
ROUND_BYTES, RECORD_BYTES = 960 + 120, 32


def _key(ctx, b, ck=None):
    import plonk_prototype_amd as pa
    pk = pa.preprocess(b.circuit(), ctx, ck)
    assert pk.set_gadgets(b.gadget_records()) > 0
    return pk


def _limbs(models, which):
    return [HM.to_limbs(m[which]) for m in models]


def _fill_and_compare(pk, only, full):
    """fill the inputs-only assignments in ONE call and compare all bytes with the model's"""
    filled, reports = pk.fill_gadgets(only)
    want = np.stack(full)
    assert filled.shape == want.shape and len(reports) == len(full)
    assert all(r.ok and r.first_gadget is None for r in reports)          # the kind never reports
    if filled.tobytes() != want.tobytes():
        p, v = np.argwhere((filled != want).any(axis=2))[0]
        raise AssertionError(f"proof {p}: variable {v} differs (and {int((filled != want).any(axis=2).sum()) - 1} more)")
    return filled


# ---------------------------------------------------------------------------------- 1. the shapes
def test_shapes_in_one_level(ctx):
    b, assignments, models = HC.shapes_case()
    assert [(g[3], g[4]) for g in b.gadgets if g[0] == "hades"] == list(HC.SHAPES)
    pk = _key(ctx, b)
    try:
        only, full = _limbs(models, 0), _limbs(models, 1)
        filled = _fill_and_compare(pk, only, full)                            # batch 64
        _fill_and_compare(pk, only[1:4], full[1:4])                           # batch 3
        one, rep = pk.fill_gadgets(only[41])                                  # batch 1
        assert rep[0].ok and one.tobytes() == filled[41].tobytes()
        pk.enable_check()
        for rep in pk.check_witnesses(variables=[filled[p] for p in (0, 14, 28, 63)]):
            assert rep.ok, rep.describe()
        assert not pk.check_witness(variables=only[63]).ok                    # the fill is what made the rows hold
    finally:
        pk.free()


# ---------------------------------------------------------------------------------- 2. dusk's size
def test_dusk_permutation(ctx):
    b, assignments, models = HC.dusk_case()
    assert b.n == 2048 and [(g[0], g[3], g[4]) for g in b.gadgets][1] == ("hades", 67, 8) and len(models) == 2
    pk = _key(ctx, b)
    try:
        _fill_and_compare(pk, _limbs(models, 0), _limbs(models, 1))
    finally:
        pk.free()


# ---------------------------------------------------------------------------------- 3. two kernels, one computation
@pytest.mark.parametrize("shape", [(5, 2), HC.DUSK])
def test_hades_equals_the_arith_run(ctx, shape):
    (b1, _, m1), (b2, _, m2) = HC.cross_case(*shape)
    r1, r2 = b1.gadget_records(), b2.gadget_records()
    assert [g.kind for g in r1] == [4, 7] and [g.kind for g in r2] == [4, 4]
    assert (r2[1].first_row, r2[1].count) == (r1[1].first_row, r1[1].rows) and r1[1].rows == HM.hades_rows(*shape)
    only = _limbs(m1, 0)
    pk = _key(ctx, b1)                    # one key: the rows are the same, only the claim differs
    try:
        as_hades, reps = pk.fill_gadgets(only)
        assert all(r.ok for r in reps)
        assert pk.set_gadgets(r2) > 0
        as_arith, reps = pk.fill_gadgets(only)
        assert all(r.ok for r in reps)
        assert as_hades.tobytes() == as_arith.tobytes()
        assert as_hades.tobytes() == np.stack(_limbs(m1, 1)).tobytes()
    finally:
        pk.free()


# ---------------------------------------------------------------------------------- 4. a sponge, end to end
def test_sponge_end_to_end(ctx, oracle):
    import plonk_prototype_amd as pa
    from plonk_prototype_amd.field import fr_to_limbs
    from test_gpu_gadgets import TAU, _pairing_verifier_accepts
    b, inputs, out, pi_row = HC.sponge_case()
    n = b.n
    recs = b.gadget_records()
    assert [(g.kind, g.level) for g in recs] == [(4, 0), (7, 1), (4, 2), (7, 3)]
    ck = pa.CommitKey.setup(n + 9, fr_to_limbs(TAU), ctx, precompute=True)
    pk = _key(ctx, b, ck)
    try:
        pk.enable_check()
        only, full, pubs = [], [], []
        for seed in (1, 2, 3):
            o, f, reasons = b.model(inputs(seed))
            assert not reasons and f[out] != 0
            pi = [0] * n
            pi[pi_row] = (-f[out]) % R                                     # the row is a + PI = 0
            only.append(HM.to_limbs(o)), full.append(HM.to_limbs(f)), pubs.append(HM.to_limbs(pi))
        sent = pa.prove(pk, ck, variables=only[0], public_inputs=pubs[0], fill=True, check=True)
        dense = pa.prove(pk, ck, variables=full[0], public_inputs=pubs[0])
        assert sent.native_bytes == dense.native_bytes and len(sent.native_bytes) == 1040
        assert pk.check_witness(variables=only[0], public_inputs=pubs[0], fill=True).ok
        assert not pk.check_witness(variables=only[0], public_inputs=pubs[0]).ok
        assert not pk.check_witness(variables=only[0], public_inputs=pubs[1], fill=True).ok       # another hash
        _pairing_verifier_accepts(oracle, pk, sent, n, pubs[0])
        got = pa.prove_batch(pk, ck, variables=only, public_inputs=pubs, fill=True, check=True)
        singles = [pa.prove(pk, ck, variables=f, public_inputs=p) for f, p in zip(full, pubs)]
        assert [g.native_bytes for g in got] == [s.native_bytes for s in singles] and got[0].native_bytes == sent.native_bytes
    finally:
        pk.free()


# ---------------------------------------------------------------------------------- 5. refusals
def test_refusals_name_the_gadget_and_keep_the_table(ctx):
    import plonk_prototype_amd as pa
    from plonk_prototype_amd import _lib
    b, a, decoys = HC.refusal_case()
    n = b.n
    pk = pa.preprocess(b.circuit(), ctx)
    lib, h = ctx._lib, ctx._h
    good = b.gadget_records()
    H = pa.Gadget.hades
    first = good[0]
    assert first.level == 0 and [g.kind for g in good] == [4, 7]

    def refuse(recs, index):
        raw = (_lib.Gadget * len(recs))(*[g._raw() for g in recs])
        out = C.c_size_t(12345)
        assert lib.pm_plonk_key_set_gadgets(h, pk._h, raw, len(recs), C.byref(out)) == _lib.PM_ERR_BAD_ARG
        assert f"gadget {index}:" in lib.pm_last_error(h).decode(), lib.pm_last_error(h).decode()

    try:
        assert pk.set_gadgets(good) > 0
        assert pk.set_gadgets([first, H(decoys["good"], 1, 0, level=1)]) > 0      # an untouched one-round permutation is fine
        assert pk.set_gadgets(good) > 0
        refuse([first, H(decoys["matrix_wire"], 1, 0, level=1)], 1)               # a matrix row reads the wrong variable
        refuse([first, H(decoys["key_q_l"], 1, 0, level=1)], 1)                   # q_l != 1 on a key row
        refuse([first, H(decoys["matrix_q_4"], 1, 0, level=1)], 1)                # q_4 != 1 on a second matrix row
        refuse([first, H(decoys["sbox_q_m"], 1, 0, level=1)], 1)                  # q_m != 1 in the s-box
        refuse([first, H(decoys["q_o"], 1, 0, level=1)], 1)                       # q_o != -1
        refuse([first, H(decoys["widget"], 1, 0, level=1)], 1)                    # a widget selector on a claimed row
        refuse([first, H(decoys["no_var"], 1, 0, level=1)], 1)                    # a written position is no variable
        refuse([H(decoys["good"], 2, 2)], 0)                                      # the rows of another shape
        refuse([first, H(decoys["good"], 5, 3, level=1)], 1)                      # F odd
        refuse([first, H(decoys["good"], 1, 2, level=1)], 1)                      # F > R
        refuse([first, H(decoys["good"], 0, 0, level=1)], 1)                      # count 0
        refuse([first, H(n - 17, 1, 0, level=1)], 1)                              # rows leave [0, n)
        refuse([H(n, 1, 0)], 0)
        # the lowest offender: a device finding before a host finding after it, and the reverse
        refuse([first, H(decoys["key_q_l"], 1, 0, level=1), H(decoys["good"], 5, 3, level=1)], 1)
        refuse([first, H(decoys["good"], 5, 3, level=1), H(decoys["key_q_l"], 1, 0, level=1)], 1)
        # after all that the key still has the table it was given, and fills correctly
        model = b.model(a)
        got, reps = pk.fill_gadgets(HM.to_limbs(model[0]))
        assert reps[0].ok and got.tobytes() == HM.to_limbs(model[1]).tobytes()
    finally:
        pk.free()


@pytest.mark.parametrize("part", range(HC.RULE_PARTS))
def test_every_set_time_rule_refuses_its_decoy(ctx, part):
    """hades_circuits.rule_decoys_case: every field the set-time check looks at, wrong in that one place only"""
    import plonk_prototype_amd as pa
    b, a, decoys = HC.rule_decoys_case(part)
    pk = pa.preprocess(b.circuit(), ctx)
    good = b.gadget_records()
    assert [g.kind for g in good] == [4, 7, 7] and good[-1].level == 1
    why = "a row it claims is not the arithmetic row its kind lays out (selectors, coefficients or wire variables)"
    try:
        added = pk.set_gadgets(good)
        assert added > 0
        assert pk.set_gadgets(good + [pa.Gadget.hades(decoys["good"], *HC.DECOY_SHAPE, level=1)]) == added + RECORD_BYTES + 4 * ROUND_BYTES
        assert pk.set_gadgets(good) == added
        for name, r0 in decoys.items():
            if name == "good":
                continue
            with pytest.raises(pa.Error) as e:
                pk.set_gadgets(good + [pa.Gadget.hades(r0, *HC.DECOY_SHAPE, level=1)])
            assert str(e.value).endswith(f"gadget {len(good)}: {why}"), (name, str(e.value))
        # after all that the key still has the table it was given: the second permutation fills from its own offset
        model = b.model(a)
        got, reps = pk.fill_gadgets(HM.to_limbs(model[0]))
        assert reps[0].ok and got.tobytes() == HM.to_limbs(model[1]).tobytes()
    finally:
        pk.free()


# ---------------------------------------------------------------------------------- 6. what a table holds
def test_added_bytes(ctx):
    import plonk_prototype_amd as pa
    from test_gpu_composed_gadgets import SMALL_CIRCUIT_ADDED_BYTES
    from test_gpu_gadgets import _small_circuit
    b, _, _ = _small_circuit()
    pk = pa.preprocess(b.circuit(), ctx)
    try:
        assert pk.set_gadgets(b.gadget_records()) == SMALL_CIRCUIT_ADDED_BYTES      # no HADES gadget: what it was
    finally:
        pk.free()
    b, _, _ = HC.dusk_case()
    glue, perm = b.gadget_records()
    pk = pa.preprocess(b.circuit(), ctx)
    try:
        without = pk.set_gadgets([glue])
        assert pk.set_gadgets([glue, perm]) == without + RECORD_BYTES + 67 * ROUND_BYTES == without + 32 + 64320 + 8040
        assert pk.set_gadgets([glue]) == without
    finally:
        pk.free()
