"""Gadget witnesses on the GPU: every variable a gadget writes against the big-integer model of
tests/gadget_model.py, byte for byte; the filled assignments against the witness check; the lane partition of the fixed-base
kernel at every run length; levels and batches; ``fill=True`` end to end against the pairing verifier; and the refusals."""
import ctypes as C
import os
import random
import sys

import numpy as np
import pytest

from oracle import bigint_oracle as B
from oracle.cpu_oracle import limbs_to_ints

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gadget_model as M  # noqa: E402

pytestmark = pytest.mark.gpu
R = M.R
TAU = 0x2B7E151628AED2A6ABF7158809CF4F3C762E7160F38B4DA56A784D9045190CFE % R
ALT01, ALT0011 = int("01" * 128, 2), int("0011" * 64, 2)


def _key(ctx, b, ck=None):
    import plonk_prototype_amd as pa
    pk = pa.preprocess(b.circuit(), ctx, ck)
    recs = b.gadget_records()
    assert [g.level for g in recs] == sorted(g.level for g in recs)
    assert pk.set_gadgets(recs) > 0
    return pk


def _run(pk, b, assignments):
    """fill the inputs-only form of every assignment in ONE call; -> (filled [B, num_vars, 4], reports, models)"""
    models = [b.model(a) for a in assignments]
    filled, reports = pk.fill_gadgets([M.to_limbs(only) for only, _, _ in models])
    assert filled.shape == (len(assignments), b.num_vars, 4) and len(reports) == len(assignments)
    return filled, reports, models


def _compare(b, filled, reports, models):
    from plonk_prototype_amd import _lib
    for p, (_, full, reasons) in enumerate(models):
        want = M.to_limbs(full)
        if not np.array_equal(filled[p], want):
            bad = np.flatnonzero((filled[p] != want).any(axis=1))
            raise AssertionError(f"proof {p}: {bad.size} variables differ, first {bad[:8]}")
        rep = reports[p]
        assert rep.failed == len(reasons) and rep.ok == (not reasons), (p, rep, reasons)
        if reasons:
            first = min(reasons)
            assert (rep.first_gadget, rep.first_reason) == (first, reasons[first]), (p, rep, reasons)
            assert rep.first_reason in _lib.PLONK_GADGET_REASONS.values()
        else:
            assert rep.first_gadget is None and rep.first_reason is None


# ---------------------------------------------------------------------------------- 1. the lane partition of the fixed-base kernel
ROUNDS = (1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 255, 256)


def test_fixed_base_lane_partition(ctx):
    b = M.Builder(2048)
    sx, sy = b.var(True), b.var(True)              # one start point for all
    svars = []
    for rounds in ROUNDS:
        s = b.var(True)
        svars.append(s)
        b.fixed_base(s, rounds, (sx, sy))
        b.equal(s, b.wires[3][b.gadgets[-1][2] + rounds])      # the scalar is the last accumulator
    arith = b.fill_arithmetic(3)
    rng = random.Random(11)
    point = M.curve_point(0x7654321)
    fitting = lambda rounds: rng.getrandbits(rounds - 1) if rounds > 1 else rng.randrange(2)   # noqa: E731: at most `rounds` digits
    assignments, fits = [], []
    for start in (M.IDENTITY, point):
        for _ in range(2):
            assignments.append({sx: start[0], sy: start[1], **{s: fitting(r) for s, r in zip(svars, ROUNDS)}, **arith})
            fits.append(True)
        # the edge scalars, the same for every gadget (long ones are cut to the gadget's rounds and reported)
        for edge in (0, 1, 2, 3, R - 1, ALT01, ALT0011, None):
            assignments.append({sx: start[0], sy: start[1],
                                **{s: (((1 << r) - 1) % R if edge is None else edge) for s, r in zip(svars, ROUNDS)}, **arith})
            fits.append(edge in (0, 1))
    pk = _key(ctx, b)
    try:
        filled, reports, models = _run(pk, b, assignments)
        _compare(b, filled, reports, models)
        assert [not m[2] for m in models] == fits
        pk.enable_check()
        ok = [filled[p] for p in range(len(assignments)) if fits[p]]
        for rep in pk.check_witnesses(variables=ok):
            assert rep.ok, rep.describe()
        # an unfilled assignment does not satisfy the circuit: the fill is what made the rows hold
        assert not pk.check_witness(variables=M.to_limbs(models[1][0])).ok
    finally:
        pk.free()


# ---------------------------------------------------------------------------------- 2. range
def test_range(ctx):
    b = M.Builder(64)
    ms = (1, 2, 3, 32)
    vvars = []
    for m in ms:
        v = b.var(True)
        vvars.append(v)
        b.equal(v, b.range(v, m))
    arith = b.fill_arithmetic(5)
    rng = random.Random(5)
    top = lambda m: (1 << (8 * m))   # noqa: E731
    # a variable is a field element: for m = 32 the values 2^256 - 1 and 2^256 are taken mod r, and no element is too wide
    assignments = [{**{v: 0 for v in vvars}, **arith},
                   {**{v: (top(m) - 1) % R for v, m in zip(vvars, ms)}, **arith},
                   {**{v: rng.getrandbits(8 * m) % R for v, m in zip(vvars, ms)}, **arith}]
    for g, m in enumerate(ms):       # 2^(8m) on gadget g alone
        assignments.append({**{v: (top(mm) % R if mm == m else rng.getrandbits(8 * mm) % R) for v, mm in zip(vvars, ms)}, **arith})
    pk = _key(ctx, b)
    try:
        filled, reports, models = _run(pk, b, assignments)
        _compare(b, filled, reports, models)
        for g, m in enumerate(ms):
            rep = reports[3 + g]
            if m < 32:
                assert (rep.failed, rep.first_gadget, rep.first_reason) == (1, g, "too_wide")
            else:
                assert rep.ok
        assert all(r.ok for r in reports[:3])
        pk.enable_check()
        for rep in pk.check_witnesses(variables=[filled[p] for p in range(3)]):
            assert rep.ok, rep.describe()
    finally:
        pk.free()


# ---------------------------------------------------------------------------------- 3. logic
def test_logic(ctx):
    b = M.Builder(512)
    cases, outs = [], []
    for quads in (1, 2, 16, 128):
        for xor in (False, True):
            x, y = b.var(True), b.var(True)
            cases.append((quads, xor, x, y))
            outs.append(b.logic(x, y, quads, xor=xor))
    arith = b.fill_arithmetic(6)
    rng = random.Random(6)
    width = lambda q: min(2 * q, 254)   # noqa: E731
    assignments = []
    for _ in range(2):
        a = dict(arith)
        for quads, _, x, y in cases:
            a[x], a[y] = rng.getrandbits(width(quads)), rng.getrandbits(width(quads))
        assignments.append(a)
    assignments.append({**assignments[0], **{x: (1 << width(q)) - 1 for q, _, x, _ in cases}})
    wide = {**assignments[1], cases[3][3]: 1 << 4}            # y of the XOR over 2 quads: 4^2
    assignments.append(wide)
    pk = _key(ctx, b)
    try:
        filled, reports, models = _run(pk, b, assignments)
        _compare(b, filled, reports, models)
        from plonk_prototype_amd.field import fr_from_limbs
        for p in range(3):
            for (quads, xor, x, y), out in zip(cases, outs):
                vx, vy = assignments[p][x], assignments[p][y]
                assert fr_from_limbs(filled[p][out]) == ((vx ^ vy) if xor else (vx & vy))
        assert (reports[3].failed, reports[3].first_gadget, reports[3].first_reason) == (1, 3, "too_wide")
        pk.enable_check()
        for rep in pk.check_witnesses(variables=[filled[p] for p in range(3)]):
            assert rep.ok, rep.describe()
    finally:
        pk.free()


# ---------------------------------------------------------------------------------- 4. curve addition
def test_curve_add(ctx):
    b = M.Builder(32)
    p, q = M.curve_point(0xABCDEF), M.curve_point(0xFEDCBA)
    pairs = [(p, q), (p, M.IDENTITY), (p, p), (p, ((-p[0]) % R, p[1])), (M.curve_point(77), M.curve_point(1234567))]
    a = {}
    for u, v in pairs:
        ids = [b.var(True) for _ in range(4)]
        b.curve_add(ids[:2], ids[2:])
        a.update(zip(ids, (u[0], u[1], v[0], v[1])))
    n_real = len(b.gadgets)
    # off the curve: 1 + d x1 x2 y1 y2 = 0
    ids = [b.var(True) for _ in range(4)]
    b.curve_add(ids[:2], ids[2:])
    a.update(zip(ids, (1, 1, 1, (-pow(M.EDWARDS_D, -1, R)) % R)))
    a.update(b.fill_arithmetic(8))
    pk = _key(ctx, b)
    try:
        filled, reports, models = _run(pk, b, [a])
        _compare(b, filled, reports, models)
        assert (reports[0].failed, reports[0].first_gadget, reports[0].first_reason) == (1, n_real, "degenerate")
        pk.enable_check()
        rep = pk.check_witness(variables=filled[0], masks=True)
        r0 = b.gadgets[n_real][2]
        assert rep.failed_rows == 1 and rep.first_row == r0 and rep.first_reasons == ("var_base",)   # only the degenerate pair
    finally:
        pk.free()


# ---------------------------------------------------------------------------------- 5. levels and batches
def _commitment_circuit(n):
    """two 256-round multiplications (level 0) feed an addition (level 1) through shared variables; a range (level 2)"""
    b = M.Builder(n)
    s1, s2, v = b.var(True), b.var(True), b.var(True)
    st = [b.var(True) for _ in range(4)]
    p1 = b.fixed_base(s1, 256, st[:2], level=0, table_seed=0x1234567)
    p2 = b.fixed_base(s2, 256, st[2:], level=0, table_seed=0x2345678)
    out = b.curve_add(p1, p2, level=1)
    b.equal(v, b.range(v, 8, level=2))
    arith = b.fill_arithmetic(9)
    return b, (s1, s2, v, st, out), arith


def test_levels_and_batch(ctx):
    b, (s1, s2, v, st, out), arith = _commitment_circuit(1024)
    rng = random.Random(13)
    start = M.curve_point(4242)
    assignments = []
    for k in range(3):
        pts = (M.IDENTITY, M.IDENTITY) if k == 0 else (start, M.IDENTITY) if k == 1 else (M.IDENTITY, start)
        assignments.append({s1: rng.randrange(R), s2: rng.randrange(R), v: rng.getrandbits(64),
                            st[0]: pts[0][0], st[1]: pts[0][1], st[2]: pts[1][0], st[3]: pts[1][1], **arith})
    pk = _key(ctx, b)
    try:
        filled, reports, models = _run(pk, b, assignments)
        _compare(b, filled, reports, models)
        assert all(r.ok for r in reports)
        # the sum is s1 B1 + s2 B2 (+ the start points): the shape of the reference's commitment gadget
        from plonk_prototype_amd.field import fr_from_limbs
        t1, t2 = M.base_table(256, 0x1234567), M.base_table(256, 0x2345678)
        want = M.jubjub_add((assignments[0][st[0]], assignments[0][st[1]]), (assignments[0][st[2]], assignments[0][st[3]]))
        for j in range(256):
            if (assignments[0][s1] >> j) & 1:
                want = M.jubjub_add(want, t1[j])
            if (assignments[0][s2] >> j) & 1:
                want = M.jubjub_add(want, t2[j])
        assert (fr_from_limbs(filled[0][out[0]]), fr_from_limbs(filled[0][out[1]])) == want
        for p in range(3):       # proof p of the batch = the single call on inputs p
            one, rep = pk.fill_gadgets(M.to_limbs(models[p][0]))
            assert rep[0].ok and one.tobytes() == filled[p].tobytes()
        again, _, _ = _run(pk, b, assignments)
        assert again.tobytes() == filled.tobytes()
        pk.enable_check()
        for rep in pk.check_witnesses(variables=[filled[p] for p in range(3)]):
            assert rep.ok, rep.describe()
    finally:
        pk.free()


# ---------------------------------------------------------------------------------- 6. end to end
def _pairing_verifier_accepts(oracle, pk, sent, n, pub):
    """The oracle's verifier on the 1040 proof bytes (as tests/test_gpu_wires.py runs it)."""
    import plonk_prototype_amd.prover as PR
    from oracle import pairing_oracle as PG
    from oracle import plonk_verifier_oracle as PV

    def ints(limbs):
        return limbs_to_ints(oracle.fr_from_mont(np.ascontiguousarray(limbs).reshape(-1, 4)))

    def pt(xy):
        if not np.asarray(xy).any():
            return None
        v = limbs_to_ints(oracle.fp_from_mont(np.ascontiguousarray(xy).reshape(2, 6)))
        return (v[0], v[1])

    proof = PR.Proof.from_bytes(sent.native_bytes)
    vk = {k: pt(v) for k, v in pk.verifier_key.items()}
    comms = {k: pt(v) for k, v in proof.commitments.items()}
    ev = {k: ints(v)[0] for k, v in proof.evaluations.items()}
    ch0 = PR.derive_challenges(proof, pk.verifier_key, n, pub, t_eval=0)
    pub_z = B.horner(B.ifft(ints(pub), n.bit_length() - 1), ch0["z"])
    t_eval = PV.quotient_evaluation(n, ev, ch0, pub_z)
    ch = PR.derive_challenges(proof, pk.verifier_key, n, pub, t_eval=t_eval)
    assert PV.verify(n, vk, comms, ev, ch, pub_z, PG.g2_mul(TAU, PG.G2_GEN)) == (True, True)


def _small_circuit():
    b = M.Builder(64)
    s, v, x, y = b.var(True), b.var(True), b.var(True), b.var(True)
    sx, sy, qx, qy = b.var(True), b.var(True), b.var(True), b.var(True)
    p = b.fixed_base(s, 8, (sx, sy))
    b.equal(s, b.wires[3][b.gadgets[-1][2] + 8])
    b.equal(v, b.range(v, 2))
    b.logic(x, y, 4, xor=True)
    b.curve_add(p, (qx, qy), level=1)
    arith = b.fill_arithmetic(2)

    def inputs(seed):
        rng = random.Random(seed)
        q = M.curve_point(1000 + seed)
        return {s: rng.getrandbits(7), v: rng.getrandbits(16), x: rng.getrandbits(8), y: rng.getrandbits(8), sx: 0, sy: 1,
                qx: q[0], qy: q[1], **arith}
    return b, inputs, v


def test_fill_end_to_end(ctx, oracle):
    import plonk_prototype_amd as pa
    from plonk_prototype_amd.field import fr_to_limbs
    b, inputs, v = _small_circuit()
    n = b.n
    ck = pa.CommitKey.setup(n + 9, fr_to_limbs(TAU), ctx, precompute=True)
    pk = _key(ctx, b, ck)
    try:
        models = [b.model(inputs(k)) for k in range(3)]
        only = [M.to_limbs(m[0]) for m in models]
        full = [M.to_limbs(m[1]) for m in models]
        sent = pa.prove(pk, ck, variables=only[0], fill=True, check=True)
        want = pa.prove(pk, ck, variables=full[0])
        assert sent.native_bytes == want.native_bytes and sent.challenges == want.challenges and len(sent.native_bytes) == 1040
        assert pa.prove(pk, ck, variables=only[0]).native_bytes != want.native_bytes       # the fill is opt-in
        _pairing_verifier_accepts(oracle, pk, sent, n, np.zeros((n, 4), np.uint64))
        got = pa.prove_batch(pk, ck, variables=only, fill=True, check=True)
        singles = [pa.prove(pk, ck, variables=f) for f in full]
        assert [g.native_bytes for g in got] == [s.native_bytes for s in singles]
        assert pk.check_witness(variables=only[1], fill=True).ok and not pk.check_witness(variables=only[1]).ok
        assert all(r.ok for r in pk.check_witnesses(variables=only, fill=True))
        # a device vector is filled in place
        d = pa.DeviceVector.from_host(ctx, np.ascontiguousarray(np.stack(only)).reshape(-1, 4))
        same, reps = pk.fill_gadgets(d)
        assert same is d and all(r.ok for r in reps) and np.array_equal(d.to_host().reshape(3, -1, 4), np.stack(full))
        d.free()
        # an input that does not fit: nothing is proved, the error names proof, gadget and reason
        bad = dict(inputs(1))
        bad[v] = 1 << 16
        with pytest.raises(pa.GadgetInputError) as e:
            pa.prove_batch(pk, ck, variables=[only[0], M.to_limbs(b.model(bad)[0])], fill=True)
        assert set(e.value.reports) == {1} and e.value.report.first_gadget == 1 and e.value.report.first_reason == "too_wide"
        assert "proof 1" in str(e.value) and "gadget 1" in str(e.value) and "range" in str(e.value)
        with pytest.raises(pa.GadgetInputError):
            pa.prove(pk, ck, variables=M.to_limbs(b.model(bad)[0]), fill=True)
    finally:
        pk.free()


# ---------------------------------------------------------------------------------- 7. refusals
def test_refusals_leave_the_key_and_the_context_usable(ctx):
    import plonk_prototype_amd as pa
    from plonk_prototype_amd import _lib
    b, inputs, _ = _small_circuit()
    n, nv = b.n, b.num_vars
    pk = pa.preprocess(b.circuit(), ctx)
    lib, h = ctx._lib, ctx._h
    good = b.gadget_records()
    G = pa.Gadget
    fb_row, rg_row = b.gadgets[0][2], b.gadgets[1][2]
    free_row = n - 2                         # an arithmetic row: no widget selector

    def refuse(recs, names):
        raw = (_lib.Gadget * len(recs))(*[g._raw() for g in recs])
        out = C.c_size_t(12345)
        assert lib.pm_plonk_key_set_gadgets(h, pk._h, raw, len(recs), C.byref(out)) == _lib.PM_ERR_BAD_ARG
        assert f"gadget {names}:" in lib.pm_last_error(h).decode(), lib.pm_last_error(h).decode()

    try:
        assert pk.set_gadgets(good) > 0
        only, full, _ = b.model(inputs(4))
        refuse([good[3], good[0]], 1)                                             # levels fall
        refuse([good[0], G.range(n - 2, 2, 1)], 1)                                # rows leave [0, n)
        refuse([good[0], G.fixed_base(n - 8, 8, 1)], 1)                           # ... the trailing row included
        refuse([good[0], G.curve_add(n - 1)], 1)
        refuse([G.range(free_row - 1, 1, 1)], 0)                                  # a claimed row without q_range
        refuse([good[0], G.logic(rg_row, 2, 1, 2)], 1)                            # ... with another widget's selector
        refuse([good[0], good[1], G.curve_add(fb_row)], 2)
        refuse([G.fixed_base(fb_row, 8, nv)], 0)                                  # in_var >= num_vars
        refuse([G.logic(b.gadgets[2][2], 4, 1, 0xFFFFFFFF, xor=True)], 0)
        refuse([good[0], G.range(rg_row, 0, 1)], 1)                               # count = 0
        refuse([G.fixed_base(fb_row, 257, 1)], 0)                                 # more than MAX_ROUNDS
        refuse([pa.Gadget(7, 0, 1)], 0)                                           # unknown kind
        refuse([good[0], G.range(free_row - 1, 1, 1), G.range(n - 2, 2, 1)], 1)   # the lowest offender: selector before rows
        refuse([good[0], G.range(n - 2, 2, 1), G.range(free_row - 1, 1, 1)], 1)
        # a key that was not built from wires
        dense = pa.preprocess(pa.synthetic.chain_circuit(16, 1)[0], ctx)
        raw = (_lib.Gadget * 1)(good[0]._raw())
        assert lib.pm_plonk_key_set_gadgets(h, dense._h, raw, 1, None) == _lib.PM_ERR_BAD_ARG
        d16 = pa.DeviceVector(ctx, 64)
        assert lib.pm_plonk_fill_gadgets_dev(h, dense._h, d16._p, 64, 1, None, None) == _lib.PM_ERR_BAD_ARG
        d16.free()
        dense.free()
        # the fill's own refusals
        d = pa.DeviceVector.from_host(ctx, M.to_limbs(only))
        rep = (_lib.GadgetReport * 1)()
        assert lib.pm_plonk_fill_gadgets_dev(h, pk._h, d._p, nv, 0, rep, None) == _lib.PM_ERR_BAD_ARG
        assert lib.pm_plonk_fill_gadgets_dev(h, pk._h, d._p, nv, _lib.PLONK_MAX_BATCH + 1, rep, None) == _lib.PM_ERR_BAD_ARG
        assert lib.pm_plonk_fill_gadgets_dev(h, pk._h, d._p, nv - 1, 1, rep, None) == _lib.PM_ERR_BAD_ARG
        assert lib.pm_plonk_fill_gadgets_dev(h, pk._h, None, nv, 1, rep, None) == _lib.PM_ERR_BAD_ARG
        assert lib.pm_plonk_fill_gadgets_dev(h, None, d._p, nv, 1, rep, None) == _lib.PM_ERR_BAD_ARG
        # after all that the key still has the table it was given first, and the context works
        assert lib.pm_plonk_fill_gadgets_dev(h, pk._h, d._p, nv, 1, None, None) == 0          # asynchronous form
        ctx.sync()
        assert np.array_equal(d.to_host(), M.to_limbs(full))
        # cleared: no table, the fill is refused; set again: it works
        assert pk.set_gadgets([]) == 0
        assert lib.pm_plonk_fill_gadgets_dev(h, pk._h, d._p, nv, 1, rep, None) == _lib.PM_ERR_BAD_ARG
        assert pk.set_gadgets(good) > 0 and pk.set_gadgets(good) > 0                          # idempotent
        got, reps = pk.fill_gadgets(M.to_limbs(only))
        assert reps[0].ok and np.array_equal(got, M.to_limbs(full))
        d.free()
    finally:
        pk.free()
