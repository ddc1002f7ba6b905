"""The witness check (pm_plonk_check_witness / _batch) against a Python-integer restatement of its
definition: row masks, counts and the first failing row on satisfied witnesses, single-wire faults, the wrap-around of the
"next" row, public inputs, failures in several workgroups, batches, the refusals of the contract and ``prove(check=True)``.

The reference evaluates each widget as the oracle's widget_* sum with four fixed random 250-bit separation challenges: a
widget bit is set when the selector is non-zero and that sum is non-zero, which agrees with "some summand is non-zero"
except with probability about 2^-250."""
import ctypes as C
import random

import numpy as np
import pytest

from oracle import plonk_rounds_oracle as O

pytestmark = pytest.mark.gpu
R = O.R
_rng = random.Random(0x5EED_C4EC)
SEPS = [_rng.getrandbits(250) for _ in range(4)]
ARITH, RANGE, LOGIC, FIXED, VAR, COPY = 1, 2, 4, 8, 16, 32
NAMES = ("arith", "range", "logic", "fixed_base", "var_base", "copy")
TAU = 0x1F2E3D4C5B6A79880123456789ABCDEF0FEDCBA9876543210A1B2C3D4E5F6071 % R
_CACHE: dict = {}


# ---------------------------------------------------------------------------------- the reference
def _ints(a, n):
    from plonk_prototype_amd.field import fr_vec_from_limbs
    return [0] * n if a is None else fr_vec_from_limbs(a)


def _circuit_ints(circuit):
    n = circuit.n
    c = {k: _ints(getattr(circuit, k), n) for k in O.SELECTORS}
    c["n"] = n
    c["sigma"] = [int(q) for q in np.asarray(circuit.sigma_index).reshape(-1)]
    return c


def ref_masks(c, w, pi):
    """c: _circuit_ints; w: the 4n wire values (position j n + i); pi: n values -> the mask of every row, [n] uint8."""
    n, out = c["n"], np.zeros(c["n"], np.uint8)
    for i in range(n):
        nx = (i + 1) % n
        a, b, cc, d = w[i], w[n + i], w[2 * n + i], w[3 * n + i]
        an, bn, dn = w[nx], w[n + nx], w[3 * n + nx]
        ql, qr, qc = c["q_l"][i], c["q_r"][i], c["q_c"][i]
        m = 0
        arith = c["q_m"][i] * a * b + ql * a + qr * b + c["q_o"][i] * cc + c["q_4"][i] * d + qc
        if (c["q_arith"][i] * arith + pi[i]) % R:
            m |= ARITH
        if c["q_range"][i] and O.widget_range(SEPS[0], a, b, cc, d, dn):
            m |= RANGE
        if c["q_logic"][i] and O.widget_logic(SEPS[1], a, an, b, bn, cc, d, dn, qc):
            m |= LOGIC
        if c["q_fixed_group_add"][i] and O.widget_fixed_base(SEPS[2], a, an, b, bn, cc, d, dn, ql, qr, qc):
            m |= FIXED
        if c["q_variable_group_add"][i] and O.widget_variable_base(SEPS[3], a, an, b, bn, cc, d, dn):
            m |= VAR
        if any(w[j * n + i] != w[c["sigma"][j * n + i]] for j in range(4)):
            m |= COPY
        out[i] = m
    return out


def _assert_report(rep, want, what=""):
    """Every field of a WitnessReport (with row_masks) against the reference masks."""
    assert rep.row_masks is not None and rep.row_masks.dtype == np.uint8
    assert np.array_equal(rep.row_masks, want), f"{what}: masks {np.flatnonzero(rep.row_masks != want)[:8]}"
    bad = np.flatnonzero(want)
    assert rep.failed_rows == bad.size, what
    assert rep.ok == (bad.size == 0), what
    assert rep.counts == {nm: int(np.count_nonzero(want & (1 << k))) for k, nm in enumerate(NAMES)}, what
    if bad.size:
        assert rep.first_row == int(bad[0]), what
        assert rep.first_reasons == tuple(nm for k, nm in enumerate(NAMES) if want[bad[0]] >> k & 1), what
    else:
        assert rep.first_row is None and rep.first_reasons == (), what


def _bump(witness, j, i, by=1):
    """A copy of the [4, n, 4] witness with wire j of row i increased by `by`."""
    from plonk_prototype_amd.field import fr_from_limbs, fr_to_limbs
    w = np.array(witness, dtype=np.uint64, copy=True)
    w[j, i] = fr_to_limbs(fr_from_limbs(w[j, i]) + by)
    return w


def _case(name, n, seed=1):
    """(circuit, witness, pi, circuit ints, witness ints, pi ints) of a synthetic circuit, built once per session."""
    import plonk_prototype_amd as pa
    key = (name, n, seed)
    if key not in _CACHE:
        circuit, wit, pi = getattr(pa.synthetic, name)(n, seed)
        _CACHE[key] = (circuit, wit, pi, _circuit_ints(circuit), _ints(wit.reshape(-1, 4), 4 * n), _ints(pi, n))
    return _CACHE[key]


def _key(ctx, circuit):
    import plonk_prototype_amd as pa
    pk = pa.ProverKey(circuit, ctx)
    pk.enable_check()
    return pk


def _raw_report(ctx, pk, witness, pos, val):
    """pm_plonk_check_witness as a C caller sees it: (status, pm_plonk_witness_report)."""
    import plonk_prototype_amd as pa
    from plonk_prototype_amd import _lib
    d = pa.DeviceVector.from_host(ctx, np.ascontiguousarray(witness, dtype=np.uint64).reshape(-1, 4))
    raw = _lib.WitnessReport()
    pos, val = np.ascontiguousarray(pos, np.uint64), np.ascontiguousarray(val, np.uint64)
    rc = ctx._lib.pm_plonk_check_witness(ctx._h, pk._h, d._p, pos.ctypes.data_as(_lib.u64p) if pos.size else None,
                                         val.ctypes.data_as(_lib.u64p) if pos.size else None, pos.size, C.byref(raw), None)
    d.free()
    return rc, raw


# ---------------------------------------------------------------------------------- satisfied witnesses
@pytest.mark.parametrize("name,n", [("chain_circuit", 4), ("chain_circuit", 16), ("chain_circuit", 1024), ("boolean_circuit", 64),
                                    ("mixed_circuit", 32), ("mixed_circuit", 64), ("mixed_circuit", 1024)])
def test_satisfied_witness_gives_an_empty_report(ctx, name, n):
    from plonk_prototype_amd.prover import sparse_public_inputs
    circuit, wit, pi, ci, wi, pii = _case(name, n)
    assert not ref_masks(ci, wi, pii).any(), "the reference itself must accept the synthetic witness"
    pk = _key(ctx, circuit)
    rep = pk.check_witness(wit, pi, masks=True)
    _assert_report(rep, np.zeros(n, np.uint8), f"{name}({n})")
    rc, raw = _raw_report(ctx, pk, wit, *sparse_public_inputs(pi))
    assert rc == 0 and raw.failed_rows == 0 and raw.first_row == 2**64 - 1 and raw.first_mask == 0 and raw.reserved == 0
    assert list(raw.count) == [0] * 6
    assert pk.check_witness(wit, pi).row_masks is None
    pk.free()


# ---------------------------------------------------------------------------------- single-wire faults
def test_single_wire_faults_on_mixed_32(ctx):
    from plonk_prototype_amd.field import fr_to_limbs
    n = 32
    circuit, wit, pi, ci, wi, pii = _case("mixed_circuit", n)
    pk = _key(ctx, circuit)
    union = 0
    for j in range(4):
        for i in range(n):
            w_ints = list(wi)
            w_ints[j * n + i] = (w_ints[j * n + i] + 1) % R
            want = ref_masks(ci, w_ints, pii)
            w = np.array(wit, dtype=np.uint64, copy=True)
            w[j, i] = fr_to_limbs(w_ints[j * n + i])
            _assert_report(pk.check_witness(w, pi, masks=True), want, f"wire {j} of row {i}")
            union |= int(np.bitwise_or.reduce(want))
    assert union == 0b111111, "the cases must reach all six reasons"
    pk.free()


# ---------------------------------------------------------------------------------- the last row's "next" is row 0
def test_next_row_wraps_around(ctx):
    import plonk_prototype_amd as pa
    from plonk_prototype_amd.field import fr_to_limbs, fr_vec_to_limbs
    n = 4
    quads = [1, 3, 0, 2, 2, 1, 0, 3]       # the last quad is 3: one more is no quad
    acc = [0]
    for q in quads:
        acc.append(4 * acc[-1] + q)
    rows = [[0, 0, 0, acc[8]], [0, 0, 0, 0], [acc[3], acc[2], acc[1], acc[0]], [acc[7], acc[6], acc[5], acc[4]]]
    wit = np.stack([fr_vec_to_limbs([r[j] for r in rows]) for j in range(4)])
    zero = np.zeros((n, 4), np.uint64)
    circuit = pa.Circuit(sigma_index=np.arange(4 * n, dtype=np.int64).reshape(4, n), q_m=zero, q_l=zero, q_r=zero, q_o=zero,
                         q_c=zero, q_4=zero, q_arith=zero, q_range=fr_vec_to_limbs([0, 0, 1, 1]))
    ci = _circuit_ints(circuit)
    wi = _ints(wit.reshape(-1, 4), 4 * n)
    assert not ref_masks(ci, wi, [0] * n).any()
    pk = _key(ctx, circuit)
    _assert_report(pk.check_witness(wit, None, masks=True), np.zeros(n, np.uint8), "as built")
    w = np.array(wit, copy=True)
    w[3, 0] = fr_to_limbs(acc[8] + 1)
    w_ints = list(wi)
    w_ints[3 * n] = acc[8] + 1
    want = ref_masks(ci, w_ints, [0] * n)
    assert want.tolist() == [0, 0, 0, RANGE], "d of row 0 is row 3's d_next and nothing else"
    rep = pk.check_witness(w, None, masks=True)
    _assert_report(rep, want, "d of row 0 changed")
    assert rep.first_row == 3 and rep.first_reasons == ("range",) and rep.failed_rows == 1
    pk.free()


# ---------------------------------------------------------------------------------- public inputs
def test_public_inputs(ctx):
    import plonk_prototype_amd as pa
    from plonk_prototype_amd import _lib
    from plonk_prototype_amd.field import fr_to_limbs
    n = 16
    circuit, wit, pi = pa.synthetic.chain_circuit(n, 5, public_rows=(0, 9))
    ci, wi, pii = _circuit_ints(circuit), _ints(wit.reshape(-1, 4), 4 * n), _ints(pi, n)
    pk = _key(ctx, circuit)
    _assert_report(pk.check_witness(wit, pi, masks=True), np.zeros(n, np.uint8), "right public inputs")
    bad = np.array(pi, copy=True)
    bad[9] = fr_to_limbs(pii[9] + 1)
    bad_ints = list(pii)
    bad_ints[9] += 1
    want = ref_masks(ci, wi, bad_ints)
    assert want.tolist() == [ARITH if i == 9 else 0 for i in range(n)]
    _assert_report(pk.check_witness(wit, bad, masks=True), want, "wrong public input")
    # a missing public input is a wrong one
    none = ref_masks(ci, wi, [0] * n)
    assert set(np.flatnonzero(none).tolist()) == {0, 9}
    _assert_report(pk.check_witness(wit, None, masks=True), none, "no public inputs")
    # more than a handful of (position, value) pairs, with repeats: the last value of a position counts
    pos = np.array([0, 9, 9] + list(range(1, 9)) * 3, np.uint64)
    val = np.stack([bad[0], bad[9], pi[9]] + [np.zeros(4, np.uint64)] * 24)
    _assert_report(pk.check_witness(wit, (pos, val), masks=True), np.zeros(n, np.uint8), "repeated positions")
    with pytest.raises(pa.Error) as e:
        pk.check_witness(wit, (np.array([n], np.uint64), pi[:1]))
    assert e.value.code == _lib.PM_ERR_LENGTH
    pk.free()


# ---------------------------------------------------------------------------------- many failures, several workgroups
def test_many_failures_across_workgroups(ctx):
    n = 1024
    circuit, wit, pi, ci, wi, pii = _case("mixed_circuit", n)
    w, w_ints = np.array(wit, copy=True), list(wi)
    hits = [(0, r) for r in range(3, 43, 2)] + [(2, r) for r in range(n - 24, n - 4)] + [(3, n - 1)]   # first and last workgroup
    for j, i in hits:
        w = _bump(w, j, i, 1 + i)
        w_ints[j * n + i] = (w_ints[j * n + i] + 1 + i) % R
    want = ref_masks(ci, w_ints, pii)
    assert np.flatnonzero(want)[0] < 256 and np.flatnonzero(want)[-1] >= n - 256 and np.count_nonzero(want) >= 40
    pk = _key(ctx, circuit)
    _assert_report(pk.check_witness(w, pi, masks=True), want, "41 corrupted wires")
    pk.free()


# ---------------------------------------------------------------------------------- batches
def test_batch_equals_single_calls(ctx):
    import plonk_prototype_amd as pa
    n = 64
    circuit, _, _ = pa.synthetic.chain_circuit(n, 3)
    pairs = pa.synthetic.chain_witnesses(n, 3, count=3, witness_seed=4, public_rows=[(0,), (5, 6), ()])
    wits = [w for w, _ in pairs]
    wits[1] = _bump(_bump(wits[1], 2, 40), 0, 11)
    pis = [p for _, p in pairs]
    ci = _circuit_ints(circuit)
    pk = _key(ctx, circuit)
    bytes_1 = pk.enable_check()
    singles = [pk.check_witness(w, p, masks=True) for w, p in zip(wits, pis)]
    for b, (s, w, p) in enumerate(zip(singles, wits, pis)):
        _assert_report(s, ref_masks(ci, _ints(w.reshape(-1, 4), 4 * n), _ints(p, n)), f"single {b}")
    assert singles[0].ok and not singles[1].ok and singles[2].ok
    got = pk.check_witnesses(wits, pis, masks=True)
    assert len(got) == 3
    for g, s in zip(got, singles):
        assert (g.ok, g.failed_rows, g.first_row, g.first_reasons, g.counts) == (s.ok, s.failed_rows, s.first_row,
                                                                                 s.first_reasons, s.counts)
        assert np.array_equal(g.row_masks, s.row_masks)
    assert pk.enable_check() > bytes_1, "the scratch has grown to three witnesses"
    # a smaller batch on the grown buffers, witnesses already on the device
    d = pa.DeviceVector.from_host(ctx, np.ascontiguousarray(wits[1]).reshape(4 * n, 4))
    one = pk.check_witnesses(d, [pis[1]], masks=True)
    assert len(one) == 1 and np.array_equal(one[0].row_masks, singles[1].row_masks) and one[0].counts == singles[1].counts
    d.free()
    got = pk.check_witnesses(wits[::-1], pis[::-1])
    assert [g.ok for g in got] == [True, False, True] and got[1].first_row == singles[1].first_row
    pk.free()


# ---------------------------------------------------------------------------------- refusals
def test_errors(ctx):
    import plonk_prototype_amd as pa
    from plonk_prototype_amd import _lib
    n = 16
    circuit, wit, pi = pa.synthetic.chain_circuit(n, 2)
    pk = pa.ProverKey(circuit, ctx)
    with pytest.raises(pa.Error) as e:
        pk.check_witness(wit, pi)
    assert e.value.code == _lib.PM_ERR_BAD_ARG
    # another permutation: two positions that hold different variables trade their successors
    other = np.array(pk.sigma_index, copy=True)
    other[[0, n - 1]] = other[[n - 1, 0]]
    assert sorted(other.tolist()) == list(range(4 * n)) and not np.array_equal(other, pk.sigma_index)
    out = C.c_size_t(0)
    enable = lambda idx: ctx._lib.pm_plonk_key_enable_check(ctx._h, pk._h, idx.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(out))   # noqa: E731
    assert enable(other) == _lib.PM_ERR_BAD_ARG
    with pytest.raises(pa.Error):
        pk.check_witness(wit, pi)                      # the refused call enabled nothing
    out_of_range = np.array(pk.sigma_index, copy=True)
    out_of_range[3] = 4 * n
    assert enable(out_of_range) == _lib.PM_ERR_BAD_ARG
    first = pk.enable_check()
    assert first > 0 and pk.enable_check() == first
    assert enable(other) == _lib.PM_ERR_BAD_ARG         # also on an enabled key
    assert pk.check_witness(wit, pi).ok
    raw = _lib.WitnessReport()
    d = pa.DeviceVector.from_host(ctx, np.ascontiguousarray(wit).reshape(4 * n, 4))
    assert ctx._lib.pm_plonk_check_witness(ctx._h, pk._h, None, None, None, 0, C.byref(raw), None) == _lib.PM_ERR_BAD_ARG
    assert ctx._lib.pm_plonk_check_witness(ctx._h, pk._h, d._p, None, None, 0, None, None) == _lib.PM_ERR_BAD_ARG
    assert ctx._lib.pm_plonk_check_witness(ctx._h, pk._h, d._p, None, None, 1, C.byref(raw), None) == _lib.PM_ERR_BAD_ARG
    reps = (_lib.WitnessReport * 1)()
    for batch in (0, _lib.PLONK_MAX_BATCH + 1):
        assert ctx._lib.pm_plonk_check_witness_batch(ctx._h, pk._h, batch, d._p, None, None, None, reps, None) == _lib.PM_ERR_BAD_ARG
    d.free()
    pk.free()


# ---------------------------------------------------------------------------------- prove(check=True)
def test_prove_with_check(ctx):
    import plonk_prototype_amd as pa
    from plonk_prototype_amd.field import fr_to_limbs
    n = 64
    ck = pa.CommitKey.setup(n - 1, fr_to_limbs(TAU), ctx)
    circuit, wit, pi, ci, wi, pii = _case("mixed_circuit", n)
    pk = pa.preprocess(circuit, ctx, ck)
    plain = pa.prove(pk, ck, wit, pi)
    assert not pk._check_enabled
    assert pa.prove(pk, ck, wit, pi, check=True).native_bytes == plain.native_bytes    # enables the check on first use
    assert pk._check_enabled
    assert pa.prove(pk, ck, wit, pi, check=True).native_bytes == plain.native_bytes    # on an enabled key
    assert pa.prove(pk, ck, wit, pi).native_bytes == plain.native_bytes                # the default path on an enabled key
    bad = _bump(wit, 1, 40)
    w_ints = list(wi)
    w_ints[n + 40] += 1
    want = ref_masks(ci, w_ints, pii)
    with pytest.raises(pa.UnsatisfiedWitness) as e:
        pa.prove(pk, ck, bad, pi, check=True)
    rep = e.value.report
    first = int(np.flatnonzero(want)[0])
    assert rep.first_row == first and rep.failed_rows == np.count_nonzero(want)
    assert rep.first_reasons == tuple(nm for k, nm in enumerate(NAMES) if want[first] >> k & 1)
    assert f"row {first}" in str(e.value) and rep.first_reasons[0] in str(e.value)
    assert len(pa.prove(pk, ck, bad, pi).native_bytes) == 1040, "without the check the prover takes any witness"
    pk.free()
    # the batch prover names the failing member
    circuit, _, _ = pa.synthetic.chain_circuit(n, 3)
    pairs = pa.synthetic.chain_witnesses(n, 3, count=3, witness_seed=6)
    wits, pis = [w for w, _ in pairs], [p for _, p in pairs]
    pk = pa.preprocess(circuit, ctx, ck)
    plain = pa.prove_batch(pk, ck, wits, pis)
    checked = pa.prove_batch(pk, ck, wits, pis, check=True)
    assert [p.native_bytes for p in checked] == [p.native_bytes for p in plain]
    wits[2] = _bump(wits[2], 2, 17)          # c of gate 17 = variable 18: the gate fails, and so do its copies
    with pytest.raises(pa.UnsatisfiedWitness) as e:
        pa.prove_batch(pk, ck, wits, pis, check=True)
    assert list(e.value.reports) == [2] and e.value.report is e.value.reports[2]
    want = ref_masks(_circuit_ints(circuit), _ints(wits[2].reshape(-1, 4), 4 * n), _ints(pis[2], n))
    assert e.value.report.first_row == int(np.flatnonzero(want)[0]) == 17
    assert "witness 2" in str(e.value) and "row 17" in str(e.value)
    pk.free()
