"""Native Poseidon on the GPU: pm_hades_permute_dev, pm_poseidon_hash_dev, pm_poseidon_merkle_dev and
pm_poseidon_merkle_paths_dev in both kernel forms against the big-integer model of tests/poseidon_model.py, against the host
form and against what the HADES gadget fills -- every comparison is byte equality."""
import ctypes as C
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hades_circuits as HC  # noqa: E402
import hades_model as HM  # noqa: E402
import poseidon_model as PM  # noqa: E402

pytestmark = pytest.mark.gpu
R = PM.R
FORMS = ("thread", "wave", "auto")
SIZES = (1, 2, 12, 13, 63, 64, 65, 130)
_CACHE = {}


def _p(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint64))


def _consts(shape, per_round, seed=None):
    """-> (ark, mds) as integers and as limbs, built once per (shape, per_round)"""
    key = (shape, per_round, seed)
    if key not in _CACHE:
        rounds = shape[0]
        ark, mds = PM.constants(rounds, rounds if per_round else 1, 1000 * rounds + per_round if seed is None else seed)
        a, m, _ = PM.flat(ark, mds)
        _CACHE[key] = (ark, mds, PM.to_limbs(a), PM.to_limbs(m))
    return _CACHE[key]


def _hades(ctx, shape, per_round, seed=None):
    import plonk_prototype_amd as pa
    ark, mds, a, m = _consts(shape, per_round, seed)
    return pa.Hades(ctx, a, m, *shape), ark, mds


def _states(n, seed):
    rng = random.Random(seed)
    edge = [[0] * 5, [R - 1] * 5, [0, R - 1, 1, R - 2, 0]]
    return [edge[i] if i < len(edge) and n > 3 else [rng.randrange(R) for _ in range(5)] for i in range(n)]


# ---------------------------------------------------------------------------------- 1. the permutation
@pytest.mark.parametrize("per_round", (False, True))
@pytest.mark.parametrize("shape", PM.SHAPES)
def test_permute_against_the_model(ctx, shape, per_round):
    h, ark, mds = _hades(ctx, shape, per_round)
    try:
        assert (h.rounds, h.full_rounds, h.n_mds) == (shape[0], shape[1], shape[0] if per_round else 1)
        states = _states(max(SIZES), shape[0])
        want = PM.to_limbs([x for s in states for x in HM.hades_model(s, ark, mds, *shape)]).reshape(-1, 5, 4)
        given = PM.to_limbs([x for s in states for x in s]).reshape(-1, 5, 4)
        for n in SIZES:
            for form in FORMS:
                got = h.permute(given[:n], form=form)
                assert got.shape == (n, 5, 4) and got.tobytes() == want[:n].tobytes(), (shape, per_round, n, form)
    finally:
        h.free()


def test_permute_many_against_the_host_form(ctx):
    """n = 2^14 at (67, 8): more than one block in both forms, the THREAD form on every lane of many waves"""
    import plonk_prototype_amd as pa
    shape, n = (67, 8), 1 << 14
    h, _, _ = _hades(ctx, shape, False)
    _, _, a, m = _consts(shape, False)
    lib = pa.load()
    rng = np.random.default_rng(14)
    given = PM.to_limbs([int.from_bytes(rng.bytes(32), "little") % R for _ in range(5 * n)]).reshape(n, 5, 4)
    want = given.copy()
    for i in range(n):
        assert lib.pm_hades_permute_host(67, 8, _p(a), _p(m), 1, want[i].ctypes.data_as(C.POINTER(C.c_uint64))) == 0
    try:
        auto = h.permute(given)
        assert auto.tobytes() == want.tobytes()
        assert h.permute(given, form="thread").tobytes() == want.tobytes()
        assert h.permute(given, form="wave").tobytes() == want.tobytes()
        assert h.permute(given).tobytes() == auto.tobytes()                 # determinism: two calls, the same bytes
    finally:
        h.free()


# ---------------------------------------------------------------------------------- 2. the sponge
@pytest.mark.parametrize("capacity", (0, 0xabcdef << 100))
def test_hash_for_every_length_and_stride(ctx, capacity):
    shape = (9, 4)
    h, ark, mds = _hades(ctx, shape, True)
    import plonk_prototype_amd as pa
    rng = random.Random(9 + capacity % 7)
    try:
        for length in range(1, 10):
            msgs = [[rng.randrange(R) for _ in range(length)] for _ in range(65)]
            msgs[1] = [0] * length
            msgs[2] = [R - 1] * length
            want = PM.to_limbs([PM.sponge(msg, ark, mds, *shape, capacity) for msg in msgs])
            arr = PM.to_limbs([x for msg in msgs for x in msg]).reshape(65, length, 4)
            stride = length + 3
            padded = np.full((65, stride, 4), 0xffffffffffffffff, np.uint64)        # the gaps are not canonical: never read
            padded[:, :length] = arr
            for n in (1, 65):
                for form in ("thread", "wave"):
                    assert h.hash(arr[:n], capacity, form=form).tobytes() == want[:n].tobytes(), (length, n, form)
                    d, out = pa.DeviceVector.from_host(ctx, padded[:n].reshape(-1, 4)), pa.DeviceVector(ctx, n)
                    h.hash_dev(d.ptr, length, n, out.ptr, capacity, msg_stride=stride, form=form)
                    assert out.to_host().tobytes() == want[:n].tobytes(), (length, n, form, "stride")
                    d.free(), out.free()
            assert h.hash(arr, capacity).tobytes() == want.tobytes()
            assert h.hash(arr[0], capacity).tobytes() == want[:1].tobytes()       # one message
    finally:
        h.free()


# ---------------------------------------------------------------------------------- 3. the constants of a key's gadget
def _gadget_io(b, rec):
    """-> (the five input variable ids, the five output variable ids) of the HADES record"""
    r0, rows = rec.first_row, HM.hades_rows(rec.count, rec.param)
    ins = [b.wires[0][r0 + j] for j in range(5)]
    outs = [b.wires[2][r0 + rows - 10 + 2 * i + 1] for i in range(5)]
    return ins, outs


def _value(assignment, var):
    return np.zeros(4, np.uint64) if var in (None, HM.NO_VAR) else assignment[var]


def test_from_key_equals_the_filled_gadgets(ctx):
    import plonk_prototype_amd as pa
    b, _, models = HC.shapes_case()
    recs = b.gadget_records()
    pk = pa.preprocess(b.circuit(), ctx)
    handles = []
    try:
        assert pk.set_gadgets(recs) > 0
        only = [HM.to_limbs(m[0]) for m in models[:8]]
        filled, reports = pk.fill_gadgets(only)
        assert all(r.ok for r in reports)
        hades = [(i, g) for i, g in enumerate(recs) if g.kind == 7]
        assert [(g.count, g.param) for _, g in hades] == list(HC.SHAPES)
        want = {}
        for i, g in hades:
            h = pa.Hades.from_key(pk, i)
            handles.append((i, g, h))
            assert (h.rounds, h.full_rounds, h.n_mds) == (g.count, g.param, g.count)
            ins, outs = _gadget_io(b, g)
            given = np.stack([np.stack([_value(a, v) for v in ins]) for a in filled])
            want[i] = np.stack([np.stack([a[v] for v in outs]) for a in filled])
            for form in FORMS:
                assert h.permute(given, form=form).tobytes() == want[i].tobytes(), (i, form)
        with pytest.raises(pa.Error) as e:
            pa.Hades.from_key(pk, 0)                                          # the glue row: an ARITH gadget
        assert e.value.code == -1
        with pytest.raises(pa.Error):
            pa.Hades.from_key(pk, len(recs))
        # the handles own their constants: the table goes, then the key
        pk.set_gadgets([])
        with pytest.raises(pa.Error):
            pa.Hades.from_key(pk, hades[0][0])                                # no table
        i, g, h = handles[2]
        ins, _ = _gadget_io(b, g)
        given = np.stack([np.stack([_value(a, v) for v in ins]) for a in filled])
        assert h.permute(given).tobytes() == want[i].tobytes()
        pk.free()
        pk = None
        assert h.permute(given, form="wave").tobytes() == want[i].tobytes()
    finally:
        for _, _, h in handles:
            h.free()
        if pk is not None:
            pk.free()


def test_from_key_sponge_public_input(ctx):
    """A sponge of three inputs (one chunk, padded) at (5, 2): its public input is minus what Hades.hash gives with the
    constants of the circuit's own permutation.  hades_circuits.sponge_case has two chunks whose permutations have DIFFERENT
    constants (the builder draws fresh ones per permutation), so there the two handles are chained by hand."""
    import plonk_prototype_amd as pa
    b = HM.Builder(256)
    ins = [b.var(True) for _ in range(3)]
    out = b.sponge(ins, 5, 2, level=0)
    pi_row = b.public_output(out)
    arith = b.fill_arithmetic(36)
    rng = random.Random(36)
    a = {**{v: rng.randrange(R) for v in ins}, **arith}
    _, full, reasons = b.model(a)
    assert not reasons
    recs = b.gadget_records()
    assert [g.kind for g in recs] == [4, 7]
    pk = pa.preprocess(b.circuit(), ctx)
    try:
        pk.set_gadgets(recs)
        h = pa.Hades.from_key(pk, 1)
        got = h.hash(HM.to_limbs([a[v] for v in ins]))
        pi = [0] * b.n
        pi[pi_row] = (-pa.field.fr_from_limbs(got[0])) % R
        assert pi[pi_row] == (-full[out]) % R
        pk.enable_check()
        assert pk.check_witness(variables=HM.to_limbs(b.model(a)[0]), public_inputs=HM.to_limbs(pi), fill=True).ok
        h.free()
    finally:
        pk.free()
    # two chunks, two sets of constants
    b, inputs, out, pi_row = HC.sponge_case()
    a = inputs(2)
    _, full, _ = b.model(a)
    recs = b.gadget_records()
    pk = pa.preprocess(b.circuit(), ctx)
    try:
        pk.set_gadgets(recs)
        h1, h2 = pa.Hades.from_key(pk, 1), pa.Hades.from_key(pk, 3)
        (r0, *_), (r1, *_) = b.permutations
        first = [full[b.wires[0][r0 + j]] for j in range(5)]
        s = pa.field.fr_vec_from_limbs(h1.permute(HM.to_limbs(first)))
        second = [full[b.wires[0][r1 + j]] for j in range(5)]
        assert s[0] == second[0] and s[4] == second[4] and (s[3] + 1) % R == second[3]
        s = pa.field.fr_vec_from_limbs(h2.permute(HM.to_limbs(second)))
        assert s[1] == full[out]
        h1.free(), h2.free()
    finally:
        pk.free()


# ---------------------------------------------------------------------------------- 4. trees and paths
def _leaves(count, seed):
    rng = random.Random(seed)
    return [0, R - 1] + [rng.randrange(R) for _ in range(count - 2)]


@pytest.mark.parametrize("height,form", [(1, "thread"), (1, "wave"), (2, "thread"), (2, "wave"), (3, "thread"), (3, "wave"),
                                         (5, "auto")])
def test_merkle_tree_and_paths(ctx, height, form):
    import plonk_prototype_amd as pa
    shape, capacity = (5, 2), (0 if height != 2 else 77)
    h, ark, mds = _hades(ctx, shape, height % 2 == 1)
    count = 4 ** height
    leaves = _leaves(count, height)
    levels = PM.tree(leaves, ark, mds, *shape, capacity)
    t = None
    try:
        t = h.merkle(PM.to_limbs(leaves), capacity, form=form)
        assert t.height == height and t.nodes.n == (count - 1) // 3
        assert t.nodes.to_host().tobytes() == PM.to_limbs(PM.flat_tree(levels)).tobytes()
        assert t.root.tobytes() == PM.to_limbs(levels[-1]).tobytes()
        assert t.level(height).to_host().tobytes() == PM.to_limbs(levels[-1]).tobytes()
        assert t.level(0).to_host().tobytes() == PM.to_limbs(leaves).tobytes()
        indices = [0, count - 1, count // 2 + 1, count // 2 + 1]
        got = t.paths(indices)
        assert got.shape == (4, height, 4, 4)
        assert got.tobytes() == PM.to_limbs([x for p in PM.paths(levels, indices) for lv in p for x in lv]).tobytes()
        for j, i in enumerate(indices):                                      # the root again, from the path the DEVICE gave
            path = [pa.field.fr_vec_from_limbs(got[j][l]) for l in range(height)]
            assert leaves[i] == path[0][i & 3]
            assert PM.root_from_path(path, i, ark, mds, *shape, capacity) == levels[-1][0]
        for bad in (count, count + 5, 1 << 63):
            with pytest.raises(pa.Error) as e:
                t.paths([1, bad, count + 1])
            assert e.value.code == -1 and "index 1 " in str(e.value)
        assert t.paths([]).shape == (0, height, 4, 4)
    finally:
        if t is not None:
            t.free()
        h.free()


def test_one_leaf_changes_exactly_its_path(ctx):
    shape, height = (5, 2), 3
    h, _, _ = _hades(ctx, shape, False)
    leaves = _leaves(64, 3)
    try:
        t1 = h.merkle(PM.to_limbs(leaves))
        i = 37
        changed = list(leaves)
        changed[i] = (changed[i] + 1) % R
        t2 = h.merkle(PM.to_limbs(changed))
        differs = (t1.nodes.to_host() != t2.nodes.to_host()).any(axis=1)
        on_path = np.zeros(21, bool)
        first = 0
        for l in range(1, height + 1):
            on_path[first + (i >> (2 * l))] = True
            first += 4 ** (height - l)
        assert differs.tolist() == on_path.tolist()
        assert h.merkle(PM.to_limbs(leaves)).nodes.to_host().tobytes() == t1.nodes.to_host().tobytes()   # determinism
    finally:
        h.free()


# ---------------------------------------------------------------------------------- 5. refusals
def test_refusals(ctx):
    import plonk_prototype_amd as pa
    from plonk_prototype_amd import _lib
    lib, c = ctx._lib, ctx._h
    ark, mds, a, m = _consts((5, 2), True)
    _, _, a1, m1 = _consts((5, 2), False)
    out = C.c_void_p()

    def create(rounds, full, a_, m_, k):
        rc = lib.pm_hades_params_create(c, rounds, full, _p(a_), _p(m_), k, C.byref(out))
        if rc == 0:
            lib.pm_hades_params_free(c, out)
        return rc

    assert create(5, 2, a, m, 5) == 0 and create(5, 2, a1, m1, 1) == 0 and create(1, 0, a, m, 1) == 0
    bad = _lib.PM_ERR_BAD_ARG
    assert create(5, 3, a, m, 5) == bad and "even" in lib.pm_last_error(c).decode()
    assert create(5, 6, a, m, 5) == bad and create(0, 0, a, m, 1) == bad and create(0, 0, a, m, 0) == bad
    assert create(5, 2, a, m, 2) == bad and create(5, 2, a, m, 0) == bad
    for v in (R, (1 << 256) - 1):
        bad_a, bad_m = a.copy(), m.copy()
        bad_a[24] = np.frombuffer(v.to_bytes(32, "little"), np.uint64)
        bad_m[124] = np.frombuffer(v.to_bytes(32, "little"), np.uint64)
        assert create(5, 2, bad_a, m, 5) == bad and "round key 24" in lib.pm_last_error(c).decode()
        assert create(5, 2, a, bad_m, 5) == bad and "matrix entry 124" in lib.pm_last_error(c).decode()
    assert lib.pm_hades_params_create(c, 5, 2, None, _p(m), 5, C.byref(out)) == bad
    assert lib.pm_hades_params_create(c, 5, 2, _p(a), None, 5, C.byref(out)) == bad
    assert lib.pm_hades_params_create(c, 5, 2, _p(a), _p(m), 5, None) == bad
    assert lib.pm_hades_params_create(None, 5, 2, _p(a), _p(m), 5, C.byref(out)) == bad
    assert lib.pm_hades_params_from_key(c, None, 0, C.byref(out)) == bad

    h = pa.Hades(ctx, a, m, 5, 2)
    d, o = pa.DeviceVector.from_host(ctx, PM.to_limbs(list(range(1, 21)))), pa.DeviceVector(ctx, 8)
    before = d.to_host().tobytes()
    cap = PM.to_limbs([0])
    idx = pa.DeviceVector.from_host(ctx, np.zeros((1, 4), np.uint64))
    try:
        vp = C.c_void_p
        assert lib.pm_hades_permute_dev(c, h._h, d._p, 4, 3, None) == bad                      # a bad flags value
        assert lib.pm_hades_permute_dev(c, h._h, d._p, 4, 0xffffffff, None) == bad
        assert lib.pm_hades_permute_dev(c, None, d._p, 4, 0, None) == bad
        assert lib.pm_hades_permute_dev(c, h._h, None, 4, 0, None) == bad
        assert lib.pm_hades_permute_dev(None, h._h, d._p, 4, 0, None) == bad
        assert lib.pm_hades_permute_dev(c, h._h, vp(d.ptr + 8), 1, 0, None) == bad             # not 16-byte aligned
        assert lib.pm_hades_permute_dev(c, h._h, None, 0, 0, None) == 0                        # n = 0: nothing to do
        assert lib.pm_poseidon_hash_dev(c, h._h, _p(cap), d._p, 0, 0, 4, o._p, 0, None) == bad  # msg_len = 0
        assert lib.pm_poseidon_hash_dev(c, h._h, _p(cap), d._p, 4, 3, 4, o._p, 0, None) == bad  # msg_stride < msg_len
        assert lib.pm_poseidon_hash_dev(c, h._h, _p(cap), d._p, 4, 4, 4, o._p, 7, None) == bad
        assert lib.pm_poseidon_hash_dev(c, h._h, None, d._p, 4, 4, 4, o._p, 0, None) == bad
        assert lib.pm_poseidon_hash_dev(c, h._h, _p(cap), None, 4, 4, 4, o._p, 0, None) == bad
        assert lib.pm_poseidon_hash_dev(c, h._h, _p(cap), d._p, 4, 4, 4, None, 0, None) == bad
        assert lib.pm_poseidon_hash_dev(c, h._h, _p(cap), d._p, 4, 4, 4, vp(d.ptr + 32 * 15), 0, None) == bad   # overlap
        not_canonical = np.frombuffer(R.to_bytes(32, "little"), np.uint64).copy()
        assert lib.pm_poseidon_hash_dev(c, h._h, _p(not_canonical), d._p, 4, 4, 4, o._p, 0, None) == bad
        assert lib.pm_poseidon_hash_dev(c, h._h, _p(cap), None, 4, 4, 0, None, 0, None) == 0
        for height in (0, 16):
            assert lib.pm_poseidon_merkle_dev(c, h._h, _p(cap), d._p, height, o._p, 0, None) == bad
            assert lib.pm_poseidon_merkle_paths_dev(c, d._p, o._p, height, idx._p, 1, o._p, None) == bad
        assert lib.pm_poseidon_merkle_dev(c, h._h, _p(cap), d._p, 1, o._p, 5, None) == bad
        assert lib.pm_poseidon_merkle_dev(c, h._h, _p(cap), None, 1, o._p, 0, None) == bad
        assert lib.pm_poseidon_merkle_dev(c, h._h, _p(cap), d._p, 1, None, 0, None) == bad
        assert lib.pm_poseidon_merkle_dev(c, h._h, _p(cap), d._p, 1, vp(d.ptr + 32), 0, None) == bad          # overlap
        assert lib.pm_poseidon_merkle_paths_dev(c, d._p, o._p, 1, None, 1, o._p, None) == bad
        assert lib.pm_poseidon_merkle_paths_dev(c, None, o._p, 1, idx._p, 1, o._p, None) == bad
        assert lib.pm_poseidon_merkle_paths_dev(c, d._p, o._p, 1, None, 0, None, None) == 0
        ctx.sync()
        assert d.to_host().tobytes() == before                                                # no refused call wrote
    finally:
        h.free(), d.free(), o.free(), idx.free()


# ---------------------------------------------------------------------------------- 6. streams
def test_a_caller_stream_and_a_fill_on_the_same_key(ctx):
    """Hashing with a key's constants on a caller stream uses nothing of the key or the context: a fill that follows writes
    the bytes it wrote before."""
    import plonk_prototype_amd as pa
    import torch
    b, _, models = HC.dusk_case()
    recs = b.gadget_records()
    pk = pa.preprocess(b.circuit(), ctx)
    try:
        pk.set_gadgets(recs)
        only, full = [HM.to_limbs(m[0]) for m in models], [HM.to_limbs(m[1]) for m in models]
        before, _ = pk.fill_gadgets(only)
        assert before.tobytes() == np.stack(full).tobytes()
        h = pa.Hades.from_key(pk, 1)
        ins, outs = _gadget_io(b, recs[1])
        given = np.stack([np.stack([_value(a, v) for v in ins]) for a in before])
        want = np.stack([np.stack([a[v] for v in outs]) for a in before])
        st = torch.cuda.Stream()
        d = pa.DeviceVector.from_host(ctx, given.reshape(-1, 4))
        h.permute_dev(d.ptr, given.shape[0], form="thread", stream=st.cuda_stream)
        after, reports = pk.fill_gadgets(only)
        st.synchronize()
        assert all(r.ok for r in reports) and after.tobytes() == before.tobytes()
        assert d.to_host().reshape(want.shape).tobytes() == want.tobytes()
        d.free(), h.free()
    finally:
        pk.free()
