"""The append-only Poseidon tree on the GPU: pm_poseidon_ledger_* in every kernel form against the
big-integer model of tests/ledger_tree_model.py and against the dense tree of pm_poseidon_merkle_dev.  Every comparison is byte equality."""
import ctypes as C
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ledger_tree_model as LM  # noqa: E402
import merkle_update_model as MU  # noqa: E402
import poseidon_model as PM  # noqa: E402

pytestmark = pytest.mark.gpu
R = PM.R
SHAPE = (5, 2)
FORMS = ("thread", "wave", "auto")
EMPTY = 0x9E3779B97F4A7C15 ** 3 % R                                              # an empty leaf that is not zero
_CONST = {}


def _p(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint64))


def _hades(ctx, per_round):
    """-> (the handle, ark, mds) at (5, 2): one matrix, or a matrix a round"""
    import plonk_prototype_amd as pa
    if per_round not in _CONST:
        _CONST[per_round] = PM.constants(SHAPE[0], SHAPE[0] if per_round else 1, 8100 + per_round)
    ark, mds = _CONST[per_round]
    a, m, _ = PM.flat(ark, mds)
    return pa.Hades(ctx, PM.to_limbs(a), PM.to_limbs(m), *SHAPE), ark, mds


def _limbs(values):
    return PM.to_limbs(list(values)) if len(values) else np.zeros((0, 4), np.uint64)


def _root_dev(ctx, t):
    import plonk_prototype_amd as pa
    d = pa.DeviceVector.from_host(ctx, np.zeros((1, 4), np.uint64))
    try:
        t.root_dev(d.ptr)
        ctx.sync()
        return d.to_host()[0]
    finally:
        d.free()


def _probe(count):
    return sorted({0, count // 2, count - 1}) if count else []


def _paths_bytes(model, indices):
    return _limbs([x for p in model.paths(indices) for lv in p for x in lv]).tobytes()


def _assert_equals_model(ctx, t, model, tag=""):
    """every stored prefix, the root through both calls, the paths of {0, count // 2, count - 1}"""
    assert t.count == model.count, tag
    for l in range(model.height + 1):
        lv = t.level(l)
        assert lv.n == len(model.levels[l]) == LM.width(model.count, l), (tag, l)
        assert lv.to_host().tobytes() == _limbs(model.levels[l]).tobytes(), (tag, l)
    want = _limbs([model.root])[0].tobytes()
    assert t.root.tobytes() == want and _root_dev(ctx, t).tobytes() == want, tag
    probe = _probe(model.count)
    assert t.paths(probe).tobytes() == _paths_bytes(model, probe), tag


# ---------------------------------------------------------------------------------- 1. a sequence of appends
@pytest.mark.parametrize("capacity,empty_leaf,per_round", [(0, 0, False), (77, EMPTY, True)], ids=["zeros", "capacity77-per-round"])
def test_append_sequence(ctx, capacity, empty_leaf, per_round):
    height, steps = 3, (1, 3, 1, 11, 1, 47)
    h, ark, mds = _hades(ctx, per_round)
    rng = random.Random(capacity + 1)
    leaves = [0, R - 1] + [rng.randrange(R) for _ in range(62)]
    model = LM.Ledger(height, ark, mds, *SHAPE, capacity, empty_leaf)
    trees = {}
    try:
        trees.update({form: h.ledger(height, capacity, empty_leaf) for form in FORMS})
        for form, t in trees.items():
            assert t.count == 0 and t.height == height and t.root.tobytes() == _limbs([model.z[height]])[0].tobytes()
            assert t.empty_roots.tobytes() == _limbs(model.z).tobytes()
        for k in steps:
            batch = leaves[model.count:model.count + k]
            want = model.append(batch)
            for form, t in trees.items():
                assert t.append(_limbs(batch), form=form) == want, (form, model.count)
                _assert_equals_model(ctx, t, model, (form, model.count))
        assert model.count == 64 and [len(lv) for lv in model.levels] == [64, 16, 4, 1]
        assert model.levels == PM.tree(leaves, ark, mds, *SHAPE, capacity)
    finally:
        for t in trees.values():
            t.free()
        h.free()


# ---------------------------------------------------------------------------------- 2. parity with the dense product
@pytest.mark.parametrize("height", (1, 2, 3, 5))
def test_parity_with_the_dense_tree(ctx, height):
    capacity, empty_leaf = (0, 0) if height % 2 else (77, EMPTY)
    h, _, _ = _hades(ctx, height == 3)
    full = 4 ** height
    rng = random.Random(height)
    leaves = [rng.randrange(R) for _ in range(full)]
    counts = sorted({0, 1, full - 1, full, rng.randrange(2, full), rng.randrange(2, full)})
    try:
        for count in counts:
            dense = h.merkle(_limbs(leaves[:count] + [empty_leaf] * (full - count)), capacity)
            t = h.ledger(height, capacity, empty_leaf, reserve=count)
            assert t.append(_limbs(leaves[:count])) == sum(LM.width(count, l) for l in range(1, height + 1))
            assert t.root.tobytes() == dense.root.tobytes(), count
            for l in range(height + 1):
                assert t.level(l).to_host().tobytes() == dense.level(l).to_host()[:LM.width(count, l)].tobytes(), (count, l)
            probe = _probe(count)
            assert t.paths(probe).tobytes() == dense.paths(probe).tobytes(), count
            if count:
                assert t.verify(t.paths(probe), probe).tolist() == dense.verify(dense.paths(probe), probe).tolist() == [0] * len(probe)
            t.free(), dense.free()
    finally:
        h.free()


# ---------------------------------------------------------------------------------- 3. ledger heights
@pytest.mark.parametrize("height", (17, 31))
def test_ledger_heights(ctx, height):
    import plonk_prototype_amd as pa
    from plonk_prototype_amd import _lib
    capacity, empty_leaf = 5, EMPTY
    h, ark, mds = _hades(ctx, height == 31)
    rng = random.Random(height)
    leaves = [rng.randrange(R) for _ in range(70)]
    model = LM.Ledger(height, ark, mds, *SHAPE, capacity, empty_leaf)
    want = [model.append(leaves[:33]), model.append(leaves[33:])]
    assert want == [9 + 3 + (height - 2), 10 + 3 + 2 + (height - 3)]
    LINK, INDEX = _lib.MERKLE_PATH_LINK, _lib.MERKLE_PATH_INDEX
    t = None
    try:
        t = h.ledger(height, capacity, empty_leaf)
        assert [t.append(_limbs(leaves[:33])), t.append(_limbs(leaves[33:]))] == want
        _assert_equals_model(ctx, t, model)
        assert t.empty_roots.tobytes() == _limbs(model.z).tobytes()
        indices = [0, 17, 35, 69]
        good = t.paths(indices)
        assert good.tobytes() == _paths_bytes(model, indices)
        for form in FORMS:
            assert t.verify(good, indices, form=form).tolist() == [0] * 4, form
        cases = [(good[j], i, 0) for j, i in enumerate(indices)]
        for l in (0, height // 2, height - 1):                                   # a flipped sibling: the lowest failing level
            for j, i in enumerate(indices):
                bad = good[j].copy()
                bad[l, ((i >> (2 * l)) & 3) ^ 1, 0] ^= np.uint64(1)
                cases.append((bad, i, LINK + l))
        cases.append((good[0], 4 ** height, INDEX))
        cases.append((good[1], indices[1] + 4 ** height, INDEX))
        cases.append((good[3], indices[3] ^ (1 << (2 * (height - 1))), LINK + height - 2))        # a wrong top digit
        root_int = model.root
        for path, i, want in cases[4:8] + cases[-3:]:                            # the model gives the codes asked for
            ints = [pa.field.fr_vec_from_limbs(lv) for lv in path]
            assert MU.verify(ints, i, root_int, ark, mds, *SHAPE, capacity) == want if i < 4 ** height else want == INDEX
        paths = np.stack([p for p, _, _ in cases])
        for form in FORMS:
            assert t.verify(paths, [i for _, i, _ in cases], form=form).tolist() == [w for _, _, w in cases], form
            assert h.verify_ledger_paths(good, indices, t.root, height, capacity, form=form).tolist() == [0] * 4
        # the limits of the two entries
        lib, c = ctx._lib, ctx._h
        d_paths, d_root = pa.DeviceVector.from_host(ctx, good.reshape(-1, 4)), pa.DeviceVector.from_host(ctx, t.root.reshape(1, 4))
        d_idx = pa.DeviceVector.from_host(ctx, np.array(indices, np.uint64))
        d_status = pa.DeviceVector.from_host(ctx, np.full((1, 4), 0x5555555555555555, np.uint64))
        cap = _limbs([capacity])
        try:
            for entry, hgt in ((lib.pm_poseidon_ledger_verify_dev, 32), (lib.pm_poseidon_ledger_verify_dev, 0),
                               (lib.pm_poseidon_merkle_verify_dev, 16), (lib.pm_poseidon_merkle_verify_dev, height)):
                assert entry(c, h._h, _p(cap), d_paths._p, d_idx._p, 4, hgt, d_root._p, d_status._p, 0, None) == _lib.PM_ERR_BAD_ARG
            ctx.sync()
            assert (d_status.to_host() == 0x5555555555555555).all()
        finally:
            d_paths.free(), d_root.free(), d_idx.free(), d_status.free()
        with pytest.raises(pa.Error):
            h.ledger(32)
    finally:
        if t is not None:
            t.free()
        h.free()


# ---------------------------------------------------------------------------------- 4. defaults are not read from storage
def _poison_beyond_the_prefixes(ctx, t):
    """0xA5 over the reserved space beyond every stored prefix: no canonical element, so a default read from there shows"""
    reserve = t.reserve
    for l in range(t.height + 1):
        lv = t.level(l)
        room = LM.width(reserve, l) - lv.n
        if room:
            junk = np.full(32 * room, 0xA5, np.uint8)
            ctx._check(ctx._lib.pm_dev_upload(ctx._h, C.c_void_p(lv.ptr + 32 * lv.n), junk.ctypes.data_as(C.c_void_p), junk.nbytes))


def test_defaults_are_not_read_from_storage(ctx):
    height, capacity = 5, 3
    h, ark, mds = _hades(ctx, False)
    rng = random.Random(5)
    leaves = [rng.randrange(R) for _ in range(60)]
    model = LM.Ledger(height, ark, mds, *SHAPE, capacity, EMPTY)
    t = None
    try:
        t = h.ledger(height, capacity, EMPTY, reserve=256)
        for form, (lo, hi) in zip(("thread", "wave", "auto"), ((0, 37), (37, 40), (40, 50))):
            _poison_beyond_the_prefixes(ctx, t)
            assert t.append(_limbs(leaves[lo:hi]), form=form) == model.append(leaves[lo:hi])
            _assert_equals_model(ctx, t, model, (form, hi))
        _poison_beyond_the_prefixes(ctx, t)
        assert t.truncate(22) == model.truncate(22) == height
        _assert_equals_model(ctx, t, model, "truncated")
        _poison_beyond_the_prefixes(ctx, t)
        assert t.append(_limbs(leaves[50:])) == model.append(leaves[50:])
        _assert_equals_model(ctx, t, model, "appended after the truncate")
        everything = list(range(model.count))
        assert t.paths(everything).tobytes() == _paths_bytes(model, everything)
        assert t.reserve == 256
    finally:
        if t is not None:
            t.free()
        h.free()


# ---------------------------------------------------------------------------------- 5. growth
def test_growth_keeps_every_byte(ctx):
    height = 5
    h, _, _ = _hades(ctx, True)
    rng = random.Random(50)
    leaves = _limbs([rng.randrange(R) for _ in range(301)])
    small = roomy = None
    try:
        small, roomy = h.ledger(height, 0, EMPTY, reserve=0), h.ledger(height, 0, EMPTY, reserve=1024)
        assert small.reserve == 0 and small.level(0).n == 0 and roomy.reserve == 1024
        sizes = [(small.reserve, small.device_bytes)]
        for lo, hi in ((0, 1), (1, 301)):
            assert small.append(leaves[lo:hi]) == roomy.append(leaves[lo:hi])
            sizes.append((small.reserve, small.device_bytes))
            for l in range(height + 1):
                assert small.level(l).to_host().tobytes() == roomy.level(l).to_host().tobytes(), (hi, l)
            assert small.root.tobytes() == roomy.root.tobytes()
        assert [s[0] for s in sizes] == [0, 1, 301] and sizes[0][1] < sizes[1][1] < sizes[2][1]
        assert sizes[2][1] - sizes[0][1] == ctx._lib.pm_poseidon_ledger_bytes(height, 301)
        assert small.paths([0, 150, 300]).tobytes() == roomy.paths([0, 150, 300]).tobytes()
        assert small.append(leaves[:200]) == roomy.append(leaves[:200])            # 501 > 301: twice the reserve
        assert small.reserve == 602 and small.root.tobytes() == roomy.root.tobytes() and roomy.reserve == 1024
        assert small.append(leaves) == roomy.append(leaves) and small.reserve == 1024   # 802 < 1204: capped at 4^5
        assert small.level(2).to_host().tobytes() == roomy.level(2).to_host().tobytes()
    finally:
        for t in (small, roomy):
            if t is not None:
                t.free()
        h.free()


# ---------------------------------------------------------------------------------- 6. the rollback
@pytest.mark.parametrize("per_round", (False, True))
def test_truncate(ctx, per_round):
    import plonk_prototype_amd as pa
    height, capacity = 3, 77
    h, ark, mds = _hades(ctx, per_round)
    rng = random.Random(23)
    leaves = [rng.randrange(R) for _ in range(23)]
    other = [rng.randrange(R) for _ in range(40)]
    model = LM.Ledger(height, ark, mds, *SHAPE, capacity, EMPTY)
    model.append(leaves)
    t = fresh = None
    try:
        t = h.ledger(height, capacity, EMPTY)
        t.append(_limbs(leaves))
        for form, count, want in (("thread", 18, 3), ("wave", 18, 0), ("auto", 16, 3), ("thread", 1, 3), ("wave", 0, 0), ("auto", 0, 0)):
            with pytest.raises(pa.Error) as e:
                t.truncate(t.count + 1, form=form)
            assert e.value.code == -1
            assert t.truncate(count, form=form) == model.truncate(count) == want, count
            _assert_equals_model(ctx, t, model, count)
        assert t.root.tobytes() == t.empty_roots[height].tobytes()
        # a path issued before a rollback verifies against the old root and fails against the new one
        t.append(_limbs(leaves)), model.append(leaves)
        old_root, old_path = t.root, t.paths([3])
        assert t.truncate(5) == model.truncate(5) == height
        assert t.append(_limbs(other)) == model.append(other)
        _assert_equals_model(ctx, t, model, "appended after the rollback")
        fresh = h.ledger(height, capacity, EMPTY)
        fresh.append(_limbs(leaves[:5] + other))
        for l in range(height + 1):
            assert t.level(l).to_host().tobytes() == fresh.level(l).to_host().tobytes(), l
        assert t.root.tobytes() == fresh.root.tobytes() != old_root.tobytes()
        ints = [pa.field.fr_vec_from_limbs(lv) for lv in old_path[0]]
        stale = MU.verify(ints, 3, model.root, ark, mds, *SHAPE, capacity)
        assert stale >= 2                                                       # a link fails: leaf 3 kept its value, not its siblings
        for form in ("thread", "wave"):
            assert t.verify(old_path, [3], root=old_root, form=form).tolist() == [0]
            assert t.verify(old_path, [3], form=form).tolist() == [stale]
            assert t.verify(t.paths([3]), [3], form=form).tolist() == [0]
    finally:
        for x in (t, fresh):
            if x is not None:
                x.free()
        h.free()


# ---------------------------------------------------------------------------------- 7. limits and refusals
def test_limits_and_refusals(ctx):
    import plonk_prototype_amd as pa
    from plonk_prototype_amd import _lib
    lib, c, vp = ctx._lib, ctx._h, C.c_void_p
    BAD, LENGTH = _lib.PM_ERR_BAD_ARG, _lib.PM_ERR_LENGTH
    height = 2
    h, ark, mds = _hades(ctx, False)
    rng = random.Random(2)
    leaves = [rng.randrange(R) for _ in range(16)]
    model = LM.Ledger(height, ark, mds, *SHAPE, 0, EMPTY)
    model.append(leaves)
    vals = pa.DeviceVector.from_host(ctx, _limbs(leaves))
    hashed = C.c_uint64(99)
    full = part = None
    try:
        full, part = h.ledger(height, 0, EMPTY), h.ledger(height, 0, EMPTY, reserve=16)
        assert full.append_dev(vals.ptr, 16) == 5 and part.append_dev(vals.ptr, 5) == 2 + 1

        def append(tree, ptr, k, flags=0, ctx_h=c):
            return lib.pm_poseidon_ledger_append_dev(ctx_h, tree, ptr, k, flags, C.byref(hashed), None)
        # a full tree
        assert append(full._h, vals._p, 1) == LENGTH and append(full._h, vals._p, 16) == LENGTH
        assert append(full._h, vals._p, 0) == 0 and hashed.value == 0 and append(full._h, None, 0) == 0
        assert lib.pm_poseidon_ledger_append_dev(c, full._h, None, 0, 0, None, None) == 0        # hashed may be NULL
        assert append(part._h, vals._p, 12) == LENGTH                                         # 5 + 12 > 16
        # arguments
        assert append(part._h, None, 1) == BAD and append(None, vals._p, 1) == BAD and append(part._h, vals._p, 1, ctx_h=None) == BAD
        assert append(part._h, vp(vals.ptr + 8), 1) == BAD                                     # not 16-byte aligned
        assert append(part._h, vals._p, 1, flags=3) == BAD and append(part._h, vals._p, 1, flags=0xffffffff) == BAD
        slab0, slab2 = part.level(0), part.level(2)
        assert append(part._h, vp(slab0.ptr), 1) == BAD and "d_values" in lib.pm_last_error(c).decode()
        assert append(part._h, vp(slab0.ptr + 32 * 15), 1) == BAD and append(part._h, vp(slab2.ptr), 1) == BAD
        assert lib.pm_poseidon_ledger_truncate_dev(c, part._h, 6, 0, C.byref(hashed), None) == BAD
        assert lib.pm_poseidon_ledger_truncate_dev(c, part._h, 3, 3, C.byref(hashed), None) == BAD
        assert lib.pm_poseidon_ledger_truncate_dev(c, None, 3, 0, C.byref(hashed), None) == BAD
        assert lib.pm_poseidon_ledger_root_dev(c, part._h, None, None) == BAD
        assert lib.pm_poseidon_ledger_root_dev(c, part._h, vp(vals.ptr + 4), None) == BAD
        for inside in (slab0.ptr, slab2.ptr, slab0.ptr + 32 * 7):                             # no call writes the tree through a caller's buffer
            assert lib.pm_poseidon_ledger_root_dev(c, part._h, vp(inside), None) == BAD and "d_root" in lib.pm_last_error(c).decode()
        assert lib.pm_poseidon_ledger_root(c, part._h, None, None) == BAD and lib.pm_poseidon_ledger_root(c, None, _p(np.zeros(4, np.uint64)), None) == BAD
        assert lib.pm_poseidon_ledger_level(part._h, 3, None, None) == BAD and lib.pm_poseidon_ledger_level(None, 0, None, None) == BAD
        assert lib.pm_poseidon_ledger_level(part._h, 2, None, None) == 0
        assert lib.pm_poseidon_ledger_info(None, None, None, None, None) == BAD and lib.pm_poseidon_ledger_info(part._h, None, None, None, None) == 0
        assert lib.pm_poseidon_ledger_empty_roots(part._h, None) == BAD
        # create
        cap, leaf, out = _limbs([0]), _limbs([EMPTY]), C.c_void_p()
        big = np.full((1, 4), 0xFFFFFFFFFFFFFFFF, np.uint64)

        def create(hgt=height, params=h._h, cap_p=_p(cap), leaf_p=_p(leaf), reserve=0, out_p=C.byref(out), ctx_h=c):
            return lib.pm_poseidon_ledger_create(ctx_h, params, cap_p, hgt, leaf_p, reserve, out_p)
        assert create(hgt=0) == BAD and create(hgt=32) == BAD and create(params=None) == BAD and create(ctx_h=None) == BAD
        assert create(cap_p=None) == BAD and create(leaf_p=None) == BAD and create(out_p=None) == BAD
        assert create(cap_p=_p(big)) == BAD and create(leaf_p=_p(big)) == BAD
        assert create(leaf_p=_p(_limbs([R - 1]))) == 0                                         # the largest canonical element
        lib.pm_poseidon_ledger_free(c, out)
        assert create(reserve=17) == BAD and create(reserve=16) == 0
        lib.pm_poseidon_ledger_free(c, out)
        lib.pm_poseidon_ledger_free(c, None)
        # nothing changed
        ctx.sync()
        _assert_equals_model(ctx, full, model, "the full tree")
        model.truncate(5)
        _assert_equals_model(ctx, part, model, "the tree of five")
        # paths: an index at or above the count names the lowest offending position, the other paths are written
        idx = pa.DeviceVector.from_host(ctx, np.array([0, 5, 4, 1 << 40], np.uint64))
        d_out = pa.DeviceVector.from_host(ctx, np.full((4 * height * 4, 4), 0xA5A5A5A5A5A5A5A5, np.uint64))
        try:
            with pytest.raises(pa.Error) as e:
                part.paths_dev(idx.ptr, 4, d_out.ptr)
            assert e.value.code == BAD and "index 1 " in str(e.value)
            got = d_out.to_host().reshape(4, height, 4, 4)
            assert got[[0, 2]].tobytes() == _paths_bytes(model, [0, 4])
            assert (got[[1, 3]] == 0xA5A5A5A5A5A5A5A5).all()
            assert lib.pm_poseidon_ledger_paths_dev(c, part._h, None, 4, d_out._p, None) == BAD
            assert lib.pm_poseidon_ledger_paths_dev(c, part._h, idx._p, 4, None, None) == BAD
            assert lib.pm_poseidon_ledger_paths_dev(c, part._h, vp(idx.ptr + 4), 1, d_out._p, None) == BAD
            assert lib.pm_poseidon_ledger_paths_dev(c, part._h, None, 0, None, None) == 0
            good = pa.DeviceVector.from_host(ctx, np.array([0, 1, 2, 3], np.uint64))
            assert lib.pm_poseidon_ledger_paths_dev(c, part._h, good._p, 4, vp(part.level(0).ptr), None) == BAD
            assert "d_out" in lib.pm_last_error(c).decode()
            good.free()
            _assert_equals_model(ctx, part, model, "after the refused outputs")
        finally:
            idx.free(), d_out.free()
    finally:
        vals.free()
        for t in (full, part):
            if t is not None:
                t.free()
        h.free()


# ---------------------------------------------------------------------------------- 8. a wide append
def test_a_wide_append(ctx):
    """1000 leaves at count 333: levels 0 and 1 span several workgroups of the THREAD form (251 and 64 nodes, 64 a group)"""
    height = 6
    h, ark, mds = _hades(ctx, False)
    rng = random.Random(6)
    leaves = [rng.randrange(R) for _ in range(1333)]
    model = LM.Ledger(height, ark, mds, *SHAPE, 0, 0)
    want = [model.append(leaves[:333]), model.append(leaves[333:])]
    assert want[1] == 251 + 64 + 16 + 5 + 2 + 1
    trees = []
    try:
        for form in ("thread", "wave"):
            t = h.ledger(height, reserve=333)
            trees.append(t)
            assert [t.append(_limbs(leaves[:333]), form=form), t.append(_limbs(leaves[333:]), form=form)] == want
            _assert_equals_model(ctx, t, model, form)
            probe = [0, 332, 333, 999, 1332]
            assert t.paths(probe).tobytes() == _paths_bytes(model, probe)
    finally:
        for t in trees:
            t.free()
        h.free()


# ---------------------------------------------------------------------------------- 9. stream order
def test_append_then_root_on_one_stream(ctx):
    import plonk_prototype_amd as pa
    import torch
    height, k = 8, 4096
    h, _, _ = _hades(ctx, False)
    rng = random.Random(8)
    leaves = _limbs([rng.randrange(R) for _ in range(k)])
    vals, d_root = pa.DeviceVector.from_host(ctx, leaves), pa.DeviceVector.from_host(ctx, np.zeros((1, 4), np.uint64))
    a = b = None
    try:
        a, b = h.ledger(height, reserve=k), h.ledger(height, reserve=k)
        b.append(leaves, form="thread")
        want = b.root
        ctx.sync()
        st = torch.cuda.Stream()
        a.append_dev(vals.ptr, k, form="thread", stream=st.cuda_stream)            # no growth: asynchronous
        a.root_dev(d_root.ptr, stream=st.cuda_stream)                              # ... and no wait in between
        host = np.zeros(4, np.uint64)
        ctx._check(ctx._lib.pm_poseidon_ledger_root(ctx._h, a._h, _p(host), C.c_void_p(st.cuda_stream)))   # waits for that stream
        assert host.tobytes() == want.tobytes() and d_root.to_host()[0].tobytes() == want.tobytes()
    finally:
        vals.free(), d_root.free()
        for t in (a, b):
            if t is not None:
                t.free()
        h.free()
