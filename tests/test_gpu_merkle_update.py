"""The incremental Poseidon tree on the GPU: pm_poseidon_merkle_update_dev and
pm_poseidon_merkle_verify_dev in both kernel forms against the big-integer model of tests/merkle_update_model.py -- every
comparison is byte equality, and the forms must agree with each other."""
import ctypes as C
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import merkle_update_model as MU  # noqa: E402
import poseidon_model as PM  # noqa: E402

pytestmark = pytest.mark.gpu
R = PM.R
FORMS = ("thread", "wave", "auto")
_CACHE = {}


def _p(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint64))


def _case(shape, per_round, height, capacity):
    """-> (ark, mds, their limbs, the leaves, the model's levels), built once per case and never changed"""
    key = (shape, per_round, height, capacity)
    if key not in _CACHE:
        rounds = shape[0]
        ark, mds = PM.constants(rounds, rounds if per_round else 1, 7000 + 10 * rounds + per_round)
        a, m, _ = PM.flat(ark, mds)
        rng = random.Random(31 * height + rounds)
        leaves = [0, R - 1] + [rng.randrange(R) for _ in range(4 ** height - 2)]
        _CACHE[key] = (ark, mds, PM.to_limbs(a), PM.to_limbs(m), leaves, PM.tree(leaves, ark, mds, *shape, capacity))
    return _CACHE[key]


def _hades(ctx, shape, per_round, height, capacity):
    import plonk_prototype_amd as pa
    ark, mds, a, m, leaves, levels = _case(shape, per_round, height, capacity)
    return pa.Hades(ctx, a, m, *shape), ark, mds, leaves, levels


def _copy(levels):
    return [list(lv) for lv in levels]


def _flat(levels):
    return PM.to_limbs(PM.flat_tree(levels)).tobytes()


def _paths_bytes(levels, indices):
    return PM.to_limbs([x for p in PM.paths(levels, indices) for lv in p for x in lv]).tobytes()


def _batches(height):
    """name -> leaf indices: the cases of the issue that fit the height"""
    count = 4 ** height
    rng = random.Random(height)
    out = {"first": [0], "last": [count - 1], "middle": [count // 2 + 1], "one parent": [1, 2], "all": list(range(count))}
    if height >= 2:
        out["a grandparent"] = [2, 5]                                   # parents 0 and 1 (at height 2 that is the root)
        out["only the root"] = [count // 4 - 1, count // 4]             # the last leaf under the root's child 0, the first under 1
        out["far apart"] = [0, count - 1]
    if height == 5:
        out["700 random"] = rng.sample(range(count), 700)               # six workgroups of the compaction at level 0, two at 1
        out["257 contiguous"] = list(range(333, 333 + 257))             # starts at 4 * 83 + 1
    return out


# ---------------------------------------------------------------------------------- 1. the update against the model
@pytest.mark.parametrize("height,capacity", [(1, 0), (2, 77), (3, 0), (5, 0)])
def test_update_against_the_model(ctx, height, capacity):
    shape = (5, 2)
    h, ark, mds, leaves, levels0 = _hades(ctx, shape, height % 2 == 1, height, capacity)
    count = 4 ** height
    rng = random.Random(100 + height)
    trees = {}
    try:
        trees = {form: h.merkle(PM.to_limbs(leaves), capacity) for form in ("thread", "wave")}
        levels = _copy(levels0)
        for name, indices in _batches(height).items():
            values = [rng.randrange(R) for _ in indices]
            if name == "first":
                values = [R - 1]
            want = MU.update(levels, indices, values, ark, mds, *shape, capacity)
            assert want == MU.hashed_count(indices, height)
            if name == "all":
                assert want == (count - 1) // 3
            for form, t in trees.items():
                hashed = t.update(indices, PM.to_limbs(values), form=form)
                assert hashed == want, (name, form)
                assert t.leaves.to_host().tobytes() == PM.to_limbs(levels[0]).tobytes(), (name, form)
                assert t.nodes.to_host().tobytes() == _flat(levels), (name, form)
                assert t.root.tobytes() == PM.to_limbs(levels[-1]).tobytes(), (name, form)
                probe = [indices[0], indices[-1], (indices[-1] + 1) % count, (indices[0] + count // 2) % count]   # changed or not
                assert t.paths(probe).tobytes() == _paths_bytes(levels, probe), (name, form)
        assert levels == PM.tree(levels[0], ark, mds, *shape, capacity)            # the model never drifted from a rebuild
        rebuilt = h.merkle(PM.to_limbs(levels[0]), capacity)
        assert rebuilt.nodes.to_host().tobytes() == trees["thread"].nodes.to_host().tobytes()   # == pm_poseidon_merkle_dev
        rebuilt.free()
        values = [rng.randrange(R) for _ in range(3)]
        assert trees["wave"].update([count - 1, 0, count // 2], PM.to_limbs(values)) == \
            trees["thread"].update([0, count // 2, count - 1], PM.to_limbs([values[1], values[2], values[0]]))   # AUTO, any order
        assert trees["wave"].nodes.to_host().tobytes() == trees["thread"].nodes.to_host().tobytes()
        assert trees["wave"].leaves.to_host().tobytes() == trees["thread"].leaves.to_host().tobytes()
    finally:
        for t in trees.values():
            t.free()
        h.free()


def test_update_at_67_rounds_with_a_matrix_a_round(ctx):
    shape, height = (67, 8), 2
    h, ark, mds, leaves, levels0 = _hades(ctx, shape, True, height, 5)
    levels = _copy(levels0)
    indices, values = [3, 4, 15], [1, R - 1, 12345]
    want = MU.update(levels, indices, values, ark, mds, *shape, 5)
    got = {}
    try:
        for form in FORMS:
            t = h.merkle(PM.to_limbs(leaves), 5)
            assert t.update(indices, PM.to_limbs(values), form=form) == want == 4
            got[form] = t.leaves.to_host().tobytes() + t.nodes.to_host().tobytes()
            assert got[form] == PM.to_limbs(levels[0]).tobytes() + _flat(levels), form
            fresh = t.paths(indices)
            assert t.verify(fresh, indices, form=form).tolist() == [0, 0, 0]
            t.free()
        assert got["thread"] == got["wave"] == got["auto"]
    finally:
        h.free()


# ---------------------------------------------------------------------------------- 2. only the ancestors are hashed
def test_an_untouched_node_is_not_hashed_again(ctx):
    """a wrong level-1 node that is no ancestor of the changed leaf stays wrong, and the ancestors above it are hashed from it"""
    shape, height = (5, 2), 3
    h, ark, mds, leaves, levels0 = _hades(ctx, shape, False, height, 0)
    wrong = 0x1234567
    try:
        for form in ("thread", "wave"):
            t = h.merkle(PM.to_limbs(leaves))
            levels = _copy(levels0)
            levels[1][5] = wrong                                              # children 20..23: a sibling of leaf 16's parent
            ctx._check(ctx._lib.pm_dev_upload(ctx._h, C.c_void_p(t.nodes.ptr + 32 * 5),
                                              PM.to_limbs([wrong]).ctypes.data_as(C.c_void_p), 32))
            before = t.nodes.to_host()
            assert MU.update(levels, [16], [99], ark, mds, *shape, check=False) == 3
            assert t.update([16], PM.to_limbs([99]), form=form) == 3
            after = t.nodes.to_host()
            assert after[5].tobytes() == PM.to_limbs([wrong]).tobytes()
            assert after.tobytes() == _flat(levels), form
            assert set(np.nonzero((before != after).any(axis=1))[0].tolist()) == MU.ancestors([16], height) == {4, 17, 20}
            t.free()
    finally:
        h.free()


def test_changed_rows_are_the_union_of_the_ancestors(ctx):
    shape, height = (5, 2), 3
    h, ark, mds, leaves, _ = _hades(ctx, shape, False, height, 0)
    try:
        for form in ("thread", "wave"):
            t = h.merkle(PM.to_limbs(leaves))
            before, leaves_before = t.nodes.to_host(), t.leaves.to_host()
            indices = [37, 5, 38, 63]
            values = [(leaves[i] + 1) % R for i in indices]
            assert t.update(indices, PM.to_limbs(values), form=form) == MU.hashed_count(indices, height) == 3 + 3 + 1
            differs = (before != t.nodes.to_host()).any(axis=1)
            assert set(np.nonzero(differs)[0].tolist()) == MU.ancestors(indices, height)
            assert set(np.nonzero((leaves_before != t.leaves.to_host()).any(axis=1))[0].tolist()) == set(indices)
            t.free()
    finally:
        h.free()


def test_the_same_update_twice_gives_the_same_bytes(ctx):
    shape, height = (5, 2), 5
    h, _, _, leaves, _ = _hades(ctx, shape, True, height, 0)
    rng = random.Random(55)
    indices = rng.sample(range(1024), 300)
    values = PM.to_limbs([rng.randrange(R) for _ in indices])
    got = []
    try:
        for _ in range(2):
            t = h.merkle(PM.to_limbs(leaves))
            hashed = t.update(indices, values)
            got.append((hashed, t.leaves.to_host().tobytes(), t.nodes.to_host().tobytes()))
            t.free()
        assert got[0] == got[1]
    finally:
        h.free()


# ---------------------------------------------------------------------------------- 3. the Python wrapper
def test_wrapper_sorts_and_refuses_duplicates(ctx):
    import plonk_prototype_amd as pa
    shape, height = (5, 2), 2
    h, _, _, leaves, _ = _hades(ctx, shape, False, height, 77)
    try:
        a, b = h.merkle(PM.to_limbs(leaves), 77), h.merkle(PM.to_limbs(leaves), 77)
        values = PM.to_limbs([5, 6, 7, 8])
        assert a.update([9, 2, 15, 3], values) == b.update([2, 3, 9, 15], values[[1, 3, 0, 2]])
        assert a.leaves.to_host().tobytes() == b.leaves.to_host().tobytes()
        assert a.nodes.to_host().tobytes() == b.nodes.to_host().tobytes()
        assert a.leaves.to_host()[9].tobytes() == values[0].tobytes()
        before = a.nodes.to_host().tobytes()
        with pytest.raises(ValueError):
            a.update([4, 1, 4], values[:3])
        assert a.nodes.to_host().tobytes() == before
        assert a.update([], np.zeros((0, 4), np.uint64)) == 0
        bare = pa.MerkleTree(ctx, a.leaves, a.nodes, height)
        with pytest.raises(ValueError):
            bare.update([1], values[:1])
        with pytest.raises(ValueError):
            bare.verify(a.paths([1]), [1])
        with pytest.raises(pa.Error) as e:                                     # the device's own verdict through the wrapper
            a.update([1, 16], values[:2])
        assert e.value.code == -1 and "index 1 " in str(e.value)
        assert a.nodes.to_host().tobytes() == before
        a.free(), b.free()
    finally:
        h.free()


# ---------------------------------------------------------------------------------- 4. refusals through the raw ABI
def test_refusals_change_nothing(ctx):
    import plonk_prototype_amd as pa
    from plonk_prototype_amd import _lib
    lib, c = ctx._lib, ctx._h
    shape, height = (5, 2), 2
    h, _, _, leaves, _ = _hades(ctx, shape, False, height, 0)
    bad, vp = _lib.PM_ERR_BAD_ARG, C.c_void_p
    cap = PM.to_limbs([0])
    t = h.merkle(PM.to_limbs(leaves))
    k = 5
    vals = pa.DeviceVector.from_host(ctx, PM.to_limbs([1, 2, 3, 4, 5]))
    work = pa.DeviceVector(ctx, (lib.pm_poseidon_merkle_update_work_bytes(k) + 31) // 32)
    before = (t.leaves.to_host().tobytes(), t.nodes.to_host().tobytes())
    hashed = C.c_uint64(99)
    held = []

    def idx(values):
        d = pa.DeviceVector.from_host(ctx, np.array(list(values) + [0] * ((-len(values)) % 4), np.uint64))
        held.append(d)
        return d._p

    def call(d_idx, n=k, hgt=height, flags=0, params=h._h, cap_p=_p(cap), **ptr):
        p = dict(leaves_p=t.leaves._p, tree_p=t.nodes._p, vals_p=vals._p, work_p=work._p)
        p.update(ptr)
        return lib.pm_poseidon_merkle_update_dev(c, params, cap_p, p["leaves_p"], p["tree_p"], hgt, d_idx, p["vals_p"], n,
                                                 p["work_p"], flags, C.byref(hashed), None)
    try:
        for indices, position in (([16, 17, 18, 19, 20], 0), ([0, 1, 16, 3, 4], 2), ([0, 1, 2, 3, 16], 4), ([0, 1, 2, 3, 1 << 63], 4),
                                  ([0, 5, 5, 6, 7], 2), ([0, 1, 2, 9, 8], 4), ([3, 2, 1, 0, 16], 1), ([7, 7, 7, 7, 7], 1)):
            for flags in (0, 1, 2):
                assert call(idx(indices), flags=flags) == bad, indices
                assert f"index {position} " in lib.pm_last_error(c).decode(), (indices, lib.pm_last_error(c))
        assert (t.leaves.to_host().tobytes(), t.nodes.to_host().tobytes()) == before
        good = idx([0, 1, 2, 3, 4])
        for hgt in (0, 16):
            assert call(good, hgt=hgt) == bad
        assert call(good, flags=3) == bad and call(good, flags=0xffffffff) == bad
        assert call(good, params=None) == bad and call(good, cap_p=None) == bad
        assert call(None) == bad and call(good, n=17) == bad                                   # more indices than leaves
        for null in ("leaves_p", "tree_p", "vals_p", "work_p"):
            assert call(good, **{null: None}) == bad, null
        assert call(good, vals_p=vp(t.leaves.ptr + 32 * 12)) == bad and "d_values" in lib.pm_last_error(c).decode()   # overlaps
        assert call(good, vals_p=vp(t.nodes.ptr)) == bad
        assert call(good, work_p=vp(t.nodes.ptr + 32 * 4)) == bad and "d_work" in lib.pm_last_error(c).decode()
        assert call(good, work_p=vp(t.leaves.ptr)) == bad
        assert call(good, work_p=vp(work.ptr + 8)) == bad                                      # not 16-byte aligned
        assert call(good, tree_p=vp(t.leaves.ptr + 32)) == bad                                 # the tree in the leaves
        assert lib.pm_poseidon_merkle_update_dev(None, h._h, _p(cap), t.leaves._p, t.nodes._p, height, good, vals._p, k, work._p, 0,
                                                 None, None) == bad
        assert call(None, n=0, leaves_p=None, tree_p=None, vals_p=None, work_p=None) == 0 and hashed.value == 0   # k = 0
        assert lib.pm_poseidon_merkle_update_dev(c, h._h, _p(cap), t.leaves._p, t.nodes._p, height, good, vals._p, 0, work._p, 0,
                                                 None, None) == 0                              # ... and hashed may be NULL
        ctx.sync()
        assert (t.leaves.to_host().tobytes(), t.nodes.to_host().tobytes()) == before
        # verify: the same argument checks; a refused call writes no status
        status = pa.DeviceVector.from_host(ctx, np.full((2, 4), 0x5555555555555555, np.uint64))
        held.append(status)
        paths = pa.DeviceVector.from_host(ctx, t.paths([0, 1, 2, 3, 4]).reshape(-1, 4))
        held.append(paths)
        root = t.level(height)

        def verify(n=k, paths_p=paths._p, idx_p=good, hgt=height, root_p=root._p, status_p=status._p, flags=0, params=h._h):
            return lib.pm_poseidon_merkle_verify_dev(c, params, _p(cap), paths_p, idx_p, n, hgt, root_p, status_p, flags, None)
        assert verify(hgt=0) == bad and verify(hgt=16) == bad and verify(flags=3) == bad and verify(params=None) == bad
        assert verify(paths_p=None) == bad and verify(idx_p=None) == bad and verify(root_p=None) == bad and verify(status_p=None) == bad
        assert verify(status_p=vp(paths.ptr + 64)) == bad and verify(paths_p=vp(paths.ptr + 8)) == bad
        assert verify(n=0, paths_p=None, idx_p=None, root_p=None, status_p=None) == 0
        ctx.sync()
        assert (status.to_host() == 0x5555555555555555).all()
        assert verify() == 0
        ctx.sync()
        assert status.to_host().view(np.uint32).reshape(-1)[:6].tolist() == [0, 0, 0, 0, 0, 0x55555555]
    finally:
        for d in held:
            d.free()
        t.free(), vals.free(), work.free(), h.free()


# ---------------------------------------------------------------------------------- 5. verification
def _corrupt(path, l, c):
    bad = path.copy()
    bad[l, c, 0] ^= np.uint64(1)                                                 # still canonical: bit 0 of the lowest limb
    return bad


@pytest.mark.parametrize("height", (1, 2, 3))
def test_verify_statuses(ctx, height):
    import plonk_prototype_amd as pa
    from plonk_prototype_amd import _lib
    shape, capacity = (5, 2), (0 if height != 2 else 77)
    h, ark, mds, leaves, levels = _hades(ctx, shape, height % 2 == 1, height, capacity)
    count = 4 ** height
    rng = random.Random(height)
    LINK = _lib.MERKLE_PATH_LINK
    t = None
    try:
        t = h.merkle(PM.to_limbs(leaves), capacity)
        indices = [0, count - 1] + [rng.randrange(count) for _ in range(8)]
        good = t.paths(indices)
        for form in FORMS:
            assert t.verify(good, indices, form=form).tolist() == [0] * len(indices)
        root = t.root
        cases = []                                                               # (path, index, the status wanted)
        for j, i in enumerate(indices[:4]):
            cases.append((_corrupt(good[j], 0, i & 3), i, LINK))                 # the leaf itself
            for l in range(height):
                cases.append((_corrupt(good[j], l, ((i >> (2 * l)) & 3) ^ 2), i, LINK + l))          # a sibling at level l
            for l in range(height - 1):
                cases.append((_corrupt(good[j], l + 1, (i >> (2 * (l + 1))) & 3), i, LINK + l))      # the path's child above
            cases.append((good[j], i + count, _lib.MERKLE_PATH_INDEX))
            cases.append((good[j], i | (1 << 63), _lib.MERKLE_PATH_INDEX))
            if height > 1:
                cases.append((good[j], i ^ (1 << (2 * (height - 1))), LINK + height - 2))            # a wrong top digit
            cases.append((good[j], i, 0))
        for path, i, want in cases:                                              # the model gives the codes asked for
            ints = [pa.field.fr_vec_from_limbs(lv) for lv in path]
            assert MU.verify(ints, i, levels[-1][0], ark, mds, *shape, capacity) == want
        paths = np.stack([p for p, _, _ in cases])
        want = [w for _, _, w in cases]
        for form in FORMS:
            assert t.verify(paths, [i for _, i, _ in cases], form=form).tolist() == want, form
        wrong_root = root.copy()
        wrong_root[1] ^= np.uint64(4)
        for form in ("thread", "wave"):
            assert t.verify(good, indices, root=wrong_root, form=form).tolist() == [LINK + height - 1] * len(indices)
            assert h.verify_paths(good, indices, root, height, capacity, form=form).tolist() == [0] * len(indices)
            assert h.verify_paths(good, indices, root, height, capacity + 1, form=form).tolist() == [LINK] * len(indices)
        assert t.verify(np.zeros((0, height, 4, 4), np.uint64), []).shape == (0,)
    finally:
        if t is not None:
            t.free()
        h.free()


def test_verify_good_and_bad_paths_mixed(ctx):
    """k = 130: both halves of a WAVE-form wave, an odd count, more than one THREAD-form wave"""
    from plonk_prototype_amd import _lib
    shape, height = (5, 2), 3
    h, _, _, leaves, _ = _hades(ctx, shape, False, height, 0)
    rng = random.Random(130)
    try:
        t = h.merkle(PM.to_limbs(leaves))
        indices = [rng.randrange(64) for _ in range(130)]
        paths = t.paths(indices)
        want = [0] * 130
        for j in range(130):
            kind = j % 5 if j < 128 else 1 + j % 2                               # the last two: a bad one on each half
            if kind == 1:
                paths[j] = _corrupt(paths[j], j % height, ((indices[j] >> (2 * (j % height))) & 3) ^ 1)
                want[j] = _lib.MERKLE_PATH_LINK + j % height
            elif kind == 2:
                indices[j] += 64 << (j % 3)
                want[j] = _lib.MERKLE_PATH_INDEX
        assert 0 in want[:64] and 0 in want[64:] and want[128] and want[129]
        got = {form: t.verify(paths, indices, form=form).tolist() for form in FORMS}
        assert got["thread"] == want and got["wave"] == want and got["auto"] == want
        t.free()
    finally:
        h.free()


def test_stale_paths_fail_and_fresh_ones_pass(ctx):
    from plonk_prototype_amd import _lib
    shape, height = (5, 2), 3
    h, _, _, leaves, _ = _hades(ctx, shape, False, height, 0)
    t = h.merkle(PM.to_limbs(leaves))
    try:
        changed, untouched = [5, 37, 38], [6, 63]                                # 6 shares leaf 5's parent, 63 only the root
        old_root = t.root
        old = t.paths(changed + untouched)
        assert t.update(changed, PM.to_limbs([11, 12, 13])) == 2 + 2 + 1
        for form in ("thread", "wave"):
            assert t.verify(old, changed + untouched, root=old_root, form=form).tolist() == [0] * 5
            stale = t.verify(old, changed + untouched, form=form).tolist()
            assert stale == [_lib.MERKLE_PATH_LINK + 2] * 5                      # every old path folds to the old root
            assert t.verify(t.paths(changed + untouched), changed + untouched, form=form).tolist() == [0] * 5
    finally:
        t.free()
        h.free()
