"""Host-side ground for the incremental Poseidon tree: the three new exports are in the header, the
ctypes table, the library and the Rust bindings, the status constants agree, the work-area size is a pure host function, and
the big-integer model of tests/merkle_update_model.py -- rehash only the ancestors, count them -- equals a rebuild.  No device
here."""
import ctypes as C
import os
import random
import re
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import merkle_update_model as MU  # noqa: E402
import poseidon_model as PM  # noqa: E402
from conftest import ROOT  # noqa: E402
from plonk_prototype_amd._lib import MERKLE_PATH_INDEX, MERKLE_PATH_LINK, MERKLE_PATH_OK  # noqa: E402  (the codes under test)

R = PM.R
EXPORTS = ("pm_poseidon_merkle_update_work_bytes", "pm_poseidon_merkle_update_dev", "pm_poseidon_merkle_verify_dev")
SHAPE = (5, 2)


def test_exports_are_declared_bound_and_documented():
    import plonk_prototype_amd as pa
    from plonk_prototype_amd import _lib
    header = open(os.path.join(ROOT, "include", "plonk_mi355x.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    lib = C.CDLL(pa.LIB_PATH)
    for name in EXPORTS:
        assert re.search(rf"\b{name}\(", header), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
        assert f"pub fn {name}(" in doc, name
    vp, sz, u32 = C.c_void_p, C.c_size_t, C.c_uint32
    assert _lib.SIGNATURES[EXPORTS[0]] == (sz, [sz])
    assert _lib.SIGNATURES[EXPORTS[1]] == (C.c_int, [vp, vp, _lib.u64p, vp, vp, u32, vp, vp, sz, vp, u32, _lib.u64p, vp])
    assert _lib.SIGNATURES[EXPORTS[2]] == (C.c_int, [vp, vp, _lib.u64p, vp, vp, sz, u32, vp, vp, u32, vp])
    for name in ("update", "update_dev", "verify"):
        assert callable(getattr(pa.MerkleTree, name)), name
    assert callable(pa.Hades.verify_paths)


def test_status_constants_agree():
    from plonk_prototype_amd import _lib
    header = open(os.path.join(ROOT, "include", "plonk_mi355x.h")).read()
    for name, value in (("OK", 0), ("INDEX", 1), ("LINK", 2)):
        assert f"#define PM_MERKLE_PATH_{name} {value}u\n" in header
        assert getattr(_lib, f"MERKLE_PATH_{name}") == value
    assert (MU.PATH_OK, MU.PATH_INDEX, MU.PATH_LINK) == (MERKLE_PATH_OK, MERKLE_PATH_INDEX, MERKLE_PATH_LINK)


def test_work_bytes_is_a_pure_host_function():
    import plonk_prototype_amd as pa
    lib = pa.load()
    size = lib.pm_poseidon_merkle_update_work_bytes
    assert size(0) == 0
    last = 0
    for k in list(range(1, 1100)) + [4096, 4097, 65536, 1 << 20, 1 << 30]:
        now = size(k)
        assert now >= last and now >= 8 * k and now % 16 == 0, k       # two worklists of 4 bytes an entry, at the least
        last = now
    assert size(1) > 0 and size(1 << 30) < 9 << 30


@pytest.mark.parametrize("height", (1, 2, 3))
def test_model_update_equals_a_rebuild(height):
    ark, mds = PM.constants(SHAPE[0], 1 if height != 2 else SHAPE[0], 70 + height)
    capacity = 0 if height != 3 else 12345
    rng = random.Random(height)
    count = 4 ** height
    leaves = [rng.randrange(R) for _ in range(count)]
    levels = PM.tree(leaves, ark, mds, *SHAPE, capacity)
    for k in (1, 2, 3, count // 2, count):
        for _ in range(3):
            indices = rng.sample(range(count), k)                        # any order: the model sorts for itself
            values = [rng.randrange(R) for _ in range(k)]
            hashed = MU.update(levels, indices, values, ark, mds, *SHAPE, capacity)     # asserts == PM.tree itself
            for i, v in zip(indices, values):
                leaves[i] = v
            assert levels == PM.tree(leaves, ark, mds, *SHAPE, capacity)
            assert hashed == MU.hashed_count(indices, height) <= min(k * height, (count - 1) // 3)
    assert MU.update(levels, list(range(count)), leaves, ark, mds, *SHAPE, capacity) == (count - 1) // 3


def test_model_count_and_ancestor_sets():
    assert MU.hashed_count([0], 3) == 3 and MU.hashed_count([0, 1], 3) == 3           # one parent
    assert MU.hashed_count([0, 4], 3) == 4 and MU.hashed_count([0, 16], 3) == 5       # a grandparent, the root alone
    assert MU.hashed_count([0, 63], 3) == 5 and MU.hashed_count(range(64), 3) == 21
    assert MU.ancestors([37], 3) == {9, 16 + 2, 20}
    assert MU.ancestors([0, 63], 3) == {0, 15, 16, 19, 20}


def test_model_update_leaves_other_nodes_alone():
    """a wrong node that is no ancestor stays wrong, and the ancestors are hashed from the children as they stand"""
    ark, mds = PM.constants(SHAPE[0], 1, 5)
    leaves = list(range(1, 65))
    levels = PM.tree(leaves, ark, mds, *SHAPE)
    levels[1][5] = 99                                                    # children 20..23; shares the grandparent of leaf 16
    hashed = MU.update(levels, [16], [7], ark, mds, *SHAPE, check=False)
    assert hashed == 3 and levels[1][5] == 99
    assert levels[2][1] == PM.node(levels[1][4:8], ark, mds, *SHAPE) and levels[1][4] == PM.node([7, 18, 19, 20], ark, mds, *SHAPE)
    assert levels[2][1] != PM.tree(levels[0], ark, mds, *SHAPE)[2][1]


def test_model_verify_codes():
    ark, mds = PM.constants(SHAPE[0], 1, 6)
    height = 3
    leaves = [(i * i + 3) % R for i in range(64)]
    levels = PM.tree(leaves, ark, mds, *SHAPE, 9)
    root = levels[-1][0]
    for i in (0, 63, 37):
        path = PM.paths(levels, [i])[0]
        assert MU.verify(path, i, root, ark, mds, *SHAPE, 9) == MERKLE_PATH_OK
        assert PM.root_from_path(path, i, ark, mds, *SHAPE, 9) == root
        assert MU.verify(path, i, root, ark, mds, *SHAPE, 8) == MERKLE_PATH_LINK             # another capacity: level 0 already
        assert MU.verify(path, i + 64, root, ark, mds, *SHAPE, 9) == MERKLE_PATH_INDEX
        assert MU.verify(path, i, root + 1, ark, mds, *SHAPE, 9) == MERKLE_PATH_LINK + 2
        for l in range(height):
            bad = [list(lv) for lv in path]
            bad[l][((i >> (2 * l)) & 3) ^ 1] += 1                                          # a sibling at level l
            assert MU.verify(bad, i, root, ark, mds, *SHAPE, 9) == MERKLE_PATH_LINK + l
        for l in range(height - 1):
            bad = [list(lv) for lv in path]
            bad[l + 1][(i >> (2 * (l + 1))) & 3] += 1                                      # the path's own child a level up
            assert MU.verify(bad, i, root, ark, mds, *SHAPE, 9) == MERKLE_PATH_LINK + l
        assert MU.verify(path, i ^ 16, root, ark, mds, *SHAPE, 9) == MERKLE_PATH_LINK + 1     # right low digits, wrong digit 2


def test_tree_still_constructs_positionally():
    import plonk_prototype_amd as pa

    class Stub:
        pass
    ctx, leaves, nodes = Stub(), Stub(), Stub()
    t = pa.MerkleTree(ctx, leaves, nodes, 4)
    assert (t.ctx, t.leaves, t.nodes, t.height) == (ctx, leaves, nodes, 4)
    assert t.hades is None and t.capacity == 0
    with pytest.raises(ValueError):
        t.update([0], [1])
    with pytest.raises(ValueError):
        t.verify([], [])
    hades = Stub()
    t = pa.MerkleTree(ctx, leaves, nodes, 4, hades=hades, capacity=7)
    assert t.hades is hades and t.capacity == 7
