"""Host-side ground for the append-only Poseidon tree: the big-integer model of
tests/ledger_tree_model.py against poseidon_model.tree over padded leaves, the header constant, the slab size and the plan of
an append (pm_test_ledger_plan) against the model's definitions.  No device here."""
import ctypes as C
import os
import random
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ledger_tree_model as LM  # noqa: E402
import poseidon_model as PM  # noqa: E402
from conftest import ROOT  # noqa: E402

R = PM.R
SHAPE = (5, 2)
BAD, LENGTH = -1, -6
EXPORTS = ("create", "free", "info", "bytes", "empty_roots", "append_dev", "truncate_dev", "root_dev", "root", "level", "paths_dev",
           "verify_dev")


@pytest.mark.parametrize("height,per_round,capacity,empty_leaf", [(1, False, 0, 0), (2, True, 77, 0), (3, False, 0, 0x1234567 ** 7 % R),
                                                                  (2, False, 5, R - 1)])
def test_model_equals_the_dense_tree_over_padded_leaves(height, per_round, capacity, empty_leaf):
    ark, mds = PM.constants(SHAPE[0], SHAPE[0] if per_round else 1, 900 + height)
    rng = random.Random(height)
    leaves = [0, R - 1] + [rng.randrange(R) for _ in range(4 ** height - 2)]
    LM.self_check(height, ark, mds, *SHAPE, capacity, empty_leaf, leaves)


def test_model_truncate_then_append_is_a_fresh_tree():
    ark, mds = PM.constants(SHAPE[0], 1, 33)
    rng = random.Random(33)
    a = LM.Ledger(3, ark, mds, *SHAPE, 9, 4)
    first, other = [rng.randrange(R) for _ in range(23)], [rng.randrange(R) for _ in range(30)]
    a.append(first)
    assert a.truncate(5) == 3 and a.truncate(5) == 0
    a.append(other)
    fresh = LM.Ledger(3, ark, mds, *SHAPE, 9, 4)
    fresh.append(first[:5] + other)
    assert a.levels == fresh.levels and a.root == fresh.root
    assert a.truncate(0) == 0 and a.root == a.z[3] and a.levels == [[], [], [], []]


def test_header_constant_and_exports():
    import plonk_prototype_amd as pa
    from plonk_prototype_amd import _lib
    header = open(os.path.join(ROOT, "include", "plonk_mi355x.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "#define PM_POSEIDON_LEDGER_MAX_HEIGHT 31u\n" in header
    assert _lib.POSEIDON_LEDGER_MAX_HEIGHT == LM.MAX_HEIGHT == 31
    assert "#define PM_POSEIDON_MERKLE_MAX_HEIGHT 15u\n" in header             # the dense tree keeps its limit
    lib = C.CDLL(pa.LIB_PATH)
    for name in ["pm_poseidon_ledger_" + e for e in EXPORTS] + ["pm_test_ledger_plan"]:
        assert re.search(rf"\b{name}\(", header), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
        assert f"pub fn {name}(" in doc, name
    assert _lib.SIGNATURES["pm_poseidon_ledger_verify_dev"] == _lib.SIGNATURES["pm_poseidon_merkle_verify_dev"]
    for name in ("append", "append_dev", "truncate", "level", "paths", "paths_dev", "verify", "root_dev", "free"):
        assert callable(getattr(pa.LedgerTree, name)), name
    for name in ("count", "reserve", "device_bytes", "root", "empty_roots"):
        assert isinstance(getattr(pa.LedgerTree, name), property), name
    assert callable(pa.Hades.ledger) and callable(pa.Hades.verify_ledger_paths)


def test_slab_bytes_against_the_model():
    import plonk_prototype_amd as pa
    size = pa.load().pm_poseidon_ledger_bytes
    rng = random.Random(7)
    for height in (1, 2, 3, 5, 10, 17, 31):
        full = 4 ** height
        reserves = {0, 1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 256, 1000, 4 ** 5 - 1, 4 ** 5, 4 ** 5 + 1, 1 << 20}
        reserves |= {rng.randrange(1 << 24) for _ in range(20)}
        for reserve in sorted(r for r in reserves if r <= full):
            assert size(height, reserve) == 32 * LM.slab_elements(height, reserve), (height, reserve)
        assert size(height, full + 1) == 0
    assert size(1, 4) == 32 * 5 and size(3, 64) == 32 * 85 and size(17, 0) == 0
    assert size(2, 5) == 32 * (5 + 2 + 1) and size(17, 1) == 32 * 18             # one leaf: a node a level
    assert size(0, 0) == 0 and size(32, 1) == 0 and size(0, 1) == 0
    assert size(31, 4 ** 31) == (1 << 64) - 1                                     # more than an address space: no allocation succeeds


def _plan(height, count, k):
    import plonk_prototype_amd as pa
    arrays = [np.full(height, 0xA5A5, np.uint64) for _ in range(3)]
    chain, hashed = C.c_uint32(99), C.c_uint64(99)
    rc = pa.load().pm_test_ledger_plan(height, count, k, *[a.ctypes.data_as(C.POINTER(C.c_uint64)) for a in arrays], C.byref(chain),
                                       C.byref(hashed))
    assert rc == 0, (height, count, k, rc)
    return [a.tolist() for a in arrays] + [chain.value, hashed.value]


def test_plan_against_the_model():
    cases = []
    for height in (1, 2, 3, 6, 17, 31):
        full = 4 ** height
        for p in range(0, min(height, 8) + 1):                                   # c + k on and around powers of 4
            for end in (4 ** p - 1, 4 ** p, 4 ** p + 1):
                for k in (1, 2, 3, 5, 64, 1000):
                    if 0 < end <= full and k <= end:
                        cases.append((height, end - k, k))
        for count in sorted({0, 1, min(5, full), full // 2, full - 1, full}):
            cases.append((height, count, 0))                                     # k = 0
            if count < full:
                cases.append((height, count, 1))
            if count >= 7:
                cases.append((height, count - 7, 7))                             # ... up to the last position
    cases.append((6, 4 ** 5 - 1, 2))                                             # straddles the boundary of level 5
    cases.append((31, 4 ** 31 - 3, 3))
    cases.append((17, 0, (1 << 31) - 1))
    rng = random.Random(11)
    for _ in range(200):
        height = rng.randrange(1, 32)
        k = rng.randrange(1, min(4 ** height, 1 << 20) + 1)
        cases.append((height, rng.randrange(0, 4 ** height - k + 1), k))
    for height, count, k in cases:
        assert _plan(height, count, k) == list(LM.plan(height, count, k)), (height, count, k)
    first, nodes, below, chain, hashed = _plan(6, 4 ** 5 - 1, 2)
    assert nodes == [2, 2, 2, 2, 2, 1] and chain == 6 and hashed == 11           # two nodes a level up to level 5
    assert first == [255, 63, 15, 3, 0, 0] and below == [1025, 257, 65, 17, 5, 2]
    assert _plan(17, 12345, 0) == [[0] * 17] * 3 + [0, 0]
    assert _plan(3, 16, 1)[3] == 1 and _plan(3, 15, 2)[3] == 3                    # 15 | 16: parents 3 and 4, grandparents 0 and 1
    assert _plan(31, 0, 1)[1] == [1] * 31


def test_plan_refusals_and_null_outputs():
    import plonk_prototype_amd as pa
    plan = pa.load().pm_test_ledger_plan
    assert plan(0, 0, 1, None, None, None, None, None) == BAD and plan(32, 0, 1, None, None, None, None, None) == BAD
    assert plan(2, 17, 0, None, None, None, None, None) == BAD                   # no tree holds more than 4^height
    assert plan(2, 16, 1, None, None, None, None, None) == LENGTH and plan(2, 10, 7, None, None, None, None, None) == LENGTH
    assert plan(31, 0, 1 << 31, None, None, None, None, None) == LENGTH
    assert plan(31, 4 ** 31, 1, None, None, None, None, None) == LENGTH
    assert plan(2, 10, 6, None, None, None, None, None) == 0 and plan(2, 16, 0, None, None, None, None, None) == 0
    hashed = C.c_uint64(0)
    assert plan(3, 5, 20, None, None, None, None, C.byref(hashed)) == 0 and hashed.value == LM.plan(3, 5, 20)[4]
