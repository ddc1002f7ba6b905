"""The buffer contracts of the append-only Poseidon tree's device entry points (DESIGN.md sections 7.2r and 8) in a guard
arena (tests/guard_arena.py): every caller buffer is carved at exactly the size the header gives it out of one allocation of
0xA5 bytes, so a write outside it, or into an input, is found by comparing bytes."""
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guard_arena as G  # noqa: E402
import ledger_tree_model as LM  # noqa: E402
import merkle_update_model as MU  # noqa: E402
import poseidon_model as PM  # noqa: E402

pytestmark = pytest.mark.gpu
R = PM.R
SHAPE = (5, 2)
FORMS = ("auto", "thread", "wave")
HEIGHT, CAPACITY, EMPTY = 17, 9, 0x123456789ABCDEF ** 2 % R
_CACHE = {}


def _case():
    """-> (ark, mds, 70 leaves, the model over them), built once and never changed"""
    if not _CACHE:
        ark, mds = PM.constants(SHAPE[0], SHAPE[0], 1717)
        rng = random.Random(17)
        leaves = [rng.randrange(R) for _ in range(70)]
        model = LM.Ledger(HEIGHT, ark, mds, *SHAPE, CAPACITY, EMPTY)
        model.append(leaves)
        _CACHE["case"] = (ark, mds, leaves, model)
    return _CACHE["case"]


@pytest.fixture(scope="module")
def hades(ctx):
    import plonk_prototype_amd as pa
    ark, mds, _, _ = _case()
    a, m, _ = PM.flat(ark, mds)
    h = pa.Hades(ctx, PM.to_limbs(a), PM.to_limbs(m), *SHAPE)
    yield h
    h.free()


def _flat_paths(paths):
    return PM.to_limbs([x for path in paths for four in path for x in four])


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("k", [1, 5, 65, 70])
def test_ledger_append_values(ctx, hades, k, form):
    """k elements of d_values, read only; the tree is the handle's own memory"""
    _, _, leaves, model = _case()
    t = hades.ledger(HEIGHT, CAPACITY, EMPTY)
    try:
        with G.GuardArena.of(ctx, values=PM.to_limbs(leaves[:k])) as ar:
            assert t.append_dev(ar.addr("values"), k, form=form) == LM.plan(HEIGHT, 0, k)[4]
            ar.check()                                                          # bands 0xA5, the input as uploaded
        if k == 70:
            assert t.root.tobytes() == PM.to_limbs([model.root])[0].tobytes()
    finally:
        t.free()


def test_ledger_paths_ragged_output(ctx, hades):
    """k = 3 at H = 17: 3 x 8 bytes of indices in, exactly 3 x 17 x 4 elements out"""
    _, _, leaves, model = _case()
    k, idx = 3, [69, 0, 34]
    t = hades.ledger(HEIGHT, CAPACITY, EMPTY)
    try:
        t.append(PM.to_limbs(leaves))
        with G.GuardArena.of(ctx, idx=np.array(idx, np.uint64), out=32 * k * HEIGHT * 4) as ar:
            t.paths_dev(ar.addr("idx"), k, ar.addr("out"))
            want = _flat_paths(model.paths(idx))
            assert np.array_equal(G.as_u64(ar.check()["out"], k * HEIGHT * 4, 4), want)
    finally:
        t.free()


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("k", [1, 5, 65])
def test_ledger_verify(ctx, hades, k, form):
    """k uint32 of status, exactly; paths, indices and the root are read only"""
    ark, mds, _, model = _case()
    rng = random.Random(k)
    idx = [69] + [rng.randrange(70) for _ in range(k - 1)]
    paths = model.paths(idx)
    if k > 1:
        idx[1] = 4 ** HEIGHT                                                    # PM_MERKLE_PATH_INDEX
        for j in list(range(2, min(k, 6))) + [k - 1]:
            l = (5 * j) % HEIGHT                                                # a sibling changes: the link above l breaks
            sibling = ((idx[j] >> (2 * l)) & 3) ^ 1
            paths[j][l][sibling] = (paths[j][l][sibling] + 1) % R
    want = [MU.verify(p, i, model.root, ark, mds, *SHAPE, CAPACITY) if i < 4 ** HEIGHT else MU.PATH_INDEX for p, i in zip(paths, idx)]
    assert want[0] == MU.PATH_OK and (k == 1 or (want[1] == MU.PATH_INDEX and want[k - 1] >= MU.PATH_LINK))
    with G.GuardArena.of(ctx, paths=_flat_paths(paths), idx=np.array(idx, np.uint64), root=PM.to_limbs([model.root]),
                         status=4 * k) as ar:
        hades.verify_ledger_paths_dev(ar.addr("paths"), ar.addr("idx"), k, HEIGHT, ar.addr("root"), ar.addr("status"), CAPACITY,
                                      form=form)
        assert ar.check()["status"].view(np.uint32).tolist() == want, (k, form)


def test_ledger_verify_refuses_a_status_on_an_input(ctx, hades):
    import plonk_prototype_amd as pa
    _, _, _, model = _case()
    k, idx = 5, [0, 1, 33, 68, 69]
    with G.GuardArena.of(ctx, paths=_flat_paths(model.paths(idx)), idx=np.array(idx, np.uint64), root=PM.to_limbs([model.root])) as ar:
        for status in (ar.addr("paths"), ar.addr("idx"), ar.addr("root"), ar.addr("root") + 16, ar.addr("idx") + 32):
            with pytest.raises(pa.Error) as e:
                hades.verify_ledger_paths_dev(ar.addr("paths"), ar.addr("idx"), k, HEIGHT, ar.addr("root"), status, CAPACITY)
            assert e.value.code == pa._lib.PM_ERR_BAD_ARG
        ar.check_unchanged()
