"""Big-integer model of the native Poseidon (include/plonk_mi355x.h, pm_poseidon_*): the sponge tests/hades_model.Builder.sponge
lays out, an arity-4 Merkle tree and its sibling paths, on top of hades_model.hades_model.  The reference of
tests/test_poseidon_host.py and tests/test_gpu_poseidon.py.  Plain Python integers throughout."""
import os
import random
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hades_model as HM  # noqa: E402

R, WIDTH = HM.R, HM.WIDTH
SHAPES = ((1, 0), (2, 2), (5, 2), (9, 4), (67, 8))      # (rounds, full rounds)


def constants(rounds, n_mds, seed):
    """-> (ark [rounds][5], mds: one matrix [5][5] when n_mds == 1, else [rounds][5][5]), random and reproducible"""
    rng = random.Random(seed)
    ark = [[rng.randrange(R) for _ in range(WIDTH)] for _ in range(rounds)]
    mats = [[[rng.randrange(R) for _ in range(WIDTH)] for _ in range(WIDTH)] for _ in range(n_mds)]
    assert n_mds in (1, rounds)
    return ark, (mats[0] if n_mds == 1 else mats)


def flat(ark, mds):
    """-> (the round keys, the matrix entries, n_mds) as flat integer lists in the order of the C interface"""
    per_round = isinstance(mds[0][0], (list, tuple))
    mats = mds if per_round else [mds]
    return [x for row in ark for x in row], [x for m in mats for row in m for x in row], len(mats)


def sponge(msg, ark, mds, rounds, full, capacity=0):
    """the state starts as (capacity, 0, 0, 0, 0); every chunk of up to four inputs is added to words 1..4, a short chunk also
    adds 1 to the word after its last input; one permutation follows each chunk.  -> word 1 of the final state"""
    assert len(msg) >= 1
    state = [capacity % R, 0, 0, 0, 0]
    for k in range(0, len(msg), 4):
        chunk = msg[k:k + 4]
        for t, x in enumerate(chunk):
            state[1 + t] = (state[1 + t] + x) % R
        if len(chunk) < 4:
            state[1 + len(chunk)] = (state[1 + len(chunk)] + 1) % R
        state = HM.hades_model(state, ark, mds, rounds, full)
    return state[1]


def node(children, ark, mds, rounds, full, capacity=0):
    """one permutation of (capacity, c0..c3), no padding: the sponge on a message of four"""
    assert len(children) == 4
    return HM.hades_model([capacity % R] + list(children), ark, mds, rounds, full)[1]


def tree(leaves, ark, mds, rounds, full, capacity=0):
    """-> [level 0 (the leaves), level 1, ..., level h (the root alone)]"""
    levels = [list(leaves)]
    while len(levels[-1]) > 1:
        below = levels[-1]
        assert len(below) % 4 == 0
        levels.append([node(below[4 * i:4 * i + 4], ark, mds, rounds, full, capacity) for i in range(len(below) // 4)])
    return levels


def flat_tree(levels):
    """levels 1..h one after the other, the root last: what pm_poseidon_merkle_dev writes"""
    return [x for level in levels[1:] for x in level]


def paths(levels, indices):
    """out[j][l][c] = node ((i >> 2l) & ~3) + c of level l, i = indices[j], l < h"""
    h = len(levels) - 1
    return [[[levels[l][((i >> (2 * l)) & ~3) + c] for c in range(4)] for l in range(h)] for i in indices]


def root_from_path(path, index, ark, mds, rounds, full, capacity=0):
    """fold a path upwards, checking that each level's hash is the child the next level holds at the path's position"""
    acc = None
    for l, children in enumerate(path):
        if acc is not None and children[(index >> (2 * l)) & 3] != acc:
            return None
        acc = node(children, ark, mds, rounds, full, capacity)
    return acc


to_limbs = HM.to_limbs
