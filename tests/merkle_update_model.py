"""Big-integer model of the incremental tree update and the path verification (include/plonk_mi355x.h,
pm_poseidon_merkle_update_dev and pm_poseidon_merkle_verify_dev) on top of poseidon_model.  The
reference of tests/test_merkle_update_host.py and tests/test_gpu_merkle_update.py.  Plain Python integers throughout."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import poseidon_model as PM  # noqa: E402

PATH_OK, PATH_INDEX, PATH_LINK = 0, 1, 2


def update(levels, indices, values, ark, mds, rounds, full, capacity=0, check=True):
    """levels[0][indices[j]] = values[j], then every ancestor of a changed leaf is hashed again, each once, from its four
    children as they stand: the distinct parents of one level's changed nodes are the changed nodes of the next.  In place.
    -> the permutations run.  With ``check`` the result must be PM.tree over the changed leaves (which holds whenever the
    nodes that are not ancestors were right before)."""
    h = len(levels) - 1
    assert len(set(indices)) == len(indices) and all(0 <= i < 4 ** h for i in indices)
    for i, v in zip(indices, values):
        levels[0][i] = v
    touched, hashed = sorted(indices), 0
    for l in range(1, h + 1):
        touched = sorted({i >> 2 for i in touched})
        for i in touched:
            levels[l][i] = PM.node(levels[l - 1][4 * i:4 * i + 4], ark, mds, rounds, full, capacity)
        hashed += len(touched)
    if check:
        assert levels == PM.tree(levels[0], ark, mds, rounds, full, capacity)
    return hashed


def hashed_count(indices, height):
    """sum over l = 1..height of |{ i >> 2l }|"""
    return sum(len({i >> (2 * l) for i in indices}) for l in range(1, height + 1))


def ancestors(indices, height):
    """the rows of the flat tree (levels 1..height one after the other) that are ancestors of the given leaves"""
    rows, first = set(), 0
    for l in range(1, height + 1):
        rows |= {first + (i >> (2 * l)) for i in indices}
        first += 4 ** (height - l)
    return rows


def verify(path, index, root, ark, mds, rounds, full, capacity=0):
    """path[l] = the four children at level l.  -> PATH_OK; PATH_INDEX for an index that is not below 4^height (nothing of
    the path is looked at); PATH_LINK + l for the lowest l at which the hash of path[l] is not child (index >> 2(l + 1)) & 3
    of path[l + 1], or not the root for the last level"""
    h = len(path)
    if index >> (2 * h):
        return PATH_INDEX
    for l in range(h):
        got = PM.node(path[l], ark, mds, rounds, full, capacity)
        want = path[l + 1][(index >> (2 * (l + 1))) & 3] if l + 1 < h else root
        if got != want:
            return PATH_LINK + l
    return PATH_OK
