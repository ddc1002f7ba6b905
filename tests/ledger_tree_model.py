"""Big-integer model of the append-only Poseidon tree (include/plonk_mi355x.h, pm_poseidon_ledger_*) on
top of tests/poseidon_model.py.  Plain Python integers throughout.

Definitions.  `count` is the number of filled leaves; level 0 is the leaves, level l stores the nodes [0, ceil(count / 4^l)),
level H the root when count > 0.  Z_0 = empty_leaf, Z_(l+1) = node(Z_l, Z_l, Z_l, Z_l); a child at or beyond the stored prefix
of its level reads as that level's Z; the root of an empty tree is Z_H.  Appending k leaves at c = count dirties, at level
l >= 1, exactly the nodes (c >> 2l) .. ((c + k - 1) >> 2l).

`self_check` holds the model to poseidon_model.tree over the leaves padded with empty_leaf: for H <= 3 and every count."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import poseidon_model as PM  # noqa: E402

MAX_HEIGHT = 31


def width(leaves, l):
    """the stored nodes of level l of a tree with `leaves` filled leaves: ceil(leaves / 4^l)"""
    return (leaves + (1 << (2 * l)) - 1) >> (2 * l)


def slab_elements(height, reserve):
    """the elements of a slab with room for `reserve` leaves: every level 0..H at its width"""
    return sum(width(reserve, l) for l in range(height + 1))


def plan(height, count, k):
    """-> (first[H], nodes[H], below[H], chain_from, hashed): level l = 1..H at index l - 1.  first = the first node an append
    of k leaves at `count` hashes, nodes = how many, below = the stored width of level l - 1 afterwards; chain_from = the first
    level whose range is one node (0 for k = 0); hashed = the sum of nodes"""
    assert 1 <= height <= MAX_HEIGHT and count + k <= 4 ** height
    if k == 0:
        return [0] * height, [0] * height, [0] * height, 0, 0
    first = [count >> (2 * l) for l in range(1, height + 1)]
    nodes = [((count + k - 1) >> (2 * l)) - (count >> (2 * l)) + 1 for l in range(1, height + 1)]
    below = [width(count + k, l - 1) for l in range(1, height + 1)]
    chain_from = 1 + next(i for i, n in enumerate(nodes) if n == 1)
    return first, nodes, below, chain_from, sum(nodes)


class Ledger:
    """levels[l] = the stored prefix of level l; what lies beyond `count` is dropped on a truncate"""

    def __init__(self, height, ark, mds, rounds, full, capacity=0, empty_leaf=0):
        assert 1 <= height <= MAX_HEIGHT
        self.height, self.hades, self.capacity = height, (ark, mds, rounds, full), capacity
        self.z = [empty_leaf % PM.R]
        for _ in range(height):
            self.z.append(self._node([self.z[-1]] * 4))
        self.levels = [[] for _ in range(height + 1)]

    def _node(self, children):
        return PM.node(children, *self.hades, self.capacity)

    @property
    def count(self):
        return len(self.levels[0])

    @property
    def root(self):
        return self.levels[self.height][0] if self.count else self.z[self.height]

    def _child(self, l, i):
        """node i of level l, the empty subtree when it is not stored"""
        return self.levels[l][i] if i < len(self.levels[l]) else self.z[l]

    def _rehash(self, l, i):
        value = self._node([self._child(l - 1, 4 * i + c) for c in range(4)])
        if i < len(self.levels[l]):
            self.levels[l][i] = value
        else:
            assert i == len(self.levels[l])
            self.levels[l].append(value)

    def append(self, values):
        """-> the permutations run"""
        c, k = self.count, len(values)
        assert c + k <= 4 ** self.height
        if k == 0:
            return 0
        self.levels[0].extend(v % PM.R for v in values)
        hashed = 0
        for l in range(1, self.height + 1):
            for i in range(c >> (2 * l), ((c + k - 1) >> (2 * l)) + 1):
                self._rehash(l, i)
                hashed += 1
        assert [len(lv) for lv in self.levels] == [width(c + k, l) for l in range(self.height + 1)]
        assert hashed == plan(self.height, c, k)[4]
        return hashed

    def truncate(self, new_count):
        """-> the permutations run: the H ancestors of leaf new_count - 1, nothing for 0 or the same count"""
        assert new_count <= self.count
        if new_count == self.count:
            return 0
        for l in range(self.height + 1):
            del self.levels[l][width(new_count, l):]
        if new_count == 0:
            return 0
        for l in range(1, self.height + 1):
            self._rehash(l, (new_count - 1) >> (2 * l))
        return self.height

    def paths(self, indices):
        """out[j][l][c] = node ((i >> 2l) & ~3) + c of level l, the level's Z when it is not stored"""
        assert all(0 <= i < self.count for i in indices)
        return [[[self._child(l, ((i >> (2 * l)) & ~3) + c) for c in range(4)] for l in range(self.height)] for i in indices]


def self_check(height, ark, mds, rounds, full, capacity, empty_leaf, leaves):
    """For every count 0..4^H: a ledger grown leaf by leaf, one appended in a single call and one truncated from the full tree
    all equal poseidon_model.tree over the leaves padded with empty_leaf -- root, every stored prefix, the paths."""
    total = 4 ** height
    assert len(leaves) == total and height <= 3
    grown = Ledger(height, ark, mds, rounds, full, capacity, empty_leaf)
    cut = Ledger(height, ark, mds, rounds, full, capacity, empty_leaf)
    assert cut.append(leaves) == (total - 1) // 3
    dense_empty = PM.tree([empty_leaf] * total, ark, mds, rounds, full, capacity)
    assert [lv[0] for lv in dense_empty] == grown.z
    for count in range(total + 1):
        if count:
            assert grown.append([leaves[count - 1]]) == height
        dense = PM.tree(leaves[:count] + [empty_leaf] * (total - count), ark, mds, rounds, full, capacity)
        once = Ledger(height, ark, mds, rounds, full, capacity, empty_leaf)
        once.append(leaves[:count])
        for t in (grown, once):
            assert t.count == count and t.root == dense[height][0], count
            assert t.levels == [dense[l][:width(count, l)] for l in range(height + 1)], count
            probe = sorted({0, count // 2, count - 1}) if count else []
            assert t.paths(probe) == PM.paths(dense, probe), count
    for count in range(total, -1, -1):                                     # ... and rolled back leaf by leaf
        assert cut.truncate(count) == (height if 0 < count < total else 0)
        dense = PM.tree(leaves[:count] + [empty_leaf] * (total - count), ark, mds, rounds, full, capacity)
        assert cut.root == dense[height][0] and cut.levels == [dense[l][:width(count, l)] for l in range(height + 1)], count
