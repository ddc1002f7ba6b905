"""The exit of the radix-4 last and single passes (fe_reduce_canon_pack, csrc/fields.hip.h), walked through the limb-exact
model of oracle/fe_model.py -- no GPU, no library.

r = fe_reduce_weak(x); the wave votes on top(r) >= top(m); without a vote the limbs of r are packed as they are, with one
the compare, subtract and select of fe_canon_pack run first.  exit_model() is that routine; `vote` stands for the other
lanes of the wave.  Checked: the packed result is value mod m whatever the other lanes vote, and the lane's own predicate
is true whenever r >= m -- on k m + d for k = 0 .. 39 and d at and around 0, m and top(m) 2^232, the limbs spread up to the
bound of the class the last step hands over (dft4's outputs: B < 5, V < 40), and on the worst members of that class."""
import random

import pytest

from oracle import fe_model as F

FR = F.FR
M8 = FR.M[8]                                    # top(m)
EDGE = M8 << 232


@pytest.fixture(autouse=True)
def _clean():
    del F.VIOLATIONS[:]
    yield
    del F.VIOLATIONS[:]


# ---------------------------------------------------------------------------- the exit
def weak_digit(x):
    """the q of fe_reduce_weak"""
    return ((x[8] + (x[7] >> 29)) * ((1 << 52) // (M8 + 1))) >> 52


def exit_model(x, vote=False):
    """fe_reduce_canon_pack: (saturated words, the lane's predicate, r >= m).  vote: another lane of the wave votes."""
    r = F.fe_reduce_weak(FR, x)
    mine = r[8] >= M8
    if mine or vote:
        s = F.fe_canon_pack(FR, r)              # its fe_norm_full leaves normalised limbs as they are
        assert F.fe_norm_full(FR, r) == r
    else:
        s = F.fe_pack_raw(FR, r)
    return s, mine, F.value_of(FR, r) >= FR.mod


def packed(v):
    return [(v >> (32 * j)) & F.M32 for j in range(8)]


def spread(v, rng):
    """limbs of v: normalised, pushed down as far as (5+) allows, and pushed down at random"""
    top = 5 * (1 << 29) + 7
    out = [F.limbs_of(FR, v), F.most_redundant(FR, v, 5, True)]
    l = F.limbs_of(FR, v)
    for i in range(7, -1, -1):
        k = rng.randint(0, min(l[i + 1], (top - l[i]) >> 29))
        l[i + 1] -= k
        l[i] += k << 29
    out.append(l)
    for l in out:
        assert F.value_of(FR, l) == v and max(l) <= top
    return out


def exit_cases(seed=0x45584954):
    """k m + d, k = 0 .. 39, d at the edges and random, each in three limb spreadings"""
    rng = random.Random(seed)
    cases = []
    for k in range(40):
        ds = [0, 1, FR.mod - 1, EDGE - 1, EDGE, EDGE + 1, rng.randrange(FR.mod), rng.randrange(EDGE, FR.mod)]
        for d in ds:
            cases += spread(k * FR.mod + d, rng)
    return cases


def test_exit_is_value_mod_m_packed():
    n_vote = n_sub = 0
    for x in exit_cases():
        v = F.value_of(FR, x)
        assert weak_digit(x) < 64
        s, mine, needs = exit_model(x)
        assert s == packed(v % FR.mod)
        assert mine or not needs                                    # no subtraction without the lane's own vote
        assert exit_model(x, vote=True)[0] == s                     # the slow path is exact for r < m too
        n_vote += mine
        n_sub += needs
    assert n_sub and n_vote > n_sub                                 # both kinds of voters occur
    assert F.VIOLATIONS == []


def test_exit_predicate_is_necessary_for_every_normalised_r_below_2m():
    """top(r) < top(m) => r < m for normalised limbs; and the slow path is exact up to 2m - 1"""
    rng = random.Random(7)
    vals = [0, EDGE - 1, EDGE, FR.mod - 1, FR.mod, FR.mod + (FR.mod >> 16), 2 * FR.mod - 1]
    vals += [rng.randrange(2 * FR.mod) for _ in range(300)]
    for v in vals:
        r = F.limbs_of(FR, v)
        assert r[8] >= M8 or v < FR.mod
        assert F.fe_canon_pack(FR, r) == packed(v % FR.mod)
    assert F.VIOLATIONS == []


def test_the_slow_path_is_rare():
    """the share of [0, m) whose top limb reaches top(m): the figure the comment at fe_reduce_canon_pack gives"""
    assert 4.2e-8 < (FR.mod - EDGE) / FR.mod < 4.4e-8


def test_exit_takes_the_worst_of_what_the_last_step_hands_over():
    """dft4's output class (B < 5, V < 40), and the same with the slack of a carry step: the digit stays below 64, no
    32- or 64-bit intermediate wraps, the result is canonical"""
    for plus in (False, True):
        for x in F.class_members(FR, 5, 40, plus, n_random=200, seed=5):
            assert weak_digit(x) < 64 and F.value_of(FR, x) < 1 << 261
            s, mine, needs = exit_model(x)
            assert s == packed(F.value_of(FR, x) % FR.mod) and (mine or not needs)
    assert F.VIOLATIONS == []
