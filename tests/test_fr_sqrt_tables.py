"""The tables of the windowed square root without a device: the input sets of tests/fr_sqrt_cases.py
reach every key in every window and every reachable table entry, EXACTLY; the kernel's algorithm restated in integers gives
the constructed roots and the model's points on them; a wrong entry or a wrong key, each in turn, changes an output of either
set; and the host forms -- another algorithm, whose loop follows the order of a^t -- agree on both sets byte for byte."""
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fr_sqrt_cases as F  # noqa: E402
import gadget_model as M  # noqa: E402
import jubjub_codec_model as CM  # noqa: E402
import jubjub_model as J  # noqa: E402

R, G = F.R, F.G
SETS = ("plain", "ratio")


def _traced(which):
    """(outputs, traces, fronts, finish, expected) of a set"""
    if which == "plain":
        want = tuple((c.root, c.flag) for c in F.plain_set())
        return F.plain_traced() + (F.plain_fronts(), lambda f, t: F.windowed_finish(*f, t), want)
    return F.ratio_traced() + (F.ratio_fronts(), F.decode_finish, F.ratio_expected(False))


def test_the_constants_of_the_restatement():
    """the exponents are the header's words, t = -1 mod 2^32, h has order 256 and the keys are distinct"""
    src = open(os.path.join(ROOT, "plonk-prototype_amd", "csrc", "fr_sqrt.hip.h")).read()
    for name, want in (("PLAIN", F.EXP_PLAIN), ("RATIO", F.EXP_RATIO)):
        words = re.search(r"FR_SQRT_EXP_%s\[4\] = \{([^}]*)\}" % name, src).group(1)
        got = sum(int(w.strip().rstrip("UL"), 16) << (64 * i) for i, w in enumerate(words.split(",")))
        assert got == want, name
        windows = int(re.search(r"FR_SQRT_WINDOWS_%s = (\d+)" % name, src).group(1))
        assert 3 * (windows - 1) < want.bit_length() <= 3 * windows, name
    assert F.T & 1 and F.T % (1 << 32) == (1 << 32) - 1 and F.T << 32 == R - 1
    assert pow(F.H, 128, R) == R - 1 and len(set(F.tables().keys)) == F.ENTRIES
    # the relation the two front ends share: x^2 = (the radicand) b
    for a in (7, CM.D, R - 2):
        x, b, _ = F.plain_front(a)
        assert x * x % R == a * b % R and b == pow(a, F.T, R)
        x, b, _ = F.ratio_front(a, 11)
        assert x * x % R == a * pow(11, -1, R) * b % R and b == pow(11 * a, -F.T, R)


def test_the_plain_search_meets_minus_k():
    """c^(2^32) g^k is met as -k mod 2^32: the edge inputs of jubjub_codec_model serve because their list is nearly closed
    under negation"""
    logs = CM.LOG_SQUARES + CM.LOG_NON_SQUARES
    edge = CM.sqrt_edge_inputs()[-len(logs):]
    assert len(CM.sqrt_edge_inputs()) == 6 + len(logs)
    for a, k in zip(edge, logs):
        assert F.seen_plain(a) == -k % (1 << 32), hex(k)
    assert F.seen_plain(pow(G, 2, R)) == 0xfffffffe            # "zero windows" is met as all-ones windows


def test_the_plain_set_holds_what_it_is_built_for():
    cases = F.plain_set()
    assert len(cases) % 64 != 0 and [c.a for c in cases[:4]] == [0, 1, 4, R - 1]
    assert [(c.root, c.flag) for c in cases[:4]] == [(0, 1), (R - 1, 1), (2, 1), (cases[3].root, 1)]
    assert cases[3].root * cases[3].root % R == R - 1 and cases[3].root % 2 == 0
    for c in cases:                                              # the logarithm by Pohlig-Hellman is the one constructed
        assert F.seen_plain(c.a) == c.k and 0 <= c.a < R
        assert c.root % 2 == 0 and (c.root * c.root % R == c.a if c.flag else c.root == 0)
        assert c.flag == (c.k is None or c.k % 2 == 0)
    met = [c.k for c in cases if c.k is not None]
    assert set(F.EDGE_LOGS) <= set(met)
    assert {0, 1, 2, 0xff, 0xff00, 0xff0000, 0xff000000, 0xff, 0x100, 0xffff, 0x10000, 0xffffff, 0x1000000, 1 << 31, (1 << 32) - 1,
            (1 << 32) - 2} <= set(F.EDGE_LOGS)
    # non-squares: every odd digit of window 0, and odd k over the other windows
    assert {k & 0xff for k in met if k & 1} == set(range(1, 256, 2))
    for i in range(1, F.WINDOWS):
        assert len({F.digit(k, i) for k in met if k & 1}) >= 16
    # g^k of every order 2^j, j = 0 .. 32: the trip counts of the host form's loop
    assert {32 - ((k & -k).bit_length() - 1) if k else 0 for k in met} == set(range(33))
    # both branches of the even-root choice: c^(2^31) g^(m / 2) is odd for some inputs and even for others, and so is the root
    # the windowed form arrives at
    assert {c.odd for c in cases if c.flag} == {0, 1} and {c.odd for c in cases if not c.flag} == {None}
    assert {t.negated for t in F.plain_traced()[1] if t.live} == {False, True}


@pytest.mark.parametrize("which", SETS)
def test_every_reachable_key_and_entry_is_read_and_no_other(which):
    """EQUALITIES with the reachable set.  The search matches each of 256 keys in each of four windows and divides entries of
    tables 0 .. 2 out of b; the correction reads the bytes of k >> 1, which is below 2^31, so entries 128 .. 255 of table 3 are
    read by no input at all -- not even by one whose root is thrown away."""
    _, traces, _, _, _ = _traced(which)
    every = {(i, j) for i in range(F.WINDOWS) for j in range(F.ENTRIES)}
    reachable = {(i, j) for (i, j) in every if i < 3 or j < 128}
    assert F.search_pairs() == every and F.correction_pairs() == reachable
    keys = set().union(*(t.keys for t in traces))
    divide = set().union(*(t.divide for t in traces))
    correct = set().union(*(t.correct for t in traces if t.live))
    assert keys == every
    assert divide == {(i, j) for (i, j) in every if i < 3}
    assert correct == reachable, "the digits of k >> 1 on square radicands"
    anything = divide | set().union(*(t.correct for t in traces))
    assert anything == reachable and not any((3, j) in anything for j in range(128, 256))
    # a key that matched on a square radicand, for each of the 256: only there does a wrong key show
    assert {j for t in traces if t.live for (_, j) in t.keys} == set(range(F.ENTRIES))


@pytest.mark.parametrize("which", SETS)
def test_the_restatement_gives_the_constructed_roots_and_the_models_points(which):
    got, _, _, _, want = _traced(which)
    bad = [i for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not bad, bad[:8]
    if which == "ratio":
        status = [s for _, s in want]
        assert {s: status.count(s) for s in set(status)}.keys() == {0, 1, 2, 3}, "every status without the flag"
        assert status.count(CM.BAD_SIGN) == 2                    # y = 1 and y = r - 1 with the sign bit


@pytest.mark.parametrize("which", SETS)
def test_a_wrong_entry_or_key_changes_an_output(which):
    """Each reachable entry in turn becomes (entry) g^e -- e = 1, 2^8, 2^16, 2^24: an error at the bottom of each window; 2^30:
    an element of order four, which survives the even-root choice where a mere sign would not -- and each key in turn becomes g,
    which no window can meet, and then its neighbour h^(j + 1).  At least one input of the set must change its output.  Only the
    inputs that read the entry or matched the key are evaluated."""
    base, traces, fronts, finish, _ = _traced(which)
    t = F.tables()
    readers, matchers = {}, {}
    for n, tr in enumerate(traces):
        for p in tr.divide | tr.correct:
            readers.setdefault(p, []).append(n)
        for (_, j) in tr.keys:
            matchers.setdefault(j, []).append(n)
    assert set(readers) == F.correction_pairs() and set(matchers) == set(range(F.ENTRIES))
    for (i, j), who in sorted(readers.items()):
        for e in (1, 1 << 8, 1 << 16, 1 << 24, 1 << 30):
            wrong = t.with_entry(i, j, t.tab[i][j] * pow(G, e, R) % R)
            assert any(finish(fronts[n], wrong) != base[n] for n in who), (i, j, e)
    for j, who in sorted(matchers.items()):
        for value in (G, t.keys[(j + 1) % F.ENTRIES]):
            wrong = t.with_key(j, value)
            assert any(finish(fronts[n], wrong) != base[n] for n in who), (j, value == G)


def test_the_host_root_on_the_whole_plain_set():
    """pm_fr_sqrt_host against the roots known by construction: every order 2^j of a^t, j = 0 .. 32, is among them"""
    import plonk_prototype_amd as pa
    cases = F.plain_set()
    limbs = M.to_limbs([c.a for c in cases])
    want = M.to_limbs([c.root for c in cases])
    bad = []
    for n, c in enumerate(cases):
        root, flag = pa.fr_sqrt_host(limbs[n])
        if flag != c.flag or root.tobytes() != want[n].tobytes():
            bad.append(n)
    assert not bad, bad[:8]


@pytest.mark.parametrize("flag", (False, True), ids=("plain", "subgroup"))
def test_the_host_decode_on_the_whole_ratio_set(flag):
    import plonk_prototype_amd as pa
    data, want = F.ratio_set(), F.ratio_expected(flag)
    points = J.to_limbs([p for p, _ in want])
    bad = []
    for n, row in enumerate(data):
        got, status = pa.jubjub_decompress_host(row, check_subgroup=flag)
        if status != want[n][1] or got.tobytes() != points[n].tobytes():
            bad.append(n)
    assert not bad, bad[:8]
    if flag:
        status = np.array([s for _, s in want])
        assert (status == CM.OK).sum() >= 64 and (status == CM.BAD_NOT_IN_SUBGROUP).sum() >= 64
