"""The limb-exact model of the binary-GCD inversion (oracle/fe_model.py: fe_canon_limbs, fe_inv_int, fe_inv_dev; the device
code is csrc/field_inv.hip.h) over the integers of tests/inv_cases.py -- no GPU, no library.  The model computes what plain
integers say, wraps no int32 / int64 / u32 / u64 intermediate, keeps |v| below the 32 m its last step relies on, and the case
lists reach what they claim to reach: every round count, the exact path, the sign repair of either row.  Then the operand class
of fe_canon_limbs: what holds, what wraps, and that every call site hands over a member.  Exact integer comparisons only."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import inv_cases as IC  # noqa: E402
from oracle import fe_model as M  # noqa: E402

FIELDS = IC.FIELDS


@pytest.fixture(autouse=True)
def clean_log():
    M.VIOLATIONS.clear()
    yield
    M.VIOLATIONS.clear()


def val(f, l):
    return M.value_of(f, l)


# ---------------------------------------------------------------------------- fe_inv_int over the case lists
@pytest.mark.parametrize("f", FIELDS, ids=repr)
def test_inverse_against_pow(f):
    """v y = 1 (mod m), 0 -> 0, limbs < 2^W, value < 64 m; nothing wrapped, no precondition or class was broken on the way"""
    m = f.mod
    walked, violations = IC.walk(f)
    assert len(walked) == len(IC.cases(f)) > 1000 and walked[0][0] == 0
    for y, r, _ in walked:
        assert val(f, r) % m == (pow(y, -1, m) if y else 0), hex(y)
        assert max(r) < 1 << f.W and val(f, r) < 64 * m, hex(y)
    assert list(walked[0][1]) == M.limbs_of(f, 32 * m)               # 0 -> v = 0, handed back as 0 + 32 m
    assert not violations, violations[:5]


@pytest.mark.parametrize("f", FIELDS, ids=repr)
def test_u_v_stay_far_below_32m(f):
    """fe_inv_int ends with v + 32 m, which needs |v| < 32 m (the header argues |v| < (ROUNDS + 1) m loosely).  Measured over
    the case lists, after every round: Fr max |u| = 3.74 m, max |v| = 3.79 m; Fp max |u| = 4.09 m, max |v| = 4.52 m.  The
    assertion is the requirement, 32 m; the figures are printed.  (No sign repair happens on the exact path or in round
    ROUNDS in these lists: an exact comparison cannot be wrong.)"""
    walked, _ = IC.walk(f)
    mu, mv = max(t["max_u"] for _, _, t in walked), max(t["max_v"] for _, _, t in walked)
    print(f"{f}: max |u| = {mu / f.mod:.3f} m, max |v| = {mv / f.mod:.3f} m")
    assert mu < 32 * f.mod and mv < 32 * f.mod


@pytest.mark.parametrize("f", FIELDS, ids=repr)
def test_lists_reach_what_they_claim(f):
    walked, _ = IC.walk(f)
    rounds = {t["rounds"] for _, _, t in walked}
    lo = min(r for r in rounds if r)
    assert rounds == {0} | set(range(lo, M.inv_rounds(f) + 1)), sorted(rounds)
    assert M.inv_rounds(f) == (18 if f is M.FR else 28)
    assert [t["rounds"] for y, _, t in walked if y == 0] == [0]
    a_rep = sum(any(s[0] for s in t["steps"]) for _, _, t in walked)
    b_rep = sum(any(s[1] for s in t["steps"]) for _, _, t in walked)
    assert a_rep >= 50 and b_rep >= 50, (a_rep, b_rep)              # Fp's b row too: the k R mod m family (inv_cases.py)
    # the exact path in some round, after a round that was not exact: the switch happens inside one inversion
    switched = 0
    for _, _, t in walked:
        e = [s[2] for s in t["steps"]]
        switched += True in e and False in e[:e.index(True)]
    assert switched >= 50
    # round ROUNDS still changes v: what a loop one round short gets wrong (the round that only turns a = b = 1 into a = 0
    # leaves v alone, so reaching ROUNDS rounds with a != 0 is not enough)
    v_last = sum(t["v_rounds"] == M.inv_rounds(f) for _, _, t in walked)
    assert v_last >= 10, v_last
    last = sum(t["rounds"] == M.inv_rounds(f) and (t["steps"][-1][0] or t["steps"][-1][1]) for _, _, t in walked)
    on_exact = sum(any((s[0] or s[1]) and s[2] for s in t["steps"]) for _, _, t in walked)
    print(f"{f}: a-row repairs in {a_rep} cases, b-row in {b_rep}, in round ROUNDS in {last}, on the exact path in {on_exact}; "
          f"v changes in round ROUNDS in {v_last}")


@pytest.mark.parametrize("f", FIELDS, ids=repr)
def test_full_round_case(f):
    y = IC.FULL_ROUND[f.name]
    assert y in IC.cases(f)
    trace = {}
    r = M.fe_inv_int(f, M.limbs_of(f, y), trace)
    assert trace["rounds"] == trace["v_rounds"] == M.inv_rounds(f) and val(f, r) * y % f.mod == 1
    assert not M.VIOLATIONS


def test_round_zero_cannot_be_exact():
    """b starts as the modulus, whose high limbs are not zero: no input takes the exact path in its first round"""
    for f in FIELDS:
        walked, _ = IC.walk(f)
        assert not any(t["steps"][0][2] for _, _, t in walked if t["steps"])


@pytest.mark.parametrize("f", FIELDS, ids=repr)
def test_inv_dev(f):
    """x^-1 in the device Montgomery form from any representative the class admits; x = 0 and x = m give 0"""
    m, r2 = f.mod, f.RADIX * f.RADIX % f.mod
    for y in IC.cases(f)[::37] + (0, 1, m - 1):
        for x in (M.limbs_of(f, y), M.limbs_of(f, y + m), IC.redundant(f, y), IC.redundant(f, y + m)):
            r = M.fe_inv_dev(f, x)
            assert M.in_class(f, r, 1, 2) and val(f, r) * y % m == (r2 if y else 0), hex(y)
    assert not M.VIOLATIONS, M.VIOLATIONS[:5]


def test_the_detector_fires():
    """a non-canonical operand, and an int32 wrap forced through an operand the routine does not admit, are both recorded"""
    f = M.FR
    M.fe_inv_int(f, M.limbs_of(f, f.mod + 5))
    assert any("fe_inv_int in" in v for v in M.VIOLATIONS)
    M.VIOLATIONS.clear()
    M.fe_inv_int(f, [f.MASK] * (f.N - 1) + [M.M32])                # a top limb of 32 bits: the approximation window overflows
    assert any("wrap" in v for v in M.VIOLATIONS)
    assert M._i32(1 << 31, "x") == -(1 << 31) and M._i64(-(1 << 63) - 1, "x") == (1 << 63) - 1 and len(M.VIOLATIONS) >= 3


# ---------------------------------------------------------------------------- fe_canon_limbs and its class
@pytest.mark.parametrize("f", FIELDS, ids=repr)
def test_canon_limbs_class(f):
    """value < 2 m, limbs < 2^32 - 2^(32-W): the canonical limbs of value mod m, nothing wraps"""
    for l in IC.canon_cases(f):
        assert M.fe_canon_limbs(f, list(l)) == M.limbs_of(f, val(f, l) % f.mod), l
    assert not M.VIOLATIONS, M.VIOLATIONS[:5]


@pytest.mark.parametrize("f", FIELDS, ids=repr)
def test_canon_limbs_any_limb_below_2_32_wraps(f):
    """The class the routine used to document, "any limbs < 2^32", does not hold: a limb of 2^32 - 1 with a carry coming in
    wraps fe_norm_full's 32-bit sum, for a value far below 2 m, and the result is wrong.  The largest limb of the settled
    class under the largest carry does not."""
    top = M.canon_limb_max(f)
    for limb1, bad in ((M.M32, True), (M.M32 - 1, True), (top, False)):
        a = [top, limb1] + [0] * (f.N - 2)                           # limb 0 sends the largest carry, 2^(32-W) - 1
        assert val(f, a) < f.mod
        r = M.fe_canon_limbs(f, a)
        assert any("u32 wrap in fe_norm_full" in v for v in M.VIOLATIONS) == bad
        assert (r != M.limbs_of(f, val(f, a))) == bad
        M.VIOLATIONS.clear()
    if f is M.FR:
        M.fe_canon_limbs(f, [1 << 29, M.M32] + [0] * 7)              # the smallest such operand: one carry bit suffices
        assert any("u32 wrap in fe_norm_full" in v for v in M.VIOLATIONS)


@pytest.mark.parametrize("f", FIELDS, ids=repr)
def test_call_sites_are_inside_the_class(f):
    """What the call sites hand to fe_canon_limbs (through fe_inv_dev, or directly in the batch inversion):
      batch_inverse_kernel (Fr), precompute_affine_kernel (Fp), jj_store_affine, the fixed- and variable-base gadget kernels
        (Fr): a running product -- fe_mul / fe_sqr of operands up to the widest the product routines take, or fe_one;
      gadget_curve_add_kernel: dd = gmul(den1, den2), a product of two weak reductions;
      gadget_maybe_equal_kernel: g_to_dev(u) = fe_reduce_weak(fr_shl5(u)), u a weak reduction of a difference.
    All are normalised (limbs < 2^W) with value < 2 m; fe_canon_limbs takes them without a wrap."""
    top = M.canon_limb_max(f)

    def handed_over(x):
        assert M.in_class(f, x, 1, 2) and max(x) <= top
        assert M.fe_canon_limbs(f, x) == M.limbs_of(f, val(f, x) % f.mod)

    wide = M.class_members(f, 5 if f is M.FR else 12, 13, True, 20, seed=3)
    prods = M.class_members(f, 1, 2, False, 20, seed=4)
    for a in wide + prods:
        for b in prods[:4] + prods[-4:]:
            handed_over(M.fe_mul(f, a, b))
    for a in prods + M.class_members(f, 2, 8, 2, 10, seed=5):
        handed_over(M.fe_sqr(f, a))
    handed_over(M.fe_one(f))
    if f is M.FR:
        canon = M.class_members(f, 1, 1, False, 20, seed=6)
        for a in canon:
            for b in canon[:4] + canon[-4:]:
                u = M.fe_reduce_weak(f, M.fe_sub(f, 2, 1, a, b))                     # gsub of two loaded variables
                handed_over(M.fe_reduce_weak(f, M.fr_shl5(u)))                       # g_to_dev(u)
                den1 = M.fe_reduce_weak(f, M.fe_add(f, M.fe_one(f), M.fe_mul(f, a, b)))   # gadd(one, k), k a product
                den2 = M.fe_reduce_weak(f, M.fe_sub(f, 2, 1, M.fe_one(f), M.fe_mul(f, a, b)))
                handed_over(M.fe_mul(f, den1, den2))                                 # dd
    assert not M.VIOLATIONS, M.VIOLATIONS[:5]
