"""The circuits of tests/test_gpu_var_base.py, built once and shared with tests/test_var_base_host.py (which checks that the
model's own output satisfies them).  Each function returns the builder(s), the assignments of the inputs, their models and what
else its test needs; nothing here touches the library."""
import functools
import random

import gadget_model as M
import var_base_model as VM

R = VM.R
# one lane; a ragged last lane; every L = ceil(R / 64) from 1 to 4; dusk's 252 and the cap
SHAPES_A = (1, 2, 5, 63, 64, 65, 129, 252)
SHAPES_B = (256,)
SCALARS = ("zero", "ones", "top", "low", "random")
POINTS = ("curve", "identity", "minus_one", "off_curve")
STARTS = ("identity", "curve")


def _scalar(kind, rounds, rng):
    return {"zero": 0, "ones": (1 << rounds) - 1, "top": 1 << (rounds - 1), "low": 1}.get(kind, rng.randrange(1 << rounds))


def _point(kind, rng):
    if kind == "curve":
        return M.curve_point(rng.randrange(R))
    if kind == "identity":
        return M.IDENTITY
    if kind == "minus_one":
        return (0, R - 1)
    return (rng.randrange(R), rng.randrange(R))


@functools.lru_cache(maxsize=None)
def shapes_case(shapes=SHAPES_A, batch=64, seed=41):
    """One gadget of every R in ``shapes``, all in ONE level, the first not at row 0 (a glue row comes before it); the start
    point and P are shared input variables, every gadget has its own bit variables (inputs).  ``batch`` assignments: every
    combination of scalar, P and start kind once (40), then random scalars on random kinds.
    -> (builder, assignments, models, [(scalar per gadget, P, start)] per assignment)"""
    b = VM.Builder(4096 if sum(shapes) * 6 > 2000 else 2048)
    g = b.var(True)
    b.add(g, g, level=0)
    start = (b.var(True), b.var(True))
    point = (b.var(True), b.var(True))
    bits = [[b.var(True) for _ in range(rounds)] for rounds in shapes]
    for bv in bits:
        b.var_base(start, bv, point, level=0)
    arith = b.fill_arithmetic(41)
    rng = random.Random(seed)
    assignments, inputs = [], []
    for i in range(batch):
        if i < 40:
            kinds = (SCALARS[i % 5], POINTS[(i // 5) % 4], STARTS[i // 20])
        else:
            kinds = ("random", rng.choice(POINTS), rng.choice(STARTS))
        p, s = _point(kinds[1], rng), _point(kinds[2], rng)
        scalars = [_scalar(kinds[0], rounds, rng) for rounds in shapes]
        a = {g: rng.randrange(R), start[0]: s[0], start[1]: s[1], point[0]: p[0], point[1]: p[1], **arith}
        for bv, sc in zip(bits, scalars):
            a.update(zip(bv, VM.scalar_bits(sc, len(bv))))
        assignments.append(a)
        inputs.append((scalars, p, s))
    return b, assignments, [b.model(a) for a in assignments], inputs


@functools.lru_cache(maxsize=None)
def cross_case(rounds):
    """One multiplication twice, after a glue row: claimed as kind 10, and the same rows in the composed form on 2 R levels.
    3 assignments: a curve point from the identity, a curve point from a curve start, field elements off the curve for both.
    -> [(builder, assignments, models)] x 2 with identical rows, variables and inputs"""
    out = []
    for as_composed in (False, True):
        b = VM.Builder(2048 if rounds > 40 else 64)
        g = b.var(True)
        b.add(g, g, level=0)
        start = (b.var(True), b.var(True))
        point = (b.var(True), b.var(True))
        bits = [b.var(True) for _ in range(rounds)]
        b.var_base(start, bits, point, level=0, as_composed=as_composed)
        arith = b.fill_arithmetic(42)
        rng = random.Random(42)
        assignments = []
        for pk, sk in (("curve", "identity"), ("curve", "curve"), ("off_curve", "off_curve")):
            p, s = _point(pk, rng), _point(sk, rng)
            a = {g: 7, start[0]: s[0], start[1]: s[1], point[0]: p[0], point[1]: p[1], **arith}
            a.update(zip(bits, VM.scalar_bits(rng.randrange(1 << rounds), rounds)))
            assignments.append(a)
        out.append((b, assignments, [b.model(a) for a in assignments]))
    assert out[0][0].wires == out[1][0].wires and out[0][0].sel == out[1][0].sel
    return out


FIXED_ROUNDS = 252
FIXED_SEED = 0x1234567


@functools.lru_cache(maxsize=None)
def fixed_base_case():
    """the same scalar (below 2^251) and base through FIXED_BASE (252 rounds, from the identity) and through BITS at level 0
    and the variable-base gadget at level 1, P = the fixed-base table's base point.
    -> (builder, assignments, models, (fixed x, y vars), (variable x, y vars), scalars)"""
    b = VM.Builder(4096)
    s = b.var(True)
    one = b.var(True)                      # the identity (0, 1): the zero variable and this one
    point = (b.var(True), b.var(True))
    fixed = b.fixed_base(s, FIXED_ROUNDS, (0, one), level=0, table_seed=FIXED_SEED)
    bit, acc = b.bits(s, FIXED_ROUNDS, level=0)
    b.equal(acc[-1], s)
    variable = b.var_base((0, one), bit[::-1], point, level=1)
    arith = b.fill_arithmetic(43)
    rng = random.Random(43)
    base = M.base_table(1, FIXED_SEED)[0]
    scalars = [rng.randrange(1 << 251), (1 << 251) - 1]
    assignments = [{s: sc, one: 1, point[0]: base[0], point[1]: base[1], **arith} for sc in scalars]
    return b, assignments, [b.model(a) for a in assignments], fixed, variable, scalars


@functools.lru_cache(maxsize=None)
def dusk_case():
    """dusk's shape: the scalar's 252 bits by a BITS gadget at level 0 (with the row that compares their sum to the scalar),
    the multiplication from the identity at level 1, and the result made public by two rows a + PI = 0; n = 2048.
    -> (builder, inputs(seed), (x var, y var), (their public-input rows))"""
    b = VM.Builder(2048)
    s = b.var(True)
    one = b.var(True)
    point = (b.var(True), b.var(True))
    bit, acc = b.bits(s, 252, level=0)
    b.equal(acc[-1], s)
    out = b.var_base((0, one), bit[::-1], point, level=1)
    pi_rows = (b.public_output(out[0]), b.public_output(out[1]))
    arith = b.fill_arithmetic(44)

    def inputs(seed):
        rng = random.Random(seed)
        p = M.curve_point(rng.randrange(R))
        return {s: rng.randrange(1 << 252), one: 1, point[0]: p[0], point[1]: p[1], **arith}
    return b, inputs, out, pi_rows


@functools.lru_cache(maxsize=None)
def report_case():
    """R = 2 from input variables.  Assignment 0 is fine; 1 has the second bit variable set to 2; 2 is the degenerate case:
    an off-curve start S, (X, Y) = S + S, P = (x2, 1 / (d X x2 Y)), bit 1 -- 1 - d X x2 Y y2 = 0 in the first addition.
    -> (builder, assignments, models)"""
    b = VM.Builder(64)
    start = (b.var(True), b.var(True))
    point = (b.var(True), b.var(True))
    bits = [b.var(True), b.var(True)]
    b.var_base(start, bits, point, level=0)
    arith = b.fill_arithmetic(45)
    rng = random.Random(45)
    p = M.curve_point(rng.randrange(R))
    good = {start[0]: 0, start[1]: 1, point[0]: p[0], point[1]: p[1], bits[0]: 1, bits[1]: 0, **arith}
    wide = dict(good)
    wide[bits[1]] = 2
    S = (rng.randrange(R), rng.randrange(R))
    X, Y = M.jubjub_add(S, S)
    x2 = rng.randrange(1, R)
    y2 = pow(VM.EDWARDS_D * X % R * x2 % R * Y % R, -1, R)
    degenerate = {start[0]: S[0], start[1]: S[1], point[0]: x2, point[1]: y2, bits[0]: 1, bits[1]: 1, **arith}
    assignments = [good, wide, degenerate]
    return b, assignments, [b.model(a) for a in assignments]


DECOY_ROUNDS = 2


@functools.lru_cache(maxsize=None)
def refusal_case():
    """a good table (a glue row and a multiplication of 2 rounds) and, beside it, multiplications of 2 rounds that are wrong
    in ONE place; the good table never claims them.  -> (builder, input assignment, {name: first row})"""
    b = VM.Builder(512)
    g = b.var(True)
    b.add(g, g, q_l=3, q_r=5, q_c=7, level=0)
    start = (b.var(True), b.var(True))
    point = (b.var(True), b.var(True))
    bits = [b.var(True) for _ in range(DECOY_ROUNDS)]
    other = b.var(True)
    b.var_base(start, bits, point, level=1)
    decoys = {}
    W, S = b.wires, b.sel

    def decoy(name, spoil):
        r0 = b.row
        b.var_base(start, bits, point, level=None)    # round 0: rows 0..5, round 1: rows 6..11
        spoil(r0)
        decoys[name] = r0

    def wire(w, row, var=other):
        return lambda r0: W[w].__setitem__(r0 + row, var)

    def sel(name, row, value):
        return lambda r0: S[name].__setitem__(r0 + row, value)

    decoy("good", lambda r0: None)
    decoy("dbl_selector", sel("q_variable_group_add", 6, 0))
    decoy("add_selector", sel("q_variable_group_add", 4, 0))
    decoy("x_q_m", sel("q_m", 2, 2))
    decoy("x_q_l", sel("q_l", 8, 1))
    decoy("x_q_c", sel("q_c", 2, 1))
    decoy("x_q_o", sel("q_o", 2, 1))
    decoy("y_q_m", sel("q_m", 9, R - 1))
    decoy("y_q_l", sel("q_l", 3, 0))
    decoy("y_q_c", sel("q_c", 3, 0))
    decoy("y_q_o", sel("q_o", 9, 0))
    decoy("y_q_r", sel("q_r", 3, 1))
    decoy("x_q_4", sel("q_4", 8, 1))
    decoy("select_widget", sel("q_range", 3, 1))
    decoy("select_no_arith", sel("q_arith", 8, 0))
    decoy("dbl_c", wire(2, 0))                        # c = a on the doubling row
    decoy("dbl_d", wire(3, 6))                        # d = b
    decoy("add_a", wire(0, 4))                        # a, b of the addition = a, b of the doubling's second row
    decoy("add_b", wire(1, 10))
    decoy("add_c", wire(2, 4))                        # c, d of the addition = c of the select rows
    decoy("add_d", wire(3, 10))
    decoy("bit", wire(0, 3))                          # the two select rows read one bit
    def both(w1, w2, row, var):
        return lambda r0: (W[w1].__setitem__(r0 + row, var), W[w2].__setitem__(r0 + row, var))

    decoy("chain_a", both(0, 2, 6, other))            # a, b of the next round = a, b of the addition's second row
    decoy("chain_b", both(1, 3, 6, other))
    decoy("point_x_round", wire(1, 8))                # P is the same two ids in every round
    decoy("point_y_round", wire(1, 9))
    decoy("no_var_dbl_a", wire(0, 1, VM.NO_VAR))      # the written positions are variables
    decoy("no_var_dbl_d", wire(3, 7, VM.NO_VAR))
    decoy("no_var_add_b", wire(1, 5, VM.NO_VAR))
    decoy("no_var_add_d", wire(3, 11, VM.NO_VAR))
    decoy("no_var_sx", lambda r0: (W[2].__setitem__(r0 + 2, VM.NO_VAR), W[2].__setitem__(r0 + 4, VM.NO_VAR)))
    decoy("no_var_sy", lambda r0: (W[2].__setitem__(r0 + 9, VM.NO_VAR), W[3].__setitem__(r0 + 10, VM.NO_VAR)))
    arith = b.fill_arithmetic(46)
    rng = random.Random(46)
    p = M.curve_point(rng.randrange(R))
    a = {g: rng.randrange(R), start[0]: 0, start[1]: 1, point[0]: p[0], point[1]: p[1], bits[0]: 1, bits[1]: 1, other: 5, **arith}
    return b, a, decoys
