"""The circuits of tests/test_gpu_hades.py, built once and shared with tests/test_hades_host.py (which checks that the model's
own output satisfies them).  Each function returns the builder, the assignments of its inputs, their models and what else its
test needs; nothing here touches the library."""
import functools
import random

import hades_model as HM

R = HM.R
SHAPES = ((1, 0), (2, 2), (5, 2), (4, 0))      # partial only; full only; both transitions; partials in a chain
DUSK = (67, 8)


@functools.lru_cache(maxsize=None)
def shapes_case():
    """One permutation of every shape, all in ONE level, the first not at row 0 (a glue row comes before it).  Their states:
    five distinct inputs; two aliased words; the zero variable five times; a word that is no variable.  64 assignments: the
    edge values 0, 1, r - 1 in every input position, then random ones."""
    b = HM.Builder(512)
    g = b.var(True)
    b.add(g, g, level=0)
    xs = [b.var(True) for _ in range(5)]
    ys = [b.var(True) for _ in range(4)]
    ws = [b.var(True) for _ in range(4)]
    states = (xs, [ys[0], ys[1], ys[0], ys[2], ys[3]], [0] * 5, [None] + ws)
    for (rounds, full), state in zip(SHAPES, states):
        b.hades(state, rounds, full, level=0)
    arith = b.fill_arithmetic(31)
    rng = random.Random(31)
    free = [g] + xs + ys + ws
    assignments = []
    for e in (0, 1, R - 1):
        assignments.append({**{v: e for v in free}, **arith})
        for k in range(len(free)):                 # one edge value among random ones, in every position in turn
            a = {v: rng.randrange(R) for v in free}
            a[free[k]] = e
            assignments.append({**a, **arith})
    assignments = assignments[:40]
    while len(assignments) < 64:
        assignments.append({**{v: rng.randrange(R) for v in free}, **arith})
    return b, assignments, [b.model(a) for a in assignments]


@functools.lru_cache(maxsize=None)
def cross_case(rounds, full):
    """One permutation twice, after a glue row: claimed as HADES, and the same rows as ONE ARITH run.  2 assignments; (67, 8)
    takes n = 2^11.  -> [(builder, assignments, models)] x 2 with identical rows, variables and inputs"""
    out = []
    for as_arith in (False, True):
        b = HM.Builder(2048 if HM.hades_rows(rounds, full) > 500 else 256)
        g = b.var(True)
        b.add(g, g, level=0)
        xs = [b.var(True) for _ in range(5)]
        b.hades(xs, rounds, full, level=0, as_arith=as_arith)
        arith = b.fill_arithmetic(32)
        rng = random.Random(32)
        assignments = [{g: 7, **{v: rng.randrange(R) for v in xs}, **arith}, {g: R - 1, **{v: (0, 1, R - 1, 2, 3)[k] for k, v in enumerate(xs)}, **arith}]
        out.append((b, assignments, [b.model(a) for a in assignments]))
    assert out[0][0].wires == out[1][0].wires and out[0][0].sel == out[1][0].sel
    return out


def dusk_case():
    return cross_case(*DUSK)[0]


@functools.lru_cache(maxsize=None)
def sponge_case():
    """a sponge over six inputs at (5, 2): absorptions at levels 0 and 2, permutations at levels 1 and 3, and the hash made
    public by a row a + PI = 0; n = 256.  -> (builder, inputs(seed), hash variable, its public-input row)"""
    b = HM.Builder(256)
    ins = [b.var(True) for _ in range(6)]
    out = b.sponge(ins, 5, 2, level=0)
    pi_row = b.public_output(out)
    arith = b.fill_arithmetic(33)

    def inputs(seed):
        rng = random.Random(seed)
        return {**{v: rng.randrange(R) for v in ins}, **arith}
    return b, inputs, out, pi_row


@functools.lru_cache(maxsize=None)
def refusal_case():
    """a good table (a glue row and a (2, 2) permutation) and, beside it, one-round permutations that are wrong in ONE place;
    the good table never claims them.  -> (builder, input assignment, {name: first row})"""
    b = HM.Builder(256)
    g = b.var(True)
    t = b.add(g, g, q_l=3, q_r=5, q_c=7, level=0)
    xs = [b.var(True) for _ in range(4)]
    b.hades([t] + xs, 2, 2, level=1)
    decoys = {}

    def decoy(name, spoil):
        r0 = b.row
        b.hades(xs + [g], 1, 0, level=None)        # rows 0..4 keys, 5..7 the s-box of word 4, 8..17 the matrix
        spoil(r0)
        decoys[name] = r0

    decoy("good", lambda r0: None)
    decoy("matrix_wire", lambda r0: b.wires[0].__setitem__(r0 + 10, b.wires[2][r0 + 1]))   # z_1 reads s'[1] for v0 = s'[0]
    decoy("key_q_l", lambda r0: b.sel["q_l"].__setitem__(r0 + 3, 2))
    decoy("matrix_q_4", lambda r0: b.sel["q_4"].__setitem__(r0 + 13, 2))
    decoy("sbox_q_m", lambda r0: b.sel["q_m"].__setitem__(r0 + 6, R - 1))
    decoy("q_o", lambda r0: b.sel["q_o"].__setitem__(r0 + 17, 1))
    decoy("widget", lambda r0: b.sel["q_range"].__setitem__(r0 + 9, 1))
    decoy("no_var", lambda r0: b.wires[2].__setitem__(r0 + 17, HM.NO_VAR))
    arith = b.fill_arithmetic(34)
    rng = random.Random(34)
    return b, {g: rng.randrange(R), **{v: rng.randrange(R) for v in xs}, **arith}, decoys


# ---------------------------------------------------------------------------------------------- every set-time rule, one decoy each
# What pm_plonk_key_set_gadgets checks on the rows a HADES gadget claims, per row-position class.  On EVERY row: q_arith is not
# zero, the four widget selectors are zero, q_o = -1 and c is a variable.  Then
#   key row j (5 a round):         q_m = q_r = q_4 = 0, q_l = 1, q_c free; after the first round a = o_j of the round before
#   s-box rows (3 a word):         q_m = 1, q_l = q_r = q_c = q_4 = 0; x2: a = b = x; x4: a = b = x2; x5: a = x4, b = x -- x the
#                                  keyed word (every word in a full round, word 4 in a partial one)
#   matrix row z_i:                q_m = q_c = 0, q_l q_r q_4 free; a, b, d = v0, v1, v2
#   matrix row o_i:                q_m = q_c = 0, q_4 = 1, q_l q_r free; a, b = v3, v4, d = z_i
#                                  v_j = x5 of word j in a full round; in a partial one the keyed word j < 4 and x5 of word 4
# b and d of the key and s-box rows (d only) are not looked at.  DECOY_SHAPE has every class: a full first round (no link
# back), a partial round after a full one, a partial round after a partial one, and a full round after a partial one.
DECOY_SHAPE = (4, 2)
_ROUND = (0, 30, 48, 66)                           # first row of each round of DECOY_SHAPE
_WIDGETS = ("q_range", "q_logic", "q_fixed_group_add", "q_variable_group_add")


def _rule_spoils():
    """[(name, spoil(builder, first row, a variable no row of the decoy names))], each wrong in ONE checked place"""
    out = []

    def sel(name, key, row, value):
        out.append((name, lambda b, r0, other: b.sel[key].__setitem__(r0 + row, value)))

    def wire(name, w, row):
        out.append((name, lambda b, r0, other: b.wires[w].__setitem__(r0 + row, other)))

    def no_var(name, row):
        """c of the row is no variable, and neither is any position that names it: only the NO_VAR test is left to object"""
        def spoil(b, r0, other):
            v = b.wires[2][r0 + row]
            for w in range(4):
                for i in range(r0, r0 + HM.hades_rows(*DECOY_SHAPE)):
                    if b.wires[w][i] == v:
                        b.wires[w][i] = HM.NO_VAR
        out.append((name, spoil))

    f0, p1, p2, f3 = _ROUND
    # one row of each class, in each kind of round: key, s-box, z, o
    classes = (("key", f0 + 2, p1 + 4, "mrq"), ("sbox", f3 + 5 + 3 * 2 + 1, p2 + 6, "lrcq"), ("z", f0 + 20 + 4, p1 + 8 + 6, "mc"),
               ("o", f3 + 20 + 9, p2 + 8 + 1, "mc"))
    coeff = {"m": "q_m", "l": "q_l", "r": "q_r", "c": "q_c", "q": "q_4"}
    for k, (cls, full_row, part_row, zeros) in enumerate(classes):
        for n, z in enumerate(zeros):              # the coefficients that must be 0, alternating full and partial rounds
            sel(f"{cls}_{coeff[z]}", coeff[z], (full_row, part_row)[n & 1], 1)
        sel(f"{cls}_q_o_full", "q_o", full_row, 1)
        sel(f"{cls}_q_o_partial", "q_o", part_row, R - 2)
        sel(f"{cls}_no_arith", "q_arith", (full_row, part_row)[k & 1], 0)
        sel(f"{cls}_widget", _WIDGETS[k], (part_row, full_row)[k & 1], 1)
    sel("key_q_l_full", "q_l", f3 + 0, 2)
    sel("key_q_l_partial", "q_l", p2 + 3, R - 1)
    sel("sbox_q_m_full", "q_m", f0 + 5 + 3 * 4 + 2, 2)
    sel("sbox_q_m_partial", "q_m", p1 + 5, 0)
    sel("o_q_4_full", "q_4", f0 + 20 + 1, 0)
    sel("o_q_4_partial", "q_4", p2 + 8 + 9, 2)
    # the link to the round before: partial after full, partial after partial, full after partial
    wire("key_link_partial_after_full", 0, p1 + 1)
    wire("key_link_partial_after_partial", 0, p2 + 4)
    wire("key_link_full_after_partial", 0, f3 + 3)
    # the s-box: word 1 of a full round, word 4 of a partial one
    for k, name in enumerate(("x2", "x4", "x5")):
        wire(f"sbox_{name}_a_full", 0, f0 + 5 + 3 * 1 + k)
        wire(f"sbox_{name}_b_full", 1, f3 + 5 + 3 * 3 + k)
        wire(f"sbox_{name}_a_partial", 0, p1 + 5 + k)
        wire(f"sbox_{name}_b_partial", 1, p2 + 5 + k)
    # the matrix rows: a, b, d of z_i and o_i
    for w, name in ((0, "a"), (1, "b"), (3, "d")):
        wire(f"z_{name}_full", w, f0 + 20 + 2 * 3)
        wire(f"o_{name}_full", w, f3 + 20 + 2 * 2 + 1)
        wire(f"z_{name}_partial", w, p2 + 8 + 2 * 0)
        wire(f"o_{name}_partial", w, p1 + 8 + 2 * 4 + 1)
    # a written position that is no variable
    no_var("no_var_key_full", f0 + 1)
    no_var("no_var_key_partial", p2 + 4)
    no_var("no_var_x2", f3 + 5)
    no_var("no_var_x4", p1 + 6)
    no_var("no_var_x5", f0 + 5 + 3 * 4 + 2)
    no_var("no_var_z", p2 + 8 + 4)
    no_var("no_var_o_inner", f0 + 20 + 5)
    no_var("no_var_o_last", f3 + 29)
    return out


RULE_DECOYS_PER_CIRCUIT = 9
RULE_PARTS = -(-len(_rule_spoils()) // RULE_DECOYS_PER_CIRCUIT)


@functools.lru_cache(maxsize=None)
def rule_decoys_case(part):
    """Circuit ``part`` of RULE_PARTS, n = 1024: a good table (a glue row and two one-round permutations, so the second one's
    rounds are gathered at a non-zero offset) and, beside it, an untouched permutation of DECOY_SHAPE and up to nine that are
    wrong in ONE place of the list above; the good table never claims them.  -> (builder, input assignment, {name: first row})"""
    spoils = _rule_spoils()[part * RULE_DECOYS_PER_CIRCUIT:(part + 1) * RULE_DECOYS_PER_CIRCUIT]
    b = HM.Builder(1024)
    g = b.var(True)
    t = b.add(g, g, q_l=3, q_r=5, q_c=7, level=0)
    xs = [b.var(True) for _ in range(4)]
    other = b.var(True)
    b.hades([t] + xs, 1, 0, level=1)
    b.hades(xs + [t], 1, 0, level=1)
    decoys = {}
    for name, spoil in [("good", lambda b, r0, other: None)] + spoils:
        r0 = b.row
        b.hades(xs + [g], *DECOY_SHAPE, level=None)
        before = ([list(w) for w in b.wires], {k: list(v) for k, v in b.sel.items()})
        spoil(b, r0, other)
        assert name == "good" or before != ([list(w) for w in b.wires], {k: list(v) for k, v in b.sel.items()}), name
        assert name not in decoys
        decoys[name] = r0
    arith = b.fill_arithmetic(35 + part)
    rng = random.Random(35 + part)
    return b, {g: rng.randrange(R), other: rng.randrange(R), **{v: rng.randrange(R) for v in xs}, **arith}, decoys
