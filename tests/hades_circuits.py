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
