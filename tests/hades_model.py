"""Big-integer model of the HADES gadget kind (include/plonk_mi355x.h, PM_PLONK_PERMUTATION_HADES): one Hades permutation of
width 5 laid out in arithmetic rows, and on top of it a sponge.  Extends the builder of tests/composed_gadget_model.py; the
reference of tests/test_hades_host.py and tests/test_gpu_hades.py.  Plain Python integers throughout."""
import os
import random
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import composed_gadget_model as CM  # noqa: E402

R, NO_VAR = CM.R, CM.NO_VAR
WIDTH = 5


# ------------------------------------------------------------------------------------------ the definition
def is_full(rho: int, rounds: int, full_rounds: int) -> bool:
    return rho < full_rounds // 2 or rho >= rounds - full_rounds // 2


def hades_rows(rounds: int, full_rounds: int) -> int:
    return 30 * full_rounds + 18 * (rounds - full_rounds)


def hades_trace(state, ark, mds, rounds: int, full_rounds: int):
    """Round by round, straight from the definition: add the round keys ark[rho][j], raise every word (full round) or the last
    word (partial round) to the fifth power, multiply by the matrix mds[i][j] -- or, when mds is a list of ``rounds`` matrices,
    by the round's own mds[rho][i][j].  -> (the final state, the c of every row in row order: per round the 5 keyed words, x^2
    x^4 x^5 of each word that goes through the s-box, then z_i, o_i for i = 0..4)"""
    assert len(state) == WIDTH and full_rounds % 2 == 0 and 0 <= full_rounds <= rounds and rounds >= 1
    per_round = isinstance(mds[0][0], (list, tuple))
    assert len(mds) == (rounds if per_round else WIDTH)
    s, out = [x % R for x in state], []
    for rho in range(rounds):
        s = [(s[j] + ark[rho][j]) % R for j in range(WIDTH)]
        out.extend(s)
        for j in (range(WIDTH) if is_full(rho, rounds, full_rounds) else (WIDTH - 1,)):
            x2 = s[j] * s[j] % R
            x4 = x2 * x2 % R
            s[j] = x4 * s[j] % R
            out.extend((x2, x4, s[j]))
        m, nxt = mds[rho] if per_round else mds, []
        for i in range(WIDTH):
            z = (m[i][0] * s[0] + m[i][1] * s[1] + m[i][2] * s[2]) % R
            nxt.append((m[i][3] * s[3] + m[i][4] * s[4] + z) % R)
            out.extend((z, nxt[-1]))
        s = nxt
    assert len(out) == hades_rows(rounds, full_rounds)
    return s, out


def hades_model(state, ark, mds, R, F):   # noqa: N803  (R, F: the rounds and the full rounds, as the header names them)
    """-> the state after the permutation"""
    return hades_trace(state, ark, mds, R, F)[0]


# ------------------------------------------------------------------------------------------ the builder
class Builder(CM.Builder):
    """composed_gadget_model.Builder with the rows of a Hades permutation.  Round keys and matrices are random, drawn from
    ``coeff_seed`` in the order of the calls: two builders with one seed and the same calls lay out the same rows."""

    def __init__(self, n: int, coeff_seed: int = 0x48414445):
        super().__init__(n)
        self.coeff_rng = random.Random(coeff_seed)
        self.permutations = []     # (first_row, rounds, full_rounds, ark, mds) of every hades() call

    def hades(self, state_vars, R, F, level=0, as_arith=False):   # noqa: N803
        """The rows of one permutation of R rounds, F of them full, on the five variables ``state_vars`` (None: no variable,
        read as zero; they may alias).  A fresh matrix for every round, so that a kernel that mixes up the rounds cannot pass.
        as_arith: the same rows claimed as ONE ARITH run; level None: the rows are laid and nothing claims them.
        -> the five variables of the final state"""
        rounds, full_rounds = R, F
        assert len(state_vars) == WIDTH
        rnd = lambda: self.coeff_rng.randrange(CM.R)   # noqa: E731
        ark = [[rnd() for _ in range(WIDTH)] for _ in range(rounds)]
        mds = [[[rnd() for _ in range(WIDTH)] for _ in range(WIDTH)] for _ in range(rounds)]
        r0, s, written = self.row, list(state_vars), []
        for rho in range(rounds):
            keyed = [self.var() for _ in range(WIDTH)]
            for j in range(WIDTH):
                self.gate(s[j], None, keyed[j], q_l=1, q_c=ark[rho][j], q_o=CM.R - 1)
            written.extend(keyed)
            v = list(keyed)
            for j in (range(WIDTH) if is_full(rho, rounds, full_rounds) else (WIDTH - 1,)):
                x2, x4, x5 = self.var(), self.var(), self.var()
                self.gate(keyed[j], keyed[j], x2, q_m=1, q_o=CM.R - 1)
                self.gate(x2, x2, x4, q_m=1, q_o=CM.R - 1)
                self.gate(x4, keyed[j], x5, q_m=1, q_o=CM.R - 1)
                written.extend((x2, x4, x5))
                v[j] = x5
            s = []
            for i in range(WIDTH):
                z, o = self.var(), self.var()
                m = mds[rho][i]
                self.gate(v[0], v[1], z, v[2], q_l=m[0], q_r=m[1], q_4=m[2], q_o=CM.R - 1)
                self.gate(v[3], v[4], o, z, q_l=m[3], q_r=m[4], q_4=1, q_o=CM.R - 1)
                written.extend((z, o))
                s.append(o)
        count = self.row - r0
        assert count == hades_rows(rounds, full_rounds) and len(written) == count
        self.permutations.append((r0, rounds, full_rounds, ark, mds))
        if level is None:
            return s
        if as_arith:
            self._claim_arith(r0, count, level)
            return s
        idx = len(self.gadgets)
        self.gadgets.append(("hades", level, r0, rounds, full_rounds, ()))

        def step(val):
            state = [self._value(val, 0, r0 + j) for j in range(WIDTH)]
            _, trace = hades_trace(state, ark, mds, rounds, full_rounds)
            for var, x in zip(written, trace):
                val[var] = x
            return None
        self.steps.append((level, idx, step))
        return s

    def sponge(self, inputs, R, F, level=0):   # noqa: N803
        """A sponge of rate 4 over the input variables: the state starts as the zero variable five times; every chunk of up to
        four inputs is added to words 1..4 by one ARITH gadget (a short last chunk is padded: the word after its last input gets
        + 1, a q_c) at level ``level`` + 2 k, the permutation follows at ``level`` + 2 k + 1.  -> the hash variable (word 1)"""
        state = [0] * WIDTH
        for k in range(0, len(inputs), 4):
            chunk = inputs[k:k + 4]
            rows = [(state[1 + t], x, None, None, dict(q_l=1, q_r=1)) for t, x in enumerate(chunk)]
            if len(chunk) < 4:
                rows.append((state[1 + len(chunk)], None, None, None, dict(q_l=1, q_c=1)))
            outs = self.arith(rows, level=level + k // 2)
            state = [state[0]] + outs + state[1 + len(outs):]
            state = self.hades(state, R, F, level=level + k // 2 + 1)
        return state[1]

    def public_output(self, var):
        """one row a + PI = 0: the variable is public.  -> the row (the public input there is minus the value)"""
        return self.gate(var, None, None, q_l=1)

    def gadget_records(self):
        import plonk_prototype_amd as pa
        keep, out = self.gadgets, []
        try:
            for g in sorted(keep, key=lambda t: t[1]):
                if g[0] == "hades":
                    out.append(pa.Gadget.hades(g[2], g[3], g[4], level=g[1]))
                else:
                    self.gadgets = [g]
                    out.extend(super().gadget_records())
        finally:
            self.gadgets = keep
        return out


to_limbs = CM.to_limbs
