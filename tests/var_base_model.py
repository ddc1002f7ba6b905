"""Big-integer model of the variable-base scalar multiplication gadget (include/plonk_mi355x.h, PM_PLONK_GADGET_VAR_BASE):
R rounds of six rows -- a doubling, the two rows that select bit P, an addition -- under the affine twisted Edwards law.
Extends the builder of tests/composed_gadget_model.py; the reference of tests/test_var_base_host.py and
tests/test_gpu_var_base.py.  Plain Python integers throughout."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import composed_gadget_model as CM  # noqa: E402
import gadget_model as M  # noqa: E402

R, NO_VAR, EDWARDS_D = CM.R, CM.NO_VAR, M.EDWARDS_D
IDENTITY = M.IDENTITY
TOO_WIDE, DEGENERATE = M.TOO_WIDE, M.DEGENERATE
ROWS_PER_ROUND = 6
MAX_ROUNDS = 256


# ------------------------------------------------------------------------------------------ the definition
def _denominators_vanish(p, q):
    (x1, y1), (x2, y2) = p, q
    k = EDWARDS_D * x1 % R * x2 % R * y1 % R * y2 % R
    return (1 + k) % R == 0 or (1 - k) % R == 0


def var_base_trace(bits, start, point):
    """bits[k]: the value of the bit variable of round k (any field element), most significant first.  Round by round as the
    header defines it.  -> (rounds, reason): per round a dict of acc, dbl, d_dbl = acc.x acc.y, sx, sy, new, d_add = dbl.x sy.
    The select values are exact for every bit; after a bit that is neither 0 nor 1 (TOO_WIDE) or a vanishing denominator
    (DEGENERATE) the points are unspecified and given as None."""
    px, py = point
    acc, reason, out = start, None, []
    for bit in bits:
        bit %= R
        sx, sy = bit * px % R, (bit * py - bit + 1) % R
        rnd = dict(sx=sx, sy=sy, acc=None, dbl=None, new=None, d_dbl=None, d_add=None)
        if reason is None and bit > 1:
            reason = TOO_WIDE
        if reason is None and _denominators_vanish(acc, acc):
            reason = DEGENERATE
        if reason is None:
            dbl = M.jubjub_add(acc, acc)
            if _denominators_vanish(dbl, (sx, sy)):
                reason = DEGENERATE
            else:
                new = M.jubjub_add(dbl, (sx, sy))
                rnd.update(acc=acc, dbl=dbl, new=new, d_dbl=acc[0] * acc[1] % R, d_add=dbl[0] * sy % R)
                acc = new
        out.append(rnd)
    if reason is None:
        return out, None
    # a wide bit anywhere comes first in the report
    return out, (TOO_WIDE if any(b % R > 1 for b in bits) else reason)


def var_base_model(scalar: int, rounds: int, start, point):
    """the end point of the gadget on the bits of ``scalar`` (below 2^rounds), most significant first"""
    assert 0 <= scalar < 1 << rounds
    trace, reason = var_base_trace(scalar_bits(scalar, rounds), start, point)
    assert reason is None
    return trace[-1]["new"]


def scalar_bits(scalar: int, rounds: int):
    """bit_k of round k: most significant first"""
    return [(scalar >> (rounds - 1 - k)) & 1 for k in range(rounds)]


def double_and_add(scalar: int, point, start=IDENTITY, rounds=None):
    """an independent statement: 2^rounds start + scalar point, the multiples by binary expansion of the INTEGERS, least
    significant bit first, with a running power of two -- no shared loop with var_base_trace"""
    def mul(k, p):
        acc, pw = IDENTITY, p
        while k:
            if k & 1:
                acc = M.jubjub_add(acc, pw)
            pw = M.jubjub_add(pw, pw)
            k >>= 1
        return acc
    out = mul(scalar, point)
    if rounds is not None and start != IDENTITY:
        out = M.jubjub_add(mul(1 << rounds, start), out)
    return out


# ------------------------------------------------------------------------------------------ the builder
class Builder(CM.Builder):
    """composed_gadget_model.Builder with the rows of a variable-base scalar multiplication.  ``var_base`` lays the rows
    once; ``as_composed`` claims them as the composed form (CURVE_ADD, ARITH of 2, CURVE_ADD per round, on 2 R levels) instead
    of one gadget of kind 10: two builders with the same calls lay out the same rows and variables."""

    def __init__(self, n: int):
        super().__init__(n)
        self.chains = []           # (first_row, rounds, result x var, result y var) of every var_base() call

    def var_base(self, start_vars, bit_vars, point_vars, level=0, as_composed=False):
        """bit_vars[k]: the bit variable of round k, most significant first; level None: the rows are laid and nothing
        claims them.  -> (x var, y var) of the result"""
        rounds = len(bit_vars)
        r0 = self._rows(ROWS_PER_ROUND * rounds)
        vga = self.sel["q_variable_group_add"]
        acc = tuple(start_vars)
        written = []               # per round: dbl.x dbl.y d_dbl sx sy new.x new.y d_add
        for k, bit in enumerate(bit_vars):
            r = r0 + ROWS_PER_ROUND * k
            dx, dy, dd, sx, sy, nx, ny, da = (self.var() for _ in range(8))
            vga[r] = vga[r + 4] = 1
            self._put(r, (acc[0], acc[1], acc[0], acc[1]))
            self._put(r + 1, (dx, dy, 0, dd))
            for row, p, c, q in ((r + 2, point_vars[0], sx, dict(q_m=1)), (r + 3, point_vars[1], sy, dict(q_m=1, q_l=R - 1, q_c=1))):
                self.sel["q_arith"][row] = 1
                for name, x in dict(q, q_o=R - 1).items():
                    self.sel[name][row] = x
                self._put(row, (bit, p, c, None))
            self._put(r + 4, (dx, dy, sx, sy))
            self._put(r + 5, (nx, ny, 0, da))
            written.append((dx, dy, dd, sx, sy, nx, ny, da))
            acc = (nx, ny)
        self.chains.append((r0, rounds, acc[0], acc[1]))
        if level is None:
            return acc
        if as_composed:
            for k in range(rounds):
                r = r0 + ROWS_PER_ROUND * k
                self._claim_curve_add(r, level + 2 * k)
                self._claim_arith(r + 2, 2, level + 2 * k)
                self._claim_curve_add(r + 4, level + 2 * k + 1)
            return acc
        idx = len(self.gadgets)
        self.gadgets.append(("var_base", level, r0, rounds, 0, ()))

        def step(val):
            start = (self._value(val, 0, r0), self._value(val, 1, r0))
            point = (self._value(val, 1, r0 + 2), self._value(val, 1, r0 + 3))
            trace, reason = var_base_trace([self._value(val, 0, r0 + ROWS_PER_ROUND * k + 2) for k in range(rounds)], start, point)
            for ids, t in zip(written, trace):
                val[ids[3]], val[ids[4]] = t["sx"], t["sy"]
                if t["new"] is not None:
                    (val[ids[0]], val[ids[1]]), val[ids[2]] = t["dbl"], t["d_dbl"]
                    (val[ids[5]], val[ids[6]]), val[ids[7]] = t["new"], t["d_add"]
            return reason
        self.steps.append((level, idx, step))
        return acc

    def _claim_curve_add(self, r0, level):
        """rows r0, r0 + 1 as a CURVE_ADD gadget, by the model of tests/gadget_model.py"""
        idx = len(self.gadgets)
        self.gadgets.append(("curve_add", level, r0, 0, 0, ()))
        x3, y3, xy = self.wires[0][r0 + 1], self.wires[1][r0 + 1], self.wires[3][r0 + 1]

        def step(val):
            p = (self._value(val, 0, r0), self._value(val, 1, r0))
            q = (self._value(val, 2, r0), self._value(val, 3, r0))
            val[x3], val[y3], val[xy], reason = M.curve_add_model(p, q)
            return reason
        self.steps.append((level, idx, step))

    def select_vars(self, chain=0):
        """the sx, sy variables of a chain, in row order"""
        r0, rounds, _, _ = self.chains[chain]
        return [self.wires[2][r0 + ROWS_PER_ROUND * k + j] for k in range(rounds) for j in (2, 3)]

    def public_output(self, var):
        """one row a + PI = 0: the variable is public.  -> the row (the public input there is minus the value)"""
        return self.gate(var, None, None, q_l=1)

    def var_rows_failures(self, val):
        """rows with q_variable_group_add whose three summands (tests/gadget_model.py, var_summands) are not all zero"""
        rows = self.rows(val)
        return [i for i in range(self.n - 1) if self.sel["q_variable_group_add"][i] and any(M.var_summands(rows[i], rows[i + 1]))]

    def gadget_records(self):
        import plonk_prototype_amd as pa
        keep, out = self.gadgets, []
        try:
            for g in sorted(keep, key=lambda t: t[1]):
                if g[0] == "var_base":
                    out.append(pa.Gadget.variable_base(g[2], g[3], level=g[1]))
                else:
                    self.gadgets = [g]
                    out.extend(super().gadget_records())
        finally:
            self.gadgets = keep
        return out


to_limbs = CM.to_limbs
