"""Big-integer model of the three composed gadget kinds (include/plonk_mi355x.h, pm_plonk_gadget: ARITH, BITS, MAYBE_EQUAL)
and, on top of them, of the gadgets a circuit composes from arithmetic rows: a bit decomposition with its comparison, the two
bound checks and the range check between two public bounds.  Extends the builder of tests/gadget_model.py; the reference of
tests/test_composed_gadgets_host.py and tests/test_gpu_composed_gadgets.py.  Plain Python integers throughout."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gadget_model as M  # noqa: E402

R, NO_VAR = M.R, M.NO_VAR
COEFFS = ("q_m", "q_l", "q_r", "q_o", "q_c", "q_4")


# ------------------------------------------------------------------------------------------ the definitions
def arith_model(coeffs, a, b, d):
    """c of one ARITH row: q_m a b + q_l a + q_r b + q_4 d + q_c (q_o = -1, no public input)"""
    return (coeffs["q_m"] * a * b + coeffs["q_l"] * a + coeffs["q_r"] * b + coeffs["q_4"] * d + coeffs["q_c"]) % R


def bits_model(v: int, num_bits: int, acc0: int):
    """-> (bit_0 .. bit_(B-1), acc_0 .. acc_(B-1)): acc_k = acc0 + (V mod 2^(k+1)), V the integer below r"""
    v %= R
    return [(v >> k) & 1 for k in range(num_bits)], [(acc0 + (v & ((1 << (k + 1)) - 1))) % R for k in range(num_bits)]


def maybe_equal_model(a: int, b: int):
    """-> (u, z, y): u = a - b, z = 1 / u or 0, y = 1 - u z"""
    u = (a - b) % R
    z = pow(u, -1, R) if u else 0
    return u, z, (1 - u * z) % R


def bound_bits(max_range: int) -> int:
    """bits of the power of two that covers [0, max_range - 1]"""
    return max(1, (max_range - 1).bit_length())


# ------------------------------------------------------------------------------------------ the builder
class Builder(M.Builder):
    """gadget_model.Builder with arithmetic rows as gadgets.  ``add`` and ``mul`` lay one row and claim it as an ARITH run of
    one; ``arith`` lays a run of several; ``bits`` and ``maybe_equal`` lay the rows of their kinds.  ``bits_as_arith``: every
    decomposition built from here on is laid out in its ARITH form (see ``bits``); ``bit_vars`` collects the bit variables."""

    def __init__(self, n: int):
        super().__init__(n)
        self.bits_as_arith = False
        self.bit_vars = []

    def gate(self, a, b, c, d=None, **q):
        """one arithmetic row (q_arith = 1) with the given wire variables and coefficients -> its row"""
        r0 = self._rows(1)
        self.sel["q_arith"][r0] = 1
        for k, x in q.items():
            assert k in COEFFS, k
            self.sel[k][r0] = x % R
        self._put(r0, (a, b, c, d))
        return r0

    def _value(self, val, wire, row):
        v = self.wires[wire][row]
        return 0 if v == NO_VAR else val[v]

    def _claim_arith(self, r0, count, level):
        """rows [r0, r0 + count) as ONE ARITH gadget: solved for c in row order from the rows' own coefficients"""
        idx = len(self.gadgets)
        self.gadgets.append(("arith", level, r0, count, 0, ()))

        def step(val):
            for i in range(r0, r0 + count):
                assert self.sel["q_o"][i] == R - 1 and self.wires[2][i] != NO_VAR
                q = {k: self.sel[k][i] for k in COEFFS}
                val[self.wires[2][i]] = arith_model(q, self._value(val, 0, i), self._value(val, 1, i), self._value(val, 3, i))
            return None
        self.steps.append((level, idx, step))
        return idx

    def arith(self, rows, level=0):
        """rows: [(a, b, c, d, {coefficient: value})] laid out consecutively and claimed as one run (q_o = -1 is set here);
        c = None makes a new variable.  -> the c variables"""
        outs, r0 = [], self.row
        for a, b, c, d, q in rows:
            c = self.var() if c is None else c
            self.gate(a, b, c, d, q_o=R - 1, **q)
            outs.append(c)
        self._claim_arith(r0, len(rows), level)
        return outs

    def add(self, a, b, q_l=1, q_r=1, q_c=0, d=None, q_4=0, level=0):
        """c = q_l a + q_r b + q_4 d + q_c -> c"""
        return self.arith([(a, b, None, d, dict(q_l=q_l, q_r=q_r, q_c=q_c, q_4=q_4))], level)[0]

    def mul(self, a, b, q_m=1, q_c=0, d=None, q_4=0, level=0):
        """c = q_m a b + q_4 d + q_c -> c"""
        return self.arith([(a, b, None, d, dict(q_m=q_m, q_c=q_c, q_4=q_4))], level)[0]

    def bits(self, value_var, num_bits, level=0, acc0=0, as_arith=False):
        """The loop of a bit decomposition, 2 num_bits rows; acc0: the variable the sum starts from.  as_arith: the same rows
        claimed as one ARITH run whose bit variables are INPUTS (the sequential form of the same computation).
        -> (bit variables, accumulator variables)"""
        r0, as_arith = self.row, as_arith or self.bits_as_arith
        bit = [self.var(as_arith) for _ in range(num_bits)]
        self.bit_vars.extend(bit)
        acc = [self.var() for _ in range(num_bits)]
        for k in range(num_bits):
            self.gate(bit[k], bit[k], bit[k], q_m=1, q_o=R - 1)
            self.gate(bit[k], acc[k - 1] if k else acc0, acc[k], q_l=1 << k, q_r=1, q_o=R - 1)
        if as_arith:
            self._claim_arith(r0, 2 * num_bits, level)
            return bit, acc
        idx = len(self.gadgets)
        self.gadgets.append(("bits", level, r0, num_bits, 0, (value_var,)))

        def step(val):
            bs, accs = bits_model(val[value_var], num_bits, val[acc0])
            for v, x in zip(bit + acc, bs + accs):
                val[v] = x
            return None
        self.steps.append((level, idx, step))
        return bit, acc

    def maybe_equal(self, a, b, level=0):
        """-> (y, u, z): y = 1 when a = b, else 0"""
        u, z, y = self.var(), self.var(), self.var()
        r0 = self.gate(a, b, u, q_l=1, q_r=R - 1, q_o=R - 1)
        self.gate(z, u, y, q_m=R - 1, q_c=1, q_o=R - 1)
        self.gate(y, u, u, q_m=1)
        idx = len(self.gadgets)
        self.gadgets.append(("maybe_equal", level, r0, 0, 0, ()))

        def step(val):
            val[u], val[z], val[y] = maybe_equal_model(self._value(val, 0, r0), self._value(val, 1, r0))
            return None
        self.steps.append((level, idx, step))
        return y, u, z

    def decomposition(self, value_var, num_bits, level=0):
        """bits at ``level``, the comparison of their sum with the value at ``level + 1`` -> (y, bit variables)"""
        bit, acc = self.bits(value_var, num_bits, level)
        return self.maybe_equal(acc[-1], value_var, level + 1)[0], bit

    def max_bound(self, max_range, x, level=0):
        """y = 1 when x < max_range: (max_range - 1) - x fits the bits of max_range - 1.  -> (y, bits)"""
        nb = bound_bits(max_range)
        t = self.add(x, x, q_l=R - 1, q_r=0, q_c=max_range - 1, level=level)
        return self.decomposition(t, nb, level + 1)[0], nb

    def min_bound(self, min_range, x, num_bits, level=0):
        """y = 1 when x >= min_range: x - min_range fits num_bits bits"""
        t = self.add(x, x, q_l=1, q_r=0, q_c=-min_range, level=level)
        return self.decomposition(t, num_bits, level + 1)[0]

    def range_check(self, min_range, max_range, x, level=0):
        """-> the variable that is 1 when min_range <= x < max_range and 0 otherwise; levels level .. level + 3"""
        y1, nb = self.max_bound(max_range, x, level)
        y2 = self.min_bound(min_range, x, nb, level)
        return self.mul(y1, y2, level=level + 3)

    # ---- what the tests take
    def gadget_records(self):
        """the records in rising levels (stable: the order of the calls inside a level)"""
        import plonk_prototype_amd as pa
        G = pa.Gadget
        out = []
        for kind, level, r0, count, param, iv in sorted(self.gadgets, key=lambda t: t[1]):
            if kind == "arith":
                out.append(G.arith(r0, count, level=level))
            elif kind == "bits":
                out.append(G.bits(r0, count, iv[0], level=level))
            elif kind == "maybe_equal":
                out.append(G.maybe_equal(r0, level=level))
            elif kind == "range":
                out.append(G.range(r0, count, iv[0], level=level))
            elif kind == "logic":
                out.append(G.logic(r0, count, iv[0], iv[1], xor=bool(param), level=level))
            elif kind == "fixed_base":
                out.append(G.fixed_base(r0, count, iv[0], level=level))
            else:
                out.append(G.curve_add(r0, level=level))
        return out

    def arithmetic_failures(self, val):
        """rows on which q_arith (q_m a b + q_l a + q_r b + q_o c + q_4 d + q_c) != 0 under an assignment"""
        bad = []
        for i in range(self.n):
            a, b, c, d = (self._value(val, j, i) for j in range(4))
            s = {k: self.sel[k][i] for k in COEFFS}
            if self.sel["q_arith"][i] * (s["q_m"] * a * b + s["q_l"] * a + s["q_r"] * b + s["q_o"] * c + s["q_4"] * d + s["q_c"]) % R:
                bad.append(i)
        return bad


to_limbs = M.to_limbs
