"""Host-side ground for the gadget witnesses (pm_plonk_key_set_gadgets / pm_plonk_fill_gadgets_dev):
the new exports are in the library, bound with the declared signatures and declared in the header; the constants and both
structs are the header's; the digit routine of the fixed-base kernel, compiled for the host (pm_test_host_naf), gives the
non-adjacent form of the model's digit loop; and the model's own output satisfies a big-integer restatement of the four widget
identities, summand by summand.  No device compute here."""
import ctypes as C
import inspect
import os
import re
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gadget_model as M  # noqa: E402

GADGET_EXPORTS = ("pm_plonk_key_set_gadgets", "pm_plonk_fill_gadgets_dev", "pm_test_host_naf")
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "plonk_mi355x.h")
R = M.R


def test_gadget_symbols_exported_and_bound():
    import plonk_prototype_amd as pa
    from plonk_prototype_amd import _lib
    lib = C.CDLL(pa.LIB_PATH)
    for name in GADGET_EXPORTS:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
    bound = pa.load()
    for name in GADGET_EXPORTS:
        assert getattr(bound, name).restype == C.c_int
        assert getattr(bound, name).argtypes == _lib.SIGNATURES[name][1]
    vp, sz = C.c_void_p, C.c_size_t
    assert _lib.SIGNATURES["pm_plonk_key_set_gadgets"][1] == [vp, vp, C.POINTER(_lib.Gadget), sz, C.POINTER(sz)]
    assert _lib.SIGNATURES["pm_plonk_fill_gadgets_dev"][1] == [vp, vp, vp, sz, C.c_uint32, C.POINTER(_lib.GadgetReport), vp]
    assert _lib.SIGNATURES["pm_test_host_naf"][1] == [_lib.u64p, C.c_uint32, C.POINTER(C.c_int8), C.POINTER(C.c_int)]


def test_header_declares_the_exports():
    text = open(HEADER).read()
    assert re.search(r"\bint pm_plonk_key_set_gadgets\(pm_ctx\* ctx, pm_prover_key\* key, const pm_plonk_gadget\* gadgets, "
                     r"size_t count, size_t\* added_bytes\);", text)
    assert re.search(r"\bint pm_plonk_fill_gadgets_dev\(pm_ctx\* ctx, const pm_prover_key\* key, void\* d_vars, size_t var_stride, "
                     r"uint32_t batch,\s+pm_plonk_gadget_report\* reports, void\* stream\);", text)
    assert re.search(r"\bint pm_test_host_naf\(const uint64_t s\[4\], uint32_t rounds, int8_t\* digits_msb_first, int\* too_long\);",
                     text)


def test_constants_match_the_header():
    from plonk_prototype_amd import _lib
    text = open(HEADER).read()
    header = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define PM_PLONK_GADGET_(\w+) (\d+)u", text)}
    assert header == {"RANGE": 0, "LOGIC": 1, "FIXED_BASE": 2, "CURVE_ADD": 3, "MAX_ROUNDS": 256, "TOO_WIDE": 1,
                      "SCALAR_TOO_LONG": 2, "DEGENERATE": 3}
    for name, value in header.items():
        assert getattr(_lib, "PLONK_GADGET_" + name) == value
    assert [getattr(_lib, "PLONK_GADGET_" + nm.upper()) for nm in _lib.PLONK_GADGET_KINDS] == [0, 1, 2, 3]
    assert {getattr(_lib, "PLONK_GADGET_" + nm.upper()): nm for nm in _lib.PLONK_GADGET_REASONS.values()} == _lib.PLONK_GADGET_REASONS


def _fields(text, name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for typ, names in re.findall(r"(uint64_t|uint32_t) ([^;]+);", body):
        for nm in names.split(","):
            m = re.match(r"\s*(\w+)(?:\[(\d+)\])?\s*$", nm)
            out.append((typ, m.group(1), int(m.group(2)) if m.group(2) else 1))
    return out


def test_structs_match_the_header():
    from plonk_prototype_amd import _lib
    text = open(HEADER).read()
    g = _fields(text, "pm_plonk_gadget")
    assert g == [("uint32_t", "kind", 1), ("uint32_t", "level", 1), ("uint64_t", "first_row", 1), ("uint32_t", "count", 1),
                 ("uint32_t", "param", 1), ("uint32_t", "in_var", 2)]
    assert [f[0] for f in _lib.Gadget._fields_] == [nm for _, nm, _ in g]
    assert C.sizeof(_lib.Gadget) == 4 + 4 + 8 + 4 + 4 + 8
    assert (_lib.Gadget.first_row.offset, _lib.Gadget.count.offset, _lib.Gadget.in_var.offset) == (8, 16, 24)
    r = _fields(text, "pm_plonk_gadget_report")
    assert r == [("uint64_t", "failed", 1), ("uint64_t", "first_gadget", 1), ("uint32_t", "first_reason", 1),
                 ("uint32_t", "reserved", 1)]
    assert [f[0] for f in _lib.GadgetReport._fields_] == [nm for _, nm, _ in r]
    assert C.sizeof(_lib.GadgetReport) == 24 and _lib.GadgetReport.first_reason.offset == 16


def test_python_surface():
    import plonk_prototype_amd as pa
    for fn in (pa.prove, pa.prove_batch, pa.ProverKey.check_witness, pa.ProverKey.check_witnesses):
        assert inspect.signature(fn).parameters["fill"].default is False
    for name in ("set_gadgets", "fill_gadgets"):
        assert callable(getattr(pa.ProverKey, name)), name
    g = pa.Gadget.range(5, 8, 3, level=2)
    assert (g.kind, g.first_row, g.count, g.level, g.in_vars) == (0, 5, 8, 2, (3,))
    raw = pa.Gadget.logic(1, 16, 7, 9, xor=True)._raw()
    assert (raw.kind, raw.count, raw.param, list(raw.in_var)) == (1, 16, 1, [7, 9])
    assert list(pa.Gadget.fixed_base(0, 256, 4, level=1)._raw().in_var) == [4, 0xFFFFFFFF]
    assert pa.Gadget.curve_add(9, level=3)._raw().first_row == 9
    rep = pa.GadgetReport(ok=False, failed=1, first_gadget=1, first_reason="too_wide")
    e = pa.GadgetInputError({2: rep}, [pa.Gadget.curve_add(0), g])
    assert issubclass(pa.GadgetInputError, ValueError) and e.report is rep
    assert "proof 2" in str(e) and "gadget 1" in str(e) and "too_wide" in str(e) and "range" in str(e)
    with pytest.raises(ValueError):
        pa.prove(types.SimpleNamespace(ctx=None, n=4), None, witness=np.zeros((4, 4, 4), np.uint64), fill=True)   # on variables only


# ------------------------------------------------------------------------------------------ the digit routine on the host
def _scalars(rounds):
    alt01 = int("01" * 128, 2)
    alt0011 = int("0011" * 64, 2)
    return [0, 1, 2, 3, R - 1, alt01, alt0011, (1 << rounds) - 1]


@pytest.mark.parametrize("rounds", [1, 4, 255, 256])
def test_host_naf_is_the_models_digit_loop(rounds):
    import plonk_prototype_amd as pa
    lib = pa.load()
    seen_long = seen_fit = False
    for s in _scalars(rounds):
        limbs = (C.c_uint64 * 4)(*[(s >> (64 * i)) & (2 ** 64 - 1) for i in range(4)])
        digits = (C.c_int8 * rounds)()
        too_long = C.c_int(-1)
        assert lib.pm_test_host_naf(limbs, rounds, digits, C.byref(too_long)) == 0
        e, long_ = M.naf_digits(s, rounds)
        assert list(digits) == [e[rounds - 1 - k] for k in range(rounds)], hex(s)
        assert too_long.value == int(long_), hex(s)
        # the issue's formula and closed form, on the side
        x = 3 * s
        assert e == [((x >> (j + 1)) & 1) - ((s >> (j + 1)) & 1) for j in range(rounds)]
        seen_long |= long_
        seen_fit |= not long_
    assert seen_fit and (seen_long or rounds == 256)           # every scalar below r has at most 256 digits
    # 2^rounds - 1 = 100..0(-1) in non-adjacent form, rounds + 1 digits -- but 2^1 - 1 = 1 is its own form
    assert M.naf_digits((1 << rounds) - 1, rounds)[1] == (rounds > 1)


def test_host_naf_refuses_bad_arguments():
    import plonk_prototype_amd as pa
    from plonk_prototype_amd import _lib
    lib = pa.load()
    limbs, digits = (C.c_uint64 * 4)(), (C.c_int8 * 300)()
    assert lib.pm_test_host_naf(limbs, 0, digits, None) == _lib.PM_ERR_BAD_ARG
    assert lib.pm_test_host_naf(limbs, 257, digits, None) == _lib.PM_ERR_BAD_ARG
    assert lib.pm_test_host_naf(None, 4, digits, None) == _lib.PM_ERR_BAD_ARG
    assert lib.pm_test_host_naf(limbs, 4, digits, None) == 0


# ------------------------------------------------------------------------------------------ the model against the identities
def test_model_output_satisfies_the_widget_identities():
    import random
    rng = random.Random(7)
    # range
    for m in (1, 2, 3, 32):
        for v in (0, (1 << min(8 * m, 254)) - 1, rng.getrandbits(min(8 * m, 254))):
            acc, reason = M.range_model(v, m)
            assert reason is None and acc[-1] == v
            rows = [[acc[4 * i + 3], acc[4 * i + 2], acc[4 * i + 1], acc[4 * i]] for i in range(m)] + [[0, 0, 0, acc[4 * m]]]
            for i in range(m):
                assert M.range_summands(rows[i], rows[i + 1][3]) == [0, 0, 0, 0]
        assert M.range_model(1 << (8 * m), m)[1] == M.TOO_WIDE if 8 * m < 255 else True
    # logic
    for quads in (1, 2, 16, 128):
        for xor in (False, True):
            bits = min(2 * quads, 254)
            x, y = rng.getrandbits(bits), rng.getrandbits(bits)
            A, Bc, D, P, reason = M.logic_model(x, y, quads, xor)
            assert reason is None and (A[-1], Bc[-1], D[-1]) == (x, y, (x ^ y) if xor else (x & y))
            rows = [[A[k], Bc[k], P[k], D[k]] for k in range(quads)] + [[A[quads], Bc[quads], 0, D[quads]]]
            for k in range(quads):
                assert M.logic_summands(rows[k], rows[k + 1], R - 1 if xor else 1) == [0, 0, 0, 0, 0]
    # fixed base
    for rounds in (1, 5, 64, 256):
        base = M.base_table(rounds)
        table = [base[rounds - 1 - k] for k in range(rounds)]
        for start in (M.IDENTITY, M.curve_point(0x7654321)):
            s = rng.getrandbits(rounds - 1) if rounds > 1 else 1
            pts, c, d, reason = M.fixed_base_model(s % R, rounds, start, table)
            assert reason is None and d[-1] == s % R
            rows = [[pts[k][0], pts[k][1], c[k], d[k]] for k in range(rounds)] + [[pts[rounds][0], pts[rounds][1], 0, d[rounds]]]
            for k in range(rounds):
                assert M.fixed_summands(rows[k], rows[k + 1], table[k]) == [0, 0, 0, 0]
            # the sum is start + s B
            want = start
            for j in range(rounds):
                if (s >> j) & 1:
                    want = M.jubjub_add(want, base[j])
            assert pts[-1] == want
    # curve addition
    p, q = M.curve_point(0xABCDEF), M.curve_point(0xFEDCBA)
    for a, b in ((p, q), (p, M.IDENTITY), (p, p), (p, ((-p[0]) % R, p[1]))):
        x3, y3, xy, reason = M.curve_add_model(a, b)
        assert reason is None and M.on_curve((x3, y3))
        assert M.var_summands([a[0], a[1], b[0], b[1]], [x3, y3, 0, xy]) == [0, 0, 0]
    assert M.curve_add_model(p, ((-p[0]) % R, p[1]))[:2] == M.IDENTITY


def test_builder_rows_satisfy_the_identities():
    b = M.Builder(64)
    s, v, x, y = b.var(True), b.var(True), b.var(True), b.var(True)
    sx, sy = b.var(True), b.var(True)
    px, py = b.fixed_base(s, 8, (sx, sy))
    b.equal(s, b.wires[3][b.gadgets[-1][2] + 8])
    out = b.range(v, 2, level=0)
    b.equal(v, out)
    b.logic(x, y, 4, xor=True)
    qx, qy = b.var(True), b.var(True)
    b.curve_add((px, py), (qx, qy), level=1)
    arith = b.fill_arithmetic()
    q = M.curve_point(99)
    only, full, reasons = b.model({s: 0xA7, v: 0xBEEF, x: 0x5A, y: 0xC3, sx: 0, sy: 1, qx: q[0], qy: q[1], **arith})
    assert not reasons and only != full
    rows = b.rows(full)
    n = b.n
    for i in range(n):
        nxt = rows[(i + 1) % n]
        sel = {k: b.sel[k][i] for k in M.SELECTORS}
        a, bb, c, d = rows[i]
        assert sel["q_arith"] * (sel["q_m"] * a * bb + sel["q_l"] * a + sel["q_r"] * bb + sel["q_o"] * c + sel["q_4"] * d
                                 + sel["q_c"]) % R == 0, i
        if sel["q_range"]:
            assert M.range_summands(rows[i], nxt[3]) == [0] * 4, i
        if sel["q_logic"]:
            assert M.logic_summands(rows[i], nxt, sel["q_c"]) == [0] * 5, i
        if sel["q_fixed_group_add"]:
            assert M.fixed_summands(rows[i], nxt, (sel["q_l"], sel["q_r"])) == [0] * 4, i
        if sel["q_variable_group_add"]:
            assert M.var_summands(rows[i], nxt) == [0] * 3, i
