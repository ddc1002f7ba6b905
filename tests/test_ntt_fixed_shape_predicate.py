"""Which pass launches take a fixed-shape kernel (csrc/ntt_kernels4.hip.h: pass4_fixed_match, option ntt_fixed_shape), pinned row by
row through the library's pure-host hook pm_test_ntt_fixed_match: no context, no device.  A launch takes the variant only if its size,
its place in the plan, the blocking of the wide vectors and its flags are the variant's exactly, in a plain transform of a whole
input; everything else keeps the generic kernel.  The rows spell the launches ntt_run() makes for the calls named beside them."""
import ctypes as C

from plonk_prototype_amd import _lib

DIRECT_TW, PRE_COSET, POST_SCALE, POST_COSET, XCD, TW_OUT, TW_APPLIED, PRIO = 1, 2, 4, 8, 16, 32, 64, 128
FIRST, MIDDLE, LAST, SINGLE = 1, 2, 3, 0
N20 = 1 << 20
FIRST_FLAGS = TW_OUT | PRIO | XCD            # the first pass of a plain 2^20 transform with the default tunables
LAST_FLAGS = TW_APPLIED | PRIO | XCD         # ... and its last pass

# (what, S, LT, role, log_n, log_ns, wide_glog, pass flags, in_len, coset, ntt_fixed_shape) -> fixed?
# ntt_fixed_shape: 0 never, 1 the variants that are on by default (the first pass), 2 every variant (the last pass too)
ROWS = [
    ("plain 2^20, first pass", 10, 1, FIRST, 20, 0, 2, FIRST_FLAGS, N20, 0, 1, True),
    ("plain 2^20, first pass, every variant", 10, 1, FIRST, 20, 0, 2, FIRST_FLAGS, N20, 0, 2, True),
    ("plain 2^20, last pass: off by default", 10, 1, LAST, 20, 10, 2, LAST_FLAGS, N20, 0, 1, False),
    ("plain 2^20, last pass, every variant", 10, 1, LAST, 20, 10, 2, LAST_FLAGS, N20, 0, 2, True),
    ("an option value that is not accepted", 10, 1, FIRST, 20, 0, 2, FIRST_FLAGS, N20, 0, 3, False),
    ("option off, first", 10, 1, FIRST, 20, 0, 2, FIRST_FLAGS, N20, 0, 0, False),
    ("option off, last", 10, 1, LAST, 20, 10, 2, LAST_FLAGS, N20, 0, 0, False),
    ("zero padding, first", 10, 1, FIRST, 20, 0, 2, FIRST_FLAGS, 1 << 18, 0, 1, False),
    ("zero padding, last", 10, 1, LAST, 20, 10, 2, LAST_FLAGS, 1 << 18, 0, 1, False),
    ("one element short, first", 10, 1, FIRST, 20, 0, 2, FIRST_FLAGS, N20 - 1, 0, 1, False),
    ("coset forward, first", 10, 1, FIRST, 20, 0, 2, FIRST_FLAGS | PRE_COSET, N20, 1, 1, False),
    ("coset forward, last", 10, 1, LAST, 20, 10, 2, LAST_FLAGS, N20, 1, 1, False),
    ("coset inverse, first", 10, 1, FIRST, 20, 0, 2, FIRST_FLAGS, N20, 1, 1, False),
    ("coset inverse, last", 10, 1, LAST, 20, 10, 2, LAST_FLAGS | POST_COSET, N20, 1, 1, False),
    ("a coset flag without the call's", 10, 1, FIRST, 20, 0, 2, FIRST_FLAGS | PRE_COSET, N20, 0, 1, False),
    ("post scale on the last pass", 10, 1, LAST, 20, 10, 2, LAST_FLAGS | POST_SCALE, N20, 0, 1, False),
    ("ntt_tw_producer 0, first", 10, 1, FIRST, 20, 0, 2, PRIO | XCD, N20, 0, 1, False),
    ("ntt_tw_producer 0, last", 10, 1, LAST, 20, 10, 2, DIRECT_TW | PRIO | XCD, N20, 0, 1, False),
    ("ntt_direct_tw 0, last", 10, 1, LAST, 20, 10, 2, PRIO | XCD, N20, 0, 1, False),
    ("ntt_step_prio 0, first", 10, 1, FIRST, 20, 0, 2, TW_OUT | XCD, N20, 0, 1, False),
    ("ntt_step_prio 0, last", 10, 1, LAST, 20, 10, 2, TW_APPLIED | XCD, N20, 0, 1, False),
    ("ntt_xcd 0, first", 10, 1, FIRST, 20, 0, 2, TW_OUT | PRIO, N20, 0, 1, False),
    ("ntt_xcd 0, last", 10, 1, LAST, 20, 10, 2, TW_APPLIED | PRIO, N20, 0, 1, False),
    ("ntt_tile_log 12, first", 10, 2, FIRST, 20, 0, 2, FIRST_FLAGS, N20, 0, 1, False),
    ("ntt_tile_log 12, last", 10, 2, LAST, 20, 10, 2, LAST_FLAGS, N20, 0, 1, False),
    ("ntt_tile_log 10, first", 10, 0, FIRST, 20, 0, 2, FIRST_FLAGS, N20, 0, 1, False),
    ("wide vectors blocked by 8", 10, 1, FIRST, 20, 0, 3, FIRST_FLAGS, N20, 0, 1, False),
    ("2^19, first <10, 1>", 10, 1, FIRST, 19, 0, 2, FIRST_FLAGS, 1 << 19, 0, 1, False),
    ("2^19, last <9, 2>", 9, 2, LAST, 19, 10, 2, LAST_FLAGS, 1 << 19, 0, 1, False),
    ("2^21, first <7, 3>", 7, 3, FIRST, 21, 0, 3, XCD, 1 << 21, 0, 1, False),
    ("2^21, middle", 7, 3, MIDDLE, 21, 7, 3, DIRECT_TW | XCD, 1 << 21, 0, 1, False),
    ("2^21 with the headline's flags", 10, 1, FIRST, 21, 0, 2, FIRST_FLAGS, 1 << 21, 0, 1, False),
    ("2^30 in three passes of 2^10, first", 10, 1, FIRST, 30, 0, 2, FIRST_FLAGS, 1 << 30, 0, 1, False),
    ("2^30, last", 10, 1, LAST, 30, 20, 2, LAST_FLAGS, 1 << 30, 0, 1, False),
    ("a <10, 1> middle pass", 10, 1, MIDDLE, 20, 10, 2, LAST_FLAGS, N20, 0, 1, False),
    ("a last pass that is not behind 2^10", 10, 1, LAST, 20, 0, 2, LAST_FLAGS, N20, 0, 1, False),
    ("a first pass that is not in front", 10, 1, FIRST, 20, 10, 2, FIRST_FLAGS, N20, 0, 1, False),
    ("the first pass with the last one's flags", 10, 1, FIRST, 20, 0, 2, LAST_FLAGS, N20, 0, 1, False),
    ("the last pass with the first one's flags", 10, 1, LAST, 20, 10, 2, FIRST_FLAGS, N20, 0, 1, False),
    ("single pass 2^10", 10, 0, SINGLE, 10, 0, 2, XCD, 1 << 10, 0, 1, False),
    ("no such shape", 40, 40, FIRST, 20, 0, 2, FIRST_FLAGS, N20, 0, 1, False),
]


def test_rows():
    fn = _lib.load().pm_test_ntt_fixed_match
    for what, *args, want in ROWS:
        assert fn(*args) == (1 if want else 0), what
        if not want and args[-1] == 1 and "off by default" not in what:   # nor when every variant is asked for
            assert fn(*args[:-1], 2) == 0, what


def test_the_plan_the_rows_assume():
    """the [10, 10] plan, two columns a tile and wide blocks of four that the variants are built for, at every batch size"""
    for batch in (1, 2, 4, 64):
        out = (C.c_uint32 * 20)()
        assert _lib.load().pm_test_ntt_plan(20, batch, 0, 0, 4, 0, out) == 0
        v = list(out)
        assert v[0] == 2 and (v[1], v[2], v[5], v[6]) == (10, 1, 10, 1) and v[18] == 2, batch


def test_the_hooks_are_declared():
    import os

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for name in ("pm_test_ntt_fixed_match", "pm_test_ntt_last_variants"):
        assert name in _lib.SIGNATURES
        for rel in (("include", "plonk_mi355x.h"), ("INTEGRATION.md",)):
            assert name in open(os.path.join(root, *rel)).read(), (name, rel)
