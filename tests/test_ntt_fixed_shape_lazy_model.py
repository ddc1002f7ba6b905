"""The fixed-shape first pass of the 2^20 transform multiplies by its step twiddles in the form PM_NTT_FIXED_FIRST_G
(csrc/ntt_kernels4.hip.h: step4_fixed_lazy_form), three rows where the generic first pass takes two.  The walk of the limb and
value classes through the five steps of a <10, 1> first pass is the one of tests/test_fe_mul_split_lazy_model.py, run here with
that form: first-layer products at the top of step 1, lazy products in steps 2 .. 4, the inter-pass product at the exit."""
import importlib.util
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _model():
    spec = importlib.util.spec_from_file_location("lazy_model_walk", os.path.join(ROOT, "tests", "test_fe_mul_split_lazy_model.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def fixed_first_form():
    src = open(os.path.join(ROOT, "plonk-prototype_amd", "csrc", "ntt_kernels4.hip.h")).read()
    m = re.search(r"#define PM_NTT_FIXED_FIRST_G (\d)\n", src)
    assert m, "PM_NTT_FIXED_FIRST_G"
    assert re.search(r"return FIX != 0 && !in_wide && step4_lazy_form\(S, LT, in_wide\) != 0 \? PM_NTT_FIXED_FIRST_G : ", src)
    return int(m.group(1))


def test_the_form_has_a_table_and_a_model():
    walk = _model()
    G = fixed_first_form()
    assert G in (3, 5) and (G, G) in walk.FORMS        # the forms the kernels read tables of (the last pass's, the generic first pass's)


def test_five_steps_of_the_fixed_first_pass(monkeypatch):
    walk = _model()
    G = fixed_first_form()
    monkeypatch.setattr(walk, "kernel_form", lambda in_wide: G)
    walk.test_five_steps_of_a_radix_1024_pass(False)
    assert not walk.M.VIOLATIONS, walk.M.VIOLATIONS[:3]
