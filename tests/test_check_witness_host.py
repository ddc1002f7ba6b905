"""Host-side ground for the witness check (pm_plonk_check_witness): the new exports are in the
library and bound with the declared signatures, the PLONK_FAIL_* constants and the report struct are the header's, and the
Python prover takes ``check``.  No device compute here."""
import ctypes as C
import inspect
import os
import re

CHECK_EXPORTS = ("pm_plonk_key_enable_check", "pm_plonk_check_witness", "pm_plonk_check_witness_batch")
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "plonk_mi355x.h")


def test_check_symbols_exported_and_bound():
    import plonk_prototype_amd as pa
    from plonk_prototype_amd import _lib
    lib = C.CDLL(pa.LIB_PATH)
    for name in CHECK_EXPORTS:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
    bound = pa.load()
    for name in CHECK_EXPORTS:
        assert getattr(bound, name).restype == C.c_int
        assert getattr(bound, name).argtypes == _lib.SIGNATURES[name][1]
    u64p, u8p, rep = _lib.u64p, C.POINTER(C.c_uint8), C.POINTER(_lib.WitnessReport)
    assert _lib.SIGNATURES["pm_plonk_key_enable_check"][1] == [C.c_void_p, C.c_void_p, C.POINTER(C.c_int64),
                                                               C.POINTER(C.c_size_t)]
    assert _lib.SIGNATURES["pm_plonk_check_witness"][1] == [C.c_void_p, C.c_void_p, C.c_void_p, u64p, u64p, C.c_size_t, rep, u8p]
    assert _lib.SIGNATURES["pm_plonk_check_witness_batch"][1] == [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p,
                                                                  C.POINTER(u64p), C.POINTER(u64p), C.POINTER(C.c_size_t), rep,
                                                                  u8p]


def test_header_declares_the_exports():
    text = open(HEADER).read()
    for name in CHECK_EXPORTS:
        assert re.search(r"\bint %s\(pm_ctx\* ctx, pm_prover_key\* key," % name, text), name


def test_fail_constants_match_the_header():
    from plonk_prototype_amd import _lib
    text = open(HEADER).read()
    header = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define PM_PLONK_FAIL_(\w+) (\d+)u", text)}
    assert header == {"ARITH": 1, "RANGE": 2, "LOGIC": 4, "FIXED_BASE": 8, "VAR_BASE": 16, "COPY": 32}
    for name, value in header.items():
        assert getattr(_lib, "PLONK_FAIL_" + name) == value
    # bit k is count[k] and name k
    assert [getattr(_lib, "PLONK_FAIL_" + nm.upper()) for nm in _lib.PLONK_FAIL_NAMES] == [1 << k for k in range(6)]


def test_report_struct_matches_the_header():
    from plonk_prototype_amd import _lib
    text = open(HEADER).read()
    body = re.search(r"typedef struct pm_plonk_witness_report \{(.*?)\} pm_plonk_witness_report;", text, re.S).group(1)
    fields = re.findall(r"(uint64_t|uint32_t) (\w+)(?:\[(\d+)\])?;", body)
    assert [(t, nm, int(k) if k else 1) for t, nm, k in fields] == [
        ("uint64_t", "failed_rows", 1), ("uint64_t", "first_row", 1), ("uint32_t", "first_mask", 1), ("uint32_t", "reserved", 1),
        ("uint64_t", "count", 6)]
    assert [f[0] for f in _lib.WitnessReport._fields_] == [nm for _, nm, _ in fields]
    assert C.sizeof(_lib.WitnessReport) == 8 + 8 + 4 + 4 + 6 * 8
    assert _lib.WitnessReport.first_mask.offset == 16 and _lib.WitnessReport.count.offset == 24


def test_python_surface():
    import plonk_prototype_amd as pa
    for fn in (pa.prove, pa.prove_batch):
        p = inspect.signature(fn).parameters["check"]
        assert p.default is False
    for name in ("enable_check", "check_witness", "check_witnesses"):
        assert callable(getattr(pa.ProverKey, name)), name
    assert inspect.signature(pa.ProverKey.check_witness).parameters["masks"].default is False
    assert issubclass(pa.UnsatisfiedWitness, Exception)
    r = pa.WitnessReport(ok=False, failed_rows=2, first_row=7, first_reasons=pa.WitnessReport.reasons(0b100001),
                         counts={}, row_masks=None)
    assert r.first_reasons == ("arith", "copy")
    e = pa.UnsatisfiedWitness(r)
    assert e.report is r and e.reports == {0: r}
    assert "row 7" in str(e) and "arith" in str(e) and "copy" in str(e)
    e2 = pa.UnsatisfiedWitness(reports={3: r})
    assert e2.report is r and "witness 3" in str(e2) and "row 7" in str(e2)
