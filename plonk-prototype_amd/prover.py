"""Host-side mirror of ``dusk_plonk::proof_system::{Prover::preprocess, Prover::prove_with_preprocessed,
Proof}`` (dusk-plonk 0.8.2, ref:Cargo.toml:19 -- the crate is not in the reference tree, so the formulas
and transcript labels are restated from the published 0.8 design: "parity unpinned") over the native
prover of the library (``pm_plonk_preprocess`` / ``pm_plonk_key_commit`` / ``pm_plonk_prove``:
``csrc/prover.hip``).  SURVEY.md section 8f rows N1 + N2 + N3, BASELINE.json configs[3].

  gates     q_arith (q_m a b + q_l a + q_r b + q_o c + q_4 d + q_c) + PI
            + q_range R + q_logic L + q_fixed_group_add F + q_variable_group_add V = 0
            (the gate kinds the reference's gadgets emit: ref:src/zk/gadgets.rs:34,37,40,88-91,211)
  copy      sigma over the cosets {1, K1, K2, K3} H            (K = 7, 13, 17)
  round 1   wire polynomials (iNTT), commitments
  round 2   beta, gamma; grand product z; commitment
  round 3   alpha + four separation challenges; quotient t on the 4n coset, split in four, commitments
  round 4   evaluation challenge; 16 openings + t(z); linearisation polynomial r
  round 5   two aggregate opening witnesses W_z, W_zw; commitments

Every polynomial stays in HBM from the witness upload to the last commitment: the five rounds run
inside ONE C-ABI call (what a Rust prover binds).  This module only marshals arguments, and holds the
verifier's side of the transcript (``derive_challenges``) for the end-to-end checks in tests/.
"""
from __future__ import annotations

import ctypes as C
import secrets
from dataclasses import dataclass, field

import numpy as np

from . import _lib
from .field import R_MOD, fr_from_limbs, fr_to_limbs
from .host import CommitKey, Context, DeviceVector
from .transcript import Transcript

# order of pm_plonk_preprocess's selector array (= dusk's ProverKey widgets)
SELECTORS = ("q_m", "q_l", "q_r", "q_o", "q_c", "q_4", "q_arith", "q_range", "q_logic", "q_fixed_group_add",
             "q_variable_group_add")
# VerifierKey::seed_transcript order
_SEED_ORDER = ("q_m", "q_l", "q_r", "q_o", "q_c", "q_4", "q_arith", "q_range", "q_logic", "q_variable_group_add",
               "q_fixed_group_add")
VK_NAMES = SELECTORS + ("sigma_1", "sigma_2", "sigma_3", "sigma_4")
CHALLENGES = ("beta", "gamma", "alpha", "range_sep", "logic_sep", "fixed_sep", "var_sep", "z", "aw", "aw_shifted")

_labels_cache: dict | None = None


def transcript_labels() -> dict:
    """Every label string of the transcript, from the ONE table both sides use (csrc/prover_transcript.h, namespace tl, through
    ``pm_plonk_transcript_labels``): {key: bytes}.  The labels are restated from the published dusk-plonk 0.8 design --
    parity-unpinned -- and that table is the single place to edit when upstream vectors become available."""
    global _labels_cache
    if _labels_cache is None:
        text = _lib.load().pm_plonk_transcript_labels().decode()
        _labels_cache = {k: v.encode() for k, v in (line.split("=", 1) for line in text.splitlines() if line)}
    return _labels_cache


@dataclass
class Circuit:
    """Selector evaluations on H ([n, 4] Montgomery limbs each; None = identically zero) and
    the copy constraints, in exactly one of two forms: ``sigma_index[j, i] = j' * n + i'`` means wire j of gate i is followed
    by wire j' of gate i'; or ``wire_vars[j, i]`` ([4, n] uint32) = the variable at wire j of gate i, an id below
    ``num_vars`` or ``_lib.PLONK_NO_VAR``, from which the library builds the permutation on the device in dusk's order
    (``pm_plonk_preprocess_wires``)."""
    sigma_index: np.ndarray | None = None
    q_m: np.ndarray | None = None
    q_l: np.ndarray | None = None
    q_r: np.ndarray | None = None
    q_o: np.ndarray | None = None
    q_c: np.ndarray | None = None
    q_4: np.ndarray | None = None
    q_arith: np.ndarray | None = None
    q_range: np.ndarray | None = None
    q_logic: np.ndarray | None = None
    q_fixed_group_add: np.ndarray | None = None
    q_variable_group_add: np.ndarray | None = None
    wire_vars: np.ndarray | None = None
    num_vars: int | None = None

    def __post_init__(self):
        if (self.sigma_index is None) == (self.wire_vars is None):
            raise ValueError("give exactly one of sigma_index and wire_vars")
        if self.wire_vars is not None and self.num_vars is None:
            raise ValueError("wire_vars needs num_vars")
        if self.wire_vars is None and self.num_vars is not None:
            raise ValueError("num_vars goes with wire_vars")

    @property
    def n(self) -> int:
        return self.q_m.shape[0]


@dataclass
class Proof:
    """``dusk_plonk::proof_system::Proof``: 11 commitments (affine [12]) and the opening evaluations ([4]
    Montgomery limbs), plus t(z) (which the verifier recomputes) and the challenges for the tests."""
    commitments: dict = field(default_factory=dict)
    evaluations: dict = field(default_factory=dict)
    challenges: dict = field(default_factory=dict)   # ints; recomputable from the transcript
    native_bytes: bytes = b""                        # pm_plonk_proof_to_bytes of the same proof

    COMMITMENTS = ("a", "b", "c", "d", "z", "t_1", "t_2", "t_3", "t_4", "w_z", "w_zw")
    # transcript order (pm_plonk_proof.evaluations) / ProofEvaluations::to_bytes order
    TRANSCRIPT_EVALS = ("a", "b", "c", "d", "a_next", "b_next", "d_next", "sigma_1", "sigma_2", "sigma_3", "q_arith",
                        "q_c", "q_l", "q_r", "z_next", "t", "r")
    EVALUATIONS = ("a", "b", "c", "d", "a_next", "b_next", "d_next", "q_arith", "q_c", "q_l", "q_r", "sigma_1",
                   "sigma_2", "sigma_3", "r", "z_next")

    def to_bytes(self) -> bytes:
        """``Proof::to_bytes``: 11 x 48-byte compressed G1 then the 16 x 32-byte little-endian canonical
        scalars of ``ProofEvaluations::to_bytes`` (1040 bytes)."""
        from .transcript import g1_compress
        return b"".join(g1_compress(self.commitments[k]) for k in self.COMMITMENTS) + \
            b"".join(fr_from_limbs(self.evaluations[k]).to_bytes(32, "little") for k in self.EVALUATIONS)

    @classmethod
    def from_bytes(cls, data: bytes) -> "Proof":
        from .transcript import g1_decompress
        if len(data) != 48 * len(cls.COMMITMENTS) + 32 * len(cls.EVALUATIONS):
            raise ValueError("wrong proof length")
        p, off = cls(), 0
        for k in cls.COMMITMENTS:
            p.commitments[k] = g1_decompress(data[off:off + 48])
            off += 48
        for k in cls.EVALUATIONS:
            v = int.from_bytes(data[off:off + 32], "little")
            if v >= R_MOD:
                raise ValueError("scalar is not reduced")
            p.evaluations[k] = fr_to_limbs(v)
            off += 32
        return p


@dataclass
class WitnessReport:
    """``pm_plonk_witness_report``: what ``ProverKey.check_witness`` found.  ``first_row`` is the lowest failing row (None
    when the witness is satisfied), ``first_reasons`` the names of that row's failed checks, ``counts[name]`` the number of
    rows failing each check (names: ``_lib.PLONK_FAIL_NAMES``), ``row_masks`` the mask of every row ([n] uint8, bit k =
    ``PLONK_FAIL_NAMES[k]``) when it was asked for."""
    ok: bool
    failed_rows: int
    first_row: int | None
    first_reasons: tuple
    counts: dict
    row_masks: np.ndarray | None = None

    @staticmethod
    def reasons(mask: int) -> tuple:
        return tuple(nm for k, nm in enumerate(_lib.PLONK_FAIL_NAMES) if (int(mask) >> k) & 1)

    @classmethod
    def _from_raw(cls, raw, row_masks=None) -> "WitnessReport":
        failed = int(raw.failed_rows)
        return cls(ok=failed == 0, failed_rows=failed, first_row=int(raw.first_row) if failed else None,
                   first_reasons=cls.reasons(raw.first_mask), counts={nm: int(raw.count[k]) for k, nm in
                                                                      enumerate(_lib.PLONK_FAIL_NAMES)},
                   row_masks=row_masks)

    def describe(self) -> str:
        if self.ok:
            return "satisfied"
        return f"row {self.first_row} fails ({', '.join(self.first_reasons)}); {self.failed_rows} failing row(s)"


class UnsatisfiedWitness(ValueError):
    """``prove(..., check=True)`` / ``prove_batch(..., check=True)``: the witness does not satisfy the circuit, nothing was
    proved.  ``report`` is the :class:`WitnessReport` (of the first failing batch member), ``reports`` maps every failing
    batch member to its report ({0: report} for ``prove``)."""

    def __init__(self, report: WitnessReport | None = None, reports: dict | None = None):
        self.reports = dict(reports) if reports is not None else {0: report}
        self.report = report if report is not None else self.reports[min(self.reports)]
        if reports is None:
            msg = "the witness does not satisfy the circuit: " + self.report.describe()
        else:
            msg = "; ".join(f"witness {b} does not satisfy the circuit: {r.describe()}" for b, r in sorted(self.reports.items()))
        super().__init__(msg)


@dataclass(frozen=True)
class Gadget:
    """``pm_plonk_gadget``: one widget gadget of a composer-form circuit whose rows ``ProverKey.fill_gadgets`` fills from
    its input variables (the definitions are in include/plonk_mi355x.h; DESIGN.md sections 7.2f to 7.2i).  Gadgets of one ``level``
    are independent; levels run in rising order, and a list given to ``ProverKey.set_gadgets`` is sorted by level."""
    kind: int
    first_row: int
    count: int = 0
    level: int = 0
    param: int = 0
    in_vars: tuple = ()

    @classmethod
    def range(cls, first_row: int, rows: int, value_var: int, level: int = 0) -> "Gadget":
        """A range check of 8 x rows bits on variable ``value_var``: rows [first_row, first_row + rows] hold the quad accumulators."""
        return cls(_lib.PLONK_GADGET_RANGE, int(first_row), int(rows), int(level), 0, (int(value_var),))

    @classmethod
    def logic(cls, first_row: int, quads: int, a_var: int, b_var: int, xor: bool = False, level: int = 0) -> "Gadget":
        """AND (or XOR) of the low 2 x quads bits of two variables: rows [first_row, first_row + quads]."""
        return cls(_lib.PLONK_GADGET_LOGIC, int(first_row), int(quads), int(level), 1 if xor else 0, (int(a_var), int(b_var)))

    @classmethod
    def fixed_base(cls, first_row: int, rounds: int, scalar_var: int, level: int = 0) -> "Gadget":
        """JubJub fixed-base scalar multiplication in ``rounds`` <= 256 rounds: rows [first_row, first_row + rounds]; the
        start point is read from a, b of the first row, the table points are the key's q_l, q_r."""
        return cls(_lib.PLONK_GADGET_FIXED_BASE, int(first_row), int(rounds), int(level), 0, (int(scalar_var),))

    @classmethod
    def curve_add(cls, first_row: int, level: int = 0) -> "Gadget":
        """JubJub addition of the points in a b and c d of ``first_row``; the sum goes to a b of the next row."""
        return cls(_lib.PLONK_GADGET_CURVE_ADD, int(first_row), 0, int(level), 0, ())

    @classmethod
    def arith(cls, first_row: int, rows: int, level: int = 0) -> "Gadget":
        """A run of ``rows`` arithmetic rows with q_o = -1, solved for c one after the other (a later row may read an earlier
        one's c).  Sequential: independent runs belong in separate gadgets of one level."""
        return cls(_lib.PLONK_COMPOSED_ARITH, int(first_row), int(rows), int(level), 0, ())

    @classmethod
    def bits(cls, first_row: int, num_bits: int, value_var: int, level: int = 0) -> "Gadget":
        """The ``num_bits`` <= 256 low bits of variable ``value_var`` and their running sums: rows [first_row, first_row +
        2 num_bits), a boolean row and an accumulating row per bit; the sum starts from b of the second row."""
        return cls(_lib.PLONK_COMPOSED_BITS, int(first_row), int(num_bits), int(level), 0, (int(value_var),))

    @classmethod
    def maybe_equal(cls, first_row: int, level: int = 0) -> "Gadget":
        """Three rows: u = a - b of ``first_row``, z = 1 / u (or 0) and y = 1 - u z, which is 1 exactly when a = b."""
        return cls(_lib.PLONK_COMPOSED_MAYBE_EQUAL, int(first_row), 0, int(level), 0, ())

    @classmethod
    def decomposition(cls, first_row: int, num_bits: int, value_var: int, level: int = 0) -> list:
        """A whole scalar decomposition: the bits at ``level``, then the comparison of their sum with the value in the three
        rows that follow, one level later.  -> [bits, maybe_equal]"""
        return [cls.bits(first_row, num_bits, value_var, level), cls.maybe_equal(int(first_row) + 2 * int(num_bits), int(level) + 1)]

    @classmethod
    def hades(cls, first_row: int, rounds: int = 67, full_rounds: int = 8, level: int = 0) -> "Gadget":
        """One Hades permutation of width 5 (a Poseidon sponge's): ``rounds`` rounds of which the first and the last
        ``full_rounds`` / 2 are full, 30 rows a full round and 18 a partial one from ``first_row`` on; the state is read from
        a of the first five rows, the round constants and the matrix are the rows' own coefficients.  The defaults are
        dusk-hades' (1302 rows)."""
        return cls(_lib.PLONK_PERMUTATION_HADES, int(first_row), int(rounds), int(level), int(full_rounds), ())

    @classmethod
    def variable_base(cls, first_row: int, rounds: int = 252, level: int = 0) -> "Gadget":
        """dusk-plonk's ``variable_base_scalar_mul``: ``rounds`` rounds of six rows from ``first_row`` on (a doubling, the two
        rows that select bit P, an addition).  The start point is read from a, b of the first row, bit k from a of row 6k + 2
        (most significant first) and P from b of rows 2 and 3; one wave fills the whole chain.  The default is dusk's 252."""
        return cls(_lib.PLONK_GADGET_VAR_BASE, int(first_row), int(rounds), int(level), 0, ())

    @property
    def rows(self) -> int:
        """The rows the gadget claims, a trailing row included (``pm_plonk_gadget_rows``); 0 for a kind, count or param that
        ``set_gadgets`` refuses whatever the circuit."""
        return int(_lib.load().pm_plonk_gadget_rows(C.byref(self._raw())))

    def _raw(self) -> "_lib.Gadget":
        iv = tuple(self.in_vars) + (_lib.PLONK_NO_VAR,) * (2 - len(self.in_vars))
        return _lib.Gadget(self.kind, self.level, self.first_row, self.count, self.param, (C.c_uint32 * 2)(*iv))


@dataclass
class GadgetReport:
    """``pm_plonk_gadget_report`` of one assignment: how many gadgets' inputs did not fit, the lowest such gadget (its index
    in the list given to ``set_gadgets``) and why (``_lib.PLONK_GADGET_REASONS``)."""
    ok: bool
    failed: int
    first_gadget: int | None
    first_reason: str | None

    @classmethod
    def _from_raw(cls, raw) -> "GadgetReport":
        failed = int(raw.failed)
        return cls(ok=failed == 0, failed=failed, first_gadget=int(raw.first_gadget) if failed else None,
                   first_reason=_lib.PLONK_GADGET_REASONS.get(int(raw.first_reason)) if failed else None)


class GadgetInputError(ValueError):
    """``fill=True``: an input does not fit its gadget (a value too wide for its range, a scalar with too many digits, a
    degenerate addition); nothing was proved or checked.  ``reports``: {proof: GadgetReport} of the failing assignments."""

    def __init__(self, reports: dict, gadgets=None):
        self.reports = dict(reports)
        self.report = self.reports[min(self.reports)]

        def one(b, r):
            kind = ""
            if gadgets is not None and r.first_gadget is not None and r.first_gadget < len(gadgets):
                k = gadgets[r.first_gadget].kind
                name = _lib.PLONK_GADGET_KINDS[k] if k < len(_lib.PLONK_GADGET_KINDS) else {**_lib.PLONK_COMPOSED_KINDS, **_lib.PLONK_PERMUTATION_KINDS, **_lib.PLONK_CHAIN_KINDS}.get(k, f"kind {k}")
                kind = f" ({name} at row {gadgets[r.first_gadget].first_row})"
            return f"proof {b}: gadget {r.first_gadget}{kind}: {r.first_reason}; {r.failed} failing gadget(s)"
        super().__init__("; ".join(one(b, r) for b, r in sorted(self.reports.items())))


class ProverKey:
    """``pm_prover_key``: selector and sigma polynomials as coefficients and on the 4n coset, the coset
    points, L_1, 1/Z_H and the per-proof workspace -- built and owned by the library, all in HBM."""

    def __init__(self, circuit: Circuit, ctx: Context):
        self.ctx, self.n = ctx, circuit.n
        keep = []
        ptrs = (_lib.u64p * len(SELECTORS))()
        for i, s in enumerate(SELECTORS):
            a = getattr(circuit, s)
            if a is not None:
                a = np.ascontiguousarray(a, dtype=np.uint64).reshape(-1, 4)
                if a.shape[0] != self.n:
                    raise ValueError(f"selector {s} has the wrong length")
                keep.append(a)
                ptrs[i] = a.ctypes.data_as(_lib.u64p)
        h = C.c_void_p()
        if circuit.wire_vars is not None:
            wv = _wire_vars(circuit.wire_vars, self.n)
            ctx._check(ctx._lib.pm_plonk_preprocess_wires(ctx._h, ptrs, wv.ctypes.data_as(_lib.u32p), int(circuit.num_vars),
                                                          self.n, C.byref(h)))
            self.wire_vars, self.num_vars = wv, int(circuit.num_vars)
            self._sigma_index = None            # filled from pm_plonk_sigma_from_wires when someone reads it
        else:
            idx = np.ascontiguousarray(circuit.sigma_index, dtype=np.int64).reshape(-1)
            ctx._check(ctx._lib.pm_plonk_preprocess(ctx._h, ptrs, idx.ctypes.data_as(C.POINTER(C.c_int64)), self.n, C.byref(h)))
            self.wire_vars, self.num_vars = None, 0
            self._sigma_index = idx             # the check (enable_check) takes the permutation again: the key keeps sigma's values
        self._h = h
        self._check_enabled = False
        self.gadgets: list = []                 # set_gadgets
        self.verifier_key: dict | None = None
        self.label = b"plonk"

    @property
    def sigma_index(self) -> np.ndarray:
        """The copy permutation (flat int64 [4n]); on a key built from wire variables, computed on first use."""
        if self._sigma_index is None:
            self._sigma_index = sigma_from_wires(self.wire_vars, self.num_vars, self.ctx).reshape(-1)
        return self._sigma_index

    def set_gadgets(self, gadgets) -> int:
        """Give the key its gadget table (``pm_plonk_key_set_gadgets``; a key built from ``wire_vars``): a list of
        :class:`Gadget` sorted by level, checked on the device against the key's selectors.  Replaces an earlier table; an
        empty list clears it.  -> the device bytes the table holds."""
        gadgets = list(gadgets)
        raw = (_lib.Gadget * max(len(gadgets), 1))(*[g._raw() for g in gadgets])
        out = C.c_size_t()
        self.ctx._check(self.ctx._lib.pm_plonk_key_set_gadgets(self.ctx._h, self._h, raw if gadgets else None, len(gadgets),
                                                               C.byref(out)))
        self.gadgets = gadgets
        return int(out.value)

    def _fill_device(self, d_ptr, B: int, stride: int) -> list:
        """``pm_plonk_fill_gadgets_dev`` on B assignments in device memory -> one GadgetReport each."""
        raws = (_lib.GadgetReport * B)()
        self.ctx._check(self.ctx._lib.pm_plonk_fill_gadgets_dev(self.ctx._h, self._h, d_ptr, stride, B, raws, None))
        return [GadgetReport._from_raw(raws[b]) for b in range(B)]

    def fill_gadgets(self, variables):
        """Fill the variables the key's gadgets define from their inputs, on the device (``set_gadgets`` first).  variables:
        host [num_vars, 4] Montgomery limbs -> the filled array; a list of B of them -> [B, num_vars, 4]; a DeviceVector of
        B x num_vars elements -> the same vector, filled in place.  Only the inputs need real values: gadget inputs, the
        start points of fixed-base gadgets and what the arithmetic gates use.  -> (filled, [GadgetReport] x B); a failing
        gadget has written the values of its input cut to the width it has."""
        ctx, nv = self.ctx, self.num_vars
        if self.wire_vars is None:
            raise ValueError("the key was not built from wire variables")
        if isinstance(variables, DeviceVector):
            if nv == 0 or variables.n == 0 or variables.n % nv:
                raise ValueError("device variables must hold a positive multiple of num_vars elements")
            return variables, self._fill_device(variables._p, variables.n // nv, nv)
        single = not isinstance(variables, (list, tuple))
        a = np.stack([np.asarray(v, dtype=np.uint64).reshape(nv, 4) for v in ([variables] if single else variables)])
        B = a.shape[0]
        d_vars = DeviceVector.from_host(ctx, np.ascontiguousarray(a).reshape(B * nv, 4))
        try:
            reports = self._fill_device(d_vars._p, B, nv)
            out = d_vars.to_host().reshape(B, nv, 4)
        finally:
            d_vars.free()
        return (out[0] if single else out), reports

    def witness_from_variables(self, variables, fill: bool = False) -> DeviceVector:
        """Expand variable assignments into witnesses on the device (``pm_plonk_witness_from_vars_dev``; a key built from
        ``wire_vars``).  variables: host [num_vars, 4] Montgomery limbs, a list of B of them, or a DeviceVector of
        B x num_vars elements.  -> a DeviceVector of B x 4n elements, proof-major: w[b][j n + i] = variables[b][wire_vars[j, i]],
        zero at ``PLONK_NO_VAR`` positions.  Values are copied as they are.  fill: run the key's gadgets on the assignments
        first (``fill_gadgets``; a DeviceVector is filled in place) and raise :class:`GadgetInputError` when an input does
        not fit."""
        ctx, n = self.ctx, self.n
        if self.wire_vars is None:
            raise ValueError("the key was not built from wire variables")
        nv = self.num_vars
        if isinstance(variables, DeviceVector):
            if nv == 0 or variables.n == 0 or variables.n % nv:
                raise ValueError("device variables must hold a positive multiple of num_vars elements")
            d_vars, own, B = variables, False, variables.n // nv
        else:
            if isinstance(variables, (list, tuple)):
                a = np.stack([np.asarray(v, dtype=np.uint64).reshape(nv, 4) for v in variables]) if len(variables) else None
            else:
                a = np.asarray(variables, dtype=np.uint64).reshape(1, nv, 4)
            if a is None:
                raise ValueError("empty batch")
            B = a.shape[0]
            d_vars, own = DeviceVector.from_host(ctx, np.ascontiguousarray(a).reshape(B * nv, 4)), True
        out = None
        try:
            if fill:
                bad = {b: r for b, r in enumerate(self._fill_device(d_vars._p, B, nv)) if not r.ok}
                if bad:
                    raise GadgetInputError(bad, self.gadgets)
            out = DeviceVector(ctx, B * 4 * n)
            ctx._check(ctx._lib.pm_plonk_witness_from_vars_dev(ctx._h, self._h, d_vars._p, nv, B, out._p, None))
        except Exception:
            if out is not None:
                out.free()
            raise
        finally:
            if own:
                d_vars.free()               # pm_dev_free waits for the context's stream: the gather has read it
        return out

    def commit(self, ck, label: bytes = b"plonk") -> dict:
        """``Prover::preprocess``'s second half: commit to the 15 polynomials of the key (the verifier
        key's G1 part) and seed the transcript every proof starts from.  -> {name: affine [12]}."""
        ctx = self.ctx
        vk = _lib.VK_POINTS()
        if hasattr(ck, "lo"):                   # dist.ShardedCommitKey
            cb = None if ck.native else _exchange_callback(ck)      # None: the library's RCCL communicator
            ctx._check(ctx._lib.pm_plonk_key_commit_sharded(ctx._h, self._h, ck._bases._h, ck.lo,
                                                            C.cast(cb, C.c_void_p) if cb else None, None, label,
                                                            C.byref(vk)))
        else:
            ctx._check(ctx._lib.pm_plonk_key_commit(ctx._h, self._h, ck._bases._h, label, C.byref(vk)))
        self.verifier_key = {nm: np.array(vk[i], dtype=np.uint64) for i, nm in enumerate(VK_NAMES)}
        self.label = label
        return self.verifier_key

    def use_lagrange(self, ck, lck):
        """Commit the wires of round 1 from the witness over the Lagrange-form key ``lck`` (``CommitKey.lagrange``),
        checked once against ``ck``; ``prove`` must then be given the same ``ck``.  The proofs do not change.
        ``lck=None`` detaches.  The key keeps a reference to ``lck`` while it is attached."""
        ctx = self.ctx
        ctx._check(ctx._lib.pm_plonk_key_set_lagrange(ctx._h, self._h, ck._bases._h if ck is not None else None,
                                                      lck._bases._h if lck is not None else None))
        self._lagrange = lck

    def enable_zk(self) -> int:
        """Make the key ready for zero-knowledge proofs (``prove(..., zero_knowledge=True)``): the selector, sigma and L_1
        polynomials on a second 4n coset and a padded per-proof workspace (``pm_plonk_key_enable_zk``; the key must be
        committed).  Idempotent.  -> the device bytes the zero-knowledge state holds (the same on every call)."""
        if self.verifier_key is None:
            raise ValueError("commit the key first")
        out = C.c_size_t()
        self.ctx._check(self.ctx._lib.pm_plonk_key_enable_zk(self.ctx._h, self._h, C.byref(out)))
        return int(out.value)

    def enable_check(self) -> int:
        """Make the key ready for ``check_witness`` (``pm_plonk_key_enable_check``; needs no commit key): the non-trivial
        selectors on H, the permutation as wire positions and the check's own scratch.  Idempotent.  -> the device bytes the
        check state holds."""
        out = C.c_size_t()
        idx = None if self.wire_vars is not None else self.sigma_index.ctypes.data_as(C.POINTER(C.c_int64))   # NULL: the key's own
        self.ctx._check(self.ctx._lib.pm_plonk_key_enable_check(self.ctx._h, self._h, idx, C.byref(out)))
        self._check_enabled = True
        return int(out.value)

    def _check_device(self, d_ptr, B: int, pairs, masks: bool) -> list:
        """``pm_plonk_check_witness_batch`` on B proof-major witnesses in device memory; pairs: B (positions, values)."""
        ctx, n = self.ctx, self.n
        p_pos, p_val, counts = (_lib.u64p * B)(), (_lib.u64p * B)(), (C.c_size_t * B)()
        for b, (pos, val) in enumerate(pairs):
            counts[b] = pos.size
            if pos.size:
                p_pos[b], p_val[b] = pos.ctypes.data_as(_lib.u64p), val.ctypes.data_as(_lib.u64p)
        raws = (_lib.WitnessReport * B)()
        rows = np.zeros((B, n), np.uint8) if masks else None
        ctx._check(ctx._lib.pm_plonk_check_witness_batch(ctx._h, self._h, B, d_ptr, p_pos, p_val, counts, raws,
                                                         rows.ctypes.data_as(C.POINTER(C.c_uint8)) if masks else None))
        return [WitnessReport._from_raw(raws[b], rows[b] if masks else None) for b in range(B)]

    def check_witness(self, witness=None, public_inputs=None, masks: bool = False, variables=None,
                      fill: bool = False) -> WitnessReport:
        """Does the witness satisfy the circuit?  One ``pm_plonk_check_witness`` call (``enable_check`` first): every gate
        identity and copy constraint on every row, on the GPU.  witness (or variables) and
        public_inputs as for ``prove``; masks: also return every row's mask (``WitnessReport.row_masks``); fill (with
        variables): fill the key's gadgets on the device first, as ``prove`` does."""
        ctx, n = self.ctx, self.n
        _one_form(witness, variables, "witness")
        _fill_needs_variables(fill, variables)
        if variables is not None:
            d_wit, own = _single(self.witness_from_variables(variables, fill), n), True
        elif isinstance(witness, DeviceVector):
            if witness.n != 4 * n:
                raise ValueError("device witness must hold 4n elements")
            d_wit, own = witness, False
        else:
            d_wit, own = DeviceVector.from_host(ctx, np.ascontiguousarray(witness, dtype=np.uint64).reshape(4 * n, 4)), True
        pos, val = _pi_pairs(public_inputs)
        raw = _lib.WitnessReport()
        rows = np.zeros(n, np.uint8) if masks else None
        try:
            ctx._check(ctx._lib.pm_plonk_check_witness(ctx._h, self._h, d_wit._p, pos.ctypes.data_as(_lib.u64p) if pos.size else None,
                                                       val.ctypes.data_as(_lib.u64p) if pos.size else None, pos.size, C.byref(raw),
                                                       rows.ctypes.data_as(C.POINTER(C.c_uint8)) if masks else None))
        finally:
            if own:
                d_wit.free()
        return WitnessReport._from_raw(raw, rows)

    def check_witnesses(self, witnesses=None, public_inputs=None, masks: bool = False, variables=None,
                        fill: bool = False) -> list:
        """``check_witness`` for B witnesses of the circuit in one ``pm_plonk_check_witness_batch`` call (B <= 64).  witnesses:
        one DeviceVector of B x 4n elements (proof-major) or a list of host arrays [4, n, 4]; or variables: what
        ``witness_from_variables`` takes; public_inputs: None or a list of B entries as for ``prove``.  -> one report per
        witness, each equal to the single call's.  fill (with variables): fill the key's gadgets on the device first."""
        ctx, n = self.ctx, self.n
        _one_form(witnesses, variables, "witnesses")
        _fill_needs_variables(fill, variables)
        if variables is not None:
            d_wit, own = self.witness_from_variables(variables, fill), True
            B = d_wit.n // (4 * n)
        elif isinstance(witnesses, DeviceVector):
            if witnesses.n % (4 * n) or witnesses.n == 0:
                raise ValueError("a batch of device witnesses must hold a positive multiple of 4n elements")
            d_wit, own, B = witnesses, False, witnesses.n // (4 * n)
        else:
            a = np.ascontiguousarray(np.stack([np.asarray(w, dtype=np.uint64).reshape(4 * n, 4) for w in witnesses]))
            B = a.shape[0]
            d_wit, own = DeviceVector.from_host(ctx, a.reshape(B * 4 * n, 4)), True
        try:
            if public_inputs is None:
                public_inputs = [None] * B
            if len(public_inputs) != B:
                raise ValueError("one public-input entry per witness")
            return self._check_device(d_wit._p, B, [_pi_pairs(p) for p in public_inputs], masks)
        finally:
            if own:
                d_wit.free()

    def batch(self, max_batch: int, zero_knowledge: bool = False) -> "BatchWorkspace":
        """A workspace for ``prove_batch`` of up to ``max_batch`` (<= 64) proofs on this key: about 42 n x 32 bytes of
        device memory per proof, held until ``free()``.  It is separate from the key's own workspace.
        zero_knowledge: make the key (``enable_zk``) and the workspace (``BatchWorkspace.enable_zk``, about 51 n x 32 bytes
        more per proof) ready for ``prove_batch(..., zero_knowledge=True)``."""
        if zero_knowledge:
            self.enable_zk()
        ws = BatchWorkspace(self, max_batch)
        if zero_knowledge:
            try:
                ws.enable_zk()
            except Exception:
                ws.free()
                raise
        return ws

    def free(self):
        if getattr(self, "_h", None) and self.ctx._h:
            self.ctx._lib.pm_plonk_key_free(self.ctx._h, self._h)
        self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class BatchWorkspace:
    """``pm_plonk_batch``: the per-proof polynomials of up to ``max_batch`` proofs on one key (``ProverKey.batch``), and the
    staging into which ``prove_batch`` copies a list of per-proof witnesses."""

    def __init__(self, pk: ProverKey, max_batch: int):
        self.pk, self.ctx, self.max_batch = pk, pk.ctx, int(max_batch)
        h = C.c_void_p()
        self.ctx._check(self.ctx._lib.pm_plonk_batch_create(self.ctx._h, pk._h, self.max_batch, C.byref(h)))
        self._h = h
        self._staging: DeviceVector | None = None

    def device_bytes(self) -> int:
        """Device bytes the workspace holds (``pm_plonk_batch_bytes``; the witness staging not included)."""
        return int(self.ctx._lib.pm_plonk_batch_bytes(self._h))

    def enable_zk(self) -> int:
        """Add the padded-stride regions of zero-knowledge batches (``pm_plonk_batch_enable_zk``; the key must have had
        ``ProverKey.enable_zk``).  Idempotent; plain batches on the workspace are unchanged.  -> the device bytes added (the
        same on every call; ``device_bytes`` keeps counting the plain regions only)."""
        out = C.c_size_t()
        self.ctx._check(self.ctx._lib.pm_plonk_batch_enable_zk(self.ctx._h, self._h, C.byref(out)))
        return int(out.value)

    def zk_device_bytes(self) -> int:
        """Device bytes ``enable_zk`` added (``pm_plonk_batch_zk_bytes``; 0 before it)."""
        return int(self.ctx._lib.pm_plonk_batch_zk_bytes(self._h))

    def staging(self) -> DeviceVector:
        """max_batch x 4n elements of device memory for proof-major witnesses, allocated on first use."""
        if self._staging is None:
            self._staging = DeviceVector(self.ctx, self.max_batch * 4 * self.pk.n)
        return self._staging

    def free(self):
        if getattr(self, "_staging", None) is not None:
            self._staging.free()
            self._staging = None
        if getattr(self, "_h", None) and self.ctx._h:
            self.ctx._lib.pm_plonk_batch_free(self.ctx._h, self._h)
        self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class DistProverKey:
    """``pm_dist_key``: this rank's share of a prover key with coefficient-range ownership end to end (rows /
    coefficients [rank n / world, (rank + 1) n / world) of every vector; SURVEY.md section 8f N5, configs[4]).
    ``circuit`` is the WHOLE circuit here (the slices are cut from it; a host that never holds the whole circuit
    passes slices to ``pm_plonk_preprocess_dist`` directly); ``group`` a ``dist.DistGroup``."""

    def __init__(self, circuit: Circuit, ctx: Context, group):
        self.ctx, self.n, self.group = ctx, circuit.n, group
        if circuit.sigma_index is None:
            raise ValueError("the distributed key takes sigma_index: build it with sigma_from_wires and pass that")
        W, r = group.world, group.rank
        if self.n % W:
            raise ValueError("the ranks must divide the circuit size")
        m = self.n // W
        self.m, self.lo = m, r * m
        keep = []
        ptrs = (_lib.u64p * len(SELECTORS))()
        for i, s in enumerate(SELECTORS):
            a = getattr(circuit, s)
            if a is not None:
                a = np.ascontiguousarray(np.asarray(a, dtype=np.uint64).reshape(-1, 4)[self.lo:self.lo + m])
                keep.append(a)
                ptrs[i] = a.ctypes.data_as(_lib.u64p)
        idx = np.ascontiguousarray(np.asarray(circuit.sigma_index, dtype=np.int64).reshape(4, self.n)[:, self.lo:self.lo + m])
        h = C.c_void_p()
        ctx._check(ctx._lib.pm_plonk_preprocess_dist(ctx._h, C.byref(group.desc), ptrs, idx.ctypes.data_as(C.POINTER(C.c_int64)),
                                                     self.n, C.byref(h)))
        self._h = h
        self.verifier_key: dict | None = None

    @property
    def device_bytes(self) -> int:
        return int(self.ctx._lib.pm_plonk_dist_key_bytes(self._h))

    def commit(self, bases_slice, label: bytes = b"plonk") -> dict:
        """bases_slice: ``host.Bases`` holding powers [rank m, (rank + 1) m) of the commit key."""
        vk = _lib.VK_POINTS()
        self.ctx._check(self.ctx._lib.pm_plonk_key_commit_dist(self.ctx._h, C.byref(self.group.desc), self._h, bases_slice._h,
                                                               label, C.byref(vk)))
        self.verifier_key = {nm: np.array(vk[i], dtype=np.uint64) for i, nm in enumerate(VK_NAMES)}
        return self.verifier_key

    def prove(self, bases_slice, witness, public_inputs=None, bind_public_inputs: bool = True) -> "Proof":
        """witness: the WHOLE [4, n, 4] wire values (this rank uploads its [4, m] slices) or a DeviceVector of this
        rank's 4m elements; public inputs as for ``prove`` (global positions)."""
        ctx, m = self.ctx, self.m
        if isinstance(witness, DeviceVector):
            d_wit, own = witness, False
        else:
            w = np.asarray(witness, dtype=np.uint64).reshape(4, self.n, 4)[:, self.lo:self.lo + m]
            d_wit, own = DeviceVector.from_host(ctx, np.ascontiguousarray(w).reshape(4 * m, 4)), True
        if isinstance(public_inputs, tuple):
            pos = np.ascontiguousarray(public_inputs[0], dtype=np.uint64).reshape(-1)
            val = np.ascontiguousarray(public_inputs[1], dtype=np.uint64).reshape(-1, 4)
        else:
            pos, val = sparse_public_inputs(public_inputs)
        raw = _lib.PlonkProof()
        flags = 0 if bind_public_inputs else _lib.PLONK_UPSTREAM_TRANSCRIPT
        try:
            ctx._check(ctx._lib.pm_plonk_prove_dist(ctx._h, C.byref(self.group.desc), self._h, bases_slice._h, d_wit._p,
                                                    pos.ctypes.data_as(_lib.u64p) if pos.size else None,
                                                    val.ctypes.data_as(_lib.u64p) if pos.size else None, pos.size, flags,
                                                    C.byref(raw)))
        finally:
            if own:
                d_wit.free()
        return _proof_from_raw(ctx, raw)

    def free(self):
        if getattr(self, "_h", None) and self.ctx._h:
            self.ctx._lib.pm_plonk_dist_key_free(self.ctx._h, self._h)
        self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def _wire_vars(wire_vars, n: int | None = None) -> np.ndarray:
    wv = np.asarray(wire_vars)
    if wv.ndim != 2 or wv.shape[0] != 4 or (n is not None and wv.shape[1] != n):
        raise ValueError("wire_vars must have the shape [4, n]")
    if wv.dtype != np.uint32 and wv.size and (wv.min() < 0 or wv.max() > _lib.PLONK_NO_VAR):
        raise ValueError("wire_vars holds 32-bit ids")
    return np.ascontiguousarray(wv, dtype=np.uint32)


def sigma_from_wires(wire_vars, num_vars: int, ctx: Context | None = None) -> np.ndarray:
    """The copy permutation of a circuit given as wire variables (``pm_plonk_sigma_from_wires``, built on the GPU):
    wire_vars [4, n] ids below num_vars or ``PLONK_NO_VAR`` -> sigma_index [4, n] int64 in which the positions of each
    variable, ordered by gate and then wire, form one cycle (dusk's order).  ctx None: a context on device 0 for the call."""
    wv = _wire_vars(wire_vars)
    own = ctx is None
    if own:
        ctx = Context(0)
    out = np.empty(wv.shape, np.int64)
    try:
        ctx._check(ctx._lib.pm_plonk_sigma_from_wires(ctx._h, wv.ctypes.data_as(_lib.u32p), int(num_vars), wv.shape[1],
                                                      out.ctypes.data_as(C.POINTER(C.c_int64))))
    finally:
        if own:
            ctx.close()
    return out


def _one_form(witness, variables, name: str):
    if (witness is None) == (variables is None):
        raise ValueError(f"give exactly one of {name} and variables")


def _fill_needs_variables(fill: bool, variables):
    if fill and variables is None:
        raise ValueError("fill=True works on variables")


def _single(d_wit: DeviceVector, n: int) -> DeviceVector:
    if d_wit.n != 4 * n:
        d_wit.free()
        raise ValueError("variables must hold one assignment")
    return d_wit


def _proof_from_raw(ctx: Context, raw) -> "Proof":
    proof = Proof()
    for i, name in enumerate(Proof.COMMITMENTS):
        proof.commitments[name] = np.array(raw.commitments[i], dtype=np.uint64)
    for i, name in enumerate(Proof.TRANSCRIPT_EVALS):
        proof.evaluations[name] = np.array(raw.evaluations[i], dtype=np.uint64)
    for i, name in enumerate(CHALLENGES):
        proof.challenges[name] = fr_from_limbs(np.array(raw.challenges[i], dtype=np.uint64))
    buf = (C.c_uint8 * _lib.PLONK_PROOF_BYTES)()
    ctx._check(ctx._lib.pm_plonk_proof_to_bytes(C.byref(raw), buf))
    proof.native_bytes = bytes(buf)
    return proof


def preprocess(circuit: Circuit, ctx: Context, ck=None, label: bytes = b"plonk") -> ProverKey:
    """``Prover::preprocess``.  With a commit key the verifier key is committed and the transcript seeded
    right away; otherwise ``prove`` does it with its commit key before the first proof."""
    pk = ProverKey(circuit, ctx)
    if ck is not None:
        pk.commit(ck, label)
    return pk


def _exchange_callback(ck):
    """pm_exchange_fn over the key's transport (torch.distributed, or the threads of a LocalGroup): all-gather the k partial points, fold with the group law.
    k = 0 marks a rank that failed locally: the marker is exchanged so that no rank blocks."""
    def exchange(_user, xyz, k):
        try:
            if k == 0:
                ck.gather_fold(None)
                return 1
            buf = np.ctypeslib.as_array(xyz, shape=(k, 18))
            res = ck.gather_fold(buf.copy())
            if res is None:          # a peer gave up
                return 1
            buf[:] = res
            return 0
        except Exception:            # never unwind through the C frames
            return 1
    return _lib.EXCHANGE_FN(exchange)


def sparse_public_inputs(public_inputs) -> tuple[np.ndarray, np.ndarray]:
    """Dense PI evaluations on H ([n, 4] limbs or None) -> (positions [k], values [k, 4]) of the non-zero ones."""
    if public_inputs is None:
        return np.zeros(0, np.uint64), np.zeros((0, 4), np.uint64)
    pi = np.ascontiguousarray(public_inputs, dtype=np.uint64).reshape(-1, 4)
    pos = np.flatnonzero(pi.any(axis=1)).astype(np.uint64)
    return pos, np.ascontiguousarray(pi[pos.astype(np.int64)])


def random_blinders(count: int | None = None) -> np.ndarray:
    """PM_PLONK_ZK_BLINDERS fresh uniform scalars below r (``secrets.randbelow``), [17, 4] Montgomery limbs; with a
    ``count``, that many independent sets ([count, 17, 4]: one per proof of a batch)."""
    if count is None:
        return np.stack([fr_to_limbs(secrets.randbelow(R_MOD)) for _ in range(_lib.PLONK_ZK_BLINDERS)])
    if count < 0:
        raise ValueError("count must not be negative")
    return np.stack([random_blinders() for _ in range(count)]) if count else np.zeros((0, _lib.PLONK_ZK_BLINDERS, 4), np.uint64)


def prove(pk: ProverKey, ck: CommitKey, witness=None, public_inputs=None, bind_public_inputs: bool = True,
          zero_knowledge: bool = False, blinders=None, check: bool = False, variables=None, fill: bool = False) -> Proof:
    """``Prover::prove_with_preprocessed``: one ``pm_plonk_prove`` call.

    check: run ``ProverKey.check_witness`` first (the key is made ready on first use) and raise
    :class:`UnsatisfiedWitness`, which names the lowest failing row and why, instead of proving a witness that does not
    satisfy the circuit.  The proof of a satisfied witness is the same bytes with and without it.

    witness: [4, n, 4] wire values (a, b, c, d rows) in Montgomery limbs, or a DeviceVector of 4n elements
    already in HBM.  variables (instead of witness, on a key built from ``wire_vars``): one assignment per variable,
    [num_vars, 4] or a DeviceVector, expanded on the device (``ProverKey.witness_from_variables``).  fill (with
    variables, ``ProverKey.set_gadgets`` first): only the inputs of the variables need values; the gadgets' internal
    variables are computed on the device between the upload and the expansion (``ProverKey.fill_gadgets``), and
    :class:`GadgetInputError` names proof, gadget and reason when an input does not fit.  public_inputs:
    dense [n, 4] evaluations of PI on H, or a (positions, values) pair, or None.
    bind_public_inputs: absorb the public inputs into the transcript before round 1 (dusk-plonk 0.8.2 does
    not; False reproduces the restated upstream transcript).

    Multi-GPU: every rank calls prove() with the same inputs and a ``dist.ShardedCommitKey``; the polynomial
    work is replicated, each MSM is split by coefficient range, and the ranks exchange 144-byte partial points.
    All ranks return the same proof.

    zero_knowledge: one ``pm_plonk_prove_zk`` call instead (single GPU; ``pk.enable_zk()`` first): the same proof format,
    transcript and verifier, with the wires, z and the quotient pieces blinded so that the proof hides the witness
    (DESIGN.md section 7.2b).  The commit key needs n + 10 points.  blinders: [17, 4] Montgomery limbs, each below r;
    None draws fresh ones with ``secrets.randbelow(r)`` -- pass fixed blinders in tests only: reusing blinders across
    proofs of different witnesses gives the witness away."""
    ctx, n = pk.ctx, pk.n
    _one_form(witness, variables, "witness")
    _fill_needs_variables(fill, variables)
    if ck.max_degree() + 1 < n:
        raise ValueError("commit key shorter than the circuit")
    if blinders is not None and not zero_knowledge:
        raise ValueError("blinders are only used with zero_knowledge=True")
    if zero_knowledge:
        if hasattr(ck, "lo"):
            raise ValueError("zero-knowledge proofs are single-GPU")
        bl = random_blinders() if blinders is None else np.ascontiguousarray(blinders, dtype=np.uint64).reshape(-1, 4)
        if bl.shape[0] != _lib.PLONK_ZK_BLINDERS:
            raise ValueError(f"need {_lib.PLONK_ZK_BLINDERS} blinders")
    if pk.verifier_key is None:
        pk.commit(ck)
    if variables is not None:
        d_wit, own = _single(pk.witness_from_variables(variables, fill), n), True
    elif isinstance(witness, DeviceVector):
        if witness.n != 4 * n:
            raise ValueError("device witness must hold 4n elements")
        d_wit, own = witness, False
    else:
        d_wit, own = DeviceVector.from_host(ctx, np.ascontiguousarray(witness, dtype=np.uint64).reshape(4 * n, 4)), True
    if isinstance(public_inputs, tuple):
        pos, val = public_inputs
        pos = np.ascontiguousarray(pos, dtype=np.uint64).reshape(-1)
        val = np.ascontiguousarray(val, dtype=np.uint64).reshape(-1, 4)
    else:
        if isinstance(public_inputs, DeviceVector):
            public_inputs = public_inputs.to_host()
        pos, val = sparse_public_inputs(public_inputs)
    raw = _lib.PlonkProof()
    flags = 0 if bind_public_inputs else _lib.PLONK_UPSTREAM_TRANSCRIPT   # binding is the library's default
    p_pos = pos.ctypes.data_as(_lib.u64p) if pos.size else None
    p_val = val.ctypes.data_as(_lib.u64p) if pos.size else None
    try:
        if check:
            if not pk._check_enabled:
                pk.enable_check()
            report = pk._check_device(d_wit._p, 1, [(pos, val)], False)[0]
            if not report.ok:
                raise UnsatisfiedWitness(report)
        if hasattr(ck, "lo"):       # dist.ShardedCommitKey: this rank's slice of the SRS, partial sums exchanged
            cb = None if ck.native else _exchange_callback(ck)      # None: the library's RCCL communicator
            ctx._check(ctx._lib.pm_plonk_prove_sharded(ctx._h, pk._h, ck._bases._h, ck.lo, d_wit._p, p_pos, p_val, pos.size,
                                                       flags, C.cast(cb, C.c_void_p) if cb else None, None, C.byref(raw)))
        elif zero_knowledge:
            ctx._check(ctx._lib.pm_plonk_prove_zk(ctx._h, pk._h, ck._bases._h, d_wit._p, p_pos, p_val, pos.size, flags,
                                                  bl.ctypes.data_as(_lib.u64p), C.byref(raw)))
        else:
            ctx._check(ctx._lib.pm_plonk_prove(ctx._h, pk._h, ck._bases._h, d_wit._p, p_pos, p_val, pos.size, flags,
                                               C.byref(raw)))
    finally:
        if own:
            d_wit.free()
    return _proof_from_raw(ctx, raw)


def _pi_pairs(public_inputs) -> tuple[np.ndarray, np.ndarray]:
    if isinstance(public_inputs, tuple):
        pos, val = public_inputs
        return (np.ascontiguousarray(pos, dtype=np.uint64).reshape(-1),
                np.ascontiguousarray(val, dtype=np.uint64).reshape(-1, 4))
    if isinstance(public_inputs, DeviceVector):
        public_inputs = public_inputs.to_host()
    return sparse_public_inputs(public_inputs)


def prove_batch(pk: ProverKey, ck: CommitKey, witnesses=None, public_inputs=None, bind_public_inputs: bool = True,
                workspace: BatchWorkspace | None = None, zero_knowledge: bool = False, blinders=None,
                check: bool = False, variables=None, fill: bool = False) -> list[Proof]:
    """B proofs of one circuit in one ``pm_plonk_prove_batch`` call; proof b equals ``prove(pk, ck, witness b, public
    inputs b)`` byte for byte.

    zero_knowledge: one ``pm_plonk_prove_batch_zk`` call instead (single GPU): every proof blinded as by
    ``prove(..., zero_knowledge=True)``, proof b byte for byte the single zero-knowledge proof of
    witness b, public inputs b and blinders b.  The key must be committed; it and the workspace are made ready
    (``ProverKey.enable_zk``, ``BatchWorkspace.enable_zk``) when they are not, and the commit key needs n + 10 points.
    blinders: [B, 17, 4] Montgomery limbs, each below r; None draws B independent sets with ``secrets.randbelow(r)``, never
    one set for the batch -- pass fixed blinders in tests only: reusing blinders across proofs of different witnesses gives
    the witness away.

    witnesses: one DeviceVector of B x 4n elements (proof-major: proof b's [a | b | c | d] at 4 n b), or a list of B
    per-proof witnesses -- DeviceVectors of 4n elements, copied device to device into the workspace's staging (one copy
    kernel per proof, 4n x 64 bytes of traffic each), or host arrays [4, n, 4], uploaded there.  variables (instead of
    witnesses, on a key built from ``wire_vars``): a list of B assignments [num_vars, 4] or a DeviceVector of B x num_vars
    elements, expanded on the device (``ProverKey.witness_from_variables``); fill: as for ``prove``, one fill for the
    batch.  public_inputs: None, or a
    list of B entries in any form ``prove`` takes (None, dense [n, 4], a (positions, values) pair).  workspace: a
    ``ProverKey.batch`` workspace with max_batch >= B; None makes one for the call.

    check: run ``ProverKey.check_witnesses`` on the batch first and raise :class:`UnsatisfiedWitness` with the reports of the
    failing members (``.reports``: {b: report}) instead of proving; satisfied batches give the same bytes as without it."""
    ctx, n = pk.ctx, pk.n
    _one_form(witnesses, variables, "witnesses")
    _fill_needs_variables(fill, variables)
    if ck.max_degree() + 1 < n:
        raise ValueError("commit key shorter than the circuit")
    if blinders is not None and not zero_knowledge:
        raise ValueError("blinders are only used with zero_knowledge=True")
    if zero_knowledge:
        if hasattr(ck, "lo"):
            raise ValueError("zero-knowledge proofs are single-GPU")
        if pk.verifier_key is None:
            raise ValueError("commit the key first")
    if pk.verifier_key is None:
        pk.commit(ck)
    expanded = None
    if variables is not None:
        if not isinstance(variables, DeviceVector):
            variables = list(variables)
            if not variables:
                raise ValueError("empty batch")
        witnesses = expanded = pk.witness_from_variables(variables, fill)
    if isinstance(witnesses, DeviceVector):
        if witnesses.n % (4 * n) or witnesses.n == 0:
            raise ValueError("a batch of device witnesses must hold a positive multiple of 4n elements")
        B = witnesses.n // (4 * n)
    else:
        witnesses = list(witnesses)
        B = len(witnesses)
    if B == 0:
        raise ValueError("empty batch")
    if zero_knowledge:
        if blinders is None:
            bl = random_blinders(B)
        else:
            bl = np.ascontiguousarray(blinders, dtype=np.uint64)
            if bl.shape != (B, _lib.PLONK_ZK_BLINDERS, 4):
                raise ValueError(f"blinders must have the shape [{B}, {_lib.PLONK_ZK_BLINDERS}, 4]: one set per proof")
    own_ws = workspace is None
    ws = pk.batch(B, zero_knowledge=zero_knowledge) if own_ws else workspace
    try:
        if zero_knowledge and not own_ws:
            pk.enable_zk()
            ws.enable_zk()
        if isinstance(witnesses, DeviceVector):
            d_wit = witnesses
        else:
            d_wit = ws.staging()
            if B > ws.max_batch:
                raise ValueError("more witnesses than the workspace's max_batch")
            one = fr_to_limbs(1).astype(np.uint64)
            vecs = (C.c_void_p * 1)()
            for b, w in enumerate(witnesses):
                dst = d_wit.view(4 * n * b, 4 * n)
                if isinstance(w, DeviceVector):
                    if w.n != 4 * n:
                        raise ValueError("each device witness must hold 4n elements")
                    vecs[0] = w.ptr
                    ctx._check(ctx._lib.pm_fr_lincomb_dev(ctx._h, 1, vecs, one.ctypes.data_as(_lib.u64p), 4 * n,
                                                          dst._p, None))   # the copy: 1 x w
                else:
                    a = np.ascontiguousarray(w, dtype=np.uint64).reshape(4 * n, 4)
                    ctx._check(ctx._lib.pm_dev_upload(ctx._h, dst._p, a.ctypes.data_as(C.c_void_p), 4 * n * 32))
        if public_inputs is None:
            public_inputs = [None] * B
        if len(public_inputs) != B:
            raise ValueError("one public-input entry per proof")
        pairs = [_pi_pairs(p) for p in public_inputs]
        p_pos = (_lib.u64p * B)()
        p_val = (_lib.u64p * B)()
        counts = (C.c_size_t * B)()
        for b, (pos, val) in enumerate(pairs):
            counts[b] = pos.size
            if pos.size:
                p_pos[b] = pos.ctypes.data_as(_lib.u64p)
                p_val[b] = val.ctypes.data_as(_lib.u64p)
        if check:
            if not pk._check_enabled:
                pk.enable_check()
            bad = {b: r for b, r in enumerate(pk._check_device(d_wit._p, B, pairs, False)) if not r.ok}
            if bad:
                raise UnsatisfiedWitness(reports=bad)
        raws = (_lib.PlonkProof * B)()
        flags = 0 if bind_public_inputs else _lib.PLONK_UPSTREAM_TRANSCRIPT
        if zero_knowledge:
            ctx._check(ctx._lib.pm_plonk_prove_batch_zk(ctx._h, pk._h, ws._h, ck._bases._h, B, d_wit._p, p_pos, p_val, counts,
                                                        flags, bl.ctypes.data_as(_lib.u64p), raws))
        else:
            ctx._check(ctx._lib.pm_plonk_prove_batch(ctx._h, pk._h, ws._h, ck._bases._h, B, d_wit._p, p_pos, p_val, counts,
                                                     flags, raws))
    finally:
        if own_ws:
            ws.free()
        if expanded is not None:
            expanded.free()
    return [_proof_from_raw(ctx, raws[b]) for b in range(B)]


def seeded_transcript(verifier_key: dict, n: int, label: bytes | None = None) -> Transcript:
    """``Prover::preprocess`` / ``Verifier::preprocess``: the transcript after ``VerifierKey::seed_transcript``."""
    L = transcript_labels()
    ts = Transcript(label if label is not None else L["protocol"])
    for i, nm in enumerate(_SEED_ORDER):
        ts.append_commitment(L[f"selector_{i}"], verifier_key[nm])
    for j in range(4):
        ts.append_commitment(L[f"sigma_{j}"], verifier_key[f"sigma_{j + 1}"])
    ts.append_message(L["dom_sep"], L["dom_sep_value"])
    ts.append_u64(L["circuit_size"], n)
    return ts


def derive_challenges(proof: Proof, verifier_key: dict, n: int, public_inputs=None, bind_public_inputs: bool = True,
                      label: bytes | None = None, t_eval=None) -> dict:
    """The verifier's side of Fiat-Shamir: replay the transcript over the verifier key, the public inputs
    and the proof's commitments and evaluations, and return the challenges (plus "batch", the one that
    folds the two opening checks).  t_eval: the verifier's own t(z); default = the prover's.  Labels and message
    order come from the library's table (``transcript_labels``)."""
    L = transcript_labels()
    ts = seeded_transcript(verifier_key, n, label)
    if bind_public_inputs:
        pos, val = public_inputs if isinstance(public_inputs, tuple) else sparse_public_inputs(public_inputs)
        ts.append_u64(L["pi_len"], len(pos))
        for p_, v_ in zip(pos, val):
            ts.append_u64(L["pi_pos"], int(p_))
            ts.append_scalar(L["pi_value"], v_)
    for j, name in enumerate("abcd"):
        ts.append_commitment(L[f"wire_{j}"], proof.commitments[name])
    ch = {"beta": ts.challenge_scalar(L["beta"])}
    ts.append_scalar(L["beta"], fr_to_limbs(ch["beta"]))
    ch["gamma"] = ts.challenge_scalar(L["gamma"])
    ts.append_commitment(L["perm"], proof.commitments["z"])
    ch["alpha"] = ts.challenge_scalar(L["alpha"])
    ch["range_sep"] = ts.challenge_scalar(L["range_sep"])
    ch["logic_sep"] = ts.challenge_scalar(L["logic_sep"])
    ch["fixed_sep"] = ts.challenge_scalar(L["fixed_sep"])
    ch["var_sep"] = ts.challenge_scalar(L["var_sep"])
    for i in range(4):
        ts.append_commitment(L[f"quotient_{i}"], proof.commitments[f"t_{i + 1}"])
    ch["z"] = ts.challenge_scalar(L["z_challenge"])
    for i, name in enumerate(Proof.TRANSCRIPT_EVALS):
        v = proof.evaluations[name] if not (name == "t" and t_eval is not None) else fr_to_limbs(t_eval)
        ts.append_scalar(L[f"eval_{i}"], v)
    ch["aw"] = ts.challenge_scalar(L["aggregate"])
    ch["aw_shifted"] = ts.challenge_scalar(L["aggregate"])
    ts.append_commitment(L["w_z"], proof.commitments["w_z"])
    ts.append_commitment(L["w_zw"], proof.commitments["w_zw"])
    ch["batch"] = ts.challenge_scalar(L["batch"])
    return ch


def check_identity(proof: Proof, n: int, pi_eval: int = 0) -> bool:
    """The verifier's scalar equation  t(z) Z_H(z) = r(z) + PI(z) - alpha (a + beta s1 + gamma)(b + beta s2 +
    gamma)(c + beta s3 + gamma)(d + gamma) z_w - alpha^2 L_1(z)  on the proof's evaluations
    (``Proof::compute_quotient_evaluation``).  The pairing checks live in oracle/plonk_verifier_oracle.py."""
    ch, ev = proof.challenges, {k: fr_from_limbs(v) for k, v in proof.evaluations.items()}
    beta, gamma, alpha, zc = ch["beta"], ch["gamma"], ch["alpha"], ch["z"]
    zn = pow(zc, n, R_MOD)
    l1_z = (zn - 1) * pow(n * (zc - 1) % R_MOD, -1, R_MOD) % R_MOD
    rhs = (ev["r"] + pi_eval
           - alpha * (ev["a"] + beta * ev["sigma_1"] + gamma) % R_MOD * (ev["b"] + beta * ev["sigma_2"] + gamma) % R_MOD
           * (ev["c"] + beta * ev["sigma_3"] + gamma) % R_MOD * (ev["d"] + gamma) % R_MOD * ev["z_next"]
           - alpha * alpha % R_MOD * l1_z) % R_MOD
    return ev["t"] * (zn - 1) % R_MOD == rhs
