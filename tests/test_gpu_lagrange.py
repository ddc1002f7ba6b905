"""The Lagrange-form commit key on the GPU: the G1 inverse NTT (pm_g1_bases_lagrange) against the big-integer oracle, on
the structured inputs that force the group law's exceptional cases, and against an independent path (fixed-base
multiplication of L_i(tau)); commitments from evaluations; and the prover's opt-in round 1
(pm_plonk_key_set_lagrange), whose proofs must be byte-identical to today's."""
import ctypes as C
import random

import numpy as np
import pytest

from oracle import bigint_oracle as B
from oracle.cpu_oracle import ints_to_limbs
from test_lagrange_host import lagrange_oracle

pytestmark = pytest.mark.gpu
R = B.R_MOD
TAU = 0x3C6EF372FE94F82BA54FF53A5F1D36F1510E527FADE682D19B05688C2B3E6C1F % R


def _mont(oracle, v):
    return oracle.fr_to_mont(ints_to_limbs([v % R], 4))[0]


def _to_limbs(pts):
    from plonk_prototype_amd.field import fp_to_limbs
    out = np.zeros((len(pts), 12), np.uint64)
    for i, p in enumerate(pts):
        if p is not None:
            out[i, :6], out[i, 6:] = fp_to_limbs(p[0]), fp_to_limbs(p[1])
    return out


def _from_limbs(xy):
    from plonk_prototype_amd.field import fp_from_limbs
    return [None if not r.any() else (fp_from_limbs(r[:6]), fp_from_limbs(r[6:])) for r in np.asarray(xy).reshape(-1, 12)]


def _gpu_lagrange(ctx, pts, log_n):
    import plonk_prototype_amd as pa
    return pa.CommitKey(_to_limbs(pts), ctx).lagrange(log_n).points()


# ---- 1. against the oracle --------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n", [0, 1, 2, 3, 4, 5])
def test_matches_oracle_random_points(ctx, log_n):
    rng = random.Random(100 + log_n)
    n = 1 << log_n
    pts = [B.g1_mul(rng.randrange(1, R), B.G1_GEN) for _ in range(n)]
    assert _from_limbs(_gpu_lagrange(ctx, pts, log_n)) == lagrange_oracle(pts, log_n)


@pytest.mark.parametrize("log_n", [1, 2, 3, 4, 5])
def test_matches_oracle_identities_repeats_and_opposites(ctx, log_n):
    rng = random.Random(200 + log_n)
    n = 1 << log_n
    P = B.g1_mul(rng.randrange(1, R), B.G1_GEN)
    Q = B.g1_mul(rng.randrange(1, R), B.G1_GEN)
    pool = [None, P, B.g1_neg(P), Q, B.g1_neg(Q), B.g1_add(P, P)]
    pts = [pool[rng.randrange(len(pool))] for _ in range(n)]
    pts[0], pts[-1] = P, B.g1_neg(P)
    assert _from_limbs(_gpu_lagrange(ctx, pts, log_n)) == lagrange_oracle(pts, log_n)
    # a longer SRS than the domain: only the first n points count
    longer = pts + [Q] * 3
    assert _from_limbs(_gpu_lagrange(ctx, longer, log_n)) == lagrange_oracle(pts, log_n)


# ---- 2. structured inputs --------------------------------------------------------------------------------------
def test_constant_vector_goes_to_one_point(ctx):
    # sum_j w^-ij = n [i == 0]: every butterfly meets a == t or a == -t
    log_n = 10
    P = B.g1_mul(0xC0FFEE, B.G1_GEN)
    got = _from_limbs(_gpu_lagrange(ctx, [P] * (1 << log_n), log_n))
    assert got[0] == P and all(g is None for g in got[1:])


def test_single_point_spreads_everywhere(ctx):
    # the identity everywhere but slot 0: identity twiddle products in every stage
    log_n = 10
    n = 1 << log_n
    P = B.g1_mul(0xBEEF, B.G1_GEN)
    got = _from_limbs(_gpu_lagrange(ctx, [P] + [None] * (n - 1), log_n))
    assert got == [B.g1_mul(pow(n, -1, R), P)] * n


# ---- 3. against an independent path -----------------------------------------------------------------------------
def _expected_by_fixed_base(ctx, oracle, log_n, tau):
    """[L_i(tau)] G by the fixed-base multiplication of the coefficients pm_domain_evaluate_all_lagrange_coefficients_dev
    gives: no inverse NTT anywhere."""
    import plonk_prototype_amd as pa
    from plonk_prototype_amd.host import G1_GENERATOR
    n = 1 << log_n
    dom = pa.EvaluationDomain(n, ctx)
    coeffs = dom.evaluate_all_lagrange_coefficients(_mont(oracle, tau), device=True)
    out = pa.DeviceVector(ctx, 3 * n)
    try:
        ctx._check(ctx._lib.pm_g1_fixed_base_mul_dev(ctx._h, G1_GENERATOR.ctypes.data_as(C.POINTER(C.c_uint64)),
                                                     C.c_void_p(coeffs.ptr), n, 0, C.c_void_p(out.ptr), None))
        return out.to_host().reshape(n, 12)
    finally:
        out.free()
        coeffs.free()


@pytest.mark.parametrize("log_n", [10, 16, 20])
def test_srs_lagrange_key_matches_fixed_base_path(ctx, oracle, log_n):
    import plonk_prototype_amd as pa
    ck = pa.CommitKey.setup((1 << log_n) - 1, _mont(oracle, TAU), ctx)
    got = ck.lagrange(log_n).points()
    assert np.array_equal(got, _expected_by_fixed_base(ctx, oracle, log_n, TAU))


def test_prefix_of_a_longer_srs(ctx, oracle):
    import plonk_prototype_amd as pa
    ck = pa.CommitKey.setup((1 << 12) - 1, _mont(oracle, TAU), ctx, precompute=True)
    got = ck.lagrange(10).points()
    assert np.array_equal(got, _expected_by_fixed_base(ctx, oracle, 10, TAU))


# ---- 4. commitments from evaluations ----------------------------------------------------------------------------
def _witness_like(rng, n):
    """90 % below 2^16, 5 % zero, 1 % one, the rest uniform (the bench's msm.witness_like shape)."""
    v = []
    for _ in range(n):
        u = rng.random()
        v.append(0 if u < 0.05 else 1 if u < 0.06 else rng.randrange(1 << 16) if u < 0.96 else rng.randrange(R))
    return v


@pytest.mark.parametrize("precompute", [False, True])
def test_commit_from_evaluations(ctx, oracle, precompute):
    import plonk_prototype_amd as pa
    log_n = 10
    n = 1 << log_n
    rng = random.Random(7 + precompute)
    ck = pa.CommitKey.setup(n - 1, _mont(oracle, TAU), ctx, precompute=precompute)
    lck = ck.lagrange(log_n, precompute=precompute)
    assert lck.n == n
    dom = pa.EvaluationDomain(n, ctx)
    cases = [[rng.randrange(R) for _ in range(n)], _witness_like(rng, n), [rng.randrange(2) for _ in range(n)],
             [0] * n]
    for vals in cases:
        ev = oracle.fr_to_mont(ints_to_limbs(vals, 4))
        assert np.array_equal(lck.commit(ev), ck.commit(dom.ifft(ev)))
    # fewer than n values: zero padded
    for m in (1, 5, n // 2 + 3):
        ev = oracle.fr_to_mont(ints_to_limbs(_witness_like(rng, m), 4))
        full = np.zeros((n, 4), np.uint64)
        full[:m] = ev
        assert np.array_equal(lck.commit(ev), ck.commit(dom.ifft(full)))
    with pytest.raises(pa.Error) as e:
        lck.commit(np.zeros((n + 1, 4), np.uint64))
    assert e.value.code == -6
    # several at once, on the host and from device memory
    evs = np.stack([oracle.fr_to_mont(ints_to_limbs(_witness_like(rng, n), 4)) for _ in range(4)])
    want = np.stack([ck.commit(dom.ifft(e_)) for e_ in evs])
    assert np.array_equal(lck.commit_many(evs), want)
    d = pa.DeviceVector.from_host(ctx, evs.reshape(-1, 4))
    try:
        assert np.array_equal(np.stack(lck.commit_batch_dev(d.ptr, n, 4)), want)
    finally:
        d.free()


def test_save_and_load_through_srs_bytes(ctx, oracle):
    import plonk_prototype_amd as pa
    from plonk_prototype_amd import srs
    n = 1 << 8
    ck = pa.CommitKey.setup(n - 1, _mont(oracle, TAU), ctx)
    lck = ck.lagrange(8)
    loaded = srs.commit_key_from_raw_bytes(srs.commit_key_to_raw_bytes(lck.points()))
    assert np.array_equal(loaded, lck.points())
    lck2 = pa.LagrangeCommitKey.from_points(loaded, ctx)
    ev = oracle.fr_to_mont(ints_to_limbs(_witness_like(random.Random(3), n), 4))
    assert np.array_equal(lck2.commit(ev), lck.commit(ev))


# ---- 5. proof bytes -------------------------------------------------------------------------------------------
_CK = {}


def _ck_and_lck(ctx, oracle, log_n):
    import plonk_prototype_amd as pa
    if log_n not in _CK:
        _CK.clear()
        ck = pa.CommitKey.setup((1 << log_n) - 1, _mont(oracle, TAU), ctx, precompute=log_n >= 10)
        _CK[log_n] = (ck, ck.lagrange(log_n))
    return _CK[log_n]


def _check_same_proofs(ctx, oracle, circuit, wit, pub, ck, lck, binds=(True, False)):
    import plonk_prototype_amd.prover as PR
    pk = PR.preprocess(circuit, ctx, ck)
    vk0 = {k: v.copy() for k, v in pk.verifier_key.items()}
    plain = [PR.prove(pk, ck, wit, pub, bind_public_inputs=b).native_bytes for b in binds]
    pk.use_lagrange(ck, lck)
    assert [PR.prove(pk, ck, wit, pub, bind_public_inputs=b).native_bytes for b in binds] == plain
    raw = PR._lib.VK_POINTS()
    ctx._check(ctx._lib.pm_plonk_verifier_key(pk._h, C.byref(raw)))
    assert all(np.array_equal(np.array(raw[i], np.uint64), vk0[nm]) for i, nm in enumerate(PR.VK_NAMES))
    pk.use_lagrange(ck, None)
    assert [PR.prove(pk, ck, wit, pub, bind_public_inputs=b).native_bytes for b in binds] == plain
    pk.free()
    return plain


@pytest.mark.parametrize("log_n", list(range(2, 17)))
def test_proofs_unchanged_all_circuits(ctx, oracle, log_n):
    import plonk_prototype_amd as pa
    ck, lck = _ck_and_lck(ctx, oracle, log_n)
    n = 1 << log_n
    for make, smallest in ((pa.synthetic.chain_circuit, 4), (pa.synthetic.mixed_circuit, 32),
                           (pa.synthetic.boolean_circuit, 8)):
        if n >= smallest:
            _check_same_proofs(ctx, oracle, *make(n, 11 + log_n), ck, lck)


def test_boolean_proof_2_20_unchanged(ctx, oracle):
    import plonk_prototype_amd as pa
    ck, lck = _ck_and_lck(ctx, oracle, 20)
    _check_same_proofs(ctx, oracle, *pa.synthetic.boolean_circuit(1 << 20, 5), ck, lck, binds=(True,))
    _CK.clear()


def test_lagrange_proof_passes_the_pairing_verifier(ctx, oracle):
    import plonk_prototype_amd as pa
    import plonk_prototype_amd.prover as PR
    from oracle import pairing_oracle as PG
    from oracle import plonk_verifier_oracle as PV
    from oracle.cpu_oracle import limbs_to_ints
    n = 16
    circuit, wit, pub = pa.synthetic.chain_circuit(n, 91)
    ck = pa.CommitKey.setup(n - 1, _mont(oracle, TAU), ctx)
    lck = ck.lagrange(4)
    pk = PR.preprocess(circuit, ctx, ck)
    pk.use_lagrange(ck, lck)
    proof = PR.Proof.from_bytes(PR.prove(pk, ck, wit, pub).native_bytes)

    def pt(xy):
        if not np.asarray(xy).any():
            return None
        v = limbs_to_ints(oracle.fp_from_mont(np.ascontiguousarray(xy).reshape(2, 6)))
        return (v[0], v[1])

    def fr(v):
        return limbs_to_ints(oracle.fr_from_mont(np.ascontiguousarray(v).reshape(-1, 4)))

    vk = {k: pt(v) for k, v in pk.verifier_key.items()}
    comms = {k: pt(v) for k, v in proof.commitments.items()}
    ev = {k: fr(v)[0] for k, v in proof.evaluations.items()}
    ch0 = PR.derive_challenges(proof, pk.verifier_key, n, pub, t_eval=0)
    pub_z = B.horner(B.ifft(fr(pub), 4), ch0["z"])
    t_eval = PV.quotient_evaluation(n, ev, ch0, pub_z)
    ch = PR.derive_challenges(proof, pk.verifier_key, n, pub, t_eval=t_eval)
    assert PV.verify(n, vk, comms, ev, ch, pub_z, PG.g2_mul(TAU, PG.G2_GEN)) == (True, True)


def test_sharded_prove_ignores_the_attachment(ctx, oracle):
    import plonk_prototype_amd as pa
    import plonk_prototype_amd.prover as PR
    n = 1 << 8
    circuit, wit, pub = pa.synthetic.boolean_circuit(n, 13)
    ck, lck = _ck_and_lck(ctx, oracle, 8)
    pk = PR.preprocess(circuit, ctx, ck)
    plain = PR.prove(pk, ck, wit, pub).native_bytes
    pk.use_lagrange(ck, lck)
    world_of_one = PR._lib.EXCHANGE_FN(lambda user, xyz, k: 0)
    d_wit = pa.DeviceVector.from_host(ctx, np.ascontiguousarray(wit).reshape(4 * n, 4))
    raw = PR._lib.PlonkProof()
    try:
        ctx._check(ctx._lib.pm_plonk_prove_sharded(ctx._h, pk._h, ck._bases._h, 0, C.c_void_p(d_wit.ptr), None, None, 0,
                                                   0, C.cast(world_of_one, C.c_void_p), None, C.byref(raw)))
    finally:
        d_wit.free()
    out = (C.c_uint8 * PR._lib.PLONK_PROOF_BYTES)()
    assert ctx._lib.pm_plonk_proof_to_bytes(C.byref(raw), out) == 0
    assert bytes(out) == plain
    pk.free()


# ---- 6. refusals -------------------------------------------------------------------------------------------------
def test_refusals(ctx, oracle):
    import plonk_prototype_amd as pa
    import plonk_prototype_amd.prover as PR
    n = 64
    circuit, wit, pub = pa.synthetic.boolean_circuit(n, 17)
    ck = pa.CommitKey.setup(n - 1, _mont(oracle, TAU), ctx)
    pk = PR.preprocess(circuit, ctx, ck)
    # a Lagrange key of the wrong size
    with pytest.raises(pa.Error) as e:
        pk.use_lagrange(ck, ck.lagrange(5))
    assert e.value.code == -6
    # built from another tau: caught at attach by sum L_i = powers[0] / sum w^i L_i = powers[1]
    other = pa.CommitKey.setup(n - 1, _mont(oracle, TAU + 1), ctx)
    with pytest.raises(pa.Error) as e:
        pk.use_lagrange(ck, other.lagrange(6))
    assert e.value.code == -1
    # a key of the right tau but another generator fails the check too
    other_g = pa.CommitKey.setup(n - 1, _mont(oracle, TAU), ctx, generator=_to_limbs([B.g1_mul(3, B.G1_GEN)])[0])
    with pytest.raises(pa.Error) as e:
        pk.use_lagrange(ck, other_g.lagrange(6))
    assert e.value.code == -1
    # attached against ck: proving with another commit key (same points, another handle) is refused
    lck = ck.lagrange(6)
    pk.use_lagrange(ck, lck)
    ck2 = pa.CommitKey.setup(n - 1, _mont(oracle, TAU), ctx)
    with pytest.raises(pa.Error) as e:
        PR.prove(pk, ck2, wit, pub)
    assert e.value.code == -1
    assert PR.prove(pk, ck, wit, pub).native_bytes
    pk.use_lagrange(None, None)
    assert PR.prove(pk, ck2, wit, pub).native_bytes == PR.prove(pk, ck, wit, pub).native_bytes
    # the conversion itself
    lib, h, b = ctx._lib, ctx._h, ck._bases._h
    out = pa.DeviceVector(ctx, 3 * 2 * n)
    try:
        assert lib.pm_g1_bases_lagrange(h, b, 7, C.c_void_p(out.ptr), None) == -6    # 2^7 > 64 bases
        assert lib.pm_g1_bases_lagrange(h, b, 32, C.c_void_p(out.ptr), None) == -2
        assert lib.pm_g1_bases_lagrange(h, b, 40, C.c_void_p(out.ptr), None) == -2
        assert lib.pm_g1_bases_lagrange(h, None, 3, C.c_void_p(out.ptr), None) == -1
        assert lib.pm_g1_bases_lagrange(h, b, 3, None, None) == -1
        assert lib.pm_g1_bases_lagrange(None, b, 3, C.c_void_p(out.ptr), None) == -1
    finally:
        out.free()
    assert lib.pm_plonk_key_set_lagrange(None, pk._h, b, lck._bases._h) == -1
    assert lib.pm_plonk_key_set_lagrange(h, None, b, lck._bases._h) == -1
    assert lib.pm_plonk_key_set_lagrange(h, pk._h, None, lck._bases._h) == -1
    with pytest.raises(pa.Error) as e:
        ck.lagrange(7)
    assert e.value.code == -6
    with pytest.raises(pa.Error) as e:
        ck.lagrange(32)
    assert e.value.code == -2
    pk.free()
