"""Zero-knowledge proofs on the GPU (pm_plonk_key_enable_zk / pm_plonk_prove_zk): zero blinders
reproduce pm_plonk_prove byte for byte, random blinders match the big-int restatement of tests/test_zk_host.py exactly,
the unchanged pairing verifier accepts, the proofs hide what they should, and nothing else moves."""
import ctypes as C
import random

import numpy as np
import pytest

from oracle import bigint_oracle as B
from oracle.cpu_oracle import ints_to_limbs, limbs_to_ints
from test_zk_host import BLINDERS, EXTRA_BASES, zk_prove

pytestmark = pytest.mark.gpu
R = B.R_MOD
TAU = 0x3C6EF372FE94F82BA54FF53A5F1D36F1510E527FADE682D19B05688C2B3E6C1F % R


def _mont(oracle, v):
    return oracle.fr_to_mont(ints_to_limbs([v % R], 4))[0]


def _ints(oracle, limbs):
    return limbs_to_ints(oracle.fr_from_mont(np.ascontiguousarray(limbs).reshape(-1, 4)))


def _g(oracle, k):
    return oracle.g1_mul(oracle.g1_generator(), ints_to_limbs([k % R], 4)[0])


def _pt(oracle, xy):
    if not np.asarray(xy).any():
        return None
    v = limbs_to_ints(oracle.fp_from_mont(np.ascontiguousarray(xy).reshape(2, 6)))
    return (v[0], v[1])


def _blinders(seed):
    from plonk_prototype_amd.field import fr_to_limbs
    rng = random.Random(seed)
    vals = [rng.randrange(R) for _ in range(BLINDERS)]
    return vals, np.stack([fr_to_limbs(v) for v in vals])


_ZERO = np.zeros((BLINDERS, 4), np.uint64)
_CK = {}


def _ck(ctx, oracle, n):
    """A powers-of-tau key with n + 10 points (kept per size: one setup serves every test of that size)."""
    import plonk_prototype_amd as pa
    if n not in _CK:
        _CK[n] = pa.CommitKey.setup(n + EXTRA_BASES - 1, _mont(oracle, TAU), ctx, precompute=(n >= 1 << 12))
    return _CK[n]


def _circuit(kind, n, seed):
    import plonk_prototype_amd as pa
    return getattr(pa.synthetic, kind + "_circuit")(n, seed)


def _pi_at(oracle, pub, n, z):
    """PI(z) = sum_i pi_i L_i(z), L_i(z) = (z^n - 1) / n * w^i / (z - w^i), over the non-zero public inputs."""
    vals = _ints(oracle, pub)
    w = B.Domain(n).group_gen
    zh_n = (pow(z, n, R) - 1) * pow(n, -1, R) % R
    acc = 0
    for i in np.flatnonzero(np.asarray(pub).reshape(-1, 4).any(axis=1)):
        wi = pow(w, int(i), R)
        acc += vals[int(i)] * zh_n % R * wi % R * pow((z - wi) % R, -1, R)
    return acc % R


def _verify(oracle, pk, n, proof_bytes, pub):
    """The unchanged verifier on challenges replayed from the proof bytes: (identity_ok, pairing_ok)."""
    import plonk_prototype_amd.prover as PR
    from oracle import pairing_oracle as PG
    from oracle import plonk_verifier_oracle as PV
    proof = PR.Proof.from_bytes(proof_bytes)
    vk = {k: _pt(oracle, v) for k, v in pk.verifier_key.items()}
    comms = {k: _pt(oracle, v) for k, v in proof.commitments.items()}
    ev = {k: _ints(oracle, v)[0] for k, v in proof.evaluations.items()}
    ch0 = PR.derive_challenges(proof, pk.verifier_key, n, pub, t_eval=0)
    pub_z = _pi_at(oracle, pub, n, ch0["z"])
    t_eval = PV.quotient_evaluation(n, ev, ch0, pub_z)
    ch = PR.derive_challenges(proof, pk.verifier_key, n, pub, t_eval=t_eval)
    tau_g2 = PG.g2_mul(TAU, PG.G2_GEN)
    return PV.verify(n, vk, comms, ev, ch, pub_z, tau_g2), (vk, comms, ev, ch, pub_z, tau_g2)


@pytest.mark.parametrize("kind,log_n", [("chain", k) for k in (2, 4, 5, 6, 8, 10, 12, 14, 16)]
                         + [("mixed", k) for k in (5, 6, 8, 10, 12, 16)])
def test_zero_blinders_reproduce_the_plain_proof(ctx, oracle, kind, log_n):
    """beta = 0: byte-identical to pm_plonk_prove, challenges included, in both transcript modes -- pins the two-coset
    quotient, the padded strides and the longer MSMs against the validated path."""
    import plonk_prototype_amd as pa
    import plonk_prototype_amd.prover as PR
    n = 1 << log_n
    circuit, wit, pub = _circuit(kind, n, 11 + log_n)
    ck = _ck(ctx, oracle, n)
    pk = pa.preprocess(circuit, ctx, ck)
    pk.enable_zk()
    for bind in (True, False):
        plain = PR.prove(pk, ck, wit, pub, bind_public_inputs=bind)
        zk = PR.prove(pk, ck, wit, pub, bind_public_inputs=bind, zero_knowledge=True, blinders=_ZERO)
        assert zk.native_bytes == plain.native_bytes, bind
        assert zk.challenges == plain.challenges
        for k in plain.evaluations:
            assert np.array_equal(zk.evaluations[k], plain.evaluations[k]), k
    pk.free()
    if n >= 1 << 14:
        _CK.pop(n, None)


@pytest.mark.parametrize("n,mixed", [(8, False), (16, False), (32, True)])
def test_matches_the_big_int_restatement(ctx, oracle, n, mixed):
    """Random blinders, public inputs: every commitment ([p(tau)] G through the trapdoor key) and every evaluation equals the
    test-local big-int zero-knowledge prover run under the GPU proof's own challenges."""
    import plonk_prototype_amd as pa
    import plonk_prototype_amd.prover as PR
    from test_zk_host import circuit_ints
    circuit, wit, pub, (sel, sigma, wi, pii) = circuit_ints(n, n + 5, mixed)
    assert any(pii)
    ck = _ck(ctx, oracle, n)
    pk = pa.preprocess(circuit, ctx, ck)
    pk.enable_zk()
    beta, bl = _blinders(n)
    proof = PR.prove(pk, ck, wit, pub, zero_knowledge=True, blinders=bl)
    exp = zk_prove(n, sel, sigma, wi, pii, proof.challenges, beta)
    got = {k: _ints(oracle, v)[0] for k, v in proof.evaluations.items()}
    assert got == exp["evals"]
    tau = lambda c: B.horner(c, TAU)   # noqa: E731
    want = {nm: tau(exp["wire_coeffs"][j]) for j, nm in enumerate("abcd")}
    want["z"] = tau(exp["z_coeffs"])
    for i in range(4):
        want[f"t_{i + 1}"] = tau(exp["t_pieces"][i])
    want["w_z"], want["w_zw"] = tau(exp["w_z"]), tau(exp["w_zw"])
    assert set(want) == set(proof.commitments)
    for k, v in want.items():
        assert np.array_equal(proof.commitments[k], _g(oracle, v)), k
    pk.free()


@pytest.mark.parametrize("n,kind", [(16, "chain"), (64, "mixed"), (1 << 10, "mixed"), (1 << 16, "boolean")])
def test_the_unchanged_verifier_accepts(ctx, oracle, n, kind):
    import plonk_prototype_amd as pa
    import plonk_prototype_amd.prover as PR
    from oracle import plonk_verifier_oracle as PV
    circuit, wit, pub = _circuit(kind, n, 3 + n)
    ck = _ck(ctx, oracle, n)
    pk = pa.preprocess(circuit, ctx, ck)
    pk.enable_zk()
    proof = PR.prove(pk, ck, wit, pub, zero_knowledge=True)          # fresh blinders from secrets
    ok, (vk, comms, ev, ch, pub_z, tau_g2) = _verify(oracle, pk, n, proof.native_bytes, pub)
    assert ok == (True, True)
    assert {k: ch[k] for k in proof.challenges} == proof.challenges
    if n <= 32:
        bad = dict(ev, c=(ev["c"] + 1) % R)
        assert PV.verify(n, vk, comms, bad, ch, pub_z, tau_g2)[1] is False
        bad = dict(ev, z_next=(ev["z_next"] + 1) % R)
        assert PV.verify(n, vk, comms, bad, ch, pub_z, tau_g2)[1] is False
        swapped = dict(comms, t_1=comms["t_2"], t_2=comms["t_1"])
        assert PV.verify(n, vk, swapped, ev, ch, pub_z, tau_g2)[1] is False
        swapped = dict(comms, t_3=comms["t_4"], t_4=comms["t_3"])
        assert PV.verify(n, vk, swapped, ev, ch, pub_z, tau_g2)[1] is False
    pk.free()
    if n >= 1 << 14:
        _CK.pop(n, None)


def test_hiding_observable_part(ctx, oracle):
    """Two blinder sets on one witness: every blinded commitment and every wire evaluation differs, both verify, and
    [a'] - [a] = (b_0 + b_1 tau + b_2 tau^2)(tau^n - 1) G against the plain proof."""
    import plonk_prototype_amd as pa
    import plonk_prototype_amd.prover as PR
    n = 32
    circuit, wit, pub = _circuit("mixed", n, 21)
    ck = _ck(ctx, oracle, n)
    pk = pa.preprocess(circuit, ctx, ck)
    pk.enable_zk()
    plain = PR.prove(pk, ck, wit, pub)
    (b1, l1), (b2, l2) = _blinders(1), _blinders(2)
    p1 = PR.prove(pk, ck, wit, pub, zero_knowledge=True, blinders=l1)
    p2 = PR.prove(pk, ck, wit, pub, zero_knowledge=True, blinders=l2)
    for k in ("a", "b", "c", "d", "z", "t_1", "t_2", "t_3", "t_4", "w_z", "w_zw"):
        assert not np.array_equal(p1.commitments[k], p2.commitments[k]), k
    for k in ("a", "b", "c", "d", "a_next", "b_next", "d_next", "z_next"):
        assert not np.array_equal(p1.evaluations[k], p2.evaluations[k]), k
    for p in (p1, p2):
        assert _verify(oracle, pk, n, p.native_bytes, pub)[0] == (True, True)
    for beta, p in ((b1, p1), (b2, p2)):
        blind = (beta[0] + beta[1] * TAU + beta[2] * TAU * TAU) * (pow(TAU, n, R) - 1) % R
        a_plain, a_zk = _pt(oracle, plain.commitments["a"]), _pt(oracle, p.commitments["a"])
        assert B.g1_add(a_zk, B.g1_neg(a_plain)) == _pt(oracle, _g(oracle, blind))
    pk.free()


@pytest.mark.parametrize("log_n", [12, 16])
def test_lagrange_key_gives_the_same_proof(ctx, oracle, log_n):
    import plonk_prototype_amd as pa
    import plonk_prototype_amd.prover as PR
    n = 1 << log_n
    circuit, wit, pub = _circuit("boolean", n, 5)
    ck = _ck(ctx, oracle, n)
    pk = pa.preprocess(circuit, ctx, ck)
    pk.enable_zk()
    _, bl = _blinders(log_n)
    want = PR.prove(pk, ck, wit, pub, zero_knowledge=True, blinders=bl).native_bytes
    lck = ck.lagrange(log_n)
    pk.use_lagrange(ck, lck)
    for bind in (True, False):
        got = PR.prove(pk, ck, wit, pub, bind_public_inputs=bind, zero_knowledge=True, blinders=bl).native_bytes
        if bind:
            assert got == want
        pk.use_lagrange(None, None)
        assert PR.prove(pk, ck, wit, pub, bind_public_inputs=bind, zero_knowledge=True, blinders=bl).native_bytes == got
        pk.use_lagrange(ck, lck)
    pk.free()
    if n >= 1 << 14:
        _CK.pop(n, None)


def test_2_20_gates(ctx, oracle):
    """One 2^20-gate zero-knowledge proof through the pairing verifier; enable_zk reports what it takes from the device."""
    import torch
    import plonk_prototype_amd as pa
    import plonk_prototype_amd.prover as PR
    n = 1 << 20
    circuit, wit, pub = _circuit("boolean", n, 9)
    ck = _ck(ctx, oracle, n)
    pk = pa.preprocess(circuit, ctx, ck)
    ctx.sync()
    free0 = torch.cuda.mem_get_info(0)[0]
    added = pk.enable_zk()
    ctx.sync()
    free1 = torch.cuda.mem_get_info(0)[0]
    assert added <= free0 - free1 <= added + (64 << 20)     # allocation granularity
    assert pk.enable_zk() == added                          # idempotent
    proof = PR.prove(pk, ck, wit, pub, zero_knowledge=True)
    assert _verify(oracle, pk, n, proof.native_bytes, pub)[0] == (True, True)
    pk.free()
    _CK.pop(n, None)


def test_plain_proofs_do_not_move(ctx, oracle):
    """pm_plonk_prove on a key with zero knowledge enabled gives the bytes it gave before, also between ZK proofs."""
    import plonk_prototype_amd as pa
    import plonk_prototype_amd.prover as PR
    n = 64
    circuit, wit, pub = _circuit("mixed", n, 31)
    ck = _ck(ctx, oracle, n)
    pk = pa.preprocess(circuit, ctx, ck)
    before = [PR.prove(pk, ck, wit, pub, bind_public_inputs=b).native_bytes for b in (True, False)]
    pk.enable_zk()
    for round_ in range(2):
        _, bl = _blinders(40 + round_)
        zk = PR.prove(pk, ck, wit, pub, zero_knowledge=True, blinders=bl).native_bytes
        assert zk not in before
        assert [PR.prove(pk, ck, wit, pub, bind_public_inputs=b).native_bytes for b in (True, False)] == before
    pk.free()


def test_refusals(ctx, oracle):
    import plonk_prototype_amd as pa
    import plonk_prototype_amd._lib as L
    from plonk_prototype_amd.host import DeviceVector
    n = 16
    circuit, wit, _ = _circuit("chain", n, 2)
    ck = _ck(ctx, oracle, n)
    pk = pa.preprocess(circuit, ctx, ck)
    lib = ctx._lib
    d_wit = DeviceVector.from_host(ctx, np.ascontiguousarray(wit, dtype=np.uint64).reshape(4 * n, 4))
    raw = L.PlonkProof()
    _, bl = _blinders(3)

    def zk(key=pk, commit_key=ck, blinders=bl, flags=0):
        p = blinders.ctypes.data_as(L.u64p) if blinders is not None else None
        return lib.pm_plonk_prove_zk(ctx._h, key._h, commit_key._bases._h, d_wit._p, None, None, 0, flags, p, C.byref(raw))

    assert zk() == L.PM_ERR_BAD_ARG                                      # not enabled
    assert lib.pm_plonk_key_enable_zk(ctx._h, pk._h, None) == L.PM_OK   # added_bytes may be NULL
    assert zk() == L.PM_OK
    short = pa.CommitKey.setup(n + EXTRA_BASES - 2, _mont(oracle, TAU), ctx)   # n + 9 points
    assert zk(commit_key=short) == L.PM_ERR_LENGTH
    assert zk(blinders=None) == L.PM_ERR_BAD_ARG
    big = bl.copy()
    big[5] = np.frombuffer(R.to_bytes(32, "little"), dtype=np.uint64)      # = r: not canonical
    assert zk(blinders=big) == L.PM_ERR_BAD_ARG
    assert zk(flags=L.PLONK_BIND_PUBLIC_INPUTS | L.PLONK_UPSTREAM_TRANSCRIPT) == L.PM_ERR_BAD_ARG
    # a busy key: a sharded proof on it holds the key while its exchange callback runs; the callback asks for a ZK proof
    seen = []

    def exchange(_user, xyz, k):
        seen.append(zk())
        return 0
    cb = L.EXCHANGE_FN(exchange)
    rc = lib.pm_plonk_prove_sharded(ctx._h, pk._h, ck._bases._h, 0, d_wit._p, None, None, 0, 0, C.cast(cb, C.c_void_p), None,
                                    C.byref(raw))
    assert rc == L.PM_OK and seen and all(s == L.PM_ERR_BUSY for s in seen)
    assert zk() == L.PM_OK                                                # none of the refusals left the key busy
    d_wit.free()
    del short
    pk.free()
    _CK.clear()
