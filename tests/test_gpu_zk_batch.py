"""Zero-knowledge proofs in the batch prover (pm_plonk_batch_enable_zk / pm_plonk_prove_batch_zk):
proof b of a blinded batch is byte-identical -- challenges included -- to pm_plonk_prove_zk of witness b, public inputs b
and blinders b.  That identity ties the batch to the path tests/test_gpu_zk.py pins against the big-int restatement and the
pairing verifier; both are checked here per slot as well, with the workspace's reuse, its size and every refusal.  Every
comparison is exact bytes."""
import ctypes as C
import random
import threading

import numpy as np
import pytest

from oracle import bigint_oracle as B
from oracle.cpu_oracle import ints_to_limbs, limbs_to_ints
from test_zk_host import BLINDERS, EXTRA_BASES, circuit_ints, zk_prove

pytestmark = pytest.mark.gpu
R = B.R_MOD
TAU = 0x3C6EF372FE94F82BA54FF53A5F1D36F1510E527FADE682D19B05688C2B3E6C1F % R   # test_gpu_zk's: its _verify is used below
_CK: dict = {}


def _mont(oracle, v):
    return oracle.fr_to_mont(ints_to_limbs([v % R], 4))[0]


def _ints(oracle, limbs):
    return limbs_to_ints(oracle.fr_from_mont(np.ascontiguousarray(limbs).reshape(-1, 4)))


def _ck(ctx, oracle, n):
    """A powers-of-tau key with n + 10 points, one size at a time (the 2^20 one is large)."""
    import plonk_prototype_amd as pa
    if n not in _CK:
        _CK.clear()
        _CK[n] = pa.CommitKey.setup(n + EXTRA_BASES - 1, _mont(oracle, TAU), ctx, precompute=(n >= 1 << 12))
    return _CK[n]


def _blinders(seed, count):
    """-> (ints [count][17], limbs [count, 17, 4]): distinct seeded blinders for every proof."""
    from plonk_prototype_amd.field import fr_to_limbs
    rng = random.Random(seed)
    vals = [[rng.randrange(R) for _ in range(BLINDERS)] for _ in range(count)]
    return vals, np.stack([np.stack([fr_to_limbs(v) for v in row]) for row in vals])


def _zk_singles(pk, ck, wits, pis, bl, bind=True):
    import plonk_prototype_amd.prover as PR
    return [PR.prove(pk, ck, w, p, bind_public_inputs=bind, zero_knowledge=True, blinders=bl[b])
            for b, (w, p) in enumerate(zip(wits, pis))]


def _same(batch, singles):
    assert len(batch) == len(singles)
    for b, (x, y) in enumerate(zip(batch, singles)):
        assert x.native_bytes == y.native_bytes, f"proof {b}: bytes differ"
        assert x.challenges == y.challenges, f"proof {b}: challenges differ"


def _check_zk_batch(pk, ck, wits, pis, bl, binds=(True, False), ws=None):
    import plonk_prototype_amd.prover as PR
    for bind in binds:
        got = PR.prove_batch(pk, ck, list(wits), list(pis), bind_public_inputs=bind, workspace=ws, zero_knowledge=True,
                             blinders=bl)
        _same(got, _zk_singles(pk, ck, wits, pis, bl, bind))


# ---- 1 equals the single zero-knowledge prover
@pytest.mark.parametrize("log_n", [4, 8, 12])
def test_chain_zk_batches_equal_single_zk_proofs(ctx, oracle, log_n):
    import plonk_prototype_amd as pa
    from test_gpu_prove_batch import _pi_variants
    n = 1 << log_n
    ck = _ck(ctx, oracle, n)
    circuit, _, _ = pa.synthetic.chain_circuit(n, 21)
    pk = pa.preprocess(circuit, ctx, ck)
    ws = pk.batch(16, zero_knowledge=True)
    for batch in (1, 2, 5, 16):
        rows = [(0,), (), tuple(range(0, n, max(1, n // 24))), (1, 2)] * 4
        pairs = pa.synthetic.chain_witnesses(n, 21, count=batch, witness_seed=batch, public_rows=rows[:batch])
        wits = [w for w, _ in pairs]
        pis = _pi_variants(n, [p for _, p in pairs])
        _, bl = _blinders(100 * log_n + batch, batch)
        _check_zk_batch(pk, ck, wits, pis, bl, ws=ws)
    ws.free()
    pk.free()


@pytest.mark.parametrize("n", [32, 128])
def test_mixed_zk_batches_every_widget(ctx, oracle, n):
    import plonk_prototype_amd as pa
    ck = _ck(ctx, oracle, n)
    circuit, wit, pub = pa.synthetic.mixed_circuit(n, 7)
    pk = pa.preprocess(circuit, ctx, ck)
    ws = pk.batch(16, zero_knowledge=True)
    for batch in (1, 2, 5, 16):
        _, bl = _blinders(n + batch, batch)
        _check_zk_batch(pk, ck, [wit] * batch, [pub] * batch, bl, ws=ws)   # one witness, its own blinders per slot
    ws.free()
    pk.free()


def test_smallest_size_n_4(ctx, oracle):
    """n = 4: n + 3 of the 16 coset points carry a blinded wire -- the smallest size the single prover is tested at."""
    import plonk_prototype_amd as pa
    n = 4
    ck = _ck(ctx, oracle, n)
    circuit, _, _ = pa.synthetic.chain_circuit(n, 13)
    pk = pa.preprocess(circuit, ctx, ck)
    pairs = pa.synthetic.chain_witnesses(n, 13, count=2, witness_seed=3, public_rows=[(0,), ()])
    _, bl = _blinders(4, 2)
    _check_zk_batch(pk, ck, [w for w, _ in pairs], [p for _, p in pairs], bl)
    pk.free()


# ---- 2 zero blinders reproduce the plain batch
@pytest.mark.parametrize("log_n", [6, 12])
def test_zero_blinders_reproduce_the_plain_batch(ctx, oracle, log_n):
    import plonk_prototype_amd as pa
    import plonk_prototype_amd.prover as PR
    n = 1 << log_n
    ck = _ck(ctx, oracle, n)
    circuit, _, _ = pa.synthetic.chain_circuit(n, 41)
    pk = pa.preprocess(circuit, ctx, ck)
    pairs = pa.synthetic.chain_witnesses(n, 41, count=5, witness_seed=6, public_rows=[(0,), (), (1, 2), (3,), ()])
    wits, pis = [w for w, _ in pairs], [p for _, p in pairs]
    zero = np.zeros((5, BLINDERS, 4), np.uint64)
    for bind in (True, False):
        plain = PR.prove_batch(pk, ck, wits, pis, bind_public_inputs=bind)
        _same(PR.prove_batch(pk, ck, wits, pis, bind_public_inputs=bind, zero_knowledge=True, blinders=zero), plain)
        _same(plain, [PR.prove(pk, ck, w, p, bind_public_inputs=bind) for w, p in zip(wits, pis)])
    pk.free()


# ---- 3 the big-int restatement, per slot
@pytest.mark.parametrize("n,mixed", [(16, False), (32, True)])
def test_members_match_the_big_int_restatement(ctx, oracle, n, mixed):
    import plonk_prototype_amd as pa
    import plonk_prototype_amd.prover as PR
    circuit, wit, pub, (sel, sigma, wi, pii) = circuit_ints(n, n + 5, mixed)
    assert any(pii)
    ck = _ck(ctx, oracle, n)
    pk = pa.preprocess(circuit, ctx, ck)
    betas, bl = _blinders(n + 1, 3)
    proofs = PR.prove_batch(pk, ck, [wit] * 3, [pub] * 3, zero_knowledge=True, blinders=bl)

    def g(k):
        return oracle.g1_mul(oracle.g1_generator(), ints_to_limbs([k % R], 4)[0])

    tau = lambda c: B.horner(c, TAU)   # noqa: E731
    for b, proof in enumerate(proofs):
        exp = zk_prove(n, sel, sigma, wi, pii, proof.challenges, betas[b])
        got = {k: _ints(oracle, v)[0] for k, v in proof.evaluations.items()}
        assert got == exp["evals"], b
        want = {nm: tau(exp["wire_coeffs"][j]) for j, nm in enumerate("abcd")}
        want["z"] = tau(exp["z_coeffs"])
        for i in range(4):
            want[f"t_{i + 1}"] = tau(exp["t_pieces"][i])
        want["w_z"], want["w_zw"] = tau(exp["w_z"]), tau(exp["w_zw"])
        assert set(want) == set(proof.commitments)
        for k, v in want.items():
            assert np.array_equal(proof.commitments[k], g(v)), (b, k)
    pk.free()


# ---- 4 the unchanged pairing verifier, fresh blinders
def test_fresh_blinder_batch_verifies_and_hides(ctx, oracle):
    import plonk_prototype_amd as pa
    import plonk_prototype_amd.prover as PR
    from test_gpu_zk import _verify
    n = 1 << 12
    ck = _ck(ctx, oracle, n)
    circuit, _, _ = pa.synthetic.chain_circuit(n, 51)
    pairs = pa.synthetic.chain_witnesses(n, 51, count=3, witness_seed=8, public_rows=[(0,), (3, 9), ()])
    pairs.append(pairs[0])                                  # slots 0 and 3: the same witness and public inputs
    pk = pa.preprocess(circuit, ctx, ck)
    proofs = PR.prove_batch(pk, ck, [w for w, _ in pairs], [p for _, p in pairs], zero_knowledge=True)   # blinders=None
    ok, _ = _verify(oracle, pk, n, proofs[1].native_bytes, pairs[1][1])
    assert ok == (True, True)
    for k in ("a", "b", "c", "d", "z", "t_1", "t_2", "t_3", "t_4", "w_z", "w_zw"):
        for x in range(4):
            for y in range(x):
                assert not np.array_equal(proofs[x].commitments[k], proofs[y].commitments[k]), (k, x, y)
    # and a second call draws new blinders: the same batch, other proofs
    again = PR.prove_batch(pk, ck, [w for w, _ in pairs], [p for _, p in pairs], zero_knowledge=True)
    assert all(p.native_bytes != q.native_bytes for p, q in zip(proofs, again))
    pk.free()


# ---- 5 no cross-talk
def test_no_cross_talk_between_zk_slots(ctx, oracle):
    import plonk_prototype_amd as pa
    import plonk_prototype_amd.prover as PR
    n = 256
    ck = _ck(ctx, oracle, n)
    circuit, _, _ = pa.synthetic.chain_circuit(n, 33)
    pk = pa.preprocess(circuit, ctx, ck)
    pairs = pa.synthetic.chain_witnesses(n, 33, count=5, witness_seed=4, public_rows=())
    wits = [w.copy() for w, _ in pairs]
    k = 2
    wits[k][0, 17] = pa.field.fr_to_limbs(12345)             # a at gate 17: the gate equation fails there
    _, bl = _blinders(55, 5)
    ws = pk.batch(5, zero_knowledge=True)
    got = PR.prove_batch(pk, ck, wits, None, workspace=ws, zero_knowledge=True, blinders=bl)
    singles = _zk_singles(pk, ck, wits, [None] * 5, bl)
    _same(got, singles)
    for b in range(5):
        assert PR.check_identity(got[b], n) == (b != k), b
    # the blinders of slot 3 changed alone change proof 3 alone
    bl2 = bl.copy()
    bl2[3] = _blinders(56, 1)[1][0]
    got2 = PR.prove_batch(pk, ck, wits, None, workspace=ws, zero_knowledge=True, blinders=bl2)
    for b in range(5):
        assert (got2[b].native_bytes == got[b].native_bytes) == (b != 3), b
    assert got2[3].native_bytes == PR.prove(pk, ck, wits[3], None, zero_knowledge=True, blinders=bl2[3]).native_bytes
    ws.free()
    pk.free()


# ---- 6 Lagrange key
def test_lagrange_key_gives_the_same_zk_batch(ctx, oracle):
    import plonk_prototype_amd as pa
    import plonk_prototype_amd.prover as PR
    n = 1 << 12
    ck = _ck(ctx, oracle, n)
    made = [pa.synthetic.boolean_circuit(n, s) for s in (1, 2, 3, 4, 5)]
    wits, pis = [m[1] for m in made], [m[2] for m in made]
    pk = pa.preprocess(made[0][0], ctx, ck)
    _, bl = _blinders(12, 5)
    ws = pk.batch(5, zero_knowledge=True)
    want = {bind: PR.prove_batch(pk, ck, wits, pis, bind_public_inputs=bind, workspace=ws, zero_knowledge=True, blinders=bl)
            for bind in (True, False)}
    _same(want[True], _zk_singles(pk, ck, wits, pis, bl))
    lck = ck.lagrange(12)
    pk.use_lagrange(ck, lck)
    for bind in (True, False):
        got = PR.prove_batch(pk, ck, wits, pis, bind_public_inputs=bind, workspace=ws, zero_knowledge=True, blinders=bl)
        _same(got, want[bind])
    _same(_zk_singles(pk, ck, wits[:2], pis[:2], bl), want[True][:2])       # the single prover over the Lagrange key
    pk.use_lagrange(None, None)
    _same(PR.prove_batch(pk, ck, wits, pis, workspace=ws, zero_knowledge=True, blinders=bl), want[True])
    ws.free()
    pk.free()


# ---- 7 one workspace, many calls; its size
def test_one_zk_workspace_many_calls_and_its_bytes(ctx, oracle):
    import torch
    import plonk_prototype_amd as pa
    import plonk_prototype_amd.prover as PR
    n = 1 << 12
    ck = _ck(ctx, oracle, n)
    circuit, _, _ = pa.synthetic.chain_circuit(n, 61)
    pk = pa.preprocess(circuit, ctx, ck)
    pk.enable_zk()
    ws = pk.batch(64)
    plain_bytes = ws.device_bytes()
    assert ws.zk_device_bytes() == 0
    ctx.sync()
    free0 = torch.cuda.mem_get_info(0)[0]
    added = ws.enable_zk()
    ctx.sync()
    free1 = torch.cuda.mem_get_info(0)[0]
    print(f"zk regions: {added} bytes = {added / (64 * n * 32):.2f} n x 32 bytes per proof; plain {plain_bytes / (64 * n * 32):.2f}")
    assert added > 0 and added <= free0 - free1 <= added + (64 << 20)     # allocation granularity
    assert ws.enable_zk() == added and ws.zk_device_bytes() == added      # idempotent, the same figure
    assert torch.cuda.mem_get_info(0)[0] == free1
    assert ws.device_bytes() == plain_bytes                               # pm_plonk_batch_bytes keeps its meaning
    pairs = pa.synthetic.chain_witnesses(n, 61, count=64, witness_seed=5)
    wits, pis = [w for w, _ in pairs], [p for _, p in pairs]
    _, bl = _blinders(64, 64)
    singles = _zk_singles(pk, ck, wits, pis, bl)
    for batch in (3, 64, 1, 17):                              # 64 x 4 wires: four MSM passes in round 1
        got = PR.prove_batch(pk, ck, wits[:batch], pis[:batch], workspace=ws, zero_knowledge=True, blinders=bl[:batch])
        _same(got, singles[:batch])
    plain = PR.prove_batch(pk, ck, wits[:5], pis[:5], workspace=ws)       # the enabled workspace still serves plain batches
    _same(plain, [PR.prove(pk, ck, w, p) for w, p in zip(wits[:5], pis[:5])])
    _same([PR.prove(pk, ck, wits[0], pis[0], zero_knowledge=True, blinders=bl[0])], singles[:1])
    ws.free()
    # free() returns both allocations (measured on a second workspace: the context's own scratch has grown to its size by now)
    ctx.sync()
    free2 = torch.cuda.mem_get_info(0)[0]
    ws2 = pk.batch(64, zero_knowledge=True)
    ctx.sync()
    free3 = torch.cuda.mem_get_info(0)[0]
    assert plain_bytes + added <= free2 - free3 <= plain_bytes + added + (64 << 20)
    ws2.free()
    ctx.sync()
    assert abs(torch.cuda.mem_get_info(0)[0] - free2) <= (4 << 20)
    pk.free()


# ---- 8 sizes
@pytest.mark.parametrize("log_n,batch", [(16, 4), (20, 2)])
def test_large_zk_batches(ctx, oracle, log_n, batch):
    import plonk_prototype_amd as pa
    n = 1 << log_n
    ck = _ck(ctx, oracle, n)
    made = [pa.synthetic.boolean_circuit(n, s) for s in range(1, batch + 1)]
    pk = pa.preprocess(made[0][0], ctx, ck)
    _, bl = _blinders(log_n, batch)
    _check_zk_batch(pk, ck, [m[1] for m in made], [m[2] for m in made], bl, binds=(True,))
    pk.free()
    _CK.clear()


# ---- 9 refusals, through the raw ABI
def test_refusals(ctx, oracle):
    import plonk_prototype_amd as pa
    from plonk_prototype_amd import _lib
    n = 64
    ck = _ck(ctx, oracle, n)
    circuit, wit, _ = pa.synthetic.chain_circuit(n, 71)
    pk = pa.preprocess(circuit, ctx, ck)
    other = pa.preprocess(pa.synthetic.chain_circuit(n, 72)[0], ctx, ck)
    uncommitted = pa.ProverKey(circuit, ctx)
    ws = pk.batch(4)
    d = pa.DeviceVector.from_host(ctx, np.concatenate([wit.reshape(4 * n, 4)] * 4))
    _, bl = _blinders(9, 4)
    lib = ctx._lib

    def call(key=pk, ws_h=None, commit_key=ck, batch=2, blinders=bl, n_pi=None, pos=None, vals=None, flags=0):
        raws = (_lib.PlonkProof * max(batch, 1))()
        p = blinders.ctypes.data_as(_lib.u64p) if blinders is not None else None
        rc = lib.pm_plonk_prove_batch_zk(ctx._h, key._h, (ws if ws_h is None else ws_h)._h, commit_key._bases._h, batch, d._p,
                                         pos, vals, n_pi, flags, p, raws)
        return rc, lib.pm_last_error(ctx._h).decode()

    # the key is not enabled: the workspace cannot be
    rc = lib.pm_plonk_batch_enable_zk(ctx._h, ws._h, None)
    assert rc == _lib.PM_ERR_BAD_ARG and "pm_plonk_key_enable_zk" in lib.pm_last_error(ctx._h).decode()
    pk.enable_zk()
    rc, msg = call()
    assert rc == _lib.PM_ERR_BAD_ARG and "pm_plonk_batch_enable_zk" in msg          # workspace without enable_zk
    assert lib.pm_plonk_batch_enable_zk(ctx._h, ws._h, None) == _lib.PM_OK           # added_bytes may be NULL
    assert call()[0] == _lib.PM_OK
    # every refusal of pm_plonk_prove_batch
    assert call(batch=0)[0] == _lib.PM_ERR_BAD_ARG
    rc, msg = call(batch=5)
    assert rc == _lib.PM_ERR_BAD_ARG and "max_batch" in msg
    rc, msg = call(key=other)
    assert rc == _lib.PM_ERR_BAD_ARG and "another key" in msg
    ws_u = pa.prover.BatchWorkspace(uncommitted, 2)
    rc, msg = call(key=uncommitted, ws_h=ws_u)
    assert rc == _lib.PM_ERR_BAD_ARG and "committed" in msg
    rc, msg = call(flags=3)
    assert rc == _lib.PM_ERR_BAD_ARG and "exclude" in msg
    counts = (C.c_size_t * 2)(0, 1)
    pos_arr = np.array([n], np.uint64)
    val_arr = np.zeros((1, 4), np.uint64)
    pp = (_lib.u64p * 2)(None, pos_arr.ctypes.data_as(_lib.u64p))
    vv = (_lib.u64p * 2)(None, val_arr.ctypes.data_as(_lib.u64p))
    rc, msg = call(n_pi=counts, pos=pp, vals=vv)
    assert rc == _lib.PM_ERR_LENGTH and "position" in msg
    # the zero-knowledge ones
    rc, msg = call(blinders=None)
    assert rc == _lib.PM_ERR_BAD_ARG and "blinders" in msg
    big = bl.copy()
    big[1, 5] = np.frombuffer(R.to_bytes(32, "little"), dtype=np.uint64)           # = r: not canonical, in proof 1
    rc, msg = call(blinders=big)
    assert rc == _lib.PM_ERR_BAD_ARG and "below r" in msg
    assert call(blinders=big, batch=1)[0] == _lib.PM_OK                              # proof 0's blinders are fine
    short = pa.CommitKey.setup(n + EXTRA_BASES - 2, _mont(oracle, TAU), ctx)         # n + 9 points
    rc, msg = call(commit_key=short)
    assert rc == _lib.PM_ERR_LENGTH and "PM_PLONK_ZK_EXTRA_BASES" in msg
    # a busy workspace: another thread proves batches on it while this one asks
    ws64 = pk.batch(64, zero_knowledge=True)
    d64 = pa.DeviceVector.from_host(ctx, np.concatenate([wit.reshape(4 * n, 4)] * 64))
    _, bl64 = _blinders(10, 64)
    seen = {"main": [], "other": []}
    stop = threading.Event()

    def one(who, batch):
        raws = (_lib.PlonkProof * batch)()
        seen[who].append(lib.pm_plonk_prove_batch_zk(ctx._h, pk._h, ws64._h, ck._bases._h, batch, d64._p, None, None, None, 0,
                                                     bl64.ctypes.data_as(_lib.u64p), raws))

    def worker():
        for _ in range(400):
            if stop.is_set():
                break
            one("other", 64)

    th = threading.Thread(target=worker)
    th.start()
    for _ in range(4000):
        one("main", 1)
        if _lib.PM_ERR_BUSY in seen["main"] or _lib.PM_ERR_BUSY in seen["other"]:
            break
    stop.set()
    th.join()
    every = seen["main"] + seen["other"]
    assert _lib.PM_ERR_BUSY in every and _lib.PM_OK in every
    assert set(every) <= {_lib.PM_OK, _lib.PM_ERR_BUSY}
    # a successful call on the same handles: none of the refusals left anything busy
    got = pa.prove_batch(pk, ck, d, None, workspace=ws, zero_knowledge=True, blinders=bl)
    want = [pa.prove(pk, ck, wit, None, zero_knowledge=True, blinders=bl[b]) for b in range(4)]
    _same(got, want)
    got64 = pa.prove_batch(pk, ck, d64, None, workspace=ws64, zero_knowledge=True, blinders=bl64)
    assert got64[3].native_bytes == pa.prove(pk, ck, wit, None, zero_knowledge=True, blinders=bl64[3]).native_bytes
    # the Python entry points refuse what they promise to
    with pytest.raises(ValueError):
        pa.prove_batch(pk, ck, d, None, workspace=ws, blinders=bl)                  # blinders without zero_knowledge
    with pytest.raises(ValueError):
        pa.prove_batch(pk, ck, d, None, workspace=ws, zero_knowledge=True, blinders=bl[:3])   # wrong shape
    with pytest.raises(ValueError):
        pa.prove_batch(pk, ck, d, None, workspace=ws, zero_knowledge=True, blinders=bl[0])
    with pytest.raises(ValueError, match="commit the key first"):
        pa.prove_batch(uncommitted, ck, d, None, zero_knowledge=True)
    with pytest.raises(ValueError, match="commit the key first"):
        uncommitted.batch(2, zero_knowledge=True)
    for h in (ws, ws_u, ws64):
        h.free()
    for v in (d, d64):
        v.free()
    del short
    for k in (pk, other, uncommitted):
        k.free()
    _CK.clear()
