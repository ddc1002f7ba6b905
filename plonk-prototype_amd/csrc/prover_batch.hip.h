// Many proofs of one circuit in one call: pm_plonk_prove_batch (included by prover.hip: the key is pm_plonk_prove's, and
// the host side of the rounds is the same prover_rounds.h, one ProofRounds per proof).
//
// B proofs run through every round together.  The workspace is laid out role-major -- every role (wire coefficients,
// z, PI, the coset forms, t, r, the aggregates, the opening witnesses) holds all B proofs at one uniform stride -- so each
// transform is ONE pm_fr_ntt_dev call over all of them, each commitment round is pm_g1_msm_batch_dev passes of at most 64
// vectors, and the O(n) work between them is one proof-batched kernel per step (blockIdx.y = the proof, the per-proof
// challenges in a device table).  One host synchronisation per round for the whole batch (the MSM's, and the openings'),
// then one affine conversion for all the round's points and B challenge derivations on the host.  The launches per call
// do not depend on B, apart from the extra MSM passes above 64 vectors.
//
//   coeffs [B][4][n]   wire coefficients (proof-major inside: vector 4 b + j, stride n)
//   zc, pi_coeffs, pi_evals, num, den  [B][n]
//   coset_w [B][4][4n]   coset_z, coset_pi, t  [B][4n]
//   r [B][n]   agg, wit [2][B][n]  (at z, then at z w)
//
// Zero-knowledge batches (pm_plonk_batch_enable_zk / pm_plonk_prove_batch_zk) keep every coefficient
// vector at the padded stride S = n + ZK_PAD in a second allocation, with the second-coset forms beside it; the evaluation
// side (pi_evals, num, den, the first-coset forms) stays where it is:
//   coeffs [B][4][S]   zc, r [B][S]   t [B][4][S]   agg, wit [2][B][S]
//   shift [B][4][S] (p(w_8n X) of the wires, then of z)   shift_pi [B][n]
//   coset2_w [B][4][4n]   coset2_z, coset2_pi [B][4n]   ab [2][B][4n]  (both coset quotients: one inverse transform)
struct BatchZk {
  void* base = nullptr;
  size_t bytes = 0, stride = 0;
  void *coeffs = nullptr, *zc = nullptr, *shift = nullptr, *shift_pi = nullptr, *coset2_w = nullptr, *coset2_z = nullptr,
       *coset2_pi = nullptr, *ab = nullptr, *t = nullptr, *r = nullptr, *agg = nullptr, *wit = nullptr, *eval_ws = nullptr,
       *ruf_ws = nullptr;
};
struct pm_plonk_batch {
  const pm_prover_key* key = nullptr;
  uint32_t max_batch = 0;
  size_t n = 0;
  void* base = nullptr;      // the one device allocation
  size_t bytes = 0;
  void *coeffs = nullptr, *zc = nullptr, *pi_coeffs = nullptr, *pi_evals = nullptr, *num = nullptr, *den = nullptr,
       *coset_w = nullptr, *coset_z = nullptr, *coset_pi = nullptr, *t = nullptr, *r = nullptr, *agg = nullptr, *wit = nullptr;
  void *pp_ctl = nullptr, *eval_ws = nullptr, *ruf_ws = nullptr;
  pm::ConstStage stage;      // per-proof challenge tables: pinned host + device (in `base`)
  void* pi_h = nullptr;      // pinned staging of the public inputs, grown on demand
  size_t pi_h_bytes = 0;
  std::atomic<bool> busy{false};
  hipStream_t side = nullptr;
  hipEvent_t ev_main = nullptr, ev_side = nullptr;
  BatchZk* zk = nullptr;     // pm_plonk_batch_enable_zk
};

namespace {
constexpr uint32_t BATCH_EVAL_SLOTS = MAX_OPENINGS;
constexpr size_t BATCH_CONST_BYTES_PER_PROOF = 16384, BATCH_CONST_BYTES_FIXED = 16384;

// commitments to `count` vectors of len coefficients at stride `stride`: passes of at most 64 vectors, one affine conversion
int batch_commit(pm_ctx* ctx, const pm_bases* ck, const void* d, size_t len, size_t stride, uint32_t count, u64 (*out_xy)[12]) {
  std::vector<u64> xyz(18 * (size_t)count);
  for (uint32_t v0 = 0; v0 < count; v0 += 64) {
    const uint32_t k = std::min<uint32_t>(64, count - v0);
    PK_TRY(pm_g1_msm_batch_dev(ctx, ck, 0, len, at((void*)d, (size_t)v0 * stride), stride, k, PM_SCALAR_MONTGOMERY,
                               &xyz[18 * (size_t)v0], nullptr));
  }
  return pm_g1_to_affine_batch(xyz.data(), count, &out_xy[0][0], nullptr);
}

// pi_evals <- 0, then every proof's public inputs in ONE staged scatter (pi_scatter_kernel over global positions b n + i; a
// repeated position keeps its last value, as in scatter_public_inputs).  The compact lists go through the round-2 scratch
// num / den, which nothing reads before round 2 (same stream).
int batch_scatter_pi(pm_ctx* ctx, pm_plonk_batch* ws, uint32_t B, const uint64_t* const* pos, const uint64_t* const* vals,
                     const size_t* n_pi) {
  const size_t n = ws->n;
  PM_HIP(ctx, hipSetDevice(ctx->device));
  PM_HIP(ctx, hipMemsetAsync(ws->pi_evals, 0, (size_t)B * n * 32, ctx->stream));
  if (!n_pi) return PM_OK;
  std::vector<unsigned long long> hp;
  std::vector<uint64_t> hv;
  for (uint32_t b = 0; b < B; ++b)
    if (n_pi[b]) compact_public_inputs(pos[b], vals[b], n_pi[b], (uint64_t)b * n, hp, hv);
  const size_t cnt = hp.size();   // <= B n: fits num (values) and den (positions)
  if (!cnt) return PM_OK;
  const size_t need = cnt * 40;
  if (ws->pi_h_bytes < need) {
    if (ws->pi_h) PM_HIP(ctx, hipHostFree(ws->pi_h));
    ws->pi_h = nullptr;
    ws->pi_h_bytes = 0;
    PM_HIP(ctx, hipHostMalloc(&ws->pi_h, need, hipHostMallocDefault));
    ws->pi_h_bytes = need;
  }
  memcpy(ws->pi_h, hv.data(), cnt * 32);
  memcpy((char*)ws->pi_h + cnt * 32, hp.data(), cnt * 8);
  PM_HIP(ctx, hipMemcpyAsync(ws->num, ws->pi_h, cnt * 32, hipMemcpyHostToDevice, ctx->stream));
  PM_HIP(ctx, hipMemcpyAsync(ws->den, (char*)ws->pi_h + cnt * 32, cnt * 8, hipMemcpyHostToDevice, ctx->stream));
  hipLaunchKernelGGL(pi_scatter_kernel, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, ctx->stream, (const uint4*)ws->num,
                     (const unsigned long long*)ws->den, cnt, (uint4*)ws->pi_evals);
  PM_HIP(ctx, hipGetLastError());
  return PM_OK;
}

// Regions of one allocation, each at a multiple of 256 bytes: the bytes they need together; with a base, their pointers
struct Region {
  void** p;
  size_t bytes;
};
template <size_t N>
size_t carve_regions(void* base, const Region (&regions)[N]) {
  size_t off = 0;
  for (const Region& r : regions) {
    if (base) *r.p = (char*)base + off;
    off += (r.bytes + 255) / 256 * 256;
  }
  return off;
}

int prove_batch_body(pm_ctx* ctx, pm_prover_key* pk, pm_plonk_batch* ws, const pm_bases* ck, uint32_t B, const void* d_wit,
                     const uint64_t* const* pi_pos, const uint64_t* const* pi_val, const size_t* n_pi, uint32_t flags,
                     const uint64_t (*blinders)[PM_PLONK_ZK_BLINDERS][4], pm_plonk_proof* out) {
  const size_t n = pk->n;
  const uint32_t lg = pk->log_n;
  ws->stage.reset();
  // zero-knowledge mode: blinded wires and z of n + 3 coefficients, quotient pieces up to n + 10, all at the padded stride S in
  // the workspace's ZK regions, and the second-coset forms for the quotient.  Otherwise S = n and the plain regions.
  BatchZk* const zk = blinders ? ws->zk : nullptr;
  const ZkState* const kz = zk ? pk->zk : nullptr;
  const size_t S = zk ? zk->stride : n, wlen = zk ? n + 3 : n;
  void* const W = zk ? zk->coeffs : ws->coeffs;      // [B][4][S]
  void* const Zc = zk ? zk->zc : ws->zc;             // [B][S]
  void* const T = zk ? zk->t : ws->t;                // [B][4][S]
  void* const R = zk ? zk->r : ws->r;                // [B][S]
  void* const AGG = zk ? zk->agg : ws->agg;          // [2][B][S]
  void* const WIT = zk ? zk->wit : ws->wit;          // [2][B][S]
  void* d_bl = nullptr;                              // the batch's blinders on the device: [B][17][4]
  if (zk) {
    void* h_bl;
    const size_t bytes = sizeof(uint64_t) * 4 * PM_PLONK_ZK_BLINDERS * B;
    if (!ws->stage.take(bytes, &h_bl, &d_bl)) return pm::set_err(ctx, PM_ERR_OOM, "constant table full");
    memcpy(h_bl, blinders, bytes);
    PM_HIP(ctx, hipSetDevice(ctx->device));
    PM_HIP(ctx, hipMemcpyAsync(d_bl, h_bl, bytes, hipMemcpyHostToDevice, ctx->stream));   // ahead of every fork of this call
  }
  // the wires + PI (round 1) or z (round 2) on the second coset: one w_8n^i scaling pass, then the coset transforms
  auto second_coset = [&](bool round1, hipStream_t st) -> int {
    pm::ZkShiftBatchArgs sa;
    memset(&sa, 0, sizeof sa);
    sa.groups = round1 ? 2 : 1;
    sa.src[0] = round1 ? W : Zc;
    sa.dst[0] = zk->shift;
    sa.vecs[0] = round1 ? 4 : 1;
    sa.stride[0] = S;
    sa.len[0] = wlen;
    sa.src[1] = ws->pi_coeffs;
    sa.dst[1] = zk->shift_pi;
    sa.vecs[1] = 1;
    sa.stride[1] = n;
    sa.len[1] = n;
    PK_TRY(pm::zk_shift_batch(ctx, sa, kz->w8, B, st));
    if (!round1) return pm_fr_ntt_dev(ctx, zk->shift, wlen, S, zk->coset2_z, 4 * n, lg + 2, B, PM_NTT_COSET, st);
    PK_TRY(pm_fr_ntt_dev(ctx, zk->shift, wlen, S, zk->coset2_w, 4 * n, lg + 2, 4 * B, PM_NTT_COSET, st));
    return pm_fr_ntt_dev(ctx, zk->shift_pi, n, n, zk->coset2_pi, 4 * n, lg + 2, B, PM_NTT_COSET, st);
  };
  std::vector<ProofRounds> pr(B, ProofRounds(pk->base));
  for (uint32_t b = 0; b < B; ++b) {
    const size_t k = n_pi ? n_pi[b] : 0;
    pr[b].begin(flags, k ? pi_pos[b] : nullptr, k ? pi_val[b] : nullptr, k);
  }
  const pm_bases* lag = pk->lagrange;
  hipStream_t side = ws->side;
  std::vector<u64> xy_buf(12 * 4 * (size_t)B);
  u64(*xy)[12] = (u64(*)[12])xy_buf.data();
  // ---- round 1 --------------------------------------------------------------------------------
  PK_TRY(batch_scatter_pi(ctx, ws, B, pi_pos, pi_val, n_pi));
  PK_TRY(pm_fr_ntt_dev(ctx, ws->pi_evals, n, n, ws->pi_coeffs, n, lg, B, PM_NTT_INVERSE, nullptr));
  if (lag) {
    // the wires are committed from their values on H: the wire iNTT goes to the side stream with the coset transforms
    PK_TRY(pm_stream_fork(ctx, side, ws->ev_main));
    PK_TRY(pm_fr_ntt_dev(ctx, d_wit, n, n, W, S, lg, 4 * B, PM_NTT_INVERSE, side));
    if (zk) {
      PK_TRY(pm::zk_blind_batch(ctx, d_bl, W, 4, 0, B, n, S, side));
      PK_TRY(pm_stream_join(ctx, side, ws->ev_side));   // the blinder MSMs below read the blinded coefficients
    }
    PK_TRY(pm_fr_ntt_dev(ctx, W, wlen, S, ws->coset_w, 4 * n, lg + 2, 4 * B, PM_NTT_COSET, side));
    PK_TRY(pm_fr_ntt_dev(ctx, ws->pi_coeffs, n, n, ws->coset_pi, 4 * n, lg + 2, B, PM_NTT_COSET, side));
    if (zk) {
      PK_TRY(second_coset(true, side));
      std::vector<u64> scratch(72 * 4 * (size_t)B);
      PK_TRY(commit_lagrange_zk(ctx, lag, ck, d_wit, W, n, S, 4 * B, scratch.data(), xy));
    } else {
      PK_TRY(batch_commit(ctx, lag, d_wit, n, n, 4 * B, xy));
    }
  } else {
    PK_TRY(pm_fr_ntt_dev(ctx, d_wit, n, n, W, S, lg, 4 * B, PM_NTT_INVERSE, nullptr));
    if (zk) PK_TRY(pm::zk_blind_batch(ctx, d_bl, W, 4, 0, B, n, S, nullptr));
    PK_TRY(pm_stream_fork(ctx, side, ws->ev_main));
    PK_TRY(pm_fr_ntt_dev(ctx, W, wlen, S, ws->coset_w, 4 * n, lg + 2, 4 * B, PM_NTT_COSET, side));
    PK_TRY(pm_fr_ntt_dev(ctx, ws->pi_coeffs, n, n, ws->coset_pi, 4 * n, lg + 2, B, PM_NTT_COSET, side));
    if (zk) PK_TRY(second_coset(true, side));
    PK_TRY(batch_commit(ctx, ck, W, wlen, S, 4 * B, xy));
  }
  for (uint32_t b = 0; b < B; ++b) {
    memcpy(out[b].commitments[0], xy[4 * b], 4 * 96);
    pr[b].absorb_wires(&out[b].commitments[0]);
  }
  // ---- round 2 --------------------------------------------------------------------------------
  std::vector<pm_plonk_perm_args> pa(B);
  for (uint32_t b = 0; b < B; ++b) {
    pr[b].draw_round2();
    // proof 0's wires; proof b's at + 4 b n
    fill_perm_args(pa[b], d_wit, n, pk->sigma_evals, n, pk->roots, pk->k, pr[b].ch[C_BETA], pr[b].ch[C_GAMMA]);
  }
  PK_TRY(pm::perm_terms_batch(ctx, ws->stage, pa.data(), B, 4 * n, n, ws->num, ws->den, ctx->stream));
  PK_TRY(pm::fr_batch_inverse_mul(ctx, ws->den, ws->num, (size_t)B * n, nullptr));   // elementwise: one call for all proofs
  int prc = pm::prefix_product_batch(ctx, ws->den, n, B, ws->num, ws->pp_ctl, ctx->stream);
  if (prc == PM_ERR_LENGTH) {   // more tiles than are resident at once: the one-vector scan, per proof
    prc = PM_OK;
    for (uint32_t b = 0; b < B && !prc; ++b) prc = pm_fr_prefix_product_dev(ctx, at(ws->den, b * n), n, at(ws->num, b * n), nullptr);
  }
  PK_TRY(prc);
  PK_TRY(pm_fr_ntt_dev(ctx, ws->num, n, n, Zc, S, lg, B, PM_NTT_INVERSE, nullptr));
  if (zk) PK_TRY(pm::zk_blind_batch(ctx, d_bl, Zc, 1, 4, B, n, S, nullptr));
  PK_TRY(pm_stream_fork(ctx, side, ws->ev_main));
  PK_TRY(pm_fr_ntt_dev(ctx, Zc, wlen, S, ws->coset_z, 4 * n, lg + 2, B, PM_NTT_COSET, side));
  if (zk) PK_TRY(second_coset(false, side));
  PK_TRY(batch_commit(ctx, ck, Zc, wlen, S, B, xy));
  for (uint32_t b = 0; b < B; ++b) {
    memcpy(out[b].commitments[4], xy[b], 96);
    pr[b].absorb_perm(out[b].commitments[4]);
  }
  // ---- round 3 --------------------------------------------------------------------------------
  std::vector<pm_plonk_quotient_args> qa(B);
  for (uint32_t b = 0; b < B; ++b) {
    pr[b].draw_round3();
    // proof 0's wires, z and PI; proof b's at + 16 b n (z, PI, t: + 4 b n)
    fill_quotient_args(qa[b], key_first_coset(pk), ws->coset_w, 4 * n, ws->coset_z, ws->coset_pi, pk->k, pr[b].ch);
  }
  PK_TRY(pm_stream_join(ctx, side, ws->ev_side));   // the wire, PI and z coset forms are ready
  if (!zk) {
    PK_TRY(pm::quotient_batch(ctx, ws->stage, qa.data(), B, 16 * n, 4 * n, n, ws->t, ctx->stream));
    PK_TRY(pm_fr_ntt_dev(ctx, ws->t, 4 * n, 4 * n, ws->t, 4 * n, lg + 2, B, PM_NTT_INVERSE | PM_NTT_COSET, nullptr));
    PK_TRY(batch_commit(ctx, ck, ws->t, n, n, 4 * B, xy));   // t_i of proof b: vector 4 b + i
  } else {
    // deg t' <= 4n + 9: the same kernel on the second coset gives t' mod (X^4n + s) beside t' mod (X^4n - s); the 2B
    // outputs (A of every proof, then B of every proof) share one inverse coset transform
    PK_TRY(pm::quotient_batch(ctx, ws->stage, qa.data(), B, 16 * n, 4 * n, n, zk->ab, ctx->stream));
    for (uint32_t b = 0; b < B; ++b)
      fill_quotient_args(qa[b], key_second_coset(pk), zk->coset2_w, 4 * n, zk->coset2_z, zk->coset2_pi, pk->k, pr[b].ch);
    PK_TRY(pm::quotient_batch(ctx, ws->stage, qa.data(), B, 16 * n, 4 * n, n, at(zk->ab, 4 * n * (size_t)B), ctx->stream));
    PK_TRY(pm_fr_ntt_dev(ctx, zk->ab, 4 * n, 4 * n, zk->ab, 4 * n, lg + 2, 2 * B, PM_NTT_INVERSE | PM_NTT_COSET, nullptr));
    u64 inv2[4], inv2s[4];
    put(inv2, kz->inv2);
    put(inv2s, kz->inv2s);
    PK_TRY(pm::zk_combine_batch(ctx, d_bl, zk->ab, kz->w8, B, n, S, inv2, inv2s, T, ctx->stream));
    PK_TRY(batch_commit(ctx, ck, T, n + pm::ZK_P1_LEN, S, 4 * B, xy));
  }
  for (uint32_t b = 0; b < B; ++b) {
    memcpy(out[b].commitments[5], xy[4 * b], 4 * 96);
    pr[b].absorb_quotient(&out[b].commitments[5]);
  }
  // ---- round 4 --------------------------------------------------------------------------------
  std::vector<u64> points(8 * (size_t)B);
  for (uint32_t b = 0; b < B; ++b) {
    pr[b].draw_z(pk->omega);
    put(&points[8 * b], pr[b].ch[C_Z]);
    put(&points[8 * b + 4], pr[b].zw);
  }
  // proof 0's vector and the stride from proof to proof: the wires, t and z are padded vectors of the batch (S coefficients),
  // a polynomial of the key (n) has stride 0
  struct Vec {
    const void* p;
    size_t stride;
  };
  auto poly = [&](PolyRef p) -> Vec {
    switch (p.role) {
      case R_WIRE: return {at(W, p.index * S), 4 * S};
      case R_T: return {at(T, p.index * S), 4 * S};
      case R_Z: return {Zc, S};
      case R_SIGMA: return {at(pk->sigma_coeffs, p.index * n), 0};
      default: return {at(pk->sel_coeffs, p.index * n), 0};
    }
  };
  // the openings as pm_plonk_prove takes them -- one batch, one synchronisation
  const OpeningPlan plan(pk->sel_zero);
  const uint32_t K = plan.count;
  const void* sp[MAX_OPENINGS];
  size_t sstride[MAX_OPENINGS], slen[MAX_OPENINGS];
  uint8_t spt[MAX_OPENINGS];
  for (uint32_t s = 0; s < K; ++s) {
    const Vec v = poly(plan.slot[s].poly);
    sp[s] = v.p;
    sstride[s] = v.stride;
    slen[s] = v.stride ? S : n;
    spt[s] = plan.slot[s].point;
  }
  std::vector<u64> ov(4 * (size_t)K * B);
  PK_TRY(pm::evaluate_batch(ctx, ws->stage, K, sp, sstride, spt, points.data(), B, S, zk ? zk->eval_ws : ws->eval_ws, ov.data(),
                            ctx->stream, zk ? slen : nullptr));
  const void* lin_v[12];
  size_t lin_s[12];
  uint32_t lk = 0;
  std::vector<u64> lin_c;   // [B][lk][4]
  std::vector<u64> cz_c;    // [B][4]: z's coefficient in r (zero-knowledge mode: the only term with a tail beyond n)
  for (uint32_t b = 0; b < B; ++b) {
    pr[b].take_openings(plan, &ov[4 * (size_t)b * K], n);
    LinTerm terms[12];
    linearise(pr[b], pk->k, n, pk->sel_zero, terms, &lk);
    for (uint32_t i = 0; i < lk; ++i) {
      if (b == 0) {
        const Vec v = poly(terms[i].poly);
        lin_v[i] = v.p;
        lin_s[i] = v.stride;
      }
      lin_c.insert(lin_c.end(), terms[i].coeff.l, terms[i].coeff.l + 4);
    }
    cz_c.insert(cz_c.end(), pr[b].c_z.l, pr[b].c_z.l + 4);
    pr[b].finish_round4(&out[b]);
  }
  PK_TRY(pm::lincomb_batch(ctx, ws->stage, lk, lin_v, lin_s, lin_c.data(), B, n, R, S, ctx->stream));
  if (zk) {   // beyond n only the blinded z has coefficients
    const void* tail_v[1] = {at(Zc, n)};
    const size_t tail_s[1] = {S};
    PK_TRY(pm::lincomb_batch(ctx, ws->stage, 1, tail_v, tail_s, cz_c.data(), B, S - n, at(R, n), S, ctx->stream));
  }
  // ---- round 5: CommitKey::compute_aggregate_witness at z and at z w ------------------------------
  {
    const void* agg_v[12];
    size_t agg_s[12];
    for (int i = 0; i < 4; ++i) {
      agg_v[i] = at(T, i * S);
      agg_s[i] = 4 * S;
    }
    agg_v[4] = R;
    agg_s[4] = S;
    for (int j = 0; j < 4; ++j) {
      agg_v[5 + j] = at(W, j * S);
      agg_s[5 + j] = 4 * S;
    }
    for (int j = 0; j < 3; ++j) {
      agg_v[9 + j] = at(pk->sigma_coeffs, j * n);
      agg_s[9 + j] = 0;
    }
    const void* sh_v[4] = {Zc, at(W, 0), at(W, S), at(W, 3 * S)};
    const size_t sh_s[4] = {S, 4 * S, 4 * S, 4 * S};
    std::vector<u64> agg_c(12 * 4 * (size_t)B), sh_c(4 * 4 * (size_t)B), zs(8 * (size_t)B);
    for (uint32_t b = 0; b < B; ++b) {
      HFr ac[12], sh[4];
      aggregation_coeffs(pr[b], n, ac, sh);
      for (int i = 0; i < 12; ++i) put(&agg_c[4 * (12 * (size_t)b + i)], ac[i]);
      for (int e = 0; e < 4; ++e) put(&sh_c[4 * (4 * (size_t)b + e)], sh[e]);
      put(&zs[4 * (size_t)b], pr[b].ch[C_Z]);
      put(&zs[4 * ((size_t)B + b)], pr[b].zw);
    }
    PK_TRY(pm::lincomb_batch(ctx, ws->stage, 12, agg_v, agg_s, agg_c.data(), B, n, AGG, S, ctx->stream));
    if (zk) {   // the padded tails: t pieces, r and the wires (the sigmas end at n)
      const void* tail_v[9];
      std::vector<u64> tail_c(9 * 4 * (size_t)B);
      for (int i = 0; i < 9; ++i) tail_v[i] = at(agg_v[i], n);
      for (uint32_t b = 0; b < B; ++b) memcpy(&tail_c[9 * 4 * (size_t)b], &agg_c[12 * 4 * (size_t)b], 9 * 32);
      PK_TRY(pm::lincomb_batch(ctx, ws->stage, 9, tail_v, agg_s, tail_c.data(), B, S - n, at(AGG, n), S, ctx->stream));
    }
    PK_TRY(pm::lincomb_batch(ctx, ws->stage, 4, sh_v, sh_s, sh_c.data(), B, S, at(AGG, (size_t)B * S), S, ctx->stream));
    PK_TRY(pm::ruffini_batch(ctx, ws->stage, AGG, S, S, zs.data(), 2 * B, WIT, zk ? zk->ruf_ws : ws->ruf_ws, ctx->stream));
  }
  std::vector<u64> wxy_buf(12 * 2 * (size_t)B);
  u64(*wxy)[12] = (u64(*)[12])wxy_buf.data();
  // deg W_z = deg t_4 - 1: n + 9 coefficients in zero-knowledge mode
  PK_TRY(batch_commit(ctx, ck, WIT, zk ? n + pm::ZK_P1_LEN - 1 : n - 1, S, 2 * B, wxy));
  for (uint32_t b = 0; b < B; ++b) {
    memcpy(out[b].commitments[9], wxy[b], 96);
    memcpy(out[b].commitments[10], wxy[B + b], 96);
    pr[b].absorb_witnesses_and_store(&out[b]);
  }
  return PM_OK;
}
}  // namespace

extern "C" void pm_plonk_batch_free(pm_ctx* ctx, pm_plonk_batch* ws) {
  if (!ws) return;
  if (ctx) (void)pm_sync(ctx);
  if (ws->side) {
    (void)hipStreamSynchronize(ws->side);
    (void)hipStreamDestroy(ws->side);
  }
  if (ws->ev_main) (void)hipEventDestroy(ws->ev_main);
  if (ws->ev_side) (void)hipEventDestroy(ws->ev_side);
  if (ws->base && ctx) (void)pm_dev_free(ctx, ws->base);
  if (ws->zk) {
    if (ws->zk->base && ctx) (void)pm_dev_free(ctx, ws->zk->base);
    delete ws->zk;
  }
  if (ws->stage.h) (void)hipHostFree(ws->stage.h);
  if (ws->pi_h) (void)hipHostFree(ws->pi_h);
  delete ws;
}

extern "C" int pm_plonk_batch_create(pm_ctx* ctx, const pm_prover_key* key, uint32_t max_batch, pm_plonk_batch** out) {
  if (!ctx || !key || !out) return PM_ERR_BAD_ARG;
  *out = nullptr;
  if (max_batch == 0 || max_batch > PM_PLONK_MAX_BATCH)
    return pm::set_err(ctx, PM_ERR_BAD_ARG, "max_batch must be in 1..PM_PLONK_MAX_BATCH");
  const size_t n = key->n, B = max_batch;
  pm_plonk_batch* ws = new pm_plonk_batch();
  ws->key = key;
  ws->max_batch = max_batch;
  ws->n = n;
  const size_t bn = B * n * 32;
  const size_t const_bytes = BATCH_CONST_BYTES_FIXED + B * BATCH_CONST_BYTES_PER_PROOF;
  void* consts_d = nullptr;
  const Region regions[] = {{&ws->coeffs, 4 * bn},   {&ws->zc, bn},           {&ws->pi_coeffs, bn},    {&ws->pi_evals, bn},
                            {&ws->num, bn},          {&ws->den, bn},          {&ws->coset_w, 16 * bn}, {&ws->coset_z, 4 * bn},
                            {&ws->coset_pi, 4 * bn}, {&ws->t, 4 * bn},        {&ws->r, bn},            {&ws->agg, 2 * bn},
                            {&ws->wit, 2 * bn},
                            {&ws->pp_ctl, pm::prefix_product_batch_ctl_bytes(max_batch, n)},
                            {&ws->eval_ws, pm::evaluate_batch_ws_bytes(BATCH_EVAL_SLOTS, max_batch, n)},
                            {&ws->ruf_ws, pm::ruffini_batch_ws_bytes(2 * max_batch, n)},
                            {&consts_d, const_bytes}};
  const size_t total = carve_regions(nullptr, regions);
  int rc = pm_dev_alloc(ctx, total, &ws->base);
  if (rc) {
    (void)hipGetLastError();   // a refused hipMalloc stays the thread's last error: the next launch check would report it
    delete ws;
    return rc == PM_ERR_OOM ? pm::set_err(ctx, PM_ERR_OOM, "the batch workspace does not fit in device memory") : rc;
  }
  ws->bytes = total;
  carve_regions(ws->base, regions);
  if (hipHostMalloc(&ws->stage.h, const_bytes, hipHostMallocDefault) != hipSuccess) {
    ws->stage.h = nullptr;
    rc = pm::set_err(ctx, PM_ERR_OOM, "pinned host memory for the batch's constant tables");
  }
  ws->stage.d = (char*)consts_d;
  ws->stage.cap = const_bytes;
  if (!rc && hipStreamCreateWithFlags(&ws->side, hipStreamNonBlocking) != hipSuccess) rc = PM_ERR_HIP;
  if (!rc && hipEventCreateWithFlags(&ws->ev_main, hipEventDisableTiming) != hipSuccess) rc = PM_ERR_HIP;
  if (!rc && hipEventCreateWithFlags(&ws->ev_side, hipEventDisableTiming) != hipSuccess) rc = PM_ERR_HIP;
  if (rc) {
    pm_plonk_batch_free(ctx, ws);
    return rc;
  }
  *out = ws;
  return PM_OK;
}

extern "C" size_t pm_plonk_batch_bytes(const pm_plonk_batch* ws) { return ws ? ws->bytes : 0; }

// The padded-stride regions of zero-knowledge batches, for max_batch proofs, in one further allocation (layout at the top).
extern "C" int pm_plonk_batch_enable_zk(pm_ctx* ctx, pm_plonk_batch* ws, size_t* added_bytes) {
  if (!ctx) return PM_ERR_BAD_ARG;
  if (!ws) return pm::set_err(ctx, PM_ERR_BAD_ARG, "null argument");
  Busy guard(ws->busy);
  if (!guard.ok) return pm::set_err(ctx, PM_ERR_BUSY, "the batch workspace is in use by another call");
  if (ws->zk) {
    if (added_bytes) *added_bytes = ws->zk->bytes;
    return PM_OK;
  }
  if (!ws->key->zk) return pm::set_err(ctx, PM_ERR_BAD_ARG, "the key is not ready for zero-knowledge proofs (pm_plonk_key_enable_zk first)");
  const size_t n = ws->n, B = ws->max_batch, S = n + ZK_PAD;
  BatchZk* zk = new BatchZk();
  zk->stride = S;
  const size_t bn = B * n * 32, bs = B * S * 32;
  const Region regions[] = {{&zk->coeffs, 4 * bs},    {&zk->zc, bs},           {&zk->shift, 4 * bs},     {&zk->shift_pi, bn},
                            {&zk->coset2_w, 16 * bn}, {&zk->coset2_z, 4 * bn}, {&zk->coset2_pi, 4 * bn}, {&zk->ab, 8 * bn},
                            {&zk->t, 4 * bs},         {&zk->r, bs},            {&zk->agg, 2 * bs},       {&zk->wit, 2 * bs},
                            {&zk->eval_ws, pm::evaluate_batch_ws_bytes(BATCH_EVAL_SLOTS, ws->max_batch, S)},
                            {&zk->ruf_ws, pm::ruffini_batch_ws_bytes(2 * ws->max_batch, S)}};
  const size_t total = carve_regions(nullptr, regions);
  const int rc = pm_dev_alloc(ctx, total, &zk->base);
  if (rc) {
    (void)hipGetLastError();   // as in pm_plonk_batch_create: a refused hipMalloc must not stay the thread's last error
    delete zk;
    return rc == PM_ERR_OOM ? pm::set_err(ctx, PM_ERR_OOM, "the zero-knowledge regions of the batch workspace do not fit in device memory") : rc;
  }
  zk->bytes = total;
  carve_regions(zk->base, regions);
  ws->zk = zk;
  if (added_bytes) *added_bytes = total;
  return PM_OK;
}

extern "C" size_t pm_plonk_batch_zk_bytes(const pm_plonk_batch* ws) { return ws && ws->zk ? ws->zk->bytes : 0; }

// the argument checks and the call shared by pm_plonk_prove_batch and pm_plonk_prove_batch_zk (zero_knowledge: blinders are expected)
static int prove_batch_entry(pm_ctx* ctx, pm_prover_key* pk, pm_plonk_batch* ws, const pm_bases* ck, uint32_t batch,
                             const void* d_witnesses, const uint64_t* const* pi_positions, const uint64_t* const* pi_values,
                             const size_t* n_pi, uint32_t flags, bool zero_knowledge,
                             const uint64_t (*blinders)[PM_PLONK_ZK_BLINDERS][4], pm_plonk_proof* out) {
  if (!ctx) return PM_ERR_BAD_ARG;
  if (!pk || !ws || !ck || !d_witnesses || !out) return pm::set_err(ctx, PM_ERR_BAD_ARG, "null argument");
  if (ws->key != pk) return pm::set_err(ctx, PM_ERR_BAD_ARG, "the batch workspace was made for another key");
  if (batch == 0 || batch > ws->max_batch) return pm::set_err(ctx, PM_ERR_BAD_ARG, "batch must be in 1..max_batch of the workspace");
  PK_TRY(check_flags(ctx, flags));
  if (!pk->committed) return pm::set_err(ctx, PM_ERR_BAD_ARG, "the key is not committed (pm_plonk_key_commit first)");
  if (zero_knowledge) {
    if (!blinders) return pm::set_err(ctx, PM_ERR_BAD_ARG, "null blinders");
    for (uint32_t b = 0; b < batch; ++b)
      for (int i = 0; i < PM_PLONK_ZK_BLINDERS; ++i)
        if (pm::host::geq<4>(blinders[b][i], FRF().m)) return pm::set_err(ctx, PM_ERR_BAD_ARG, "a blinder is not below r");
  }
  Busy guard(ws->busy);
  if (!guard.ok) return pm::set_err(ctx, PM_ERR_BUSY, "the batch workspace is in use by another call");
  if (zero_knowledge && (!ws->zk || !pk->zk))
    return pm::set_err(ctx, PM_ERR_BAD_ARG, "the batch workspace is not ready for zero-knowledge proofs (pm_plonk_batch_enable_zk first)");
  const size_t n = pk->n;
  if (pm_g1_bases_len(ck) < (zero_knowledge ? n + PM_PLONK_ZK_EXTRA_BASES : n))
    return pm::set_err(ctx, PM_ERR_LENGTH, zero_knowledge ? "commit key shorter than n + PM_PLONK_ZK_EXTRA_BASES" : "commit key shorter than n");
  for (uint32_t b = 0; n_pi && b < batch; ++b) {
    if (!n_pi[b]) continue;
    if (!pi_positions || !pi_values || !pi_positions[b] || !pi_values[b])
      return pm::set_err(ctx, PM_ERR_BAD_ARG, "public inputs announced without positions or values");
    for (size_t i = 0; i < n_pi[b]; ++i)
      if (pi_positions[b][i] >= n) return pm::set_err(ctx, PM_ERR_LENGTH, "a public-input position is not below n");
  }
  if (pk->lagrange && ck != pk->lagrange_ck)
    return pm::set_err(ctx, PM_ERR_BAD_ARG, "the key's Lagrange form was checked against another commit key");
  const int rc = prove_batch_body(ctx, pk, ws, ck, batch, d_witnesses, pi_positions, pi_values, n_pi, flags,
                                  zero_knowledge ? blinders : nullptr, out);
  if (rc) {   // nothing of this call may still run on the side stream when the next one starts
    (void)hipStreamSynchronize(ws->side);
    (void)pm_sync(ctx);
  }
  return rc;
}

extern "C" int pm_plonk_prove_batch(pm_ctx* ctx, pm_prover_key* pk, pm_plonk_batch* ws, const pm_bases* ck, uint32_t batch,
                                    const void* d_witnesses, const uint64_t* const* pi_positions, const uint64_t* const* pi_values,
                                    const size_t* n_pi, uint32_t flags, pm_plonk_proof* out) {
  return prove_batch_entry(ctx, pk, ws, ck, batch, d_witnesses, pi_positions, pi_values, n_pi, flags, false, nullptr, out);
}

extern "C" int pm_plonk_prove_batch_zk(pm_ctx* ctx, pm_prover_key* pk, pm_plonk_batch* ws, const pm_bases* ck, uint32_t batch,
                                       const void* d_witnesses, const uint64_t* const* pi_positions,
                                       const uint64_t* const* pi_values, const size_t* n_pi, uint32_t flags,
                                       const uint64_t (*blinders)[PM_PLONK_ZK_BLINDERS][4], pm_plonk_proof* out) {
  return prove_batch_entry(ctx, pk, ws, ck, batch, d_witnesses, pi_positions, pi_values, n_pi, flags, true, blinders, out);
}
