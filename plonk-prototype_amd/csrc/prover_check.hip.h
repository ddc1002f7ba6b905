// Witness check: pm_plonk_key_enable_check / pm_plonk_check_witness / pm_plonk_check_witness_batch (included by prover.hip: the
// key is pm_plonk_prove's).  The kernel and what "satisfied" means are in plonk_rounds.hip
// (check_witness_kernel); here is the state a key holds for it and the host side of a call.
//
// The state owns everything a check writes -- dense public inputs [B][n], row masks [B][n], counters, the staging of the
// compact public inputs -- so a check never touches the key's per-proof workspace and may run beside a proof on the key.
struct CheckState {
  size_t bytes = 0;                    // device bytes held
  void* sel_evals = nullptr;           // the stored selectors on H, n elements each
  const void* sel[NSEL] = {};          // into sel_evals; nullptr = identically zero (q_arith: or identically one)
  uint32_t* sigma = nullptr;           // 4n wire positions
  std::vector<uint32_t> sigma_host;    // the same, to recognise another permutation on a repeated enable
  uint32_t cap = 0;                    // witnesses the three arrays below hold
  void *pi = nullptr, *masks = nullptr, *counters = nullptr;
  size_t pi_cap = 0;                   // (position, value) pairs the staging holds
  void *pi_vals = nullptr, *pi_pos = nullptr;
  std::atomic<bool> busy{false};       // a check is running on this state
};

namespace {
void check_state_free(pm_ctx* ctx, CheckState* cs) {
  if (!cs) return;
  for (void* p : {cs->sel_evals, (void*)cs->sigma, cs->pi, cs->masks, cs->counters, cs->pi_vals, cs->pi_pos})
    if (p && ctx) (void)pm_dev_free(ctx, p);
  delete cs;
}

// the per-witness arrays for at least `batch` witnesses
int check_state_reserve(pm_ctx* ctx, CheckState* cs, size_t n, uint32_t batch) {
  if (batch <= cs->cap) return PM_OK;
  const size_t per = n * 32 + n + pm::CHECK_COUNTERS * 8;
  for (void** p : {&cs->pi, &cs->masks, &cs->counters}) {
    if (*p) PK_TRY(pm_dev_free(ctx, *p));
    *p = nullptr;
  }
  cs->bytes -= per * cs->cap;
  cs->cap = 0;
  PK_TRY(pm_dev_alloc(ctx, (size_t)batch * n * 32, &cs->pi));
  PK_TRY(pm_dev_alloc(ctx, (size_t)batch * n, &cs->masks));
  PK_TRY(pm_dev_alloc(ctx, (size_t)batch * pm::CHECK_COUNTERS * 8, &cs->counters));
  cs->cap = batch;
  cs->bytes += per * batch;
  return PM_OK;
}

// pi <- 0, then every witness's public inputs in one staged scatter over the global positions b n + i (a repeated position
// keeps its last value, as in scatter_public_inputs)
int check_scatter_pi(pm_ctx* ctx, CheckState* cs, size_t n, uint32_t B, const uint64_t* const* pos, const uint64_t* const* vals,
                     const size_t* n_pi) {
  PM_HIP(ctx, hipSetDevice(ctx->device));
  PM_HIP(ctx, hipMemsetAsync(cs->pi, 0, (size_t)B * n * 32, ctx->stream));
  if (!n_pi) return PM_OK;
  std::vector<unsigned long long> hp;
  std::vector<uint64_t> hv;
  for (uint32_t b = 0; b < B; ++b)
    if (n_pi[b]) compact_public_inputs(pos[b], vals[b], n_pi[b], (uint64_t)b * n, hp, hv);
  const size_t cnt = hp.size();
  if (!cnt) return PM_OK;
  if (cnt > cs->pi_cap) {
    for (void** p : {&cs->pi_vals, &cs->pi_pos}) {
      if (*p) PK_TRY(pm_dev_free(ctx, *p));
      *p = nullptr;
    }
    cs->bytes -= cs->pi_cap * 40;
    cs->pi_cap = 0;
    const size_t want = std::max<size_t>(cnt, 256);
    PK_TRY(pm_dev_alloc(ctx, want * 32, &cs->pi_vals));
    PK_TRY(pm_dev_alloc(ctx, want * 8, &cs->pi_pos));
    cs->pi_cap = want;
    cs->bytes += want * 40;
  }
  PK_TRY(pm_dev_upload(ctx, cs->pi_vals, hv.data(), cnt * 32));
  PK_TRY(pm_dev_upload(ctx, cs->pi_pos, hp.data(), cnt * 8));
  hipLaunchKernelGGL(pi_scatter_kernel, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, ctx->stream, (const uint4*)cs->pi_vals,
                     (const unsigned long long*)cs->pi_pos, cnt, (uint4*)cs->pi);
  PM_HIP(ctx, hipGetLastError());
  return PM_OK;
}

int check_witness_impl(pm_ctx* ctx, pm_prover_key* pk, uint32_t B, const void* d_wit, const uint64_t* const* pi_pos,
                       const uint64_t* const* pi_val, const size_t* n_pi, pm_plonk_witness_report* reports, uint8_t* masks_out) {
  if (!ctx || !pk || !d_wit || !reports) return PM_ERR_BAD_ARG;
  if (B == 0 || B > PM_PLONK_MAX_BATCH) return pm::set_err(ctx, PM_ERR_BAD_ARG, "batch must be in 1..PM_PLONK_MAX_BATCH");
  CheckState* cs = pk->check;
  if (!cs) return pm::set_err(ctx, PM_ERR_BAD_ARG, "pm_plonk_key_enable_check first");
  if (n_pi && (!pi_pos || !pi_val)) return PM_ERR_BAD_ARG;
  const size_t n = pk->n;
  if (n_pi)
    for (uint32_t b = 0; b < B; ++b) {
      if (n_pi[b] && (!pi_pos[b] || !pi_val[b])) return PM_ERR_BAD_ARG;
      for (size_t i = 0; i < n_pi[b]; ++i)
        if (pi_pos[b][i] >= n) return PM_ERR_LENGTH;
    }
  Busy guard(cs->busy);
  if (!guard.ok) return PM_ERR_BUSY;
  PK_TRY(check_state_reserve(ctx, cs, n, B));
  PK_TRY(check_scatter_pi(ctx, cs, n, B, pi_pos, pi_val, n_pi));
  pm::WitnessCheckArgs a;
  memset(&a, 0, sizeof a);
  a.wires = d_wit;
  for (int s = 0; s < NSEL; ++s) a.sel[s] = cs->sel[s];
  a.arith_is_one = pk->arith_is_one;
  a.pi = cs->pi;
  a.sigma = cs->sigma;
  a.masks = (uint8_t*)cs->masks;
  a.counters = (unsigned long long*)cs->counters;
  PK_TRY(pm::check_witness_rows(ctx, a, n, B, ctx->stream));
  uint64_t ctr[pm::CHECK_COUNTERS * PM_PLONK_MAX_BATCH];
  PK_TRY(pm_dev_download(ctx, ctr, cs->counters, (size_t)B * pm::CHECK_COUNTERS * 8));
  if (masks_out) PK_TRY(pm_dev_download(ctx, masks_out, cs->masks, (size_t)B * n));
  for (uint32_t b = 0; b < B; ++b) {
    pm_plonk_witness_report& r = reports[b];
    memset(&r, 0, sizeof r);
    for (int k = 0; k < 6; ++k) r.count[k] = ctr[7 * b + k];
    r.failed_rows = ctr[7 * b + 6];
    const uint64_t first = ctr[7 * (size_t)B + b];
    r.first_row = r.failed_rows ? first >> 6 : UINT64_MAX;
    r.first_mask = r.failed_rows ? (uint32_t)(first & 63) : 0;
  }
  return PM_OK;
}
}  // namespace

extern "C" int pm_plonk_key_enable_check(pm_ctx* ctx, pm_prover_key* pk, const int64_t* sigma_index, size_t* added_bytes) {
  if (!ctx || !pk || (!sigma_index && !pk->wire_vars)) return PM_ERR_BAD_ARG;
  Busy guard(pk->busy);
  if (!guard.ok) return PM_ERR_BUSY;
  const size_t n = pk->n;
  const uint32_t lg = pk->log_n;
  if (4 * n > ((size_t)1 << 32)) return pm::set_err(ctx, PM_ERR_LENGTH, "the check keeps 32-bit wire positions");
  if (!sigma_index && pk->check) {          // a key built from wires checks against its own permutation: nothing to compare
    if (added_bytes) *added_bytes = pk->check->bytes;
    return PM_OK;
  }
  std::vector<int64_t> own;                 // a key built from wires and no sigma_index: its permutation, rebuilt from the wire map
  if (!sigma_index) {
    void* d_idx = nullptr;
    own.resize(4 * n);
    int rc = pm_dev_alloc(ctx, 4 * n * 8, &d_idx);
    if (!rc) rc = pm::sigma_index_from_wires(ctx, pk->wire_vars, pk->num_vars, n, d_idx, nullptr);
    if (!rc) rc = pm_dev_download(ctx, own.data(), d_idx, 4 * n * 8);
    if (d_idx) (void)pm_dev_free(ctx, d_idx);
    if (rc != PM_OK) return rc;
    sigma_index = own.data();
  }
  std::vector<uint32_t> idx(4 * n);
  for (size_t p = 0; p < 4 * n; ++p) {
    if (sigma_index[p] < 0 || (size_t)sigma_index[p] >= 4 * n) return pm::set_err(ctx, PM_ERR_BAD_ARG, "sigma_index out of range");
    idx[p] = (uint32_t)sigma_index[p];
  }
  if (CheckState* have = pk->check) {
    if (idx != have->sigma_host) return pm::set_err(ctx, PM_ERR_BAD_ARG, "sigma_index is not the key's permutation");
    if (added_bytes) *added_bytes = have->bytes;
    return PM_OK;
  }
  CheckState* cs = new CheckState();
  void* tmp = nullptr;   // the recomputed sigma values (4n), then all selectors on H (11n)
  auto body = [&]() -> int {
    PK_TRY(check_state_reserve(ctx, cs, n, 1));
    PK_TRY(pm_dev_alloc(ctx, (size_t)NSEL * n * 32, &tmp));
    // the key keeps sigma's values only: they are a one-to-one image of the positions (k_j w^i are 4n different elements), so
    // the caller's positions are the key's exactly when they give the key's values
    u64 kk[3][4];
    for (int j = 0; j < 3; ++j) put(kk[j], pk->k[j]);
    PK_TRY(pm::sigma_evals_from_index(ctx, sigma_index, 4 * n, lg, pk->omega.l, kk, tmp));
    uint32_t differs = 0;
    PM_HIP(ctx, hipSetDevice(ctx->device));
    PM_HIP(ctx, hipMemsetAsync(cs->counters, 0, 4, ctx->stream));
    PK_TRY(pm::vec_differs(ctx, tmp, pk->sigma_evals, 4 * n, (uint32_t*)cs->counters, ctx->stream));
    PK_TRY(pm_dev_download(ctx, &differs, cs->counters, 4));
    if (differs) return pm::set_err(ctx, PM_ERR_BAD_ARG, "sigma_index is not the key's permutation");
    void* d_sigma = nullptr;
    PK_TRY(pm_dev_alloc(ctx, 4 * n * 4, &d_sigma));
    cs->sigma = (uint32_t*)d_sigma;
    cs->bytes += 4 * n * 4;
    PK_TRY(pm_dev_upload(ctx, d_sigma, idx.data(), 4 * n * 4));
    // selectors: coefficients -> values on H, one batched transform; the ones that are not trivial are kept
    int keep[NSEL], kept = 0;
    for (int s = 0; s < NSEL; ++s)
      if (!pk->sel_zero[s] && !(s == Q_ARITH && pk->arith_is_one)) keep[kept++] = s;
    if (kept) {
      PK_TRY(pm_fr_ntt_dev(ctx, pk->sel_coeffs, n, n, tmp, n, lg, NSEL, 0, nullptr));
      PK_TRY(pm_dev_alloc(ctx, (size_t)kept * n * 32, &cs->sel_evals));
      cs->bytes += (size_t)kept * n * 32;
      for (int k = 0; k < kept; ++k) {
        PM_HIP(ctx, hipMemcpyAsync(at(cs->sel_evals, (size_t)k * n), at(tmp, (size_t)keep[k] * n), n * 32, hipMemcpyDeviceToDevice,
                                   ctx->stream));
        cs->sel[keep[k]] = at(cs->sel_evals, (size_t)k * n);
      }
    }
    return pm_sync(ctx);
  };
  const int rc = body();
  if (tmp) (void)pm_dev_free(ctx, tmp);
  if (rc != PM_OK) {
    check_state_free(ctx, cs);
    return rc;
  }
  cs->sigma_host = std::move(idx);
  pk->check = cs;
  if (added_bytes) *added_bytes = cs->bytes;
  return PM_OK;
}

extern "C" int pm_plonk_check_witness(pm_ctx* ctx, pm_prover_key* pk, const void* d_witness, const uint64_t* pi_positions,
                                      const uint64_t* pi_values, size_t n_pi, pm_plonk_witness_report* out, uint8_t* row_mask_out) {
  if (n_pi && (!pi_positions || !pi_values)) return PM_ERR_BAD_ARG;
  const uint64_t* pos[1] = {pi_positions};
  const uint64_t* val[1] = {pi_values};
  return check_witness_impl(ctx, pk, 1, d_witness, pos, val, &n_pi, out, row_mask_out);
}

extern "C" int pm_plonk_check_witness_batch(pm_ctx* ctx, pm_prover_key* pk, uint32_t batch, const void* d_witnesses,
                                            const uint64_t* const* pi_positions, const uint64_t* const* pi_values, const size_t* n_pi,
                                            pm_plonk_witness_report* reports, uint8_t* row_masks_out) {
  return check_witness_impl(ctx, pk, batch, d_witnesses, (pi_positions && pi_values) ? pi_positions : nullptr, pi_values,
                            (pi_positions && pi_values) ? n_pi : nullptr, reports, row_masks_out);
}
