// Gadget witnesses: pm_plonk_key_set_gadgets / pm_plonk_fill_gadgets_dev (included by prover.hip: the key is pm_plonk_prove's;
// DESIGN.md sections 7.2f to 7.2i).  The kernels and what each gadget writes are in gadgets.hip, what the host needs to know of a
// kind in gadget_kinds.h; here is the table a key holds and the host side of the two calls.
#include "gadget_kinds.h"

struct GadgetState {
  size_t bytes = 0;                        // device bytes held
  pm::GadgetTables dev;
  std::vector<pm::GadgetGroup> groups;     // one launch each, levels rising
  std::vector<pm::GadgetRec> recs;         // the host's copy of dev.recs (launch order): pm_hades_params_from_key, pm_jubjub_base_from_key
};

// the rows a gadget claims (the widget kinds: the trailing row included); 0: a kind, count or param that is refused whatever the
// circuit
extern "C" uint64_t pm_plonk_gadget_rows(const pm_plonk_gadget* g) {
  if (!g) return 0;
  return pm::gadget_kind_rows(pm::gadget_kind(g->kind), g->count, g->param);
}

namespace {
void gadget_state_free(pm_ctx* ctx, GadgetState* gs) {
  if (!gs) return;
  gs->dev.each_array([&](void* p, size_t, size_t) {
    if (p && ctx) (void)pm_dev_free(ctx, p);
  });
  delete gs;
}

// what the host can tell about gadget g; empty = nothing
std::string gadget_host_fault(const pm_plonk_gadget& g, const pm_plonk_gadget* prev, size_t n, size_t num_vars) {
  if (prev && g.level < prev->level) return "levels must not fall";
  const pm::GadgetKind k = pm::gadget_kind(g.kind);
  if (k.launch == pm::GadgetLaunch::NONE) return "unknown kind";
  if (!k.rows_per_param && g.param > k.max_param) return "unknown param";
  if (k.rows_per && g.count == 0) return "count is 0";
  if (k.max_count && g.count > k.max_count) return k.over_max;
  const uint64_t rows = pm::gadget_kind_rows(k, g.count, g.param);   // 0: what is left, the param of a kind with rows_per_param
  if (!rows) return "its full rounds (param) must be even and at most its rounds (count)";
  if (g.first_row >= n || rows > n - g.first_row) return "its rows leave [0, n)";
  for (uint32_t i = 0; i < k.in_vars; ++i)
    if (g.in_var[i] >= num_vars) return "in_var is not below num_vars";
  return "";
}
}  // namespace

extern "C" int pm_plonk_key_set_gadgets(pm_ctx* ctx, pm_prover_key* pk, const pm_plonk_gadget* gadgets, size_t count,
                                        size_t* added_bytes) {
  if (!ctx || !pk || (count && !gadgets)) return PM_ERR_BAD_ARG;
  if (!pk->wire_vars) return pm::set_err(ctx, PM_ERR_BAD_ARG, "the key was not built from wire variables (pm_plonk_preprocess_wires)");
  if (count > 0xffffffffull / 4) return pm::set_err(ctx, PM_ERR_BAD_ARG, "too many gadgets");
  const size_t n = pk->n;
  if (count == 0) {
    PK_TRY(pm_sync(ctx));
    gadget_state_free(ctx, pk->gadgets);
    pk->gadgets = nullptr;
    if (added_bytes) *added_bytes = 0;
    return PM_OK;
  }
  // the host's part of the check: the first gadget it objects to; the device then looks at the selectors of the ones before
  size_t lim = count;
  std::string why;
  for (size_t i = 0; i < count && why.empty(); ++i) {
    why = gadget_host_fault(gadgets[i], i ? &gadgets[i - 1] : nullptr, n, pk->num_vars);
    if (!why.empty()) lim = i;
  }
  // launch order: level, kind, index (the levels already rise: a stable order by kind inside each level)
  std::vector<pm::GadgetRec> recs;
  std::vector<pm::GadgetGroup> groups;
  uint64_t units[4] = {0, 0, 0, 0};        // by pm::GadgetTab: what the gadgets so far take of each gathered array
  uint64_t hades_rows = 0;
  bool all11 = false;
  for (size_t lo = 0; lo < lim;) {
    size_t hi = lo;
    while (hi < lim && gadgets[hi].level == gadgets[lo].level) ++hi;
    for (uint32_t kind = 0; kind < pm::GADGET_KINDS; ++kind) {
      const pm::GadgetKind k = pm::gadget_kind(kind);
      pm::GadgetGroup grp{kind, (uint32_t)recs.size(), 0, 0};
      for (size_t i = lo; i < hi; ++i) {
        const pm_plonk_gadget& g = gadgets[i];
        if (g.kind != kind) continue;
        uint64_t& used = units[(size_t)k.tab];
        recs.push_back({g.kind, g.param, (uint32_t)g.first_row, g.count, {g.in_var[0], g.in_var[1]}, (uint32_t)i, (uint32_t)used});
        if (k.tab != pm::GadgetTab::NONE) used += g.count;
        if (k.tab == pm::GadgetTab::COEF && used > 0xffffffffull) return pm::set_err(ctx, PM_ERR_BAD_ARG, "too many ARITH rows");
        if (k.tab == pm::GadgetTab::ROUNDS) hades_rows += pm::gadget_kind_rows(k, g.count, g.param);
        if (hades_rows > 0x100000000ull) return pm::set_err(ctx, PM_ERR_BAD_ARG, "too many HADES rows");
        all11 |= k.all_selectors;
        if (k.launch == pm::GadgetLaunch::BITS_X) grp.span = std::max(grp.span, g.count);
        ++grp.count;
      }
      if (grp.count) groups.push_back(grp);
    }
    lo = hi;
  }
  GadgetState* gs = new GadgetState();
  void* sel6 = nullptr;
  uint32_t bad = 0xffffffffu;
  auto body = [&]() -> int {
    if (recs.empty()) return PM_OK;
    pm::GadgetTables& t = gs->dev;
    t.count = recs.size(), t.points = units[(size_t)pm::GadgetTab::POINTS], t.arith_rows = units[(size_t)pm::GadgetTab::COEF];
    t.hades_rounds = units[(size_t)pm::GadgetTab::ROUNDS];
    int rc = PM_OK;
    t.each_array([&](void*& p, size_t n_units, size_t unit_bytes) {
      if (rc == PM_OK && n_units) rc = pm_dev_alloc(ctx, n_units * unit_bytes, &p), gs->bytes += n_units * unit_bytes;
    });
    PK_TRY(rc);
    PK_TRY(pm_dev_upload(ctx, t.recs, recs.data(), recs.size() * sizeof(pm::GadgetRec)));
    // q_l q_r | q_range q_logic q_fixed_group_add q_variable_group_add: coefficients -> values on H, one batched transform
    // a table with a kind that says so: all eleven (the rows' coefficients are part of what is checked)
    PM_HIP(ctx, hipSetDevice(ctx->device));
    if (all11) {
      PK_TRY(pm_dev_alloc(ctx, (size_t)NSEL * n * 32, &sel6));
      PK_TRY(pm_fr_ntt_dev(ctx, pk->sel_coeffs, n, n, sel6, n, pk->log_n, NSEL, 0, nullptr));
    } else {
      PK_TRY(pm_dev_alloc(ctx, 6 * n * 32, &sel6));
      PM_HIP(ctx, hipMemcpyAsync(sel6, at(pk->sel_coeffs, (size_t)Q_L * n), 2 * n * 32, hipMemcpyDeviceToDevice, ctx->stream));
      PM_HIP(ctx, hipMemcpyAsync(at(sel6, 2 * n), at(pk->sel_coeffs, (size_t)Q_RANGE * n), 4 * n * 32, hipMemcpyDeviceToDevice,
                                 ctx->stream));
      PK_TRY(pm_fr_ntt_dev(ctx, sel6, n, n, sel6, n, pk->log_n, 6, 0, nullptr));
    }
    PK_TRY(pm::gadget_verify(ctx, t, n, sel6, all11, pk->wire_vars, nullptr));
    PK_TRY(pm_dev_download(ctx, &bad, t.rep, 4));
    return pm_sync(ctx);
  };
  int rc = body();
  if (sel6) (void)pm_dev_free(ctx, sel6);
  if (rc == PM_OK && bad != 0xffffffffu)
    rc = pm::set_err(ctx, PM_ERR_BAD_ARG, "gadget " + std::to_string(bad) + pm::gadget_kind(gadgets[bad].kind).refusal);
  else if (rc == PM_OK && lim < count)
    rc = pm::set_err(ctx, PM_ERR_BAD_ARG, "gadget " + std::to_string(lim) + ": " + why);
  if (rc != PM_OK) {
    gadget_state_free(ctx, gs);
    return rc;
  }
  gs->groups = std::move(groups);
  gs->recs = std::move(recs);
  PK_TRY(pm_sync(ctx));                    // a fill on the table being replaced has finished
  gadget_state_free(ctx, pk->gadgets);
  pk->gadgets = gs;
  if (added_bytes) *added_bytes = gs->bytes;
  return PM_OK;
}

extern "C" int pm_plonk_fill_gadgets_dev(pm_ctx* ctx, const pm_prover_key* pk, void* d_vars, size_t var_stride, uint32_t batch,
                                         pm_plonk_gadget_report* reports, void* stream) {
  if (!ctx || !pk || !d_vars) return PM_ERR_BAD_ARG;
  if (!pk->wire_vars) return pm::set_err(ctx, PM_ERR_BAD_ARG, "the key was not built from wire variables (pm_plonk_preprocess_wires)");
  const GadgetState* gs = pk->gadgets;
  if (!gs) return pm::set_err(ctx, PM_ERR_BAD_ARG, "pm_plonk_key_set_gadgets first");
  if (batch == 0 || batch > PM_PLONK_MAX_BATCH) return pm::set_err(ctx, PM_ERR_BAD_ARG, "batch must be in 1..PM_PLONK_MAX_BATCH");
  if (var_stride < pk->num_vars) return pm::set_err(ctx, PM_ERR_BAD_ARG, "var_stride is below the key's num_vars");
  unsigned long long rep[2 * PM_PLONK_MAX_BATCH];
  PK_TRY(pm::gadget_fill(ctx, gs->dev, gs->groups, pk->wire_vars, pk->n, d_vars, var_stride, batch, reports ? rep : nullptr,
                         (hipStream_t)stream));
  if (reports)
    for (uint32_t b = 0; b < batch; ++b) {
      pm_plonk_gadget_report& r = reports[b];
      memset(&r, 0, sizeof r);
      r.failed = rep[b];
      r.first_gadget = r.failed ? rep[batch + b] >> 2 : UINT64_MAX;
      r.first_reason = r.failed ? (uint32_t)(rep[batch + b] & 3) : 0;
    }
  return PM_OK;
}

// Native Poseidon with the constants of a HADES gadget (hades.hip): the rounds set time gathered for it
extern "C" int pm_hades_params_from_key(pm_ctx* ctx, const pm_prover_key* pk, size_t gadget_index, pm_hades_params** out) {
  if (!ctx || !pk || !out) return PM_ERR_BAD_ARG;
  const GadgetState* gs = pk->gadgets;
  if (!gs) return pm::set_err(ctx, PM_ERR_BAD_ARG, "the key has no gadget table (pm_plonk_key_set_gadgets first)");
  for (const pm::GadgetRec& rec : gs->recs) {
    if (rec.index != gadget_index) continue;
    if (rec.kind != PM_PLONK_PERMUTATION_HADES)
      return pm::set_err(ctx, PM_ERR_BAD_ARG, "gadget " + std::to_string(gadget_index) + " is not of kind PM_PLONK_PERMUTATION_HADES");
    return pm::hades_params_from_rounds(ctx, at(gs->dev.hcoef, (size_t)rec.tab * pm::GADGET_ROUND_COEFS), rec.count, rec.param, out);
  }
  return pm::set_err(ctx, PM_ERR_BAD_ARG, "gadget_index is not below the table's count");
}

// Native JubJub with the base of a FIXED_BASE gadget (jubjub.hip): the table points set time gathered for it
extern "C" int pm_jubjub_base_from_key(pm_ctx* ctx, const pm_prover_key* pk, size_t gadget_index, pm_jubjub_base** out) {
  if (!ctx || !pk || !out) return PM_ERR_BAD_ARG;
  const GadgetState* gs = pk->gadgets;
  if (!gs) return pm::set_err(ctx, PM_ERR_BAD_ARG, "the key has no gadget table (pm_plonk_key_set_gadgets first)");
  for (const pm::GadgetRec& rec : gs->recs) {
    if (rec.index != gadget_index) continue;
    if (rec.kind != PM_PLONK_GADGET_FIXED_BASE)
      return pm::set_err(ctx, PM_ERR_BAD_ARG, "gadget " + std::to_string(gadget_index) + " is not of kind PM_PLONK_GADGET_FIXED_BASE");
    return pm::jubjub_base_from_table(ctx, at(gs->dev.tab, 2 * (size_t)rec.tab), rec.count, out);
  }
  return pm::set_err(ctx, PM_ERR_BAD_ARG, "gadget_index is not below the table's count");
}
