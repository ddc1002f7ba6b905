// Gadget witnesses: pm_plonk_key_set_gadgets / pm_plonk_fill_gadgets_dev (included by prover.hip: the key is pm_plonk_prove's;
// DESIGN.md sections 7.2f to 7.2i).  The kernels and what each gadget writes are in gadgets.hip; here is the table a key holds and the
// host side of the two calls.
struct GadgetState {
  size_t bytes = 0;                        // device bytes held
  size_t count = 0;                        // gadgets
  void* recs = nullptr;                    // pm::GadgetRec x count, in launch order
  void* tab = nullptr;                     // table points of the fixed-base rounds, 64 bytes each
  void* coef = nullptr;                    // q_m q_l q_r q_4 q_c of the ARITH rows, 160 bytes each; nullptr without such rows
  void* hcoef = nullptr;                   // round keys and matrix entries of the HADES rounds, 960 bytes each; nullptr without
  void* hids = nullptr;                    // c ids of the rows of the HADES rounds, 120 bytes each; nullptr without
  void* rep = nullptr;                     // 2 x PM_PLONK_MAX_BATCH report words
  std::vector<pm::GadgetGroup> groups;     // one launch each, levels rising
};

// the rows a gadget claims (the widget kinds: the trailing row included; the composed kinds, HADES and VAR_BASE have none); 0: a kind,
// count or param that is refused whatever the circuit
extern "C" uint64_t pm_plonk_gadget_rows(const pm_plonk_gadget* g) {
  if (!g) return 0;
  const uint64_t c = g->count, f = g->param;
  switch (g->kind) {
    case PM_PLONK_GADGET_RANGE:
    case PM_PLONK_GADGET_LOGIC:
      return c ? c + 1 : 0;
    case PM_PLONK_GADGET_FIXED_BASE:
      return c && c <= PM_PLONK_GADGET_MAX_ROUNDS ? c + 1 : 0;
    case PM_PLONK_GADGET_CURVE_ADD:
      return 2;
    case PM_PLONK_COMPOSED_ARITH:
      return c;
    case PM_PLONK_COMPOSED_BITS:
      return c && c <= PM_PLONK_COMPOSED_MAX_BITS ? 2 * c : 0;
    case PM_PLONK_COMPOSED_MAYBE_EQUAL:
      return 3;
    case PM_PLONK_PERMUTATION_HADES:   // 30 rows a full round, 18 a partial one
      return c && !(f & 1) && f <= c ? 30 * f + 18 * (c - f) : 0;
    case PM_PLONK_GADGET_VAR_BASE:     // doubling, select x, select y, addition: 2 + 1 + 1 + 2 rows a round
      return c && c <= PM_PLONK_GADGET_MAX_ROUNDS ? 6 * c : 0;
    default:
      return 0;
  }
}

namespace {
void gadget_state_free(pm_ctx* ctx, GadgetState* gs) {
  if (!gs) return;
  for (void* p : {gs->recs, gs->tab, gs->coef, gs->hcoef, gs->hids, gs->rep})
    if (p && ctx) (void)pm_dev_free(ctx, p);
  delete gs;
}

// what the host can tell about gadget g; empty = nothing
std::string gadget_host_fault(const pm_plonk_gadget& g, const pm_plonk_gadget* prev, size_t n, size_t num_vars) {
  if (prev && g.level < prev->level) return "levels must not fall";
  const bool hades = g.kind == PM_PLONK_PERMUTATION_HADES, vbase = g.kind == PM_PLONK_GADGET_VAR_BASE;
  if (g.kind > PM_PLONK_PERMUTATION_HADES && !vbase) return "unknown kind";   // 8 and 9 are no kinds
  if (!hades && g.param > (g.kind == PM_PLONK_GADGET_LOGIC ? 1u : 0u)) return "unknown param";
  const bool add = g.kind == PM_PLONK_GADGET_CURVE_ADD, eq = g.kind == PM_PLONK_COMPOSED_MAYBE_EQUAL;
  const bool run = g.kind == PM_PLONK_COMPOSED_ARITH, bits = g.kind == PM_PLONK_COMPOSED_BITS;
  if (!add && !eq && g.count == 0) return "count is 0";
  if ((g.kind == PM_PLONK_GADGET_FIXED_BASE || vbase) && g.count > PM_PLONK_GADGET_MAX_ROUNDS) return "more than PM_PLONK_GADGET_MAX_ROUNDS rounds";
  if (bits && g.count > PM_PLONK_COMPOSED_MAX_BITS) return "more than PM_PLONK_COMPOSED_MAX_BITS bits";
  if (hades && ((g.param & 1u) || g.param > g.count)) return "its full rounds (param) must be even and at most its rounds (count)";
  const uint64_t rows = pm_plonk_gadget_rows(&g);   // not 0: what makes it 0 was refused above
  if (g.first_row >= n || rows > n - g.first_row) return "its rows leave [0, n)";
  const int used = add || eq || run || hades || vbase ? 0 : g.kind == PM_PLONK_GADGET_LOGIC ? 2 : 1;
  for (int i = 0; i < used; ++i)
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
  uint32_t rounds = 0;
  uint64_t arith_rows = 0, hades_rounds = 0, hades_rows = 0;
  bool composed = false;                   // a kind that needs all eleven selectors on H
  for (size_t lo = 0; lo < lim;) {
    size_t hi = lo;
    while (hi < lim && gadgets[hi].level == gadgets[lo].level) ++hi;
    for (uint32_t kind = 0; kind <= PM_PLONK_GADGET_VAR_BASE; ++kind) {
      pm::GadgetGroup grp{kind, (uint32_t)recs.size(), 0, 0};
      for (size_t i = lo; i < hi; ++i) {
        const pm_plonk_gadget& g = gadgets[i];
        if (g.kind != kind) continue;
        const bool run = kind == PM_PLONK_COMPOSED_ARITH, hades = kind == PM_PLONK_PERMUTATION_HADES;
        pm::GadgetRec r{g.kind, g.param, (uint32_t)g.first_row, g.count, {g.in_var[0], g.in_var[1]}, (uint32_t)i,
                        run ? (uint32_t)arith_rows : hades ? (uint32_t)hades_rounds : rounds};
        if (kind == PM_PLONK_GADGET_FIXED_BASE) rounds += g.count;
        if (run) arith_rows += g.count;
        if (arith_rows > 0xffffffffull) return pm::set_err(ctx, PM_ERR_BAD_ARG, "too many ARITH rows");
        if (hades) hades_rounds += g.count, hades_rows += pm_plonk_gadget_rows(&g);
        if (hades_rows > 0x100000000ull) return pm::set_err(ctx, PM_ERR_BAD_ARG, "too many HADES rows");
        composed |= kind >= PM_PLONK_COMPOSED_ARITH;
        if (kind == PM_PLONK_COMPOSED_BITS) grp.span = std::max(grp.span, g.count);
        recs.push_back(r);
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
    PK_TRY(pm_dev_alloc(ctx, recs.size() * sizeof(pm::GadgetRec), &gs->recs));
    PK_TRY(pm_dev_alloc(ctx, std::max<size_t>(rounds, 1) * 64, &gs->tab));
    PK_TRY(pm_dev_alloc(ctx, 2 * (size_t)PM_PLONK_MAX_BATCH * 8, &gs->rep));
    gs->bytes = recs.size() * sizeof(pm::GadgetRec) + std::max<size_t>(rounds, 1) * 64 + 2 * (size_t)PM_PLONK_MAX_BATCH * 8;
    if (arith_rows) {
      PK_TRY(pm_dev_alloc(ctx, (size_t)arith_rows * 160, &gs->coef));
      gs->bytes += (size_t)arith_rows * 160;
    }
    if (hades_rounds) {
      PK_TRY(pm_dev_alloc(ctx, (size_t)hades_rounds * 960, &gs->hcoef));
      PK_TRY(pm_dev_alloc(ctx, (size_t)hades_rounds * 120, &gs->hids));
      gs->bytes += (size_t)hades_rounds * 1080;
    }
    PK_TRY(pm_dev_upload(ctx, gs->recs, recs.data(), recs.size() * sizeof(pm::GadgetRec)));
    // q_l q_r | q_range q_logic q_fixed_group_add q_variable_group_add: coefficients -> values on H, one batched transform
    // a table with a composed kind: all eleven (the rows' coefficients are part of what is checked)
    PM_HIP(ctx, hipSetDevice(ctx->device));
    if (composed) {
      PK_TRY(pm_dev_alloc(ctx, (size_t)NSEL * n * 32, &sel6));
      PK_TRY(pm_fr_ntt_dev(ctx, pk->sel_coeffs, n, n, sel6, n, pk->log_n, NSEL, 0, nullptr));
    } else {
      PK_TRY(pm_dev_alloc(ctx, 6 * n * 32, &sel6));
      PM_HIP(ctx, hipMemcpyAsync(sel6, at(pk->sel_coeffs, (size_t)Q_L * n), 2 * n * 32, hipMemcpyDeviceToDevice, ctx->stream));
      PM_HIP(ctx, hipMemcpyAsync(at(sel6, 2 * n), at(pk->sel_coeffs, (size_t)Q_RANGE * n), 4 * n * 32, hipMemcpyDeviceToDevice,
                                 ctx->stream));
      PK_TRY(pm_fr_ntt_dev(ctx, sel6, n, n, sel6, n, pk->log_n, 6, 0, nullptr));
    }
    PK_TRY(pm::gadget_verify(ctx, gs->recs, (uint32_t)recs.size(), n, sel6, composed, pk->wire_vars, gs->tab, gs->coef,
                             gs->hcoef, gs->hids, (size_t)hades_rounds, (uint32_t*)gs->rep, nullptr));
    PK_TRY(pm_dev_download(ctx, &bad, gs->rep, 4));
    return pm_sync(ctx);
  };
  int rc = body();
  if (sel6) (void)pm_dev_free(ctx, sel6);
  if (rc == PM_OK && bad != 0xffffffffu)
    rc = pm::set_err(ctx, PM_ERR_BAD_ARG,
                     "gadget " + std::to_string(bad) +
                         (gadgets[bad].kind == PM_PLONK_GADGET_VAR_BASE
                              ? ": a row it claims is not the row a variable-base round lays out (selectors, coefficients or wire variables)"
                          : gadgets[bad].kind >= PM_PLONK_COMPOSED_ARITH
                              ? ": a row it claims is not the arithmetic row its kind lays out (selectors, coefficients or wire variables)"
                              : ": a row it claims does not have its kind's selector"));
  else if (rc == PM_OK && lim < count)
    rc = pm::set_err(ctx, PM_ERR_BAD_ARG, "gadget " + std::to_string(lim) + ": " + why);
  if (rc != PM_OK) {
    gadget_state_free(ctx, gs);
    return rc;
  }
  gs->count = count;
  gs->groups = std::move(groups);
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
  PK_TRY(pm::gadget_fill(ctx, gs->recs, gs->groups.data(), gs->groups.size(), pk->wire_vars, pk->n, gs->tab, gs->coef, gs->hcoef, gs->hids, d_vars,
                         var_stride, batch, gs->rep, reports ? rep : nullptr, (hipStream_t)stream));
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
