// Host-only C++: the five PLONK prover rounds behind ONE C-ABI call (pm_plonk_preprocess /
// pm_plonk_prove), so that a Rust (or Go, or C) prover needs no host logic of its own between the
// NTT and MSM kernels -- SURVEY.md section 8f rows N1 + N2 + N3, BASELINE.json configs[3].
//
// Restates dusk_plonk::proof_system::{Prover::preprocess, Prover::prove_with_preprocessed} (dusk-plonk
// 0.8.2, ref:Cargo.toml:19; not in the reference tree) from the published design: 11 selector
// polynomials (arithmetic + q_arith, range, logic, fixed-base, variable-base), the 4-wire
// permutation, a Merlin / STROBE-128 transcript seeded with the verifier key, the 16-evaluation
// Proof, aggregate opening witnesses.  These are the gate kinds the reference's own gadgets emit
// (ref:src/zk/gadgets.rs:34,37,40,88-91,211; ref:src/zk/circuits.rs:64-70).  PARITY UNPINNED:
// formulas and transcript labels are restated, not compared with upstream bytes.  Everything here is
// sequencing and scalar arithmetic on a few dozen field elements: the vector work is done by the
// library's own entry points, called like any client would call them.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <string>
#include <unordered_map>
#include <vector>

#include "context.h"
#include "prover_rounds.h"

// Zero-knowledge mode (pm_plonk_key_enable_zk): the second 4n coset 7 w_8n H_4n of the key and a
// per-proof workspace whose coefficient vectors have the padded stride S = n + ZK_PAD (zero tails).
constexpr size_t ZK_PAD = 16;
struct ZkState {
  size_t stride = 0, bytes = 0;
  HFr zh_inv2[4], inv2, inv2s;        // 1 / Z_H on the second coset by i mod 4; 1 / 2; 1 / (2 * 7^4n)
  void *w8 = nullptr /* w_8n^i, 4n */, *x2 = nullptr /* 7 w_8n w_4n^i, 4n */, *sigma_coset2 = nullptr /* 16n */,
       *l1_coset2 = nullptr;
  void* sel_coset2[NSEL] = {};        // where the key has sel_coset
  // per proof: coeffs [a b c d z pi] 6 S | shift 6 S | coset2 [a b c d z pi] 24 n | ab 8 n | t 4 S | r S | agg S | wit 2 S
  void *coeffs = nullptr, *shift = nullptr, *coset2 = nullptr, *ab = nullptr, *t = nullptr, *r = nullptr, *agg = nullptr,
       *wit = nullptr;
};

// Witness check (pm_plonk_key_enable_check): prover_check.hip.h
struct CheckState;
// Gadget witnesses (pm_plonk_key_set_gadgets): prover_gadgets.hip.h
struct GadgetState;
namespace {
void check_state_free(pm_ctx* ctx, CheckState* cs);
void gadget_state_free(pm_ctx* ctx, GadgetState* gs);
}

struct pm_prover_key {
  size_t n = 0;
  uint32_t log_n = 0;
  HFr omega, k[3], zh_inv[4];
  // device arrays (pm_dev_alloc)
  void *roots = nullptr, *x4 = nullptr, *sel_coeffs = nullptr /* 11 n */, *sigma_evals = nullptr,
       *sigma_coeffs = nullptr, *sigma_coset = nullptr, *l1_coset = nullptr;
  void* sel_coset[NSEL] = {};         // 4n each; nullptr where the quotient kernel does not read it
  bool sel_zero[NSEL] = {};           // identically zero
  bool arith_is_one = false;          // q_arith = 1 everywhere: the kernel skips the multiplication
  // per-proof workspace: coeffs [a b c d z pi] 6n | num n | den n | coset 24n | t 4n | r n | agg n | wit 2n | pi n
  void *coeffs = nullptr, *num = nullptr, *den = nullptr, *coset = nullptr, *t = nullptr, *r = nullptr, *agg = nullptr,
       *wit = nullptr, *pi_evals = nullptr;
  // verifier key (commitments to the 11 selector and 4 sigma polynomials) and the transcript seeded with it
  bool committed = false;
  u64 vk[NSEL + 4][12] = {};
  Transcript base{std::string("plonk")};   // overwritten by key_commit (tl::PROTOCOL or the caller's label)
  std::atomic<bool> busy{false};       // a proof is running on this key's workspace
  hipStream_t side = nullptr;         // second stream: work that does not depend on the next challenge
  hipEvent_t ev_main = nullptr, ev_side = nullptr;
  // Lagrange-form commit key (pm_plonk_key_set_lagrange; not owned) and the commit key it was checked against
  const pm_bases* lagrange = nullptr;
  const pm_bases* lagrange_ck = nullptr;
  ZkState* zk = nullptr;               // pm_plonk_key_enable_zk
  CheckState* check = nullptr;         // pm_plonk_key_enable_check
  // pm_plonk_preprocess_wires: the wire map (4n x uint32) the permutation was built from; nullptr on a key from sigma_index
  void* wire_vars = nullptr;
  size_t num_vars = 0;
  GadgetState* gadgets = nullptr;      // pm_plonk_key_set_gadgets
};

// side stream <- everything submitted on the context's stream so far / the reverse
static int pm_stream_fork(pm_ctx* ctx, hipStream_t side, hipEvent_t ev) {
  PM_HIP(ctx, hipEventRecord(ev, ctx->stream));
  PM_HIP(ctx, hipStreamWaitEvent(side, ev, 0));
  return PM_OK;
}
static int pm_stream_join(pm_ctx* ctx, hipStream_t side, hipEvent_t ev) {
  PM_HIP(ctx, hipEventRecord(ev, side));
  PM_HIP(ctx, hipStreamWaitEvent(ctx->stream, ev, 0));
  return PM_OK;
}

#define PK_TRY(call)            \
  do {                          \
    int rc_ = (call);           \
    if (rc_ != PM_OK) return rc_; \
  } while (0)

// the flags of a prove call, on every path
static int check_flags(pm_ctx* ctx, uint32_t flags) {
  if (flags & ~(PM_PLONK_BIND_PUBLIC_INPUTS | PM_PLONK_UPSTREAM_TRANSCRIPT)) return pm::set_err(ctx, PM_ERR_BAD_ARG, "unknown flags");
  if (flags == (PM_PLONK_BIND_PUBLIC_INPUTS | PM_PLONK_UPSTREAM_TRANSCRIPT))
    return pm::set_err(ctx, PM_ERR_BAD_ARG, "PM_PLONK_BIND_PUBLIC_INPUTS and PM_PLONK_UPSTREAM_TRANSCRIPT exclude each other");
  return PM_OK;
}

extern "C" void pm_plonk_key_free(pm_ctx* ctx, pm_prover_key* pk) {
  if (!pk) return;
  if (ctx) (void)pm_sync(ctx);
  if (pk->side) {
    (void)hipStreamSynchronize(pk->side);
    (void)hipStreamDestroy(pk->side);
  }
  if (pk->ev_main) (void)hipEventDestroy(pk->ev_main);
  if (pk->ev_side) (void)hipEventDestroy(pk->ev_side);
  for (void* p : {pk->roots, pk->x4, pk->sel_coeffs, pk->sigma_evals, pk->sigma_coeffs, pk->sigma_coset,
                  pk->l1_coset, pk->coeffs, pk->num, pk->den, pk->coset, pk->t, pk->r, pk->agg, pk->wit, pk->pi_evals,
                  pk->wire_vars})
    if (p && ctx) (void)pm_dev_free(ctx, p);
  for (void* p : pk->sel_coset)
    if (p && ctx) (void)pm_dev_free(ctx, p);
  if (ZkState* zs = pk->zk) {
    for (void* p : {zs->w8, zs->x2, zs->sigma_coset2, zs->l1_coset2, zs->coeffs, zs->shift, zs->coset2, zs->ab, zs->t, zs->r,
                    zs->agg, zs->wit})
      if (p && ctx) (void)pm_dev_free(ctx, p);
    for (void* p : zs->sel_coset2)
      if (p && ctx) (void)pm_dev_free(ctx, p);
    delete zs;
  }
  check_state_free(ctx, pk->check);
  gadget_state_free(ctx, pk->gadgets);
  delete pk;
}

// pm_plonk_preprocess (the permutation as sigma_index, host) and pm_plonk_preprocess_wires (as wire_vars, host: sigma_index is
// built on the device and never leaves it) -- exactly one of the two is given
static int preprocess_impl(pm_ctx* ctx, const uint64_t* const selectors[PM_PLONK_SELECTORS], const int64_t* sigma_index,
                           const uint32_t* wire_vars, size_t num_vars, size_t n, pm_prover_key** out) {
  if (!ctx || !selectors || (!sigma_index && !wire_vars) || !out) return PM_ERR_BAD_ARG;
  *out = nullptr;
  if (n < 4 || (n & (n - 1))) return PM_ERR_LENGTH;
  pm_prover_key* pk = new pm_prover_key();
  pk->n = n;
  while (((size_t)1 << pk->log_n) < n) ++pk->log_n;
  const uint32_t lg = pk->log_n;
  u64 w[4], wi[4], si[4], w4[4];
  int rc = pm_domain_info(lg, w, wi, si);
  if (!rc) rc = pm_domain_info(lg + 2, w4, wi, wi);
  if (rc) {
    delete pk;
    return rc;
  }
  pk->omega = get(w);
  const HFr n_inv = get(si), omega4 = get(w4), one = fone(), g = fr_u64(7);
  pk->k[0] = fr_u64(7);
  pk->k[1] = fr_u64(13);
  pk->k[2] = fr_u64(17);
  // which selector polynomials are trivial: the quotient kernel skips what it can
  pk->arith_is_one = selectors[Q_ARITH] != nullptr;
  for (int s = 0; s < NSEL; ++s) {
    bool zero = true;
    if (selectors[s]) {
      for (size_t i = 0; i < 4 * n && zero; ++i) zero = selectors[s][i] == 0;
    }
    pk->sel_zero[s] = zero;
  }
  if (selectors[Q_ARITH])
    for (size_t i = 0; i < n && pk->arith_is_one; ++i) pk->arith_is_one = memcmp(selectors[Q_ARITH] + 4 * i, one.l, 32) == 0;
  struct Alloc { void** p; size_t elems; };
  std::vector<Alloc> allocs = {{&pk->roots, n},          {&pk->x4, 4 * n},           {&pk->sel_coeffs, (size_t)NSEL * n},
                               {&pk->sigma_evals, 4 * n}, {&pk->sigma_coeffs, 4 * n}, {&pk->sigma_coset, 16 * n},
                               {&pk->l1_coset, 4 * n},    {&pk->coeffs, 6 * n},       {&pk->num, n},
                               {&pk->den, n},             {&pk->coset, 24 * n},       {&pk->t, 4 * n},
                               {&pk->r, n},               {&pk->agg, n},              {&pk->wit, 2 * n},
                               {&pk->pi_evals, n}};
  for (int s = 0; s < NSEL; ++s) {
    const bool need = s <= Q_4 || (s == Q_ARITH ? !pk->arith_is_one : !pk->sel_zero[s]);
    if (need) allocs.push_back({&pk->sel_coset[s], 4 * n});
  }
  for (const Alloc& a : allocs)
    if ((rc = pm_dev_alloc(ctx, a.elems * 32, a.p)) != PM_OK) break;
  void* tmp = nullptr;
  if (!rc) rc = pm_fr_powers_dev(ctx, pk->omega.l, one.l, n, pk->roots, nullptr);
  if (!rc) rc = pm_fr_powers_dev(ctx, omega4.l, g.l, 4 * n, pk->x4, nullptr);
  // selectors: evaluations -> coefficients -> 4n coset (only the coset forms the quotient kernel reads)
  if (!rc) rc = pm_dev_alloc(ctx, (size_t)NSEL * n * 32, &tmp);
  const HFr zero = pm::host::zero<4>();
  for (int s = 0; s < NSEL && !rc; ++s) {
    if (pk->sel_zero[s]) rc = pm_fr_powers_dev(ctx, zero.l, zero.l, n, at(tmp, s * n), nullptr);
    else rc = pm_dev_upload(ctx, at(tmp, s * n), selectors[s], n * 32);
  }
  if (!rc) rc = pm_fr_ntt_dev(ctx, tmp, n, n, pk->sel_coeffs, n, lg, NSEL, PM_NTT_INVERSE, nullptr);
  for (int s = 0; s < NSEL && !rc; ++s)
    if (pk->sel_coset[s])
      rc = pm_fr_ntt_dev(ctx, at(pk->sel_coeffs, s * n), n, n, pk->sel_coset[s], 4 * n, lg + 2, 1, PM_NTT_COSET, nullptr);
  // sigma_j(w^i) = k_j' w^i': the indices are checked here (a permutation of the 4n wire positions), the values gathered on
  // the device (r01 - r04: a 4n x 32-byte table went to the host and back)
  if (!rc && sigma_index) {
    std::vector<uint8_t> seen(4 * n, 0);
    for (size_t p = 0; p < 4 * n && !rc; ++p) {
      const int64_t q = sigma_index[p];
      if (q < 0 || (size_t)q >= 4 * n || seen[q]) rc = PM_ERR_BAD_ARG;   // not a permutation
      else seen[q] = 1;
    }
  }
  u64 kk[3][4];
  for (int j = 0; j < 3; ++j) put(kk[j], pk->k[j]);
  if (!rc && sigma_index) rc = pm::sigma_evals_from_index(ctx, sigma_index, 4 * n, lg, pk->omega.l, kk, pk->sigma_evals);
  if (!rc && wire_vars) {
    // the cycles of the wire map are a permutation by construction: nothing to check on the host
    void* d_idx = nullptr;
    rc = pm_dev_alloc(ctx, 4 * n * 4, &pk->wire_vars);
    if (!rc) rc = pm_dev_upload(ctx, pk->wire_vars, wire_vars, 4 * n * 4);
    if (!rc) rc = pm_dev_alloc(ctx, 4 * n * 8, &d_idx);
    if (!rc) rc = pm::sigma_index_from_wires(ctx, pk->wire_vars, num_vars, n, d_idx, nullptr);
    if (!rc) rc = pm::sigma_evals_from_index_dev(ctx, d_idx, 4 * n, lg, pk->omega.l, kk, pk->sigma_evals);
    if (d_idx) (void)pm_dev_free(ctx, d_idx);
    pk->num_vars = num_vars;
  }
  if (!rc) rc = pm_fr_ntt_dev(ctx, pk->sigma_evals, n, n, pk->sigma_coeffs, n, lg, 4, PM_NTT_INVERSE, nullptr);
  if (!rc) rc = pm_fr_ntt_dev(ctx, pk->sigma_coeffs, n, n, pk->sigma_coset, 4 * n, lg + 2, 4, PM_NTT_COSET, nullptr);
  // L_1 = (1/n) sum X^i on the coset
  if (!rc) rc = pm_fr_powers_dev(ctx, one.l, n_inv.l, n, tmp, nullptr);
  if (!rc) rc = pm_fr_ntt_dev(ctx, tmp, n, n, pk->l1_coset, 4 * n, lg + 2, 1, PM_NTT_COSET, nullptr);
  if (!rc) rc = pm_sync(ctx);
  if (tmp) (void)pm_dev_free(ctx, tmp);
  if (!rc) zh_inv_period4(g, omega4, n, pk->zh_inv);
  if (!rc && hipStreamCreateWithFlags(&pk->side, hipStreamNonBlocking) != hipSuccess) rc = PM_ERR_HIP;
  if (!rc && hipEventCreateWithFlags(&pk->ev_main, hipEventDisableTiming) != hipSuccess) rc = PM_ERR_HIP;
  if (!rc && hipEventCreateWithFlags(&pk->ev_side, hipEventDisableTiming) != hipSuccess) rc = PM_ERR_HIP;
  if (rc) {
    pm_plonk_key_free(ctx, pk);
    return rc;
  }
  *out = pk;
  return PM_OK;
}

extern "C" int pm_plonk_preprocess(pm_ctx* ctx, const uint64_t* const selectors[PM_PLONK_SELECTORS],
                                   const int64_t* sigma_index, size_t n, pm_prover_key** out) {
  if (!sigma_index) return PM_ERR_BAD_ARG;
  return preprocess_impl(ctx, selectors, sigma_index, nullptr, 0, n, out);
}

extern "C" int pm_plonk_preprocess_wires(pm_ctx* ctx, const uint64_t* const selectors[PM_PLONK_SELECTORS],
                                         const uint32_t* wire_vars, size_t num_vars, size_t n, pm_prover_key** out) {
  if (!wire_vars) return PM_ERR_BAD_ARG;
  return preprocess_impl(ctx, selectors, nullptr, wire_vars, num_vars, n, out);
}

extern "C" size_t pm_plonk_key_num_vars(const pm_prover_key* pk) { return pk && pk->wire_vars ? pk->num_vars : 0; }

extern "C" int pm_plonk_witness_from_vars_dev(pm_ctx* ctx, const pm_prover_key* pk, const void* d_vars, size_t var_stride,
                                              uint32_t batch, void* d_witness_out, void* stream) {
  if (!ctx || !pk || !d_vars || !d_witness_out) return PM_ERR_BAD_ARG;
  if (!pk->wire_vars) return pm::set_err(ctx, PM_ERR_BAD_ARG, "the key was not built from wire variables (pm_plonk_preprocess_wires)");
  if (batch == 0 || batch > PM_PLONK_MAX_BATCH) return pm::set_err(ctx, PM_ERR_BAD_ARG, "batch must be in 1..PM_PLONK_MAX_BATCH");
  if (var_stride < pk->num_vars) return pm::set_err(ctx, PM_ERR_BAD_ARG, "var_stride is below the key's num_vars");
  return pm::witness_from_vars(ctx, pk->wire_vars, pk->n, d_vars, var_stride, batch, d_witness_out, (hipStream_t)stream);
}

// Commitments to `batch` coefficient vectors of n elements.  With the SRS split over ranks (shard.fn set)
// this rank's bases cover coefficients [shard.lo, shard.lo + len(ck)): it computes the partial sums of its
// slice and the exchange callback returns the sums over all ranks (all-gather + group-law fold).  A rank
// whose local MSM fails still enters the exchange (with an abort marker) so that its peers do not block.
struct Shard {
  size_t lo = 0;
  bool on = false;             // the SRS is split: partial sums are exchanged
  pm_exchange_fn fn = nullptr; // nullptr with on = true: the context's RCCL communicator (pm_g1_allgather_fold)
  void* user = nullptr;
  mutable bool aborted = false;   // an exchange of this call already carried / returned the abort marker
  // How many exchanges the call makes on every rank (key commit: slice cover + two batches; proof: four commit batches)
  // and how many this rank has completed: an error AFTER the last one must not put one more collective on the wire
  // -- no peer would be waiting for it, and it would pair with the first exchange of the peers' next call.
  int expect = 0;
  mutable int done = 0;
};
// One exchange of k partial points (k = 0: the abort marker).
static int shard_exchange(pm_ctx* ctx, const Shard& sh, u64* xyz, uint32_t k) {
  {
    std::lock_guard<std::mutex> lk(ctx->mu);
    ++ctx->stat_allgather_calls;
  }
  const int rc = sh.fn ? (sh.fn(sh.user, xyz, k) != 0 ? PM_ERR_EXCHANGE : PM_OK) : pm_g1_allgather_fold(ctx, xyz, k);
  ++sh.done;
  if (k == 0 || rc != PM_OK) sh.aborted = true;
  return k == 0 && rc == PM_OK ? PM_ERR_EXCHANGE : rc;
}
// A sharded call that fails anywhere OUTSIDE an exchange -- an NTT, the quotient, an allocation, an argument that is
// wrong on this rank only -- must still meet its peers in their next collective, or they block in it for ever
// (ncclAllGather has no timeout): one abort marker, after which every rank returns an error.
static int shard_leave(pm_ctx* ctx, const Shard& sh, int rc) {
  if (rc != PM_OK && sh.on && ctx && !sh.aborted && sh.done < sh.expect) {
    u64 xyz[18] = {0};
    (void)shard_exchange(ctx, sh, xyz, 0);
  }
  return rc;
}
static int commit_batch(pm_ctx* ctx, const pm_bases* ck, const Shard& sh, const void* d, size_t n, size_t stride,
                        uint32_t batch, u64 (*out_xy)[12]) {
  u64 xyz[16 * 18];
  if (batch > 16) return PM_ERR_BAD_ARG;
  const size_t have = pm_g1_bases_len(ck);
  size_t cnt = n;
  if (sh.on) cnt = sh.lo < n ? std::min(have, n - sh.lo) : 0;
  int rc = PM_OK;
  if (cnt > 0) {
    rc = pm_g1_msm_batch_dev(ctx, ck, 0, cnt, at((void*)d, sh.lo), stride, batch, PM_SCALAR_MONTGOMERY, xyz, nullptr);
  } else {
    memset(xyz, 0, sizeof xyz);
    for (uint32_t b = 0; b < batch; ++b) memcpy(xyz + 18 * b + 6, pm::host::FP().one, 48);   // (0, 1, 0)
  }
  if (sh.on) {
    // k = 0 tells the peers that this rank gave up: they get an error back and stop too
    const int xrc = shard_exchange(ctx, sh, xyz, rc == PM_OK ? batch : 0);
    if (rc == PM_OK && xrc != PM_OK) rc = xrc;
  }
  if (rc) return rc;
  return pm_g1_to_affine_batch(xyz, batch, &out_xy[0][0], nullptr);   // one host inversion per batch
}

// The ranks' SRS slices must tile [0, n): a gap or an overlap would give a well-formed but wrong commitment that no
// rank can see.  One extra exchange per key: every rank contributes len * G and S_rank * G with
//     S_rank = sum over its coefficient indices i of rho^i      (G the group generator, host-side scalar multiplications),
// rho a fixed element of Fr of no special structure; the folded sums must be n * G and (rho^n - 1) / (rho - 1) * G.
// sum_ranks S_rank is the polynomial  sum_i m_i X^i  at rho, m_i = how many ranks hold coefficient i: it equals
// 1 + X + ... + X^(n-1) as a polynomial exactly when every m_i is 1, and two different polynomials of degree < 2^32
// agree at a point that was fixed without looking at them with probability < 2^-220 -- this is a guard against
// mis-configured ranks, not against an adversary.  (r03 compared two moments, count and index sum: slices shifted
// symmetrically about a centre passed both)
static const u64 COVER_RHO[4] = {0x9e3779b97f4a7c15ULL, 0xbf58476d1ce4e5b9ULL, 0x94d049bb133111ebULL, 0x2545f4914f6cdd1dULL};
static HFr cover_rho() {                      // the 254-bit constant above (< r), into Montgomery form
  HFr raw, r2;
  memcpy(raw.l, COVER_RHO, 32);
  memcpy(r2.l, FRF().r2, 32);
  return fmul(raw, r2);
}
// sum_{i = lo}^{lo + cnt - 1} rho^i = rho^lo (rho^cnt - 1) / (rho - 1)
static HFr cover_sum(u64 lo, u64 cnt) {
  const HFr rho = cover_rho();
  return fmul(fmul(fpow(rho, lo), fsub(fpow(rho, cnt), fone())), finv(fsub(rho, fone())));
}
static pm::host::XYZZ host_mul_generator(const u64 k[4]) {
  using namespace pm::host;
  // the BLS12-381 G1 generator, canonical limbs -> Montgomery
  static const u64 GX[6] = {0xfb3af00adb22c6bbULL, 0x6c55e83ff97a1aefULL, 0xa14e3a3f171bac58ULL,
                            0xc3688c4f9774b905ULL, 0x2695638c4fa9ac0fULL, 0x17f1d3a73197d794ULL};
  static const u64 GY[6] = {0x0caa232946c5e7e1ULL, 0xd03cc744a2888ae4ULL, 0x00db18cb2c04b3edULL,
                            0xfcf5e095d5d00af6ULL, 0xa09e30ed741d8ae4ULL, 0x08b3f481e3aaa0f1ULL};
  const Field<6>& F = FP();
  HFp r2, x, y;
  memcpy(r2.l, F.r2, 48);
  memcpy(x.l, GX, 48);
  memcpy(y.l, GY, 48);
  XYZZ g;
  g.x = mul(x, r2, F);
  g.y = mul(y, r2, F);
  g.zz = one(F);
  g.zzz = one(F);
  XYZZ acc = xyzz_identity();
  for (int bit = 255; bit >= 0; --bit) {
    acc = xyzz_double(acc);
    if ((k[bit >> 6] >> (bit & 63)) & 1) acc = xyzz_add(acc, g);
  }
  return acc;
}
static pm::host::XYZZ host_mul_generator(u64 k) {
  const u64 kk[4] = {k, 0, 0, 0};
  return host_mul_generator(kk);
}
static pm::host::XYZZ host_mul_generator(const HFr& k) { return host_mul_generator(fr_canonical(k).l); }
static void host_to_projective(const pm::host::XYZZ& p, u64 out[18]) {
  pm::host::HFp x, y;
  memset(out, 0, 144);
  if (!pm::host::xyzz_to_affine(p, x, y)) {
    memcpy(out + 6, pm::host::FP().one, 48);   // (0, 1, 0)
    return;
  }
  memcpy(out, x.l, 48);
  memcpy(out + 6, y.l, 48);
  memcpy(out + 12, pm::host::FP().one, 48);
}
static int check_slice_cover(pm_ctx* ctx, const pm_bases* ck, const Shard& sh, size_t n) {
  const size_t have = pm_g1_bases_len(ck);
  const u64 cnt = sh.lo < n ? std::min<size_t>(have, n - sh.lo) : 0;
  u64 xyz[2 * 18], want[2 * 18], got_xy[2 * 12], want_xy[2 * 12];
  host_to_projective(host_mul_generator(cnt), xyz);
  host_to_projective(host_mul_generator(cover_sum(sh.lo, cnt)), xyz + 18);
  host_to_projective(host_mul_generator((u64)n), want);
  host_to_projective(host_mul_generator(cover_sum(0, n)), want + 18);
  PK_TRY(shard_exchange(ctx, sh, xyz, 2));
  PK_TRY(pm_g1_to_affine_batch(xyz, 2, got_xy, nullptr));
  PK_TRY(pm_g1_to_affine_batch(want, 2, want_xy, nullptr));
  if (memcmp(got_xy, want_xy, sizeof got_xy) != 0) {
    ctx->err = "the ranks' commit-key slices do not tile [0, n): a gap or an overlap";
    return PM_ERR_LENGTH;
  }
  return PM_OK;
}

static int key_commit_body(pm_ctx* ctx, pm_prover_key* pk, const pm_bases* ck, const Shard& shard,
                           const char* transcript_label, uint64_t (*vk_out)[12]) {
  if (!ctx || !pk || !ck) return PM_ERR_BAD_ARG;
  const size_t n = pk->n;
  if (!shard.on && pm_g1_bases_len(ck) < n) return PM_ERR_LENGTH;
  if (shard.on) PK_TRY(check_slice_cover(ctx, ck, shard, n));
  // the verifier key: commitments to the 11 selector and the 4 sigma polynomials
  PK_TRY(commit_batch(ctx, ck, shard, pk->sel_coeffs, n, n, NSEL, &pk->vk[0]));
  PK_TRY(commit_batch(ctx, ck, shard, pk->sigma_coeffs, n, n, 4, &pk->vk[NSEL]));
  pk->base = key_transcript(transcript_label, pk->vk, n);
  pk->committed = true;
  if (vk_out) memcpy(vk_out, pk->vk, sizeof pk->vk);
  return PM_OK;
}
static int key_commit_impl(pm_ctx* ctx, pm_prover_key* pk, const pm_bases* ck, const Shard& shard,
                           const char* transcript_label, uint64_t (*vk_out)[12]) {
  return shard_leave(ctx, shard, key_commit_body(ctx, pk, ck, shard, transcript_label, vk_out));
}

// The label table of prover_transcript.h as text, one "key=label" line per entry in transcript order (the verifier side in Python reads it:
// one table for both sides).
extern "C" const char* pm_plonk_transcript_labels(void) {
  static const std::string text = [] {
    std::string t;
    auto add = [&](const std::string& k, const char* v) { t += k + "=" + v + "\n"; };
    add("protocol", tl::PROTOCOL);
    for (int i = 0; i < NSEL; ++i) add("selector_" + std::to_string(i), tl::SELECTORS[i]);
    for (int i = 0; i < 4; ++i) add("sigma_" + std::to_string(i), tl::SIGMAS[i]);
    add("dom_sep", tl::DOM_SEP);
    add("dom_sep_value", tl::DOM_SEP_VALUE);
    add("circuit_size", tl::CIRCUIT_SIZE);
    add("pi_len", tl::PI_LEN);
    add("pi_pos", tl::PI_POS);
    add("pi_value", tl::PI_VALUE);
    for (int i = 0; i < 4; ++i) add("wire_" + std::to_string(i), tl::WIRES[i]);
    add("beta", tl::BETA);
    add("gamma", tl::GAMMA);
    add("perm", tl::PERM);
    add("alpha", tl::ALPHA);
    add("range_sep", tl::RANGE_SEP);
    add("logic_sep", tl::LOGIC_SEP);
    add("fixed_sep", tl::FIXED_SEP);
    add("var_sep", tl::VAR_SEP);
    for (int i = 0; i < 4; ++i) add("quotient_" + std::to_string(i), tl::QUOTIENT[i]);
    add("z_challenge", tl::Z_CHALLENGE);
    for (int i = 0; i < 17; ++i) add("eval_" + std::to_string(i), tl::EVALS[i]);
    add("aggregate", tl::AGGREGATE);
    add("w_z", tl::W_Z);
    add("w_zw", tl::W_ZW);
    add("batch", tl::BATCH);
    return t;
  }();
  return text.c_str();
}

extern "C" int pm_plonk_key_commit(pm_ctx* ctx, pm_prover_key* key, const pm_bases* commit_key, const char* transcript_label,
                                   uint64_t (*verifier_key_out)[12]) {
  return key_commit_impl(ctx, key, commit_key, Shard(), transcript_label, verifier_key_out);
}
extern "C" int pm_plonk_key_commit_sharded(pm_ctx* ctx, pm_prover_key* key, const pm_bases* commit_key_slice,
                                           size_t first_coefficient, pm_exchange_fn exchange, void* user,
                                           const char* transcript_label, uint64_t (*verifier_key_out)[12]) {
  Shard sh;
  sh.on = true;
  sh.lo = first_coefficient;
  sh.fn = exchange;
  sh.user = user;
  sh.expect = 3;
  return key_commit_impl(ctx, key, commit_key_slice, sh, transcript_label, verifier_key_out);
}

// sum_i L_i = powers[0] and sum_i w^i L_i = powers[1]: two MSMs over the Lagrange key (scalars 1 and the key's roots of
// unity) against the first two points of the commit key.  Together they pin the key to the commit key's tau.
extern "C" int pm_plonk_key_set_lagrange(pm_ctx* ctx, pm_prover_key* key, const pm_bases* commit_key, const pm_bases* lagrange) {
  if (!ctx || !key) return PM_ERR_BAD_ARG;
  Busy guard(key->busy);
  if (!guard.ok) return PM_ERR_BUSY;
  if (!lagrange) {
    key->lagrange = nullptr;
    key->lagrange_ck = nullptr;
    return PM_OK;
  }
  if (!commit_key) return PM_ERR_BAD_ARG;
  const size_t n = key->n;
  if (pm_g1_bases_len(lagrange) != n) return pm::set_err(ctx, PM_ERR_LENGTH, "the Lagrange key must hold exactly n points");
  if (pm_g1_bases_len(commit_key) < std::max<size_t>(n, 2)) return pm::set_err(ctx, PM_ERR_LENGTH, "commit key shorter than n");
  void* d_sc = nullptr;
  PK_TRY(pm_dev_alloc(ctx, 2 * n * 32, &d_sc));
  const HFr one = fone();
  u64 xyz[2 * 18], got[2][12];
  int ident[2];
  int rc = pm_fr_powers_dev(ctx, one.l, one.l, n, d_sc, nullptr);
  if (!rc) rc = pm_fr_powers_dev(ctx, key->omega.l, one.l, n, at(d_sc, n), nullptr);
  if (!rc) rc = pm_g1_msm_batch_dev(ctx, lagrange, 0, n, d_sc, n, 2, PM_SCALAR_MONTGOMERY, xyz, nullptr);
  (void)pm_dev_free(ctx, d_sc);
  if (!rc) rc = pm_g1_to_affine_batch(xyz, 2, &got[0][0], ident);
  // the commit key's first two points: device form (x 2^392) -> ABI Montgomery (x 2^384): one product by 2^376
  u64 want[2][12];
  if (!rc) rc = pm_dev_download(ctx, want, commit_key->d_xy, sizeof want);
  if (rc) return rc;
  const pm::host::Field<6>& F = pm::host::FP();
  const pm::host::HFp c = pm::host::inv(pm::host::from_u64(256, F), F);
  for (int p = 0; p < 2; ++p)
    for (int h = 0; h < 2; ++h) {
      pm::host::HFp v;
      memcpy(v.l, want[p] + 6 * h, 48);
      v = pm::host::mul(v, c, F);
      memcpy(want[p] + 6 * h, v.l, 48);
    }
  if (memcmp(got, want, sizeof want) != 0)
    return pm::set_err(ctx, PM_ERR_BAD_ARG, "the Lagrange key does not match the commit key (sum L_i != powers[0] or sum w^i L_i != powers[1])");
  key->lagrange = lagrange;
  key->lagrange_ck = commit_key;
  return PM_OK;
}

// The key's side of the zero-knowledge mode.  A blinded quotient t' has degree up to 4n + 9, more
// than the 4n points of the coset 7 H_4n determine; the second coset 7 w_8n H_4n (x^4n = -7^4n there, against +7^4n on the
// first) gives t' mod (X^4n + s) beside t' mod (X^4n - s).  On it x^n = 7^n w_8 w_4^i, so 1 / Z_H still has period 4 and the
// next row is still index + 4: pm_plonk_quotient_dev runs unchanged, given this coset's x, 1 / Z_H and the key's
// polynomials there -- the selectors it reads, the sigmas and L_1, built here once.
extern "C" int pm_plonk_key_enable_zk(pm_ctx* ctx, pm_prover_key* pk, size_t* added_bytes) {
  if (!ctx || !pk) return PM_ERR_BAD_ARG;
  if (!pk->committed) return pm::set_err(ctx, PM_ERR_BAD_ARG, "pm_plonk_key_commit first");
  Busy guard(pk->busy);
  if (!guard.ok) return PM_ERR_BUSY;
  if (pk->zk) {
    if (added_bytes) *added_bytes = pk->zk->bytes;
    return PM_OK;
  }
  const size_t n = pk->n, S = n + ZK_PAD;
  const uint32_t lg = pk->log_n;
  u64 w8[4], w4[4], unused[4], si[4];
  PK_TRY(pm_domain_info(lg + 3, w8, unused, unused));
  PK_TRY(pm_domain_info(lg + 2, w4, unused, unused));
  PK_TRY(pm_domain_info(lg, unused, unused, si));
  ZkState* zs = new ZkState();
  zs->stride = S;
  struct Alloc { void** p; size_t elems; };
  std::vector<Alloc> allocs = {{&zs->w8, 4 * n},     {&zs->x2, 4 * n},     {&zs->sigma_coset2, 16 * n}, {&zs->l1_coset2, 4 * n},
                               {&zs->coeffs, 6 * S}, {&zs->shift, 6 * S},  {&zs->coset2, 24 * n},      {&zs->ab, 8 * n},
                               {&zs->t, 4 * S},      {&zs->r, S},          {&zs->agg, S},              {&zs->wit, 2 * S}};
  for (int s_ = 0; s_ < NSEL; ++s_)
    if (pk->sel_coset[s_]) allocs.push_back({&zs->sel_coset2[s_], 4 * n});
  int rc = PM_OK;
  for (const Alloc& a : allocs) {
    if ((rc = pm_dev_alloc(ctx, a.elems * 32, a.p)) != PM_OK) break;
    zs->bytes += a.elems * 32;
  }
  const HFr one = fone(), g = fr_u64(7), omega8 = get(w8), omega4 = get(w4), g2 = fmul(g, omega8);
  if (!rc) rc = pm_fr_powers_dev(ctx, omega8.l, one.l, 4 * n, zs->w8, nullptr);
  if (!rc) rc = pm_fr_powers_dev(ctx, omega4.l, g2.l, 4 * n, zs->x2, nullptr);
  // the padded tails start (and, for the public-input slot, stay) zero
  if (!rc && hipMemsetAsync(zs->coeffs, 0, 6 * S * 32, ctx->stream) != hipSuccess) rc = PM_ERR_HIP;
  // key polynomials -> the second coset: p(w_8n X) on the first coset's transform.  coset2 is scratch until the first proof.
  pm::ZkShiftArgs sa;
  memset(&sa, 0, sizeof sa);
  for (int s_ = 0; s_ < NSEL; ++s_)
    if (pk->sel_coset[s_]) {
      sa.src[sa.count] = at(pk->sel_coeffs, s_ * n);
      sa.dst[sa.count++] = at(zs->coset2, s_ * n);
    }
  for (int j = 0; j < 4; ++j) {
    sa.src[sa.count] = at(pk->sigma_coeffs, j * n);
    sa.dst[sa.count++] = at(zs->coset2, (NSEL + j) * n);
  }
  void* l1_src = at(zs->coset2, (NSEL + 5) * n);   // L_1 = (1 / n) sum X^i
  if (!rc) rc = pm_fr_powers_dev(ctx, one.l, si, n, l1_src, nullptr);
  sa.src[sa.count] = l1_src;
  sa.dst[sa.count++] = at(zs->coset2, (NSEL + 4) * n);
  if (!rc) rc = pm::zk_shift(ctx, sa, zs->w8, n, ctx->stream);
  for (int s_ = 0; s_ < NSEL && !rc; ++s_)
    if (pk->sel_coset[s_])
      rc = pm_fr_ntt_dev(ctx, at(zs->coset2, s_ * n), n, n, zs->sel_coset2[s_], 4 * n, lg + 2, 1, PM_NTT_COSET, nullptr);
  if (!rc) rc = pm_fr_ntt_dev(ctx, at(zs->coset2, NSEL * n), n, n, zs->sigma_coset2, 4 * n, lg + 2, 4, PM_NTT_COSET, nullptr);
  if (!rc) rc = pm_fr_ntt_dev(ctx, at(zs->coset2, (NSEL + 4) * n), n, n, zs->l1_coset2, 4 * n, lg + 2, 1, PM_NTT_COSET, nullptr);
  if (!rc) rc = pm_sync(ctx);
  if (!rc) {
    zh_inv_period4(g2, omega4, n, zs->zh_inv2);   // the second coset 7 w_8n <w_4n>; s = 7^4n
    zs->inv2 = finv(fr_u64(2));
    zs->inv2s = finv(fmul(fr_u64(2), fpow(g, 4 * n)));
  }
  if (rc) {
    for (const Alloc& a : allocs)
      if (*a.p) (void)pm_dev_free(ctx, *a.p);
    delete zs;
    return rc;
  }
  pk->zk = zs;
  if (added_bytes) *added_bytes = zs->bytes;
  return PM_OK;
}

// (position, value) pairs of one statement's public inputs without repeats -- a repeated position keeps its last value --
// appended to hp (as offset + position) and hv
static void compact_public_inputs(const uint64_t* pos, const uint64_t* vals, size_t n_pi, uint64_t offset,
                                  std::vector<unsigned long long>& hp, std::vector<uint64_t>& hv) {
  std::unordered_map<uint64_t, size_t> last;
  last.reserve(2 * n_pi);
  for (size_t i = 0; i < n_pi; ++i) last[pos[i]] = i;
  for (size_t i = 0; i < n_pi; ++i) {
    if (last[pos[i]] != i) continue;
    hp.push_back(offset + pos[i]);
    hv.insert(hv.end(), vals + 4 * i, vals + 4 * i + 4);
  }
}

// pi_evals <- 0, then the sparse public inputs (a repeated position keeps its last value).  A handful goes up
// element by element; longer lists are staged as compact (position, value) arrays in the round-2 scratch
// (num / den are not written before round 2, which is ordered after this on the same stream) and scattered by
// one kernel, so a statement with thousands of public inputs costs two copies, not thousands.
__global__ void pi_scatter_kernel(const uint4* vals, const unsigned long long* pos, size_t cnt, uint4* out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= cnt) return;
  out[2 * pos[i]] = vals[2 * i];
  out[2 * pos[i] + 1] = vals[2 * i + 1];
}
static int scatter_public_inputs(pm_ctx* ctx, pm_prover_key* pk, const uint64_t* pos, const uint64_t* vals, size_t n_pi) {
  PM_HIP(ctx, hipSetDevice(ctx->device));
  PM_HIP(ctx, hipMemsetAsync(pk->pi_evals, 0, pk->n * 32, ctx->stream));
  if (n_pi <= 16) {
    for (size_t i = 0; i < n_pi; ++i)
      PM_HIP(ctx, hipMemcpyAsync(at(pk->pi_evals, pos[i]), vals + 4 * i, 32, hipMemcpyHostToDevice, ctx->stream));
    return PM_OK;
  }
  std::vector<unsigned long long> hp;
  std::vector<uint64_t> hv;
  compact_public_inputs(pos, vals, n_pi, 0, hp, hv);
  const size_t cnt = hp.size();   // <= n: fits the n-element scratch arrays
  PM_HIP(ctx, hipMemcpyAsync(pk->num, hv.data(), cnt * 32, hipMemcpyHostToDevice, ctx->stream));
  PM_HIP(ctx, hipMemcpyAsync(pk->den, hp.data(), cnt * 8, hipMemcpyHostToDevice, ctx->stream));
  hipLaunchKernelGGL(pi_scatter_kernel, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, ctx->stream,
                     (const uint4*)pk->num, (const unsigned long long*)pk->den, cnt, (uint4*)pk->pi_evals);
  PM_HIP(ctx, hipGetLastError());
  PM_HIP(ctx, hipStreamSynchronize(ctx->stream));   // the staging vectors die with this scope
  return PM_OK;
}

// Blinded wire commitments over a Lagrange key, for `count` vectors: [w] from the witness values, plus the blinder's
// sum_i b_i ([tau^(n+i)] - [tau^i]).  The blinded coefficients hold b_i at n + i, so two MSMs of 3 points take those same
// scalars, over the commit key at offset n and at offset 0, and the second result is negated before the host fold.  Passes of
// at most 64 vectors, one host fold per vector, one affine conversion.  scratch: 72 words per vector.
static int commit_lagrange_zk(pm_ctx* ctx, const pm_bases* lag, const pm_bases* ck, const void* d_wit, const void* coeffs, size_t n,
                              size_t S, uint32_t count, u64* scratch, u64 (*out_xy)[12]) {
  u64* part[3] = {scratch, scratch + 18 * (size_t)count, scratch + 36 * (size_t)count};
  u64* sum = scratch + 54 * (size_t)count;
  for (uint32_t v0 = 0; v0 < count; v0 += 64) {
    const uint32_t k = std::min<uint32_t>(64, count - v0);
    const void* tails = at(coeffs, (size_t)v0 * S + n);
    PK_TRY(pm_g1_msm_batch_dev(ctx, lag, 0, n, at(d_wit, (size_t)v0 * n), n, k, PM_SCALAR_MONTGOMERY, part[0] + 18 * (size_t)v0, nullptr));
    PK_TRY(pm_g1_msm_batch_dev(ctx, ck, n, 3, tails, S, k, PM_SCALAR_MONTGOMERY, part[1] + 18 * (size_t)v0, nullptr));
    PK_TRY(pm_g1_msm_batch_dev(ctx, ck, 0, 3, tails, S, k, PM_SCALAR_MONTGOMERY, part[2] + 18 * (size_t)v0, nullptr));
  }
  for (uint32_t v = 0; v < count; ++v) {
    u64 parts[3][18];
    for (int k = 0; k < 3; ++k) memcpy(parts[k], part[k] + 18 * (size_t)v, sizeof parts[k]);
    HFp y;
    memcpy(y.l, parts[2] + 6, 48);
    y = pm::host::sub(pm::host::zero<6>(), y, pm::host::FP());   // -P = (X, -Y, Z)
    memcpy(parts[2] + 6, y.l, 48);
    PK_TRY(pm_g1_fold(&parts[0][0], 3, sum + 18 * (size_t)v));
  }
  return pm_g1_to_affine_batch(sum, count, &out_xy[0][0], nullptr);
}

// The key on the first 4n coset 7 H_4n, and (zero-knowledge mode) on the second, 7 w_8n H_4n
static QuotientTables key_first_coset(const pm_prover_key* pk) {
  QuotientTables t{{}, pk->sigma_coset, 4 * pk->n, pk->l1_coset, pk->x4, pk->zh_inv};
  for (int s = 0; s < NSEL; ++s) t.sel[s] = pk->sel_coset[s];   // q_arith: nullptr when q_arith = 1
  return t;
}
static QuotientTables key_second_coset(const pm_prover_key* pk) {
  const ZkState* zs = pk->zk;
  QuotientTables t{{}, zs->sigma_coset2, 4 * pk->n, zs->l1_coset2, zs->x2, zs->zh_inv2};
  for (int s = 0; s < NSEL; ++s) t.sel[s] = zs->sel_coset2[s];
  return t;
}

static int prove_body(pm_ctx* ctx, pm_prover_key* pk, const pm_bases* ck, const Shard& shard, const void* d_witness,
                      const uint64_t* pi_positions, const uint64_t* pi_values, size_t n_pi, uint32_t flags,
                      const uint64_t (*blinders)[4], pm_plonk_proof* out) {
  if (!ctx || !pk || !ck || !d_witness || !out) return PM_ERR_BAD_ARG;
  if (n_pi && (!pi_positions || !pi_values)) return PM_ERR_BAD_ARG;
  PK_TRY(check_flags(ctx, flags));
  if (!pk->committed) return PM_ERR_BAD_ARG;   // pm_plonk_key_commit first: the transcript starts from the verifier key
  if (blinders)
    for (int i = 0; i < PM_PLONK_ZK_BLINDERS; ++i)
      if (pm::host::geq<4>(blinders[i], FRF().m)) return pm::set_err(ctx, PM_ERR_BAD_ARG, "a blinder is not below r");
  Busy guard(pk->busy);
  if (!guard.ok) return PM_ERR_BUSY;
  const size_t n = pk->n;
  const uint32_t lg = pk->log_n;
  // zero-knowledge mode (pm_plonk_prove_zk): blinded wires and z of n + 3 coefficients, quotient pieces up to n + 10, all
  // at the padded stride S in the key's ZK workspace.  Otherwise S = n and the key's own workspace.
  ZkState* const zs = blinders ? pk->zk : nullptr;
  if (blinders && !zs) return pm::set_err(ctx, PM_ERR_BAD_ARG, "pm_plonk_key_enable_zk first");
  if (!shard.on && pm_g1_bases_len(ck) < (zs ? n + PM_PLONK_ZK_EXTRA_BASES : n)) return PM_ERR_LENGTH;
  const size_t S = zs ? zs->stride : n;
  const size_t wlen = zs ? n + 3 : n;                // coefficients of the wires and of z
  void* const wc = zs ? zs->coeffs : pk->coeffs;     // [a b c d z pi] at stride S
  auto blind = [&](uint32_t first, uint32_t count, hipStream_t st) -> int {   // vectors first.. of wc with their Z_H blinders
    static const uint32_t TERMS[5] = {3, 3, 2, 3, 3}, FIRST[5] = {0, 3, 6, 8, 11};
    pm::ZkBlindArgs ba;
    memset(&ba, 0, sizeof ba);
    for (uint32_t v = 0; v < count; ++v) {
      const uint32_t w = first + v;
      ba.v[v] = at(wc, w * S);
      ba.terms[v] = TERMS[w];
      for (uint32_t i = 0; i < TERMS[w]; ++i) memcpy(ba.beta[v][i], blinders[FIRST[w] + i], 32);
    }
    return pm::zk_blind(ctx, ba, count, n, S, st);
  };
  // coefficient slots of wc -> the same slots of zs->coset2 on the second coset: one w_8n^i scaling pass for all of them,
  // then the coset NTT per run of consecutive slots
  auto second_coset = [&](std::initializer_list<uint32_t> slots, hipStream_t st) -> int {
    pm::ZkShiftArgs sa;
    memset(&sa, 0, sizeof sa);
    for (uint32_t w : slots) {
      sa.src[sa.count] = at(wc, w * S);
      sa.dst[sa.count++] = at(zs->shift, w * S);
    }
    PK_TRY(pm::zk_shift(ctx, sa, zs->w8, wlen, st));
    const uint32_t* p = slots.begin();
    for (size_t i = 0; i < slots.size();) {
      size_t j = i + 1;
      while (j < slots.size() && p[j] == p[j - 1] + 1) ++j;
      PK_TRY(pm_fr_ntt_dev(ctx, at(zs->shift, p[i] * S), wlen, S, at(zs->coset2, 4 * n * p[i]), 4 * n, lg + 2,
                           (uint32_t)(j - i), PM_NTT_COSET, st));
      i = j;
    }
    return PM_OK;
  };
  for (size_t i = 0; i < n_pi; ++i)
    if (pi_positions[i] >= n) return PM_ERR_LENGTH;
  ProofRounds pr(pk->base);
  pr.begin(flags, pi_positions, pi_values, n_pi);
  // a Lagrange-form key commits the wires from their values on H: the same group elements (no blinding), so the same proof
  const pm_bases* lag = shard.on ? nullptr : pk->lagrange;
  if (lag && ck != pk->lagrange_ck) return PM_ERR_BAD_ARG;   // checked against another commit key
  // ---- round 1 --------------------------------------------------------------------------------
  pm::host_mark(ctx, "round 1");
  hipStream_t side = pk->side;
  void* pi_coeffs = at(wc, 5 * S);
  if (lag) {
    // nothing waits for the wire iNTT before the MSM: it runs on the side stream ahead of the coset transforms
    PK_TRY(scatter_public_inputs(ctx, pk, pi_positions, pi_values, n_pi));
    PK_TRY(pm_fr_ntt_dev(ctx, pk->pi_evals, n, n, pi_coeffs, n, lg, 1, PM_NTT_INVERSE, nullptr));
    PK_TRY(pm_stream_fork(ctx, side, pk->ev_main));
    PK_TRY(pm_fr_ntt_dev(ctx, d_witness, n, n, wc, S, lg, 4, PM_NTT_INVERSE, side));
    if (zs) {
      PK_TRY(blind(0, 4, side));
      PK_TRY(pm_stream_join(ctx, side, pk->ev_side));   // the blinder MSMs below read the blinded coefficients
    }
    PK_TRY(pm_fr_ntt_dev(ctx, wc, wlen, S, pk->coset, 4 * n, lg + 2, 4, PM_NTT_COSET, side));
    PK_TRY(pm_fr_ntt_dev(ctx, pi_coeffs, wlen, S, at(pk->coset, 4 * n * 5), 4 * n, lg + 2, 1, PM_NTT_COSET, side));
    if (zs) PK_TRY(second_coset({0, 1, 2, 3, 5}, side));
    if (zs) {
      u64 scratch[72 * 4];
      PK_TRY(commit_lagrange_zk(ctx, lag, ck, d_witness, wc, n, S, 4, scratch, &out->commitments[0]));
    } else {
      PK_TRY(commit_batch(ctx, lag, shard, d_witness, n, n, 4, &out->commitments[0]));
    }
  } else {
    PK_TRY(pm_fr_ntt_dev(ctx, d_witness, n, n, wc, S, lg, 4, PM_NTT_INVERSE, nullptr));
    if (zs) PK_TRY(blind(0, 4, nullptr));
    // work no challenge depends on goes to the side stream and runs under the MSMs of rounds 1 and 2:
    // the public-input polynomial and the wire polynomials on the 4n coset (round 3 reads them)
    {
      PK_TRY(scatter_public_inputs(ctx, pk, pi_positions, pi_values, n_pi));
      PK_TRY(pm_fr_ntt_dev(ctx, pk->pi_evals, n, n, pi_coeffs, n, lg, 1, PM_NTT_INVERSE, nullptr));
      PK_TRY(pm_stream_fork(ctx, side, pk->ev_main));
      PK_TRY(pm_fr_ntt_dev(ctx, wc, wlen, S, pk->coset, 4 * n, lg + 2, 4, PM_NTT_COSET, side));
      PK_TRY(pm_fr_ntt_dev(ctx, pi_coeffs, wlen, S, at(pk->coset, 4 * n * 5), 4 * n, lg + 2, 1, PM_NTT_COSET, side));
      if (zs) PK_TRY(second_coset({0, 1, 2, 3, 5}, side));
    }
    PK_TRY(commit_batch(ctx, ck, shard, wc, wlen, S, 4, &out->commitments[0]));
  }
  pr.absorb_wires(&out->commitments[0]);
  // ---- round 2 --------------------------------------------------------------------------------
  pm::host_mark(ctx, "round 2");
  pr.draw_round2();
  pm_plonk_perm_args pa;
  fill_perm_args(pa, d_witness, n, pk->sigma_evals, n, pk->roots, pk->k, pr.ch[C_BETA], pr.ch[C_GAMMA]);
  PK_TRY(pm_plonk_perm_terms_dev(ctx, &pa, n, pk->num, pk->den, nullptr));
  PK_TRY(pm::fr_batch_inverse_mul(ctx, pk->den, pk->num, n, nullptr));       // den <- num / den (r06: one kernel, was two)
  PK_TRY(pm_fr_prefix_product_dev(ctx, pk->den, n, pk->num, nullptr));       // num <- z on H
  void* z_coeffs = at(wc, 4 * S);
  PK_TRY(pm_fr_ntt_dev(ctx, pk->num, n, n, z_coeffs, n, lg, 1, PM_NTT_INVERSE, nullptr));
  if (zs) PK_TRY(blind(4, 1, nullptr));
  // z on the 4n coset depends on no further challenge: side stream, under the commitment to z
  PK_TRY(pm_stream_fork(ctx, side, pk->ev_main));
  PK_TRY(pm_fr_ntt_dev(ctx, z_coeffs, wlen, S, at(pk->coset, 4 * n * 4), 4 * n, lg + 2, 1, PM_NTT_COSET, side));
  if (zs) PK_TRY(second_coset({4}, side));
  PK_TRY(commit_batch(ctx, ck, shard, z_coeffs, wlen, S, 1, &out->commitments[4]));
  pr.absorb_perm(out->commitments[4]);
  // ---- round 3 --------------------------------------------------------------------------------
  pm::host_mark(ctx, "round 3");
  pr.draw_round3();
  PK_TRY(pm_stream_join(ctx, side, pk->ev_side));   // the wire, PI and z coset forms are ready
  pm_plonk_quotient_args qa;
  fill_quotient_args(qa, key_first_coset(pk), pk->coset, 4 * n, at(pk->coset, 4 * n * 4), at(pk->coset, 4 * n * 5), pk->k, pr.ch);
  void* const t_coeffs = zs ? zs->t : pk->t;   // t_1..t_4 at stride S
  if (!zs) {
    PK_TRY(pm_plonk_quotient_dev(ctx, &qa, n, pk->t, nullptr));
    PK_TRY(pm_fr_ntt_dev(ctx, pk->t, 4 * n, 4 * n, pk->t, 4 * n, lg + 2, 1, PM_NTT_INVERSE | PM_NTT_COSET, nullptr));
    PK_TRY(commit_batch(ctx, ck, shard, pk->t, n, n, 4, &out->commitments[5]));
  } else {
    // deg t' <= 4n + 9: the same kernel on the second coset 7 w_8n H_4n gives t' mod (X^4n + s) beside t' mod (X^4n - s)
    PK_TRY(pm_plonk_quotient_dev(ctx, &qa, n, zs->ab, nullptr));
    fill_quotient_args(qa, key_second_coset(pk), zs->coset2, 4 * n, at(zs->coset2, 4 * n * 4), at(zs->coset2, 4 * n * 5), pk->k, pr.ch);
    PK_TRY(pm_plonk_quotient_dev(ctx, &qa, n, at(zs->ab, 4 * n), nullptr));
    PK_TRY(pm_fr_ntt_dev(ctx, zs->ab, 4 * n, 4 * n, zs->ab, 4 * n, lg + 2, 2, PM_NTT_INVERSE | PM_NTT_COSET, nullptr));
    u64 inv2[4], inv2s[4], tb[3][4];
    put(inv2, zs->inv2);
    put(inv2s, zs->inv2s);
    memcpy(tb, blinders[14], sizeof tb);
    PK_TRY(pm::zk_combine(ctx, zs->ab, zs->w8, n, S, inv2, inv2s, tb, zs->t, ctx->stream));
    PK_TRY(commit_batch(ctx, ck, shard, zs->t, n + pm::ZK_P1_LEN, S, 4, &out->commitments[5]));
  }
  pr.absorb_quotient(&out->commitments[5]);
  // ---- round 4 --------------------------------------------------------------------------------
  pm::host_mark(ctx, "round 4");
  pr.draw_z(pk->omega);
  const HFr &zc = pr.ch[C_Z], &zw = pr.zw;
  auto poly = [&](PolyRef p) -> const void* {   // the wires, t and z at stride S, the key's polynomials at n
    switch (p.role) {
      case R_WIRE: return at(wc, p.index * S);
      case R_T: return at(t_coeffs, p.index * S);
      case R_Z: return z_coeffs;
      case R_SIGMA: return at(pk->sigma_coeffs, p.index * n);
      default: return at(pk->sel_coeffs, p.index * n);
    }
  };
  {
    // ONE host synchronisation for all openings (r01 - r04: three, with r's own evaluation behind the linear combination)
    const OpeningPlan plan(pk->sel_zero);
    const void* ptr[MAX_OPENINGS];
    u64 val[MAX_OPENINGS][4];
    for (uint32_t s = 0; s < plan.count; ++s) ptr[s] = poly(plan.slot[s].poly);
    const uint32_t w0 = plan.next_row();
    if (!zs) {
      const uint32_t gk[3] = {OPENINGS_AT_Z, plan.nx, 4};
      const void* const* gp[3] = {ptr, ptr + OPENINGS_AT_Z, ptr + w0};
      const uint64_t* gpt[3] = {zc.l, zc.l, zw.l};
      uint64_t* gout[3] = {val[0], val[OPENINGS_AT_Z], val[w0]};
      PK_TRY(pm::poly_evaluate_groups(ctx, 3, gk, gp, gpt, gout, n));
    } else {
      // the same openings, grouped by length: padded polynomials (S) at z, key polynomials (n) at z, padded at z w
      const void* gptr[2][MAX_OPENINGS];
      u64 gval[2][MAX_OPENINGS][4];
      uint32_t gk[3] = {0, 0, 4}, from[MAX_OPENINGS];
      for (uint32_t s = 0; s < w0; ++s) {
        const int g = plan.slot[s].poly.per_proof() ? 0 : 1;
        from[s] = gk[g];
        gptr[g][gk[g]++] = ptr[s];
      }
      const void* const* gp[3] = {gptr[0], gptr[1], ptr + w0};
      const uint64_t* gpt[3] = {zc.l, zc.l, zw.l};
      uint64_t* gout[3] = {gval[0][0], gval[1][0], val[w0]};
      const size_t gn[3] = {S, n, S};
      PK_TRY(pm::poly_evaluate_groups_n(ctx, 3, gk, gp, gpt, gout, gn));
      for (uint32_t s = 0; s < w0; ++s) memcpy(val[s], gval[plan.slot[s].poly.per_proof() ? 0 : 1][from[s]], 32);
    }
    pm::host_mark(ctx, "openings at z, z w");
    pr.take_openings(plan, val[0], n);
  }
  void* const r_coeffs = zs ? zs->r : pk->r;       // S coefficients
  void* const agg = zs ? zs->agg : pk->agg;        // S
  void* const wit = zs ? zs->wit : pk->wit;        // 2 x S
  {
    LinTerm terms[12];
    const void* lin_v[12];
    u64 lin_c[12][4];
    uint32_t k;
    linearise(pr, pk->k, n, pk->sel_zero, terms, &k);
    for (uint32_t i = 0; i < k; ++i) {
      lin_v[i] = poly(terms[i].poly);
      put(lin_c[i], terms[i].coeff);
    }
    PK_TRY(pm_fr_lincomb_dev(ctx, k, lin_v, &lin_c[0][0], n, r_coeffs, nullptr));   // r itself: round 5 divides it
    if (zs) {   // beyond n only the blinded z has coefficients
      const void* tail_v[1] = {at(z_coeffs, n)};
      PK_TRY(pm_fr_lincomb_dev(ctx, 1, tail_v, pr.c_z.l, S - n, at(r_coeffs, n), nullptr));
    }
  }
  pr.finish_round4(out);
  // ---- round 5: CommitKey::compute_aggregate_witness at z and at z w ------------------------------
  HFr ac[12], sh[4];
  aggregation_coeffs(pr, n, ac, sh);
  {
    const void* agg_v[12];
    u64 agg_c[12][4];
    for (int i = 0; i < 4; ++i) agg_v[i] = at(t_coeffs, i * S);
    agg_v[4] = r_coeffs;
    for (int j = 0; j < 4; ++j) agg_v[5 + j] = at(wc, j * S);
    for (int j = 0; j < 3; ++j) agg_v[9 + j] = at(pk->sigma_coeffs, j * n);
    for (int i = 0; i < 12; ++i) put(agg_c[i], ac[i]);
    PK_TRY(pm_fr_lincomb_dev(ctx, 12, agg_v, &agg_c[0][0], n, agg, nullptr));
    if (zs) {   // the padded tails: t pieces, r and the wires (the sigmas end at n)
      const void* tail_v[9];
      for (int i = 0; i < 9; ++i) tail_v[i] = at(agg_v[i], n);
      PK_TRY(pm_fr_lincomb_dev(ctx, 9, tail_v, &agg_c[0][0], S - n, at(agg, n), nullptr));
    }
    PK_TRY(pm_fr_poly_ruffini_dev(ctx, agg, S, zc.l, wit, nullptr));
  }
  {
    const void* sh_v[4] = {z_coeffs, at(wc, 0), at(wc, S), at(wc, 3 * S)};
    u64 sh_c[4][4];
    for (int e = 0; e < 4; ++e) put(sh_c[e], sh[e]);
    PK_TRY(pm_fr_lincomb_dev(ctx, 4, sh_v, &sh_c[0][0], S, agg, nullptr));
    PK_TRY(pm_fr_poly_ruffini_dev(ctx, agg, S, zw.l, at(wit, S), nullptr));
  }
  // deg W_z = deg t_4 - 1: n + 9 coefficients in zero-knowledge mode
  PK_TRY(commit_batch(ctx, ck, shard, wit, zs ? n + pm::ZK_P1_LEN - 1 : n - 1, S, 2, &out->commitments[9]));
  pr.absorb_witnesses_and_store(out);
  return PM_OK;
}

static int prove_impl(pm_ctx* ctx, pm_prover_key* pk, const pm_bases* ck, const Shard& shard, const void* d_witness,
                      const uint64_t* pi_positions, const uint64_t* pi_values, size_t n_pi, uint32_t flags,
                      const uint64_t (*blinders)[4], pm_plonk_proof* out) {
  if (ctx && ctx->marks_on) ctx->marks.clear();
  pm::host_mark(ctx, "prove: start");
  const int rc = shard_leave(ctx, shard, prove_body(ctx, pk, ck, shard, d_witness, pi_positions, pi_values, n_pi, flags, blinders, out));
  pm::host_mark(ctx, "prove: end");
  if (ctx && ctx->marks_on && !ctx->marks.empty()) {   // PM_HOST_MARKS=1: where the host's time between the kernels goes
    const double t0 = ctx->marks.front().second;
    double prev = t0;
    for (const auto& mk : ctx->marks) {
      fprintf(stderr, "[host] %9.1f us  +%7.1f  %s\n", mk.second - t0, mk.second - prev, mk.first);
      prev = mk.second;
    }
  }
  return rc;
}

extern "C" int pm_plonk_prove_sharded(pm_ctx* ctx, pm_prover_key* pk, const pm_bases* ck_slice, size_t first_coefficient,
                                      const void* d_witness, const uint64_t* pi_positions, const uint64_t* pi_values,
                                      size_t n_pi, uint32_t flags, pm_exchange_fn exchange, void* user,
                                      pm_plonk_proof* out) {
  Shard sh;
  sh.on = true;
  sh.lo = first_coefficient;
  sh.fn = exchange;
  sh.user = user;
  sh.expect = 4;
  return prove_impl(ctx, pk, ck_slice, sh, d_witness, pi_positions, pi_values, n_pi, flags, nullptr, out);
}

extern "C" int pm_plonk_prove(pm_ctx* ctx, pm_prover_key* pk, const pm_bases* ck, const void* d_witness,
                              const uint64_t* pi_positions, const uint64_t* pi_values, size_t n_pi, uint32_t flags,
                              pm_plonk_proof* out) {
  return prove_impl(ctx, pk, ck, Shard(), d_witness, pi_positions, pi_values, n_pi, flags, nullptr, out);
}

extern "C" int pm_plonk_prove_zk(pm_ctx* ctx, pm_prover_key* pk, const pm_bases* ck, const void* d_witness,
                                 const uint64_t* pi_positions, const uint64_t* pi_values, size_t n_pi, uint32_t flags,
                                 const uint64_t (*blinders)[4], pm_plonk_proof* out) {
  if (!blinders) return PM_ERR_BAD_ARG;
  return prove_impl(ctx, pk, ck, Shard(), d_witness, pi_positions, pi_values, n_pi, flags, blinders, out);
}

// Proof::to_bytes of dusk-plonk 0.8: 11 compressed G1 (a b c d z t_1..t_4 w_z w_zw) then the 16 scalars of
// ProofEvaluations::to_bytes (a b c d a_next b_next d_next q_arith q_c q_l q_r left right out sigma, lin_poly, perm).
extern "C" int pm_plonk_proof_to_bytes(const pm_plonk_proof* proof, uint8_t out[PM_PLONK_PROOF_BYTES]) {
  if (!proof || !out) return PM_ERR_BAD_ARG;
  for (int i = 0; i < 11; ++i) Transcript::g1_compress(out + 48 * i, proof->commitments[i]);
  static const int order[16] = {0, 1, 2, 3, 4, 5, 6, 10, 11, 12, 13, 7, 8, 9, 16, 14};
  for (int i = 0; i < 16; ++i) Transcript::scalar_bytes(out + 528 + 32 * i, get(proof->evaluations[order[i]]));
  return PM_OK;
}

extern "C" int pm_plonk_verifier_key(const pm_prover_key* key, uint64_t (*out)[12]) {
  if (!key || !out || !key->committed) return PM_ERR_BAD_ARG;
  memcpy(out, key->vk, sizeof key->vk);
  return PM_OK;
}

// Pure host, no context: linearise of prover_rounds.h -- the one copy of the linearisation scalars -- on given openings
// and challenges (include/plonk_mi355x.h).
extern "C" int pm_test_plonk_linearise(size_t n, const uint64_t (*evaluations)[4], const uint64_t (*extras)[4],
                                       const uint64_t (*challenges)[4], uint32_t selector_present_mask, uint64_t (*out_coeffs)[4],
                                       uint32_t* out_roles, uint32_t* out_count, uint64_t out_r_z[4]) {
  if (!evaluations || !extras || !challenges || !out_coeffs || !out_roles || !out_count || !out_r_z) return PM_ERR_BAD_ARG;
  if (n == 0) return PM_ERR_LENGTH;
  ProofRounds pr{Transcript(tl::PROTOCOL)};
  struct In { HFr* dst; const uint64_t (*src)[4]; int count; };
  for (const In& in : {In{pr.ev, evaluations, NEV}, In{pr.xv, extras, NX}, In{pr.ch, challenges, NCHAL}})
    for (int i = 0; i < in.count; ++i) {
      if (pm::host::geq<4>(in.src[i], FRF().m)) return PM_ERR_BAD_ARG;
      in.dst[i] = get(in.src[i]);
    }
  bool sel_zero[NSEL];
  for (int s = 0; s < NSEL; ++s) sel_zero[s] = !((selector_present_mask >> s) & 1);
  const HFr k[3] = {fr_u64(7), fr_u64(13), fr_u64(17)};
  LinTerm terms[12];
  linearise(pr, k, n, sel_zero, terms, out_count);
  for (uint32_t i = 0; i < *out_count; ++i) {
    put(out_coeffs[i], terms[i].coeff);
    out_roles[i] = (uint32_t)terms[i].poly.role << 8 | terms[i].poly.index;
  }
  put(out_r_z, pr.r_z);
  return PM_OK;
}

#include "prover_batch.hip.h"
#include "prover_check.hip.h"
#include "prover_gadgets.hip.h"
#include "prover_dist.hip.h"
