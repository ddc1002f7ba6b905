// The Hades permutation of width 5 one lane at a time, shared by hades.hip (native Poseidon),
// schnorr.hip (the challenge of a signature, section 7.2l) and cipher.hip (the Poseidon cipher, section 7.2o): the handle, the definition on the host, the per-lane rounds and
// the sponge's absorption.  The forms, their bounds and the kernels are described in hades.hip.
#pragma once
#include <string>
#include <vector>

#include "context.h"
#include "poly_common.hip.h"

struct pm_hades_params {
  int device = 0;
  uint32_t rounds = 0, full = 0, n_mds = 0;
  void* d_tab = nullptr;   // u32: mds [n_mds][25][9], then ark [rounds + 1][5][9] (the last row zero), device form
  std::vector<uint64_t> ark, mds;   // the constants as _create took them, for host_permute: the empty roots of a ledger tree
};

namespace pm {

// ------------------------------------------------------------------ the definition on the host (csrc/host_field.h)
inline bool round_is_full(uint32_t rho, uint32_t R, uint32_t F) { return rho < F / 2 || rho >= R - F / 2; }

inline void host_permute(uint32_t R, uint32_t F, const uint64_t* ark, const uint64_t* mds, uint32_t n_mds, HFr (&s)[5]) {
  const host::Field<4>& Fq = host::FR();
  for (uint32_t rho = 0; rho < R; ++rho) {
    for (int j = 0; j < 5; ++j) s[j] = host::add(s[j], hfr_load(ark + 4 * (5 * (size_t)rho + j)), Fq);
    for (int j = round_is_full(rho, R, F) ? 0 : 4; j < 5; ++j) {
      const HFr x2 = host::mul(s[j], s[j], Fq), x4 = host::mul(x2, x2, Fq);
      s[j] = host::mul(x4, s[j], Fq);
    }
    const uint64_t* m = mds + 100 * (size_t)(n_mds == 1 ? 0 : rho);
    HFr o[5];
    for (int i = 0; i < 5; ++i) {
      o[i] = host::zero<4>();
      for (int j = 0; j < 5; ++j) o[i] = host::add(o[i], host::mul(hfr_load(m + 4 * (5 * i + j)), s[j], Fq), Fq);
    }
    for (int i = 0; i < 5; ++i) s[i] = o[i];
  }
}

// R, F, n_mds and every constant; empty = fine
inline std::string params_fault(uint32_t R, uint32_t F, const uint64_t* ark, const uint64_t* mds, uint32_t n_mds) {
  if (!ark || !mds) return "null constants";
  if (R == 0) return "rounds must be at least 1";
  if (F & 1u) return "full_rounds must be even";
  if (F > R) return "full_rounds exceeds rounds";
  if (n_mds != 1 && n_mds != R) return "n_mds must be 1 or rounds";
  for (size_t k = 0; k < 5 * (size_t)R; ++k)
    if (!hfr_canonical(ark + 4 * k)) return "round key " + std::to_string(k) + " is not canonical";
  for (size_t k = 0; k < 25 * (size_t)n_mds; ++k)
    if (!hfr_canonical(mds + 4 * k)) return "matrix entry " + std::to_string(k) + " is not canonical";
  return "";
}

// ------------------------------------------------------------------ device side
struct HadesTab {
  const PM_KCONST u32* mds;   // [n_mds][25][9]
  const PM_KCONST u32* ark;   // [rounds + 1][5][9], the last row zero
  u32 rounds, half_full;      // R, F / 2
  u32 mds_stride;             // words between the matrices of two rounds: 225 or 0
};
PM_DEV Fr h_to_dev(const Fr& abi) { return fe_reduce_weak<FrP>(fr_shl5(abi)); }
PM_DEV Fr h_to_abi(const Fr& dev) { return fe_mul<FrP>(dev, fe_pow2<FrP, 256>()); }
PM_DEV Fr h_const(const PM_KCONST u32* p) {
  Fr r;
#pragma unroll
  for (int i = 0; i < 9; ++i) r.l[i] = p[i];
  return r;
}
PM_DEV Fr h_sbox(const Fr& x) {
  const Fr x2 = fe_sqr<FrP>(x), x4 = fe_sqr<FrP>(x2);
  return fe_mul<FrP>(x4, x);
}
// (sum_j m[j] v[j]) / 2^261 + key: one reduction for the row (the bound is in the file comment); v normalised, m and key canonical
PM_DEV Fr h_row(const Fr (&v)[5], const PM_KCONST u32* m, const PM_KCONST u32* key) {
  Fr t;
  Fr* const out[1] = {&t};
  fe_mont_cols<FrP, 1>(
      [&](int k, u64* acc, u32& tok) {
#pragma unroll
        for (int j = 0; j < 5; ++j)
#pragma unroll
          for (int i = 0; i < 9; ++i) {
            const int l = k - i;
            if (l < 0 || l >= 9) continue;
            fe_mac(acc[0], v[j].l[i], m[9 * j + l], tok);
          }
        if (k >= 9) acc[0] += key[k - 9];
      },
      out);
  t.l[8] += key[8];   // the top limb keeps the rest
  return t;
}
// the rounds of one permutation on a lane's own state; s already holds the keys of round 0
PM_DEV void h_rounds_thread(Fr (&s)[5], const HadesTab& tab) {
#pragma unroll 1
  for (u32 rho = 0; rho < tab.rounds; ++rho) {
    if (rho < tab.half_full || rho >= tab.rounds - tab.half_full) {
#pragma unroll
      for (int j = 0; j < 4; ++j) s[j] = h_sbox(s[j]);
    }
    s[4] = h_sbox(s[4]);
    const PM_KCONST u32* const m = tab.mds + (size_t)tab.mds_stride * rho;
    const PM_KCONST u32* const key = tab.ark + 45 * (size_t)(rho + 1);
    Fr o[5];
#pragma unroll
    for (int i = 0; i < 5; ++i) o[i] = h_row(s, m + 45 * i, key + 9 * i);
#pragma unroll
    for (int i = 0; i < 5; ++i) s[i] = o[i];
  }
}
// s += add + the keys of round 0 (limbs below 3 * 2^29, value below 4.2 r)
PM_DEV Fr h_absorb(const Fr& s, const Fr& add, const PM_KCONST u32* key0) {
  return fe_reduce_weak<FrP>(fe_add<FrP>(fe_add<FrP>(s, add), h_const(key0)));
}
// word t (0..3) of the chunk that starts at element `at` of a message with `left` elements to go: the input, the padding 1
// after a short chunk's last input, or nothing
PM_DEV Fr h_chunk_word(const u32x4* msg, size_t at, u32 left, u32 t) {
  if (t < left) return h_to_dev(ld_canon(msg, at + t));
  return t == left ? fe_one<FrP>() : fe_zero<FrP>();
}

inline HadesTab tab_of(const pm_hades_params* p) {
  const u32* t = (const u32*)p->d_tab;
  return HadesTab{(const PM_KCONST u32*)t, (const PM_KCONST u32*)(t + 225 * (size_t)p->n_mds), p->rounds, p->full / 2,
                  p->n_mds == 1 ? 0u : 225u};
}
// the handle a device call was given
inline int params_fault(pm_ctx* ctx, const pm_hades_params* p) {
  if (!p) return set_err(ctx, PM_ERR_BAD_ARG, "null params");
  if (p->device != ctx->device) return set_err(ctx, PM_ERR_BAD_ARG, "the params belong to another device");
  return PM_OK;
}
inline int capacity_to_dev(pm_ctx* ctx, const uint64_t* capacity, u32 (&out)[9]) {
  if (!capacity) return set_err(ctx, PM_ERR_BAD_ARG, "null capacity");
  if (!hfr_canonical(capacity)) return set_err(ctx, PM_ERR_BAD_ARG, "capacity is not canonical");
  to_limbs29(out, hfr_load(capacity));
  return PM_OK;
}

}  // namespace pm
