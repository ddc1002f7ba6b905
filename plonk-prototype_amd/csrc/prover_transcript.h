// Plain host C++: the prover's Fiat-Shamir transcript -- Merlin over STROBE-128 -- and THE table of its labels and message
// order.  Included by prover.hip; every path of the prover (single, batch, distributed) absorbs and squeezes through
// ProofRounds in prover_rounds.h, which only refers to the table here.
#pragma once
#include <cstdint>
#include <cstring>
#include <string>

#include "../../include/plonk_mi355x.h"
#include "host_field.h"

namespace {
using pm::host::HFp;
using pm::host::HFr;
typedef uint64_t u64;
const pm::host::Field<4>& FRF() { return pm::host::FR(); }

HFr fr_u64(u64 v) { return pm::host::from_u64(v, FRF()); }
HFr fmul(const HFr& a, const HFr& b) { return pm::host::mul(a, b, FRF()); }
HFr fadd(const HFr& a, const HFr& b) { return pm::host::add(a, b, FRF()); }
HFr fsub(const HFr& a, const HFr& b) { return pm::host::sub(a, b, FRF()); }
HFr finv(const HFr& a) { return pm::host::inv(a, FRF()); }
HFr fpow(const HFr& a, u64 e) { return pm::host::pow(a, &e, 1, FRF()); }
HFr fone() { return pm::host::one(FRF()); }
HFr fneg(const HFr& a) { return fsub(pm::host::zero<4>(), a); }
// Montgomery -> canonical limbs
HFr fr_canonical(const HFr& a) {
  HFr raw1 = pm::host::zero<4>();
  raw1.l[0] = 1;
  return fmul(a, raw1);
}

// ------------------------------------------------------------------ Merlin over STROBE-128
struct Strobe128 {
  static const int R = 166;
  uint8_t st[200];
  uint8_t pos = 0, pos_begin = 0, cur_flags = 0;
  explicit Strobe128(const std::string& label) {
    memset(st, 0, sizeof st);
    const uint8_t head[6] = {1, R + 2, 1, 0, 1, 96};
    memcpy(st, head, 6);
    memcpy(st + 6, "STROBEv1.0.2", 12);
    pm_keccak_f1600(st);
    meta_ad((const uint8_t*)label.data(), label.size(), false);
  }
  void run_f() {
    st[pos] ^= pos_begin;
    st[pos + 1] ^= 0x04;
    st[R + 1] ^= 0x80;
    pm_keccak_f1600(st);
    pos = 0;
    pos_begin = 0;
  }
  void absorb(const uint8_t* d, size_t n) {
    for (size_t i = 0; i < n; ++i) {
      st[pos++] ^= d[i];
      if (pos == R) run_f();
    }
  }
  void squeeze(uint8_t* d, size_t n) {
    for (size_t i = 0; i < n; ++i) {
      d[i] = st[pos];
      st[pos++] = 0;
      if (pos == R) run_f();
    }
  }
  void begin_op(uint8_t flags, bool more) {
    if (more) return;                       // continued operation (same flags by construction here)
    const uint8_t old_begin = pos_begin;
    pos_begin = (uint8_t)(pos + 1);
    cur_flags = flags;
    const uint8_t hdr[2] = {old_begin, flags};
    absorb(hdr, 2);
    if ((flags & (4 | 32)) && pos != 0) run_f();   // C or K
  }
  void meta_ad(const uint8_t* d, size_t n, bool more) { begin_op(16 | 2, more); absorb(d, n); }
  void ad(const uint8_t* d, size_t n, bool more) { begin_op(2, more); absorb(d, n); }
  void prf(uint8_t* d, size_t n) { begin_op(1 | 2 | 4, false); squeeze(d, n); }
};

struct Transcript {
  Strobe128 s;
  explicit Transcript(const std::string& label) : s("Merlin v1.0") { append("dom-sep", (const uint8_t*)label.data(), label.size()); }
  static void scalar_bytes(uint8_t b[32], const HFr& v) {
    const HFr c = fr_canonical(v);
    for (int i = 0; i < 32; ++i) b[i] = (uint8_t)(c.l[i / 8] >> (8 * (i % 8)));
  }
  void append(const char* label, const uint8_t* msg, size_t n) {
    s.meta_ad((const uint8_t*)label, strlen(label), false);
    uint8_t len[4] = {(uint8_t)n, (uint8_t)(n >> 8), (uint8_t)(n >> 16), (uint8_t)(n >> 24)};
    s.meta_ad(len, 4, true);
    s.ad(msg, n, false);
  }
  void append_u64(const char* label, u64 v) {
    uint8_t b[8];
    for (int i = 0; i < 8; ++i) b[i] = (uint8_t)(v >> (8 * i));
    append(label, b, 8);
  }
  void append_commitment(const char* label, const u64 xy[12]) {
    uint8_t out[48];
    g1_compress(out, xy);
    append(label, out, 48);
  }
  // 48-byte zcash compressed G1 (big-endian x; bit 7 compressed, bit 6 infinity, bit 5 = y > (p-1)/2)
  static void g1_compress(uint8_t out[48], const u64 xy[12]) {
    memset(out, 0, 48);
    bool any = false;
    for (int i = 0; i < 12; ++i) any = any || xy[i];
    if (!any) {
      out[0] = 0xC0;
    } else {
      HFp x, y, raw1 = pm::host::zero<6>();
      memcpy(x.l, xy, 48);
      memcpy(y.l, xy + 6, 48);
      raw1.l[0] = 1;
      x = pm::host::mul(x, raw1, pm::host::FP());
      y = pm::host::mul(y, raw1, pm::host::FP());
      for (int i = 0; i < 48; ++i) out[i] = (uint8_t)(x.l[(47 - i) / 8] >> (8 * ((47 - i) % 8)));
      out[0] |= 0x80;
      // y > (p - 1) / 2  <=>  2 y > p - 1  <=>  2 y >= p + 1 ... compare y with p - y
      HFp ny = pm::host::sub(pm::host::zero<6>(), y, pm::host::FP());   // canonical limbs: p - y
      if (pm::host::geq<6>(y.l, ny.l) && !pm::host::eq(y, ny)) out[0] |= 0x20;
    }
  }
  void append_scalar(const char* label, const HFr& v) {
    const HFr c = fr_canonical(v);
    uint8_t b[32];
    for (int i = 0; i < 32; ++i) b[i] = (uint8_t)(c.l[i / 8] >> (8 * (i % 8)));
    append(label, b, 32);
  }
  // 64 challenge bytes as a little-endian integer mod r (BlsScalar::from_bytes_wide)
  HFr challenge_scalar(const char* label) {
    s.meta_ad((const uint8_t*)label, strlen(label), false);
    uint8_t len[4] = {64, 0, 0, 0};
    s.meta_ad(len, 4, true);
    uint8_t b[64];
    s.prf(b, 64);
    const HFr k256 = fr_u64(256);
    HFr acc = pm::host::zero<4>();
    for (int i = 63; i >= 0; --i) acc = fadd(fmul(acc, k256), fr_u64(b[i]));
    return acc;
  }
};

// selector order of dusk's VerifierKey::seed_transcript (and of the ABI)
enum { Q_M, Q_L, Q_R, Q_O, Q_C, Q_4, Q_ARITH, Q_RANGE, Q_LOGIC, Q_FIXED, Q_VAR, NSEL };
const int SEL_SEED_ORDER[NSEL] = {Q_M, Q_L, Q_R, Q_O, Q_C, Q_4, Q_ARITH, Q_RANGE, Q_LOGIC, Q_VAR, Q_FIXED};

// ================================================================================================================
// THE transcript table: every label string and the order of every message of a proof's Fiat-Shamir transcript, in
// the order they are absorbed / squeezed.  Restated from the published dusk-plonk 0.8 design (ref:Cargo.toml:19); the
// crate is not in the reference tree and no upstream proof bytes exist here, so these strings are PARITY-UNPINNED:
// byte-equality of a proof with dusk's stands or falls with them.  THIS IS THE SINGLE PLACE TO EDIT when upstream
// vectors become available -- the prover (prover_rounds.h) only refers to this table, and the verifier side in Python
// (plonk-prototype_amd/prover.py: derive_challenges) reads the same table through pm_plonk_transcript_labels().
// ================================================================================================================
namespace tl {
const char* const PROTOCOL = "plonk";                       // default Transcript::new(label)
// VerifierKey::seed_transcript: the 11 selector commitments in SEL_SEED_ORDER (variable before fixed), the 4 sigmas
const char* const SELECTORS[NSEL] = {"q_m", "q_l", "q_r", "q_o", "q_c", "q_4", "q_arith", "q_range", "q_logic",
                                     "q_variable_group_add", "q_fixed_group_add"};
const char* const SIGMAS[4] = {"left_sigma", "right_sigma", "out_sigma", "fourth_sigma"};
// circuit_domain_sep(n)
const char* const DOM_SEP = "dom-sep";
const char* const DOM_SEP_VALUE = "circuit_size";
const char* const CIRCUIT_SIZE = "n";
// this library's public-input binding (flags = 0; absent with PM_PLONK_UPSTREAM_TRANSCRIPT): count, then (position, value)
const char* const PI_LEN = "pi_len";
const char* const PI_POS = "pi_pos";
const char* const PI_VALUE = "pi";
// round 1: the wire commitments
const char* const WIRES[4] = {"w_l", "w_r", "w_o", "w_4"};
// round 2: beta (re-absorbed under its own label), gamma, then the permutation commitment
const char* const BETA = "beta";
const char* const GAMMA = "gamma";
const char* const PERM = "z";
// round 3: the quotient's challenges, then the four quotient commitments
const char* const ALPHA = "alpha";
const char* const RANGE_SEP = "range separation challenge";
const char* const LOGIC_SEP = "logic separation challenge";
const char* const FIXED_SEP = "fixed base separation challenge";
const char* const VAR_SEP = "variable base separation challenge";
const char* const QUOTIENT[4] = {"t_1", "t_2", "t_3", "t_4"};
// round 4: the evaluation challenge and the 17 evaluations in transcript order (pm_plonk_proof.evaluations)
const char* const Z_CHALLENGE = "z";
const char* const EVALS[17] = {"a_eval", "b_eval", "c_eval", "d_eval", "a_next_eval", "b_next_eval", "d_next_eval",
                               "left_sig_eval", "right_sig_eval", "out_sig_eval", "q_arith_eval", "q_c_eval", "q_l_eval",
                               "q_r_eval", "perm_eval", "t_eval", "r_eval"};
// round 5: the two aggregation challenges (same label twice), then the opening commitments; the verifier's batch challenge
const char* const AGGREGATE = "aggregate_witness";
const char* const W_Z = "w_z";
const char* const W_ZW = "w_z_w";
const char* const BATCH = "batch";
}  // namespace tl
}  // namespace
