// Plain host C++, no HIP calls: the ONE copy of what a proof's five rounds do on the host -- the transcript sequence and the
// challenges, the argument structs of the permutation and quotient kernels, which polynomials are opened where, the
// linearisation and aggregation scalars.  pm_plonk_prove, pm_plonk_prove_batch and pm_plonk_prove_dist (prover.hip,
// prover_batch.hip.h, prover_dist.hip.h) differ in buffers, strides, launches and exchanges only: each names its polynomials
// by role (PolyRef) and maps a role to its own pointer.
#pragma once
#include <atomic>

#include "prover_transcript.h"

namespace {
void put(u64 dst[4], const HFr& v) { memcpy(dst, v.l, 32); }
HFr get(const u64 src[4]) {
  HFr r;
  memcpy(r.l, src, 32);
  return r;
}
char* at(const void* base, size_t elems) { return (char*)base + 32 * elems; }
static_assert(sizeof(HFr) == 32, "arrays of HFr are read as rows of four limbs");

// one call at a time on a key or a batch workspace: it owns the per-proof buffers
struct Busy {
  std::atomic<bool>& flag;
  const bool ok;
  explicit Busy(std::atomic<bool>& f) : flag(f), ok(!f.exchange(true)) {}
  ~Busy() {
    if (ok) flag.store(false);
  }
};

// 1 / Z_H on the 4n coset g <w4>: Z_H(g w4^i) = g^n (w4^n)^i - 1 has period 4
void zh_inv_period4(const HFr& g, const HFr& omega4, size_t n, HFr out[4]) {
  const HFr gn = fpow(g, n), i4 = fpow(omega4, n), one = fone();
  HFr p = one;
  for (int k = 0; k < 4; ++k) {
    out[k] = finv(fsub(fmul(gn, p), one));
    p = fmul(p, i4);
  }
}

// Prover::preprocess: Transcript::new(label), VerifierKey::seed_transcript (the 11 selector and 4 sigma commitments),
// circuit_domain_sep(n) -- where every proof of the key starts
Transcript key_transcript(const char* label, const u64 (*vk)[12], size_t n) {
  Transcript ts(label ? label : tl::PROTOCOL);
  for (int i = 0; i < NSEL; ++i) ts.append_commitment(tl::SELECTORS[i], vk[SEL_SEED_ORDER[i]]);
  for (int j = 0; j < 4; ++j) ts.append_commitment(tl::SIGMAS[j], vk[NSEL + j]);
  ts.append(tl::DOM_SEP, (const uint8_t*)tl::DOM_SEP_VALUE, strlen(tl::DOM_SEP_VALUE));
  ts.append_u64(tl::CIRCUIT_SIZE, n);
  return ts;
}

// A polynomial of a proof by what it is; the index is the wire, the quotient piece, the sigma or the selector (Q_*).
enum : uint8_t { R_WIRE, R_T, R_Z, R_SIGMA, R_SELECTOR };
struct PolyRef {
  uint8_t role, index;
  bool per_proof() const { return role <= R_Z; }   // wires, t and z belong to the proof, sigmas and selectors to the key
};

// pm_plonk_proof.evaluations in transcript order (tl::EVALS), the values r(z) needs beside them, pm_plonk_proof.challenges
enum { E_A, E_B, E_C, E_D, E_AN, E_BN, E_DN, E_S1, E_S2, E_S3, E_QARITH, E_QC, E_QL, E_QR, E_ZN, E_T, E_R, NEV };
enum { X_QM, X_QO, X_Q4, X_Z, X_S4, X_RANGE, X_LOGIC, X_FIXED, X_VAR, NX };
enum { C_BETA, C_GAMMA, C_ALPHA, C_RANGE_SEP, C_LOGIC_SEP, C_FIXED_SEP, C_VAR_SEP, C_Z, C_AW, C_AWS, NCHAL };
static_assert(NEV == 17, "tl::EVALS lists the evaluations in this enum's order");
const int WIDGET_SEL[4] = {Q_RANGE, Q_LOGIC, Q_FIXED, Q_VAR};

// Which polynomials a proof opens, in the order every path evaluates them: the 15 openings at z (a b c d, sigma_1..3,
// q_arith q_c q_l q_r, t_1..t_4), then at z what r(z) needs beyond them -- r is a linear combination of key and round
// polynomials, so r(z) is the same combination of their values: q_m, q_o, q_4, z, sigma_4 and the widget selectors the
// circuit uses ride along and r needs no pass of its own --, then the four openings at z w (a b d z).
constexpr uint32_t OPENINGS_AT_Z = 15, MAX_OPENINGS = OPENINGS_AT_Z + NX + 4;
enum { O_WIRES = 0, O_SIGMAS = 4, O_QARITH = 7, O_QC, O_QL, O_QR, O_T = 11 };
struct OpeningPlan {
  struct Slot {
    PolyRef poly;
    uint8_t point;   // 0: z, 1: z w
  };
  Slot slot[MAX_OPENINGS];
  uint32_t count = 0;
  uint32_t nx = X_RANGE;                 // the r(z) extras: slots [15, 15 + nx)
  int xslot[4] = {-1, -1, -1, -1};       // the extra that holds widget selector w, where the circuit uses it
  uint32_t next_row() const { return OPENINGS_AT_Z + nx; }   // first of the four slots at z w
  explicit OpeningPlan(const bool sel_zero[NSEL]) {
    auto add = [&](uint8_t role, int index, uint8_t point) { slot[count++] = Slot{{role, (uint8_t)index}, point}; };
    for (int j = 0; j < 4; ++j) add(R_WIRE, j, 0);
    for (int j = 0; j < 3; ++j) add(R_SIGMA, j, 0);
    for (int s : {Q_ARITH, Q_C, Q_L, Q_R}) add(R_SELECTOR, s, 0);
    for (int i = 0; i < 4; ++i) add(R_T, i, 0);
    for (int s : {Q_M, Q_O, Q_4}) add(R_SELECTOR, s, 0);
    add(R_Z, 0, 0);
    add(R_SIGMA, 3, 0);
    for (int w = 0; w < 4; ++w)
      if (!sel_zero[WIDGET_SEL[w]]) {
        xslot[w] = (int)nx++;
        add(R_SELECTOR, WIDGET_SEL[w], 0);
      }
    for (int j : {0, 1, 3}) add(R_WIRE, j, 1);
    add(R_Z, 0, 1);
  }
};

// ---- the widgets' linearisation scalars: the same identities as plonk_rounds.hip's quotient kernel,
// on the opening evaluations (widget::*::ProverKey::compute_linearisation)
HFr small(u64 v) { return fr_u64(v); }
HFr wdelta(const HFr& f) {
  return fmul(fmul(fmul(f, fsub(f, small(1))), fsub(f, small(2))), fsub(f, small(3)));
}
HFr edwards_d() { return fneg(fmul(small(10240), finv(small(10241)))); }
struct RowEvals {
  HFr a, b, c, d, an, bn, dn, q_l, q_r, q_c;
};
HFr widget_range(const HFr& sep, const RowEvals& e) {
  const HFr k = fmul(sep, sep), k2 = fmul(k, k), k3 = fmul(k2, k), four = small(4);
  HFr t = wdelta(fsub(e.c, fmul(four, e.d)));
  t = fadd(t, fmul(wdelta(fsub(e.b, fmul(four, e.c))), k));
  t = fadd(t, fmul(wdelta(fsub(e.a, fmul(four, e.b))), k2));
  t = fadd(t, fmul(wdelta(fsub(e.dn, fmul(four, e.a))), k3));
  return fmul(t, sep);
}
HFr widget_logic(const HFr& sep, const RowEvals& e) {
  const HFr k = fmul(sep, sep), k2 = fmul(k, k), k3 = fmul(k2, k), k4 = fmul(k2, k2), four = small(4);
  const HFr qa = fsub(e.an, fmul(four, e.a)), qb = fsub(e.bn, fmul(four, e.b)), qd = fsub(e.dn, fmul(four, e.d));
  const HFr s = fadd(qa, qb), w = e.c;
  HFr in = fadd(fsub(fmul(four, w), fmul(small(18), s)), small(81));
  in = fadd(fmul(w, in), fmul(small(18), fadd(fmul(qa, qa), fmul(qb, qb))));
  in = fadd(fsub(in, fmul(small(81), s)), small(83));
  const HFr f = fmul(w, in);
  const HFr ee = fsub(fmul(small(3), fadd(s, qd)), fadd(f, f));
  const HFr bb = fmul(e.q_c, fsub(fmul(small(9), qd), fmul(small(3), s)));
  HFr t = wdelta(qa);
  t = fadd(t, fmul(wdelta(qb), k));
  t = fadd(t, fmul(wdelta(qd), k2));
  t = fadd(t, fmul(fsub(w, fmul(qa, qb)), k3));
  t = fadd(t, fmul(fadd(bb, ee), k4));
  return fmul(t, sep);
}
HFr widget_fixed(const HFr& sep, const RowEvals& e) {
  const HFr k = fmul(sep, sep), k2 = fmul(k, k), k3 = fmul(k2, k), one = fone();
  const HFr bit = fsub(e.dn, fadd(e.d, e.d));
  HFr t = fmul(fmul(bit, fsub(bit, one)), fadd(bit, one));
  const HFr ya = fadd(fmul(fmul(bit, bit), fsub(e.q_r, one)), one), xa = fmul(e.q_l, bit);
  t = fadd(t, fmul(fsub(fmul(bit, e.q_c), e.c), k));
  const HFr dxy = fmul(fmul(fmul(e.c, e.a), e.b), edwards_d());
  t = fadd(t, fmul(fsub(fadd(e.an, fmul(e.an, dxy)), fadd(fmul(e.a, ya), fmul(e.b, xa))), k2));
  t = fadd(t, fmul(fsub(fsub(e.bn, fmul(e.bn, dxy)), fadd(fmul(e.b, ya), fmul(e.a, xa))), k3));
  return fmul(t, sep);
}
HFr widget_var(const HFr& sep, const RowEvals& e) {
  const HFr k = fmul(sep, sep), k2 = fmul(k, k);
  const HFr y1x2 = fmul(e.b, e.c), y1y2 = fmul(e.b, e.d), x1x2 = fmul(e.a, e.c);
  HFr t = fsub(fmul(e.a, e.d), e.dn);
  const HFr dd = fmul(fmul(e.dn, y1x2), edwards_d());
  t = fadd(t, fmul(fsub(fadd(e.dn, y1x2), fadd(e.an, fmul(e.an, dd))), k));
  t = fadd(t, fmul(fsub(fadd(y1y2, x1x2), fsub(e.bn, fmul(e.bn, dd))), k2));
  return fmul(t, sep);
}

// One proof's host state: its transcript, what it drew and what it opened.  The members are the transcript's sequence, in
// order; the caller does the device work between them.
struct ProofRounds {
  Transcript ts;
  HFr ch[NCHAL], zw;        // the challenges in the order of pm_plonk_proof.challenges; z w
  HFr ev[NEV], xv[NX];      // the openings (a widget selector the circuit does not use: zero)
  HFr r_z, c_z;             // linearise: r(z), and z's coefficient in r
  explicit ProofRounds(const Transcript& base) : ts(base) {}   // the key's transcript, seeded with the verifier key

  void begin(uint32_t flags, const uint64_t* pi_pos, const uint64_t* pi_val, size_t n_pi) {
    if (flags & PM_PLONK_UPSTREAM_TRANSCRIPT) return;
    // the default; not in dusk-plonk 0.8.2 (its transcript never sees the public inputs): binds the statement to
    // the challenges so that it cannot be chosen after them
    ts.append_u64(tl::PI_LEN, n_pi);
    for (size_t i = 0; i < n_pi; ++i) {
      ts.append_u64(tl::PI_POS, pi_pos[i]);
      ts.append_scalar(tl::PI_VALUE, get(pi_val + 4 * i));
    }
  }
  void absorb_wires(const u64 (*xy)[12]) {
    for (int j = 0; j < 4; ++j) ts.append_commitment(tl::WIRES[j], xy[j]);
  }
  void draw_round2() {
    ch[C_BETA] = ts.challenge_scalar(tl::BETA);
    ts.append_scalar(tl::BETA, ch[C_BETA]);
    ch[C_GAMMA] = ts.challenge_scalar(tl::GAMMA);
  }
  void absorb_perm(const u64 xy[12]) { ts.append_commitment(tl::PERM, xy); }
  void draw_round3() {
    ch[C_ALPHA] = ts.challenge_scalar(tl::ALPHA);
    ch[C_RANGE_SEP] = ts.challenge_scalar(tl::RANGE_SEP);
    ch[C_LOGIC_SEP] = ts.challenge_scalar(tl::LOGIC_SEP);
    ch[C_FIXED_SEP] = ts.challenge_scalar(tl::FIXED_SEP);
    ch[C_VAR_SEP] = ts.challenge_scalar(tl::VAR_SEP);
  }
  void absorb_quotient(const u64 (*xy)[12]) {
    for (int i = 0; i < 4; ++i) ts.append_commitment(tl::QUOTIENT[i], xy[i]);
  }
  void draw_z(const HFr& omega) {
    ch[C_Z] = ts.challenge_scalar(tl::Z_CHALLENGE);
    zw = fmul(ch[C_Z], omega);
  }
  // values: plan.count rows of four limbs in the plan's order, each the polynomial's value at its point
  void take_openings(const OpeningPlan& plan, const u64* values, size_t n) {
    auto val = [&](uint32_t s) { return get(values + 4 * s); };
    for (int j = 0; j < 4; ++j) ev[E_A + j] = val(O_WIRES + j);
    for (int j = 0; j < 3; ++j) ev[E_S1 + j] = val(O_SIGMAS + j);
    ev[E_QARITH] = val(O_QARITH);
    ev[E_QC] = val(O_QC);
    ev[E_QL] = val(O_QL);
    ev[E_QR] = val(O_QR);
    const uint32_t w0 = plan.next_row();
    ev[E_AN] = val(w0);
    ev[E_BN] = val(w0 + 1);
    ev[E_DN] = val(w0 + 2);
    ev[E_ZN] = val(w0 + 3);
    const HFr zn = fpow(ch[C_Z], n);   // t = t_1 + z^n t_2 + z^2n t_3 + z^3n t_4
    ev[E_T] = fadd(val(O_T), fmul(zn, fadd(val(O_T + 1), fmul(zn, fadd(val(O_T + 2), fmul(zn, val(O_T + 3)))))));
    for (int j = 0; j < X_RANGE; ++j) xv[j] = val(OPENINGS_AT_Z + j);
    for (int w = 0; w < 4; ++w) xv[X_RANGE + w] = plan.xslot[w] >= 0 ? val(OPENINGS_AT_Z + plan.xslot[w]) : pm::host::zero<4>();
  }
  // after linearise: the 17 evaluations go into the transcript and the proof, then both aggregation challenges are drawn
  void finish_round4(pm_plonk_proof* out) {
    for (int i = 0; i < NEV; ++i) {
      ts.append_scalar(tl::EVALS[i], ev[i]);
      put(out->evaluations[i], ev[i]);
    }
    ch[C_AW] = ts.challenge_scalar(tl::AGGREGATE);
    ch[C_AWS] = ts.challenge_scalar(tl::AGGREGATE);
  }
  void absorb_witnesses_and_store(pm_plonk_proof* out) {
    ts.append_commitment(tl::W_Z, out->commitments[9]);
    ts.append_commitment(tl::W_ZW, out->commitments[10]);
    for (int i = 0; i < NCHAL; ++i) put(out->challenges[i], ch[i]);
  }
};

// wires and sigma_evals: four vectors each on the rows of H, at these strides
void fill_perm_args(pm_plonk_perm_args& pa, const void* wires, size_t wire_stride, const void* sigma_evals, size_t sigma_stride,
                    const void* roots, const HFr k[3], const HFr& beta, const HFr& gamma) {
  memset(&pa, 0, sizeof pa);
  for (int j = 0; j < 4; ++j) {
    pa.wires[j] = at(wires, j * wire_stride);
    pa.sigmas[j] = at(sigma_evals, j * sigma_stride);
  }
  pa.roots = roots;
  put(pa.beta, beta);
  put(pa.gamma, gamma);
  for (int j = 0; j < 3; ++j) put(pa.k[j], k[j]);
}

// One coset's view of a key: what the quotient kernel reads besides the proof's own polynomials
struct QuotientTables {
  const void* sel[NSEL];   // nullptr: q_arith = 1, a widget selector the circuit does not use
  const void* sigma;       // four vectors at sigma_stride
  size_t sigma_stride;
  const void *l1, *x;
  const HFr* zh_inv;       // [4]
};
void fill_quotient_args(pm_plonk_quotient_args& qa, const QuotientTables& t, const void* wires, size_t wire_stride, const void* z,
                        const void* pi, const HFr k[3], const HFr ch[NCHAL]) {
  memset(&qa, 0, sizeof qa);
  for (int j = 0; j < 4; ++j) {
    qa.wires[j] = at(wires, j * wire_stride);
    qa.sigmas[j] = at(t.sigma, j * t.sigma_stride);
  }
  qa.z = z;
  qa.pi = pi;
  qa.q_m = t.sel[Q_M];
  qa.q_l = t.sel[Q_L];
  qa.q_r = t.sel[Q_R];
  qa.q_o = t.sel[Q_O];
  qa.q_c = t.sel[Q_C];
  qa.q_4 = t.sel[Q_4];
  qa.q_arith = t.sel[Q_ARITH];
  qa.q_range = t.sel[Q_RANGE];
  qa.q_logic = t.sel[Q_LOGIC];
  qa.q_fixed_group_add = t.sel[Q_FIXED];
  qa.q_variable_group_add = t.sel[Q_VAR];
  qa.l1 = t.l1;
  qa.x = t.x;
  put(qa.alpha, ch[C_ALPHA]);
  put(qa.beta, ch[C_BETA]);
  put(qa.gamma, ch[C_GAMMA]);
  put(qa.range_sep, ch[C_RANGE_SEP]);
  put(qa.logic_sep, ch[C_LOGIC_SEP]);
  put(qa.fixed_sep, ch[C_FIXED_SEP]);
  put(qa.var_sep, ch[C_VAR_SEP]);
  for (int j = 0; j < 3; ++j) put(qa.k[j], k[j]);
  for (int j = 0; j < 4; ++j) put(qa.zh_inv[j], t.zh_inv[j]);
}

// The linearisation polynomial r = sum of coefficient x polynomial, from the openings and the challenges: terms[0 .. count)
// in the order of the device's linear combination.  Sets r(z) (the same sum over the values at z, term by term: ev[E_R] and
// r_z) and c_z, the coefficient of z.
struct LinTerm {
  PolyRef poly;
  HFr coeff;
};
void linearise(ProofRounds& pr, const HFr key_k[3], size_t n, const bool sel_zero[NSEL], LinTerm terms[12], uint32_t* count) {
  const HFr *ev = pr.ev, *xv = pr.xv, *ch = pr.ch;
  const HFr &a_ = ev[E_A], &b_ = ev[E_B], &c_ = ev[E_C], &d_ = ev[E_D], &s1 = ev[E_S1], &s2 = ev[E_S2], &s3 = ev[E_S3],
            &z_next = ev[E_ZN], &qar = ev[E_QARITH];
  const HFr &beta = ch[C_BETA], &gamma = ch[C_GAMMA], &alpha = ch[C_ALPHA], &zc = ch[C_Z];
  const HFr one = fone(), zn = fpow(zc, n);
  const HFr l1_z = fmul(fsub(zn, one), finv(fmul(fr_u64(n), fsub(zc, one))));
  const HFr bz = fmul(beta, zc);
  HFr ident = fadd(fadd(a_, bz), gamma);
  const HFr* wv[3] = {&b_, &c_, &d_};
  for (int j = 0; j < 3; ++j) ident = fmul(ident, fadd(fadd(*wv[j], fmul(bz, key_k[j])), gamma));
  const HFr copy3 = fmul(fmul(fadd(fadd(a_, fmul(beta, s1)), gamma), fadd(fadd(b_, fmul(beta, s2)), gamma)),
                         fadd(fadd(c_, fmul(beta, s3)), gamma));
  const HFr alpha2 = fmul(alpha, alpha);
  const RowEvals re{a_, b_, c_, d_, ev[E_AN], ev[E_BN], ev[E_DN], ev[E_QL], ev[E_QR], ev[E_QC]};
  uint32_t k = 0;
  HFr r_z = pm::host::zero<4>();
  auto term = [&](uint8_t role, int index, const HFr& c, const HFr& value_at_z) {
    terms[k++] = LinTerm{{role, (uint8_t)index}, c};
    r_z = fadd(r_z, fmul(c, value_at_z));
  };
  // arithmetic: q_arith(z) (a b q_m + a q_l + b q_r + c q_o + d q_4 + q_c)
  term(R_SELECTOR, Q_M, fmul(qar, fmul(a_, b_)), xv[X_QM]);
  term(R_SELECTOR, Q_L, fmul(qar, a_), ev[E_QL]);
  term(R_SELECTOR, Q_R, fmul(qar, b_), ev[E_QR]);
  term(R_SELECTOR, Q_O, fmul(qar, c_), xv[X_QO]);
  term(R_SELECTOR, Q_4, fmul(qar, d_), xv[X_Q4]);
  term(R_SELECTOR, Q_C, qar, ev[E_QC]);
  if (!sel_zero[Q_RANGE]) term(R_SELECTOR, Q_RANGE, widget_range(ch[C_RANGE_SEP], re), xv[X_RANGE]);
  if (!sel_zero[Q_LOGIC]) term(R_SELECTOR, Q_LOGIC, widget_logic(ch[C_LOGIC_SEP], re), xv[X_LOGIC]);
  if (!sel_zero[Q_FIXED]) term(R_SELECTOR, Q_FIXED, widget_fixed(ch[C_FIXED_SEP], re), xv[X_FIXED]);
  if (!sel_zero[Q_VAR]) term(R_SELECTOR, Q_VAR, widget_var(ch[C_VAR_SEP], re), xv[X_VAR]);
  pr.c_z = fadd(fmul(alpha, ident), fmul(alpha2, l1_z));
  term(R_Z, 0, pr.c_z, xv[X_Z]);
  term(R_SIGMA, 3, fneg(fmul(fmul(fmul(alpha, copy3), beta), z_next)), xv[X_S4]);
  *count = k;
  pr.r_z = r_z;
  pr.ev[E_R] = r_z;
}

// CommitKey::compute_aggregate_witness: the coefficients of the polynomial opened at z -- t_1..t_4 by powers of z^n (the
// quotient comes first, power 0 of the challenge), then r, a, b, c, d, sigma_1..3 by powers 1..8 of the first aggregation
// challenge -- and of the one opened at z w: z, a, b, d by powers 0..3 of the second.
void aggregation_coeffs(const ProofRounds& pr, size_t n, HFr ac[12], HFr sh[4]) {
  const HFr one = fone(), zn = fpow(pr.ch[C_Z], n);
  ac[0] = one;
  ac[1] = zn;
  ac[2] = fmul(zn, zn);
  ac[3] = fmul(ac[2], zn);
  HFr vp = one;
  for (int e = 0; e < 8; ++e) {
    vp = fmul(vp, pr.ch[C_AW]);
    ac[4 + e] = vp;
  }
  vp = one;
  for (int e = 0; e < 4; ++e) {
    sh[e] = vp;
    vp = fmul(vp, pr.ch[C_AWS]);
  }
}
}  // namespace
