// Gadget witnesses (DESIGN.md sections 7.2f to 7.2i): the inverse of the witness check.  Given the inputs of a gadget, write the
// variables that make its rows hold (definitions: include/plonk_mi355x.h, pm_plonk_gadget).  A kind is three things: its record
// in gadget_kinds.h (rows, limits, what set time gathers for it, launch shape), its set-time rule here -- the widget kinds have
// their selector on every row but the last (gadget_verify_kernel, which also gathers the table points of the fixed-base rounds
// from q_l / q_r); the kinds laid out in arithmetic rows have a rule_<kind> function that says what each row must be, and
// composed_verify_kernel compares and gathers what the rule names -- and its fill kernel, entered in FILL_KERNELS.  To add a
// kind: a row of the table, a rule function with its case in composed_verify_kernel, and a fill kernel.
//
// The fill kernels carry their reasoning where they stand.  One thread per (gadget, proof): range and logic (quads of the
// canonical inputs, accumulators by 4 acc + quad, the quad products), curve_add, arith, maybe_equal; per bit as well: bits; one
// WAVE per (gadget, proof): hades, fixed_base (the hot path) and var_base.
//
// Forms: variables are canonical Montgomery ("ABI", x 2^256); the point arithmetic runs in the device form x 2^261
// (poly_common.hip.h).  Everything written goes through fe_store, i.e. is canonical.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "context.h"
#include "field_inv.hip.h"
#include "gadget_kinds.h"
#include "jubjub.hip.h"
#include "poly_common.hip.h"

namespace pm {
namespace {

#define PM_HOSTDEV __host__ __device__ inline

// ------------------------------------------------------------------ bit work on little-endian 32-bit words (host and device)
// w[i] without a dynamic index (the arrays stay in registers); 0 past the end
template <int NW>
PM_HOSTDEV u32 word_at(const u32 (&w)[NW], u32 i) {
  u32 r = 0;
#pragma unroll
  for (int k = 0; k < NW; ++k) r = (u32)k == i ? w[k] : r;
  return r;
}
template <int NW>
PM_HOSTDEV u32 bit_at(const u32 (&w)[NW], u32 pos) {
  return (word_at<NW>(w, pos >> 5) >> (pos & 31u)) & 1u;
}
template <int NW>
PM_HOSTDEV u32 quad_at(const u32 (&w)[NW], u32 pos) {   // pos even
  return (word_at<NW>(w, pos >> 5) >> (pos & 31u)) & 3u;
}
// w >> nbits != 0
template <int NW>
PM_HOSTDEV bool any_above(const u32 (&w)[NW], u32 nbits) {
  u32 acc = 0;
#pragma unroll
  for (int k = 0; k < NW; ++k) {
    const u32 lo = 32u * (u32)k;
    if (lo >= nbits) acc |= w[k];
    else if (lo + 32u > nbits) acc |= w[k] >> ((nbits - lo) & 31u);
  }
  return acc != 0;
}
// word w of the mask of the low `keep` bits
PM_HOSTDEV u32 low_bits_mask(u32 w, u32 keep) {
  const u32 lo = 32 * w;
  return lo + 32 <= keep ? 0xffffffffu : (lo >= keep ? 0u : ((1u << ((keep - lo) & 31u)) - 1u));
}
template <int NW>
PM_HOSTDEV u32 words_or(const u32 (&w)[NW]) {
  u32 acc = 0;
#pragma unroll
  for (int k = 0; k < NW; ++k) acc |= w[k];
  return acc;
}
// s (8 words) as 9 words and x = 3 s
PM_HOSTDEV void naf_operands(const u32 (&s)[8], u32 (&s9)[9], u32 (&x9)[9]) {
  u64 c = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    s9[i] = s[i];
    c += 3ull * s[i];
    x9[i] = (u32)c;
    c >>= 32;
  }
  s9[8] = 0;
  x9[8] = (u32)c;
}
// e_j = bit_(j+1)(3 s) - bit_(j+1)(s) in {-1, 0, 1}
PM_HOSTDEV int naf_digit(const u32 (&x9)[9], const u32 (&s9)[9], u32 j) {
  return (int)bit_at<9>(x9, j + 1) - (int)bit_at<9>(s9, j + 1);
}
// some e_j with j >= rounds is non-zero
PM_HOSTDEV bool naf_too_long(const u32 (&x9)[9], const u32 (&s9)[9], u32 rounds) {
  u32 t[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) t[i] = x9[i] ^ s9[i];
  return any_above<9>(t, rounds + 1);
}

// ------------------------------------------------------------------ device records and arguments
struct GadgetFill {
  const GadgetRec* recs;
  const u32* wire_vars;     // [4][n]
  const u32x4* tab;         // table points, 4 x 16 bytes per round: x | y canonical
  const u32x4* coef;        // ARITH rows, 10 x 16 bytes each: q_m q_l q_r q_4 q_c canonical
  const u32x4* hcoef;       // HADES rounds, 60 x 16 bytes each: 25 matrix entries, 5 round keys, canonical (context.h)
  const u32* hids;          // HADES rounds, 30 ids each: the c variables of the round's rows (context.h)
  u32x4* vars;              // [batch][var_stride] canonical
  size_t var_stride, n;
  unsigned long long* rep;  // [batch] failing gadgets, then [batch] min(index * 4 + reason)
  u32 edwards_d[9];         // device form
};

PM_DEV void gadget_fail(const GadgetFill& a, u32 proof, u32 index, u32 reason) {   // batch = gridDim.y: not for a BITS_X kernel
  atomicAdd(a.rep + proof, 1ull);                                              // a count and a minimum: order-free
  atomicMin(a.rep + gridDim.y + proof, (unsigned long long)index * 4 + reason);
}
PM_DEV u32 var_id(const GadgetFill& a, u32 wire, size_t row) { return a.wire_vars[(size_t)wire * a.n + row]; }
PM_DEV Fr ld_var(const u32x4* vars, u32 id) { return id == PM_PLONK_NO_VAR ? fe_zero<FrP>() : ld_canon(vars, id); }
PM_DEV void st_var(u32x4* vars, u32 id, const Fr& v) {
  if (id != PM_PLONK_NO_VAR) st_canon(vars, id, v);
}

// ------------------------------------------------------------------ field helpers: gadd .. g_sel are in jubjub.hip.h
PM_DEV bool g_is_zero(const Fr& v) {   // a zero may arrive as r: test the canonical words
  u32 s[8];
  fe_canon_pack<FrP>(s, v);
  return words_or<8>(s) == 0;
}
// canonical Montgomery element -> the integer below r it stands for
PM_DEV void g_to_int(const Fr& abi, u32 (&w)[8]) { fe_canon_pack<FrP>(w, fe_mul_limb<FrP>(abi, 32u)); }   // x 2^256 * 2^5 / 2^261
// integer below 2^256 -> Montgomery (ABI) element, value < 2 r
PM_DEV Fr g_from_int(const u32 (&w)[8]) { return fe_mul<FrP>(fe_unpack<FrP>(w), fe_pow2<FrP, 256 + 261>()); }
PM_DEV Fr g_small(u32 c) {             // c < 2^29
  Fr t = fe_zero<FrP>();
  t.l[0] = c;
  return fe_mul<FrP>(t, fe_pow2<FrP, 256 + 261>());
}
// 4 acc + q, q in 0..3 (ABI form in and out): limbs < 2^31 + 3 * 2^29, value < 8 r before the reduction
PM_DEV Fr g_acc_step(const Fr& acc, u32 q) {
  const Fr one = g_one_abi();
  Fr t = fe_add<FrP>(acc, acc);
  t = fe_add<FrP>(t, t);
#pragma unroll
  for (int i = 0; i < 9; ++i) t.l[i] += q * one.l[i];
  return fe_reduce_weak<FrP>(t);
}

// ------------------------------------------------------------------ set time: selectors of the claimed rows, table points
PM_DEV void sel_words(const u32x4* sel, size_t n, u32 s, size_t row, u32 (&w)[8]) {
  const u32x4 lo = sel[2 * (n * s + row)], hi = sel[2 * (n * s + row) + 1];
  w[0] = lo.x, w[1] = lo.y, w[2] = lo.z, w[3] = lo.w, w[4] = hi.x, w[5] = hi.y, w[6] = hi.z, w[7] = hi.w;
}
PM_DEV u32 sel_or(const u32x4* sel, size_t n, u32 s, size_t row) {   // 0: the selector vanishes on the row
  u32 w[8];
  sel_words(sel, n, s, row, w);
  return words_or<8>(w);
}
PM_DEV void st_words8(u32x4* o, const u32 (&w)[8]) {
  o[0] = u32x4{w[0], w[1], w[2], w[3]};
  o[1] = u32x4{w[4], w[5], w[6], w[7]};
}
// The widget kinds.  sel: vectors of n values on H; q_l, q_r are vectors ql, ql + 1 and the four widget selectors wid .. wid + 3
// (0 and 2 of q_l q_r q_range q_logic q_fixed_group_add q_variable_group_add; 1 and 7 of all eleven)
__global__ void __launch_bounds__(256) gadget_verify_kernel(const GadgetRec* recs, const u32x4* sel, size_t n, u32 ql, u32 wid,
                                                            u32x4* tab, u32* bad) {
  const GadgetRec rec = recs[blockIdx.x];
  const GadgetKind kind = gadget_kind(rec.kind);
  if (kind.all_selectors) return;   // composed_verify_kernel
  const u32 rows = (u32)gadget_kind_rows(kind, rec.count, rec.param) - kind.trailing;
  bool miss = false;
  for (u32 t = threadIdx.x; t < rows; t += 256) {
    const size_t row = (size_t)rec.first_row + t;
    u32 w[8];
    miss |= sel_or(sel, n, wid + rec.kind, row) == 0;
    if (kind.tab == GadgetTab::POINTS)
      for (u32 s = 0; s < 2; ++s) {   // x | y of the round's table point
        sel_words(sel, n, ql + s, row, w);
        st_words8(tab + 4 * ((size_t)rec.tab + t) + 2 * s, w);
      }
  }
  if (miss) atomicMin(bad, rec.index);
}

// The kinds laid out in arithmetic rows (include/plonk_mi355x.h).  A kind's rule says what row t of a gadget must be;
// composed_verify_kernel below reads the row and compares.
enum : u32 { ROW_ARITH, ROW_VAR_ADD, ROW_RESULT };   // q_arith and no widget selector; q_variable_group_add; selectors not looked at
constexpr u32 NO_SLOT = ~0u;
struct Wires { const u32 *a, *b, *c, *d; };   // [n] each
struct RowRule {
  const char* want = "***-**";            // q_m q_l q_r q_o q_c q_4: 0, 1, - (minus one), P (the power of two pw) or * (free)
  u32 pw[8] = {0, 0, 0, 0, 0, 0, 0, 0}, sel = ROW_ARITH;
  bool miss = false;                      // a wire id is not what the layout implies, or a written position is no variable
  // gathered for the fill: coefficient s to 32-byte slot[s] of unit `unit` (an ARITH row, a HADES round), the c id to id_slot
  size_t unit = 0;
  u32 slot[6] = {NO_SLOT, NO_SLOT, NO_SLOT, NO_SLOT, NO_SLOT, NO_SLOT}, id_slot = NO_SLOT;
};

// c = q_m a b + q_l a + q_r b + q_4 d + q_c: q_o = -1 and c is written; q_m q_l q_r q_4 q_c are gathered in that order
PM_DEV RowRule rule_arith(const GadgetRec& rec, u32 t, size_t row, const Wires& w) {
  RowRule r;
  r.miss = w.c[row] == PM_PLONK_NO_VAR;
  r.unit = (size_t)rec.tab + t;
  r.slot[0] = 0, r.slot[1] = 1, r.slot[2] = 2, r.slot[4] = 4, r.slot[5] = 3;
  return r;
}

// two rows a bit k: bit * bit - bit, then 2^k bit + acc_(k-1) - acc_k
PM_DEV RowRule rule_bits(const GadgetRec& rec, u32 t, size_t row, const Wires& w) {
  RowRule r;
  const u32 k = t >> 1, va = w.a[row], vb = w.b[row], vc = w.c[row];
  if ((t & 1u) == 0) {
    r.want = "100-00";
    r.miss = va == PM_PLONK_NO_VAR || vb != va || vc != va;
  } else {
    r.want = "0P1-00";
    u32 e[8];
#pragma unroll
    for (u32 i = 0; i < 8; ++i) e[i] = i == (k >> 5) ? 1u << (k & 31u) : 0u;
    fe_canon_pack<FrP>(r.pw, g_from_int(e));
    r.miss = vc == PM_PLONK_NO_VAR || va != w.a[row - 1] || (k && vb != w.c[row - 2]);
  }
  return r;
}

// a - b - u, then 1 - z u - y, then y u
PM_DEV RowRule rule_maybe_equal(const GadgetRec& rec, u32 t, size_t row, const Wires& w) {
  RowRule r;
  const u32 va = w.a[row], vb = w.b[row], vc = w.c[row], u = w.c[rec.first_row], y = w.c[(size_t)rec.first_row + 1];
  r.want = t == 0 ? "01--00" : t == 1 ? "-00-10" : "100000";
  r.miss = t == 0 ? vc == PM_PLONK_NO_VAR : t == 1 ? va == PM_PLONK_NO_VAR || vc == PM_PLONK_NO_VAR || vb != u : va != y || vb != u;
  return r;
}

// H = param / 2 full rounds, count - 2 H partial ones, H full ones; 30 rows a full round and 18 a partial one: 5 key rows, 3
// s-box rows for every word (full) or for word 4 (partial), 10 matrix rows.  Every c is written; its id and the round's keys
// and matrix entries are gathered (context.h, GADGET_ROUND_COEFS)
PM_DEV RowRule rule_hades(const GadgetRec& rec, u32 t, size_t row, const Wires& w) {
  RowRule r;
  const u32 H = rec.param >> 1, rows_head = 30 * H, rows_mid = 18 * (rec.count - 2 * H);
  const bool head = t < rows_head, full = head || t >= rows_head + rows_mid;
  const u32 first = head ? 0u : full ? rec.count - H : H;                      // the first round of the row's run of rounds ...
  const u32 tr = head ? t : full ? t - rows_head - rows_mid : t - rows_head;   // ... and the row within that run
  const u32 rho = first + tr / (full ? 30u : 18u), pos = tr % (full ? 30u : 18u);   // the round and the row's place in it
  const size_t rb = row - pos;                     // the round's first row
  const u32 sbox_rows = full ? 15u : 3u, va = w.a[row], vb = w.b[row];
  r.unit = (size_t)rec.tab + rho;
  r.miss = w.c[row] == PM_PLONK_NO_VAR;
  if (pos < 5) {                                   // s'[j] = s[j] + q_c; s[j] is o_j of the round before
    r.want = "010-*0";
    r.slot[4] = 25 + pos;
    if (rho) r.miss |= va != w.c[rb - 10 + 2 * pos + 1];
    r.id_slot = pos;
  } else if (pos < 5 + sbox_rows) {                // x2 = x x, x4 = x2 x2, x5 = x4 x
    const u32 u = pos - 5, j = full ? u / 3 : 4u, k = u % 3;
    const u32 x = w.c[rb + j];
    r.want = "100-00";
    r.miss |= va != (k ? w.c[row - 1] : x) || vb != (k == 1 ? w.c[row - 1] : x);
    r.id_slot = 5 * (k + 1) + j;
  } else {                                         // z_i = M_i0 v0 + M_i1 v1 + M_i2 v2, o_i = M_i3 v3 + M_i4 v4 + z_i
    const u32 u = pos - 5 - sbox_rows, i = u >> 1, k = u & 1u;
    u32 v[3];
#pragma unroll
    for (u32 e = 0; e < 3; ++e) {
      const u32 j = 3 * k + e;                     // j = 5 (k = 1, e = 2) is z_i
      v[e] = j == 5 ? w.c[row - 1] : full ? w.c[rb + 5 + 3 * j + 2] : j == 4 ? w.c[rb + 7] : w.c[rb + j];
    }
    r.want = k ? "0**-01" : "0**-0*";
    r.slot[1] = 5 * i + 3 * k, r.slot[2] = 5 * i + 3 * k + 1;
    if (!k) r.slot[5] = 5 * i + 2;
    r.miss |= va != v[0] || vb != v[1] || w.d[row] != v[2];
    r.id_slot = 20 + u;
  }
  return r;
}

// six rows a round: the doubling (q_variable_group_add) and its result row, sx = bit P.x, sy = bit P.y - bit + 1 (arithmetic
// rows), the addition of (sx, sy) and its result row
PM_DEV RowRule rule_var_base(const GadgetRec& rec, u32 t, size_t row, const Wires& w) {
  RowRule r;
  const u32 pos = t % 6, va = w.a[row], vb = w.b[row], vc = w.c[row], vd = w.d[row];
  const size_t r0 = rec.first_row, rb = row - pos;   // the gadget's and the round's first row
  r.want = pos == 2 ? "100-00" : pos == 3 ? "1-0-10" : "******";
  r.sel = pos == 0 || pos == 4 ? ROW_VAR_ADD : pos == 1 || pos == 5 ? ROW_RESULT : ROW_ARITH;
  switch (pos) {
    case 0: r.miss = vc != va || vd != vb || (rb != r0 && (va != w.a[rb - 1] || vb != w.b[rb - 1])); break;   // acc + acc; acc: the round before
    case 2: r.miss = vc == PM_PLONK_NO_VAR || vb != w.b[r0 + 2]; break;                                       // sx = bit P.x
    case 3: r.miss = vc == PM_PLONK_NO_VAR || va != w.a[row - 1] || vb != w.b[r0 + 3]; break;                 // sy = bit P.y - bit + 1
    case 4: r.miss = va != w.a[rb + 1] || vb != w.b[rb + 1] || vc != w.c[rb + 2] || vd != w.c[rb + 3]; break;   // dbl + (sx, sy)
    default: r.miss = va == PM_PLONK_NO_VAR || vb == PM_PLONK_NO_VAR || vd == PM_PLONK_NO_VAR; break;         // a result row: x, y, product
  }
  return r;
}

// sel: all eleven selectors on H in the order of PM_PLONK_SELECTORS -- q_m q_l q_r q_o q_c q_4 q_arith, then the four widget
// selectors, q_variable_group_add last
__global__ void __launch_bounds__(256) composed_verify_kernel(const GadgetRec* recs, const u32x4* sel, size_t n, const u32* wire_vars,
                                                              u32x4* coef, u32x4* hcoef, u32* hids, u32* bad) {
  const GadgetRec rec = recs[blockIdx.x];
  const GadgetKind kind = gadget_kind(rec.kind);
  if (!kind.all_selectors) return;   // gadget_verify_kernel
  const u32 rows = (u32)gadget_kind_rows(kind, rec.count, rec.param);
  const Wires wires{wire_vars, wire_vars + n, wire_vars + 2 * n, wire_vars + 3 * n};
  u32 one[8], neg[8];
  fe_canon_pack<FrP>(one, g_one_abi());
  fe_canon_pack<FrP>(neg, gneg(g_one_abi()));
  bool miss = false;
  for (u32 t = threadIdx.x; t < rows; t += 256) {
    const size_t row = (size_t)rec.first_row + t;
    RowRule r;
    switch (rec.kind) {
      case PM_PLONK_COMPOSED_ARITH: r = rule_arith(rec, t, row, wires); break;
      case PM_PLONK_COMPOSED_BITS: r = rule_bits(rec, t, row, wires); break;
      case PM_PLONK_COMPOSED_MAYBE_EQUAL: r = rule_maybe_equal(rec, t, row, wires); break;
      case PM_PLONK_PERMUTATION_HADES: r = rule_hades(rec, t, row, wires); break;
      case PM_PLONK_GADGET_VAR_BASE: r = rule_var_base(rec, t, row, wires); break;
    }
    miss |= r.miss;
    const bool no_arith = sel_or(sel, n, 6, row) == 0;
    u32 w[8], widget = 0, last = 0;
#pragma unroll
    for (u32 s = 7; s < 11; ++s) widget |= last = sel_or(sel, n, s, row);
    if (r.sel == ROW_ARITH) miss |= no_arith || widget != 0;
    else if (r.sel == ROW_VAR_ADD) miss |= last == 0;
    u32x4* const out = kind.tab == GadgetTab::COEF ? coef + 2 * (GADGET_COEF_BYTES / 32) * r.unit : hcoef + 2 * GADGET_ROUND_COEFS * r.unit;
    if (r.id_slot != NO_SLOT) hids[GADGET_ROUND_IDS * r.unit + r.id_slot] = wires.c[row];
#pragma unroll
    for (u32 s = 0; s < 6; ++s) {
      sel_words(sel, n, s, row, w);
      u32 diff = 0;
#pragma unroll
      for (u32 i = 0; i < 8; ++i) {
        const u32 x = r.want[s] == '1' ? one[i] : r.want[s] == '-' ? neg[i] : r.want[s] == 'P' ? r.pw[i] : 0u;
        diff |= w[i] ^ x;
      }
      miss |= r.want[s] != '*' && diff != 0;
      if (r.slot[s] != NO_SLOT) st_words8(out + 2 * r.slot[s], w);
    }
  }
  if (miss) atomicMin(bad, rec.index);
}

// ------------------------------------------------------------------ range and logic
__global__ void __launch_bounds__(64) gadget_range_kernel(const GadgetFill a, u32 first, u32 count) {
  const u32 g = blockIdx.x * 64 + threadIdx.x, proof = blockIdx.y;
  if (g >= count) return;
  const GadgetRec rec = a.recs[first + g];
  u32x4* const vars = a.vars + 2 * a.var_stride * proof;
  u32 v[8];
  g_to_int(ld_canon(vars, rec.in_var[0]), v);
  const u32 quads = 4 * rec.count;
  if (any_above<8>(v, 2 * quads)) gadget_fail(a, proof, rec.index, PM_PLONK_GADGET_TOO_WIDE);
  Fr acc = fe_zero<FrP>();
  for (u32 k = 0;; ++k) {   // acc_k sits at row k / 4, wire d, c, b, a for k mod 4 = 0, 1, 2, 3
    st_var(vars, var_id(a, 3 - (k & 3u), (size_t)rec.first_row + (k >> 2)), acc);
    if (k == quads) break;
    acc = g_acc_step(acc, quad_at<8>(v, 2 * (quads - 1 - k)));
  }
}

__global__ void __launch_bounds__(64) gadget_logic_kernel(const GadgetFill a, u32 first, u32 count) {
  const u32 g = blockIdx.x * 64 + threadIdx.x, proof = blockIdx.y;
  if (g >= count) return;
  const GadgetRec rec = a.recs[first + g];
  u32x4* const vars = a.vars + 2 * a.var_stride * proof;
  u32 x[8], y[8];
  g_to_int(ld_canon(vars, rec.in_var[0]), x);
  g_to_int(ld_canon(vars, rec.in_var[1]), y);
  const u32 Q = rec.count;
  if (any_above<8>(x, 2 * Q) || any_above<8>(y, 2 * Q)) gadget_fail(a, proof, rec.index, PM_PLONK_GADGET_TOO_WIDE);
  Fr A = fe_zero<FrP>(), B = A, D = A;
  for (u32 k = 0;; ++k) {
    const size_t row = (size_t)rec.first_row + k;
    st_var(vars, var_id(a, 0, row), A);
    st_var(vars, var_id(a, 1, row), B);
    st_var(vars, var_id(a, 3, row), D);
    if (k == Q) break;
    const u32 qx = quad_at<8>(x, 2 * (Q - 1 - k)), qy = quad_at<8>(y, 2 * (Q - 1 - k));
    st_var(vars, var_id(a, 2, row), g_small(qx * qy));
    A = g_acc_step(A, qx);
    B = g_acc_step(B, qy);
    D = g_acc_step(D, rec.param ? (qx ^ qy) : (qx & qy));
  }
}

// ------------------------------------------------------------------ JubJub: -x^2 + y^2 = 1 + d x^2 y^2, device form throughout
// (x1, y1) + (x2, y2) = ((x1 y2 + y1 x2) / (1 + k), (y1 y2 + x1 x2) / (1 - k)), k = d x1 x2 y1 y2: complete on the curve.
// One thread per (gadget, proof) of a kernel whose inversion votes across the wave (field_inv.hip.h), so that no lane may leave
// early: a lane past the end works on the last gadget and, not being `live`, writes nothing.
PM_DEV GadgetRec clamped_rec(const GadgetFill& a, u32 first, u32 count, bool& live) {
  const u32 g = blockIdx.x * 64 + threadIdx.x;
  live = g < count;
  return a.recs[first + (live ? g : count - 1)];
}
__global__ void __launch_bounds__(64) gadget_curve_add_kernel(const GadgetFill a, u32 first, u32 count) {
  const u32 proof = blockIdx.y;
  bool live;
  const GadgetRec rec = clamped_rec(a, first, count, live);
  u32x4* const vars = a.vars + 2 * a.var_stride * proof;
  const size_t row = rec.first_row;
  const Fr x1 = g_to_dev(ld_var(vars, var_id(a, 0, row))), y1 = g_to_dev(ld_var(vars, var_id(a, 1, row)));
  const Fr x2 = g_to_dev(ld_var(vars, var_id(a, 2, row))), y2 = g_to_dev(ld_var(vars, var_id(a, 3, row)));
  const Fr one = fe_one<FrP>();
  const Fr x1y2 = gmul(x1, y2), y1x2 = gmul(y1, x2), y1y2 = gmul(y1, y2), x1x2 = gmul(x1, x2);
  const Fr k = gmul(gmul(x1y2, y1x2), fr_limbs(a.edwards_d));
  const Fr den1 = gadd(one, k), den2 = gsub(one, k);
  const Fr dd = gmul(den1, den2);
  const Fr inv = fe_inv_dev<FrP>(dd);                  // 0 -> 0: a degenerate pair gets x3 = y3 = 0
  const Fr x3 = gmul(gmul(gadd(x1y2, y1x2), den2), inv), y3 = gmul(gmul(gadd(y1y2, x1x2), den1), inv);
  if (!live) return;
  if (g_is_zero(dd)) gadget_fail(a, proof, rec.index, PM_PLONK_GADGET_DEGENERATE);
  st_var(vars, var_id(a, 0, row + 1), g_to_abi(x3));
  st_var(vars, var_id(a, 1, row + 1), g_to_abi(y3));
  st_var(vars, var_id(a, 3, row + 1), g_to_abi(x1y2));
}

// ------------------------------------------------------------------ composed gadgets
// A run of arithmetic rows with q_o = -1 (verified at set time): c = q_m a b + q_l a + q_r b + q_4 d + q_c, one row after the
// other, so a row reads what the rows before it wrote.  One thread per (gadget, proof); the coefficients were gathered at set time.
__global__ void __launch_bounds__(64) gadget_arith_kernel(const GadgetFill a, u32 first, u32 count) {
  const u32 g = blockIdx.x * 64 + threadIdx.x, proof = blockIdx.y;
  if (g >= count) return;
  const GadgetRec rec = a.recs[first + g];
  u32x4* const vars = a.vars + 2 * a.var_stride * proof;
#pragma unroll 1
  for (u32 i = 0; i < rec.count; ++i) {
    const size_t row = (size_t)rec.first_row + i;
    const u32x4* q = a.coef + 10 * ((size_t)rec.tab + i);
    const Fr A = ld_var(vars, var_id(a, 0, row)), B = ld_var(vars, var_id(a, 1, row)), D = ld_var(vars, var_id(a, 3, row));
    // coefficient in the device form x value in the ABI form -> ABI
    Fr c = gmul(g_to_dev(gmul(g_to_dev(ld_canon(q, 0)), A)), B);
    c = gadd(c, gmul(g_to_dev(ld_canon(q, 1)), A));
    c = gadd(c, gmul(g_to_dev(ld_canon(q, 2)), B));
    c = gadd(c, gmul(g_to_dev(ld_canon(q, 3)), D));
    c = gadd(c, ld_canon(q, 4));
    st_var(vars, var_id(a, 2, row), c);
  }
}

// Bit decomposition: blockIdx.x * 64 + threadIdx.x = the bit k, blockIdx.y = the gadget within the launch, blockIdx.z = the
// proof.  acc_k = acc_(-1) + (V mod 2^(k+1)): every thread masks its own copy of V, nothing is passed from bit to bit.
__global__ void __launch_bounds__(64) gadget_bits_kernel(const GadgetFill a, u32 first, u32) {
  const u32 k = blockIdx.x * 64 + threadIdx.x, proof = blockIdx.z;
  const GadgetRec rec = a.recs[first + blockIdx.y];
  if (k >= rec.count) return;
  u32x4* const vars = a.vars + 2 * a.var_stride * proof;
  const size_t row0 = rec.first_row;
  u32 v[8], m[8];
  g_to_int(ld_canon(vars, rec.in_var[0]), v);
#pragma unroll
  for (u32 w = 0; w < 8; ++w) m[w] = v[w] & low_bits_mask(w, k + 1);
  const Fr acc = gadd(g_from_int(m), ld_var(vars, var_id(a, 1, row0 + 1)));
  st_var(vars, var_id(a, 0, row0 + 2 * (size_t)k), g_sel(bit_at<8>(v, k) != 0, g_one_abi(), fe_zero<FrP>()));
  st_var(vars, var_id(a, 2, row0 + 2 * (size_t)k + 1), acc);
}

// u = a - b, z = 1 / u or 0, y = 1 - u z = [u = 0].  One thread per (gadget, proof), clamped as in gadget_curve_add_kernel.
__global__ void __launch_bounds__(64) gadget_maybe_equal_kernel(const GadgetFill a, u32 first, u32 count) {
  const u32 proof = blockIdx.y;
  bool live;
  const GadgetRec rec = clamped_rec(a, first, count, live);
  u32x4* const vars = a.vars + 2 * a.var_stride * proof;
  const size_t row = rec.first_row;
  const Fr u = gsub(ld_var(vars, var_id(a, 0, row)), ld_var(vars, var_id(a, 1, row)));
  const Fr inv = fe_inv_dev<FrP>(g_to_dev(u));         // 0 -> 0
  if (!live) return;
  st_var(vars, var_id(a, 2, row), u);
  st_var(vars, var_id(a, 0, row + 1), g_to_abi(inv));
  st_var(vars, var_id(a, 2, row + 1), g_sel(g_is_zero(u), g_one_abi(), fe_zero<FrP>()));
}

// ------------------------------------------------------------------ the wave kernels: an element from another lane
PM_DEV Fr fr_shfl(const Fr& v, u32 src) {
  Fr r;
#pragma unroll
  for (int i = 0; i < 9; ++i) r.l[i] = __shfl(v.l[i], (int)src);
  return r;
}
PM_DEV Fr fr_shfl_up(const Fr& v, u32 delta) {
  Fr r;
#pragma unroll
  for (int i = 0; i < 9; ++i) r.l[i] = __shfl_up(v.l[i], delta);
  return r;
}
constexpr u32 GADGET_RUN = PM_PLONK_GADGET_MAX_ROUNDS / 64;   // rounds a lane of a wave kernel owns at most

// ------------------------------------------------------------------ a Hades permutation of width 5
// One wave per (gadget, proof): blockIdx.x = the gadget within the launch, blockIdx.y = the proof.  Lane 5 i + j (i, j < 5) holds
// state word j and the matrix entry (i, j); lanes 25..63 leave at once and no cross-lane read names them: every source below is
// 5 i + e or 5 j with e < 5.  The loop and the kind of a round depend on the gadget only, so the 25 lanes stay together; which of
// x and x^5 a lane keeps is a select.  Every lane of row group i ends a round with z_i and o_i, every lane of column j with
// x, x^2, x^4, x^5 of word j, so the stores are spread: lane (k, j), k < 4, writes the k-th of the latter four, lanes (i, 0) and
// (i, 1) write z_i and o_i -- two stores a round and lane, their ids gathered at set time in exactly that order (NO_VAR where a
// partial round has no such row).  The next round's two coefficients and two ids are loaded before this round's arithmetic.
// Forms as in gadget_arith_kernel: the state is in the ABI form, one operand of each product goes through g_to_dev.
__global__ void __launch_bounds__(64) gadget_hades_kernel(const GadgetFill a, u32 first, u32) {
  const u32 lane = threadIdx.x, proof = blockIdx.y;
  if (lane >= 25) return;
  const GadgetRec rec = a.recs[first + blockIdx.x];
  u32x4* const vars = a.vars + 2 * a.var_stride * proof;
  const u32 i = lane / 5, j = lane - 5 * i;
  const u32 R = rec.count, H = rec.param >> 1;
  const u32x4* const q = a.hcoef + 60 * (size_t)rec.tab;
  const u32* const ids = a.hids + 30 * (size_t)rec.tab;
  const u32 slot_a = lane < 20 ? lane : 0, slot_b = 20 + 2 * i + (j & 1u);
  Fr s = ld_var(vars, var_id(a, 0, (size_t)rec.first_row + j));
  Fr key = ld_canon(q, 25 + j), m = ld_canon(q, lane);
  u32 id_a = ids[slot_a], id_b = ids[slot_b];
#pragma unroll 1
  for (u32 rho = 0; rho < R; ++rho) {
    const size_t nx = rho + 1 < R ? rho + 1 : rho;   // the last round loads its own again
    const Fr key_n = ld_canon(q, 30 * nx + 25 + j), m_n = ld_canon(q, 30 * nx + lane);
    const u32 id_a_n = ids[30 * nx + slot_a], id_b_n = ids[30 * nx + slot_b];
    const bool full = rho < H || rho >= R - H;
    const Fr x = gadd(s, key), xd = g_to_dev(x);
    const Fr x2 = gmul(xd, x), x4 = gmul(g_to_dev(x2), x2), x5 = gmul(xd, x4);
    st_var(vars, lane < 20 ? id_a : PM_PLONK_NO_VAR, g_sel(i < 2, g_sel(i == 0, x, x2), g_sel(i == 2, x4, x5)));
    const Fr p = gmul(g_to_dev(m), g_sel(full || j == 4, x5, x));
    const Fr z = gadd(gadd(fr_shfl(p, 5 * i), fr_shfl(p, 5 * i + 1)), fr_shfl(p, 5 * i + 2));
    const Fr o = gadd(gadd(fr_shfl(p, 5 * i + 3), fr_shfl(p, 5 * i + 4)), z);
    st_var(vars, j < 2 ? id_b : PM_PLONK_NO_VAR, g_sel(j == 0, z, o));
    s = fr_shfl(o, 5 * j);
    key = key_n, m = m_n, id_a = id_a_n, id_b = id_b_n;
  }
}

// EdPoint, ed_add, ed_madd, ed_sel: jubjub.hip.h
PM_DEV EdPoint ed_shfl_up(const EdPoint& p, u32 delta) {
  return EdPoint{fr_shfl_up(p.X, delta), fr_shfl_up(p.Y, delta), fr_shfl_up(p.Z, delta), fr_shfl_up(p.T, delta)};
}

// the addend of a round in device form: bit (x_b, y_b) = (bit x_b, bit^2 (y_b - 1) + 1), t = bit x_b y_b; c_abi = t in ABI form
struct Addend {
  Fr x, y, t;
};
PM_DEV Addend fb_addend(const u32x4* tab, size_t round, int bit, Fr* c_abi) {
  const Fr xb_abi = ld_canon(tab, 2 * round), xb = g_to_dev(xb_abi), yb = g_to_dev(ld_canon(tab, 2 * round + 1));
  const Fr t = gmul(xb, yb), one = fe_one<FrP>(), zero = fe_zero<FrP>();
  if (c_abi) {
    const Fr c = gmul(xb_abi, yb);                      // ABI x device -> ABI
    *c_abi = g_sel(bit == 0, zero, g_sel(bit < 0, gneg(c), fe_reduce_weak<FrP>(c)));
  }
  Addend r;
  r.x = g_sel(bit == 0, zero, g_sel(bit < 0, gneg(xb), xb));
  r.y = g_sel(bit == 0, one, yb);
  r.t = g_sel(bit == 0, zero, g_sel(bit < 0, gneg(t), t));
  return r;
}

// One wave per (gadget, proof): blockIdx.x = the gadget within the launch, blockIdx.y = the proof.  Every branch below that
// holds field work is wave-uniform (L, `used` and the loop bounds depend on the gadget only).
// The hot path.  Every lane derives the width-2 NAF digits of its rounds from s and 3 s (e_j = bit_(j+1)(3s) - bit_(j+1)(s): no
// carry travels between lanes), owns a contiguous run of ceil(R / 64) rounds and sums its addends in extended coordinates; the
// lane totals go through an inclusive prefix scan with __shfl_up under the complete twisted Edwards law; each lane then walks
// its run again from the scanned start and normalises its <= 4 prefixes with one inversion (Montgomery's trick).  No lane ever
// runs more than one inversion and there is no chain of dependent per-round inversions.  The addends are re-derived from the
// table in both walks rather than kept across the scan: what stays live over the scan is one point, and over the second walk
// the run's X, Y, Z (the variant kept: see DESIGN.md for the registers).
__global__ void __launch_bounds__(64) gadget_fixed_base_kernel(const GadgetFill a, u32 first, u32) {
  const u32 lane = threadIdx.x, proof = blockIdx.y;
  const GadgetRec rec = a.recs[first + blockIdx.x];
  u32x4* const vars = a.vars + 2 * a.var_stride * proof;
  const u32 R = rec.count, L = (R + 63) >> 6, k0 = lane * L, used = (R + L - 1) / L;   // lanes that own a round
  const size_t row0 = rec.first_row;
  const Fr d = fr_limbs(a.edwards_d), one = fe_one<FrP>(), zero = fe_zero<FrP>();

  // ---- digits: this lane's rounds k0 .. k0 + L - 1, bit_k = e_(R - 1 - k)
  u32 s8[8], s9[9], x9[9];
  g_to_int(ld_canon(vars, rec.in_var[0]), s8);
  naf_operands(s8, s9, x9);
  if (lane == 0 && naf_too_long(x9, s9, R)) gadget_fail(a, proof, rec.index, PM_PLONK_GADGET_SCALAR_TOO_LONG);
  int bit[GADGET_RUN];
#pragma unroll
  for (u32 j = 0; j < GADGET_RUN; ++j) {
    const u32 k = k0 + j;
    bit[j] = (j < L && k < R) ? naf_digit(x9, s9, R - 1 - (k < R ? k : 0)) : 0;
  }
  // ---- the start point (a, b of row 0), every lane reads the same words
  const Fr sx = g_to_dev(ld_var(vars, var_id(a, 0, row0))), sy = g_to_dev(ld_var(vars, var_id(a, 1, row0)));
  const EdPoint start{sx, sy, one, gmul(sx, sy)}, neutral{zero, one, one, zero};

  // ---- the scalar accumulator d: d_k = (x' >> (R - k + 1)) - (s' >> (R - k + 1)) on x', s' cut to R + 1 bits, then
  // d_(k+1) = 2 d_k + bit_k along the run; c_k = bit_k x_b y_b on the way
  {
    const u32 sh = k0 <= R ? R - k0 + 1 : 1, ws = sh >> 5, bs = sh & 31u;
    u32 xm[9], sm[9], xs[8], ss[8];
#pragma unroll
    for (u32 w = 0; w < 9; ++w) xm[w] = x9[w] & low_bits_mask(w, R + 1), sm[w] = s9[w] & low_bits_mask(w, R + 1);
#pragma unroll
    for (u32 i = 0; i < 8; ++i) {
      const u32 xl = word_at<9>(xm, i + ws), xh = word_at<9>(xm, i + ws + 1);
      const u32 sl = word_at<9>(sm, i + ws), sh2 = word_at<9>(sm, i + ws + 1);
      xs[i] = bs ? (xl >> bs) | (xh << (32 - bs)) : xl;
      ss[i] = bs ? (sl >> bs) | (sh2 << (32 - bs)) : sl;
    }
    Fr dk = gsub(g_from_int(xs), g_from_int(ss));
    if (lane == 0) st_var(vars, var_id(a, 3, row0), zero);                          // d_0 = 0
    const Fr one_abi = g_one_abi();
#pragma unroll
    for (u32 j = 0; j < GADGET_RUN; ++j) {
      if (j < L) {
        const u32 k = k0 + j;
        const bool valid = k < R;
        const Fr d2 = gadd(dk, dk);
        dk = g_sel(bit[j] == 0, d2, g_sel(bit[j] < 0, gsub(d2, one_abi), gadd(d2, one_abi)));
        if (valid) st_var(vars, var_id(a, 3, row0 + k + 1), dk);
      }
    }
  }

  // ---- first walk: the lane's total (lane 0 starts from the start point) and c_k
  EdPoint P = ed_sel(lane == 0, start, neutral);
#pragma unroll
  for (u32 j = 0; j < GADGET_RUN; ++j) {
    if (j < L) {
      const u32 k = k0 + j;
      const bool valid = k < R;
      Fr c;
      const Addend ad = fb_addend(a.tab, (size_t)rec.tab + (valid ? k : R - 1), bit[j], &c);
      if (valid) st_var(vars, var_id(a, 2, row0 + k), c);
      P = ed_madd(P, ad.x, ad.y, ad.t, d);
    }
  }
  // ---- inclusive scan of the lane totals
#pragma unroll 1
  for (u32 delta = 1; delta < used; delta <<= 1) {
    const EdPoint Q = ed_shfl_up(P, delta);
    const EdPoint S = ed_add(Q, P, d);
    P = ed_sel(lane >= delta, S, P);
  }
  // ---- second walk from the exclusive prefix; X, Y, Z of the run's points are kept for the shared inversion
  EdPoint Q = ed_shfl_up(P, 1);
  Q = ed_sel(lane == 0, start, Q);
  Fr PX[GADGET_RUN], PY[GADGET_RUN], PZ[GADGET_RUN], pre[GADGET_RUN];
  Fr prod = one;
#pragma unroll
  for (u32 j = 0; j < GADGET_RUN; ++j) {
    if (j < L) {
      const u32 k = k0 + j;
      const Addend ad = fb_addend(a.tab, (size_t)rec.tab + (k < R ? k : R - 1), bit[j], nullptr);
      Q = ed_madd(Q, ad.x, ad.y, ad.t, d);
      PX[j] = Q.X, PY[j] = Q.Y, PZ[j] = Q.Z;
      pre[j] = prod;
      prod = gmul(prod, Q.Z);
    }
  }
  Fr inv = fe_inv_dev<FrP>(prod);      // the lane's one inversion; all 64 lanes are here
#pragma unroll
  for (int j = GADGET_RUN - 1; j >= 0; --j) {
    if ((u32)j < L) {
      const u32 k = k0 + j;
      const Fr zi = g_to_abi(gmul(inv, pre[j]));          // 1 / Z_j, ABI form: device x ABI -> ABI below
      inv = gmul(inv, PZ[j]);
      if (k < R) {
        st_var(vars, var_id(a, 0, row0 + k + 1), gmul(PX[j], zi));
        st_var(vars, var_id(a, 1, row0 + k + 1), gmul(PY[j], zi));
      }
    }
  }
}

// ------------------------------------------------------------------ variable-base scalar multiplication
// One wave per (gadget, proof): blockIdx.x = the gadget within the launch, blockIdx.y = the proof.  Round k of the chain is
// dbl = acc + acc (the unified law: start and P may lie off the curve, so no formula that uses the curve equation) and
// new = dbl + (bit_k P.x, bit_k P.y - bit_k + 1), which for a bit of 0 is dbl itself.  The chain is R rounds deep whatever is
// done, so ALL 64 lanes walk ALL of it, in step: the loop, the bit of a round and the branch on it are wave-uniform.  What the
// lanes share out is the rest: lane l owns rounds l L .. (l + 1) L - 1, L = ceil(R / 64).  It reads the bits of its rounds
// (a ballot per slot turns them into wave-uniform masks), writes their select rows, keeps X, Y, Z of dbl and new when the
// chain passes through them, inverts the product of those <= 2 L values of Z once (all 64 lanes reach fe_inv_dev, which votes
// across the wave) and writes its rounds.  A lane without a round keeps Z = 1.  Some Z of the chain is zero exactly when a
// denominator of the affine law vanishes in that round, and the lane that owns the round sees it in its product.
__global__ void __launch_bounds__(64) gadget_var_base_kernel(const GadgetFill a, u32 first, u32) {
  const u32 lane = threadIdx.x, proof = blockIdx.y;
  const GadgetRec rec = a.recs[first + blockIdx.x];
  u32x4* const vars = a.vars + 2 * a.var_stride * proof;
  const u32 R = rec.count, L = (R + 63) >> 6, k0 = lane * L;
  const size_t row0 = rec.first_row;
  const Fr d = fr_limbs(a.edwards_d), one = fe_one<FrP>(), zero = fe_zero<FrP>(), one_abi = g_one_abi();

  // ---- the start point and P, every lane reads the same words
  const Fr sx_abi = ld_var(vars, var_id(a, 0, row0)), sy_abi = ld_var(vars, var_id(a, 1, row0));
  const Fr px_abi = ld_var(vars, var_id(a, 1, row0 + 2)), py_abi = ld_var(vars, var_id(a, 1, row0 + 3));
  const Fr px = g_to_dev(px_abi), py = g_to_dev(py_abi), pt = gmul(px, py);

  // ---- this lane's bits and select rows: exact for any value of the bit variable
  unsigned long long ones[GADGET_RUN];   // bit l of ones[j]: the bit of round l L + j is 1
  u32 mine = 0;
  bool wide = false;
#pragma unroll
  for (u32 j = 0; j < GADGET_RUN; ++j) {
    const u32 k = k0 + j;
    const bool valid = j < L && k < R;
    const size_t row = row0 + 6 * (size_t)(valid ? k : 0);
    const Fr bit = ld_var(vars, var_id(a, 0, row + 2)), bit_dev = g_to_dev(bit);
    const bool is_one = g_is_zero(gsub(bit, one_abi));
    wide |= valid && !is_one && !g_is_zero(bit);
    if (valid) {
      st_var(vars, var_id(a, 2, row + 2), gmul(bit_dev, px_abi));
      st_var(vars, var_id(a, 2, row + 3), gadd(gsub(gmul(bit_dev, py_abi), bit), one_abi));
    }
    ones[j] = __ballot(valid && is_one);
    mine |= valid && is_one ? 1u << j : 0u;
  }

  // ---- the chain
  const Fr sx = g_to_dev(sx_abi), sy = g_to_dev(sy_abi);
  EdPoint Q{sx, sy, one, gmul(sx, sy)};
  Fr DX[GADGET_RUN], DY[GADGET_RUN], DZ[GADGET_RUN], NX[GADGET_RUN], NY[GADGET_RUN], NZ[GADGET_RUN];
#pragma unroll
  for (u32 j = 0; j < GADGET_RUN; ++j) DX[j] = NX[j] = zero, DY[j] = NY[j] = DZ[j] = NZ[j] = one;
  u32 owner = 0, slot = 0;           // round k = owner L + slot
#pragma unroll 1
  for (u32 k = 0; k < R; ++k) {
    const unsigned long long m = slot == 0 ? ones[0] : slot == 1 ? ones[1] : slot == 2 ? ones[2] : ones[3];
    const EdPoint D = ed_add(Q, Q, d);
    Q = D;
    if ((m >> owner) & 1ull) Q = ed_madd(D, px, py, pt, d);
#pragma unroll
    for (u32 j = 0; j < GADGET_RUN; ++j) {
      const bool keep = owner == lane && slot == j;
      DX[j] = g_sel(keep, D.X, DX[j]), DY[j] = g_sel(keep, D.Y, DY[j]), DZ[j] = g_sel(keep, D.Z, DZ[j]);
      NX[j] = g_sel(keep, Q.X, NX[j]), NY[j] = g_sel(keep, Q.Y, NY[j]), NZ[j] = g_sel(keep, Q.Z, NZ[j]);
    }
    if (++slot == L) slot = 0, ++owner;
  }

  // ---- one inversion for the lane's <= 2 L points (Montgomery's trick), then its rows
  Fr pre[2 * GADGET_RUN];
  Fr prod = one;
#pragma unroll
  for (u32 j = 0; j < GADGET_RUN; ++j) {
    if (j < L) {
      pre[2 * j] = prod;
      prod = gmul(prod, DZ[j]);
      pre[2 * j + 1] = prod;
      prod = gmul(prod, NZ[j]);
    }
  }
  const bool any_wide = __any(wide), any_zero = __any(g_is_zero(prod));
  if (lane == 0 && (any_wide || any_zero))   // one report a gadget; a wide bit comes first
    gadget_fail(a, proof, rec.index, any_wide ? PM_PLONK_GADGET_TOO_WIDE : PM_PLONK_GADGET_DEGENERATE);
  Fr inv = fe_inv_dev<FrP>(prod);    // 0 -> 0: the lane that owns a degenerate round writes zeros; all 64 lanes are here
  if (lane == 0) st_var(vars, var_id(a, 3, row0 + 1), gmul(sx, sy_abi));
#pragma unroll
  for (int j = GADGET_RUN - 1; j >= 0; --j) {
    if ((u32)j < L) {
      const u32 k = k0 + j;
      const Fr zn = g_to_abi(gmul(inv, pre[2 * j + 1]));   // 1 / Z, ABI form: device x ABI -> ABI below
      inv = gmul(inv, NZ[j]);
      const Fr zd = g_to_abi(gmul(inv, pre[2 * j]));
      inv = gmul(inv, DZ[j]);
      if (k < R) {
        const size_t row = row0 + 6 * (size_t)k;
        const Fr dx = gmul(DX[j], zd), dy = gmul(DY[j], zd), nx = gmul(NX[j], zn), ny = gmul(NY[j], zn);
        st_var(vars, var_id(a, 0, row + 1), dx);
        st_var(vars, var_id(a, 1, row + 1), dy);
        st_var(vars, var_id(a, 0, row + 5), nx);
        st_var(vars, var_id(a, 1, row + 5), ny);
        // dbl.x sy with sy = P.y or 1; new.x new.y belongs to the next round's doubling
        st_var(vars, var_id(a, 3, row + 5), g_sel((mine >> j) & 1u, gmul(g_to_dev(dx), py_abi), dx));
        if (k + 1 < R) st_var(vars, var_id(a, 3, row + 7), gmul(g_to_dev(nx), ny));
      }
    }
  }
}

// a kind's fill kernel: (arguments, first record of the launch, records); the kind table has the launch shape
void (*const FILL_KERNELS[GADGET_KINDS])(GadgetFill, u32, u32) = {
    gadget_range_kernel,       gadget_logic_kernel, gadget_fixed_base_kernel, gadget_curve_add_kernel, gadget_arith_kernel, gadget_bits_kernel,
    gadget_maybe_equal_kernel, gadget_hades_kernel, nullptr /* 8 */,          nullptr /* 9 */,         gadget_var_base_kernel};
}  // namespace

int gadget_verify(pm_ctx* ctx, const GadgetTables& t, size_t n, const void* d_sel, bool all11, const void* d_wire_vars, hipStream_t st) {
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (!st) st = ctx->stream;
  PM_HIP(ctx, hipSetDevice(ctx->device));
  u32* const d_bad = (u32*)t.rep;
  PM_HIP(ctx, hipMemsetAsync(d_bad, 0xff, 4, st));
  if (t.hades_rounds) PM_HIP(ctx, hipMemsetAsync(t.hids, 0xff, t.hades_rounds * GADGET_ROUND_ID_BYTES, st));   // PM_PLONK_NO_VAR where no row writes
  hipLaunchKernelGGL(gadget_verify_kernel, dim3(t.count), dim3(256), 0, st, (const GadgetRec*)t.recs, (const u32x4*)d_sel, n,
                     all11 ? 1u : 0u, all11 ? 7u : 2u, (u32x4*)t.tab, d_bad);
  if (all11)
    hipLaunchKernelGGL(composed_verify_kernel, dim3(t.count), dim3(256), 0, st, (const GadgetRec*)t.recs, (const u32x4*)d_sel, n,
                       (const u32*)d_wire_vars, (u32x4*)t.coef, (u32x4*)t.hcoef, (u32*)t.hids, d_bad);
  PM_HIP(ctx, hipGetLastError());
  return PM_OK;
}

int gadget_fill(pm_ctx* ctx, const GadgetTables& t, const std::vector<GadgetGroup>& groups, const void* d_wire_vars, size_t n,
                void* d_vars, size_t var_stride, uint32_t batch, unsigned long long* rep_host, hipStream_t st) {
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (!st) st = ctx->stream;
  PM_HIP(ctx, hipSetDevice(ctx->device));
  GadgetFill a{.recs = (const GadgetRec*)t.recs, .wire_vars = (const u32*)d_wire_vars, .tab = (const u32x4*)t.tab, .coef = (const u32x4*)t.coef,
               .hcoef = (const u32x4*)t.hcoef, .hids = (const u32*)t.hids, .vars = (u32x4*)d_vars, .var_stride = var_stride, .n = n,
               .rep = (unsigned long long*)t.rep, .edwards_d = {}};
  jubjub_d_limbs(a.edwards_d);
  PM_HIP(ctx, hipMemsetAsync(t.rep, 0, (size_t)batch * 8, st));
  PM_HIP(ctx, hipMemsetAsync((char*)t.rep + (size_t)batch * 8, 0xff, (size_t)batch * 8, st));
  {
    ProfScope prof(ctx, st, "plonk_gadget_fill");
    for (const GadgetGroup& g : groups) {
      const auto kernel = FILL_KERNELS[g.kind];   // a group's kind is one set time knew
      const GadgetLaunch shape = gadget_kind(g.kind).launch;
      if (shape == GadgetLaunch::NONE) return set_err(ctx, PM_ERR_BAD_ARG, "a gadget group of no kind");
      // a thread or a wave per gadget: the gadgets along x, one launch (at most 2^31 - 1).  BITS_X: along y, at most 65535 a launch
      const u32 most = shape == GadgetLaunch::BITS_X ? 65535u : g.count;
      for (u32 lo = 0; lo < g.count; lo += most) {
        const u32 part = std::min(g.count - lo, most);
        const dim3 grid = shape == GadgetLaunch::BITS_X ? dim3((g.span + 63) / 64, part, batch)
                                                        : dim3(shape == GadgetLaunch::PER_WAVE ? part : (part + 63) / 64, batch);
        hipLaunchKernelGGL(kernel, grid, dim3(64), 0, st, a, g.first + lo, part);
      }
    }
  }
  PM_HIP(ctx, hipGetLastError());
  if (rep_host) {
    PM_HIP(ctx, hipMemcpyAsync(rep_host, t.rep, (size_t)batch * 16, hipMemcpyDeviceToHost, st));
    PM_HIP(ctx, hipStreamSynchronize(st));
  }
  return PM_OK;
}

}  // namespace pm

using namespace pm;

extern "C" int pm_test_host_naf(const uint64_t s[4], uint32_t rounds, int8_t* digits_msb_first, int* too_long) {
  if (!s || !digits_msb_first || rounds == 0 || rounds > PM_PLONK_GADGET_MAX_ROUNDS) return PM_ERR_BAD_ARG;
  u32 s8[8], s9[9], x9[9];
  for (int i = 0; i < 4; ++i) {
    s8[2 * i] = (u32)s[i];
    s8[2 * i + 1] = (u32)(s[i] >> 32);
  }
  naf_operands(s8, s9, x9);
  for (u32 k = 0; k < rounds; ++k) digits_msb_first[k] = (int8_t)naf_digit(x9, s9, rounds - 1 - k);
  if (too_long) *too_long = naf_too_long(x9, s9, rounds) ? 1 : 0;
  return PM_OK;
}
