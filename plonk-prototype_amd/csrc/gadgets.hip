// Gadget witnesses: the inverse of the witness check.  Given the inputs of a range, logic, fixed-base
// or curve-addition gadget, write the variables that make its rows hold (definitions: include/plonk_mi355x.h, pm_plonk_gadget).
// Section 7.2g adds the gadgets a circuit composes from arithmetic rows: runs of them, bit decompositions and maybe_equal;
// section 7.2h the rows of a whole Hades permutation; section 7.2i those of a variable-base scalar multiplication.
//
//   gadget_verify_kernel       set time: every claimed row has its kind's selector, the table points of the fixed-base rounds
//                              are gathered from q_l / q_r into a compact array
//   composed_verify_kernel     set time, composed kinds: arithmetic rows without a widget, the coefficients and wire ids a BITS,
//                              MAYBE_EQUAL or HADES layout implies; gathers q_m q_l q_r q_4 q_c of the ARITH rows and, round by
//                              round, the round keys, matrix entries and c ids of the HADES rows; VAR_BASE: the selectors,
//                              select-row coefficients and wire ids of its six rows a round
//   gadget_arith_kernel        one thread per (gadget, proof): c = q_m a b + q_l a + q_r b + q_4 d + q_c, row after row
//   gadget_bits_kernel         one thread per (gadget, proof, bit): acc_k = acc_(-1) + (V mod 2^(k+1)) is a masked copy of V, so
//                              no bit waits for another
//   gadget_maybe_equal_kernel  one thread per (gadget, proof): u = a - b, z = 1 / u (0 -> 0), y = [u = 0]
//   gadget_hades_kernel        one WAVE per (gadget, proof): lane 5 i + j < 25 holds state word j and matrix entry (i, j); a round
//                              is four dependent products (x^2, x^4, x^5, M x) and the row sums go across lanes
//   gadget_range_kernel        one thread per (gadget, proof): quads of the canonical input, accumulators by 4 acc + quad
//   gadget_logic_kernel        the same over two inputs, three accumulator columns and the quad products
//   gadget_curve_add_kernel    one thread per (gadget, proof): the affine law with ONE inversion (of the two denominators' product)
//   gadget_fixed_base_kernel   one WAVE per (gadget, proof), the hot path:
//        every lane derives the width-2 NAF digits of its rounds from s and 3 s (e_j = bit_(j+1)(3s) - bit_(j+1)(s): no carry
//        travels between lanes), owns a contiguous run of ceil(R / 64) rounds and sums its addends in extended coordinates;
//        the lane totals go through an inclusive prefix scan with __shfl_up under the complete twisted Edwards law; each lane
//        then walks its run again from the scanned start and normalises its <= 4 prefixes with one inversion (Montgomery's
//        trick).  No lane ever runs more than one inversion and there is no chain of dependent per-round inversions.
//        The addends are re-derived from the table in both walks rather than kept across the scan: what stays live over the
//        scan is one point, and over the second walk the run's X, Y, Z (the variant kept: see DESIGN.md for the registers).
//   gadget_var_base_kernel     one WAVE per (gadget, proof): every lane walks the same double-and-add chain in extended
//        coordinates (a wave instruction costs the same for 64 lanes as for one), lane l keeps the points of rounds
//        l L .. (l + 1) L - 1, L = ceil(R / 64), and normalises them with its one inversion.  No per-round inversion.
//
// Forms: variables are canonical Montgomery ("ABI", x 2^256); the point arithmetic runs in the device form x 2^261
// (poly_common.hip.h).  Everything written goes through fe_store, i.e. is canonical.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "context.h"
#include "field_inv.hip.h"
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
  unsigned long long* rep;  // [batch] failing gadgets, then [batch] min(index * 4 + reason); batch = gridDim.y
  u32 edwards_d[9];         // device form
};

PM_DEV void gadget_fail(const GadgetFill& a, u32 proof, u32 index, u32 reason) {
  atomicAdd(a.rep + proof, 1ull);                                              // a count and a minimum: order-free
  atomicMin(a.rep + gridDim.y + proof, (unsigned long long)index * 4 + reason);
}
PM_DEV u32 var_id(const GadgetFill& a, u32 wire, size_t row) { return a.wire_vars[(size_t)wire * a.n + row]; }
PM_DEV Fr ld_var(const u32x4* vars, u32 id) { return id == PM_PLONK_NO_VAR ? fe_zero<FrP>() : ld_canon(vars, id); }
PM_DEV void st_var(u32x4* vars, u32 id, const Fr& v) {
  if (id != PM_PLONK_NO_VAR) st_canon(vars, id, v);
}

// ------------------------------------------------------------------ field helpers (operands normalised, values < 2 r)
PM_DEV Fr gadd(const Fr& a, const Fr& b) { return fe_reduce_weak<FrP>(fe_add<FrP>(a, b)); }
PM_DEV Fr gsub(const Fr& a, const Fr& b) { return fe_reduce_weak<FrP>(fe_sub<FrP, 2, 1>(a, b)); }
PM_DEV Fr gmul(const Fr& a, const Fr& b) { return fe_mul<FrP>(a, b); }
PM_DEV Fr gneg(const Fr& a) { return gsub(fe_zero<FrP>(), a); }
PM_DEV Fr g_to_dev(const Fr& abi) { return fe_reduce_weak<FrP>(fr_shl5(abi)); }
PM_DEV Fr g_to_abi(const Fr& dev) { return fe_mul<FrP>(dev, fe_pow2<FrP, 256>()); }          // x 2^261 * 2^256 / 2^261
PM_DEV Fr g_one_abi() { return fe_pow2<FrP, 256>(); }
PM_DEV Fr g_sel(bool c, const Fr& a, const Fr& b) {
  Fr r;
#pragma unroll
  for (int i = 0; i < 9; ++i) r.l[i] = c ? a.l[i] : b.l[i];
  return r;
}
PM_DEV bool g_is_zero(const Fr& v) {   // a zero may arrive as r: test the canonical words
  u32 s[8];
  fe_canon_pack<FrP>(s, v);
  return (s[0] | s[1] | s[2] | s[3] | s[4] | s[5] | s[6] | s[7]) == 0;
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
// sel: vectors of n values on H; q_l, q_r are vectors ql, ql + 1 and the four widget selectors wid .. wid + 3 (0 and 2 of
// q_l q_r q_range q_logic q_fixed_group_add q_variable_group_add; 1 and 7 of all eleven)
__global__ void __launch_bounds__(256) gadget_verify_kernel(const GadgetRec* recs, const u32x4* sel_all, size_t n, u32 ql, u32 wid,
                                                            u32x4* tab, u32* bad) {
  const GadgetRec rec = recs[blockIdx.x];
  if (rec.kind > PM_PLONK_GADGET_CURVE_ADD) return;   // composed_verify_kernel
  const u32 rows = rec.kind == PM_PLONK_GADGET_CURVE_ADD ? 1u : rec.count;
  const u32x4* sel = sel_all + 2 * n * ql;
  const u32x4* q = sel_all + 2 * n * (wid + (size_t)rec.kind);
  bool miss = false;
  for (u32 t = threadIdx.x; t < rows; t += 256) {
    const size_t row = (size_t)rec.first_row + t;
    const u32x4 lo = q[2 * row], hi = q[2 * row + 1];
    miss |= (lo.x | lo.y | lo.z | lo.w | hi.x | hi.y | hi.z | hi.w) == 0;
    if (rec.kind == PM_PLONK_GADGET_FIXED_BASE) {
      u32x4* o = tab + 4 * ((size_t)rec.tab + t);
      o[0] = sel[2 * row];
      o[1] = sel[2 * row + 1];
      o[2] = sel[2 * (n + row)];
      o[3] = sel[2 * (n + row) + 1];
    }
  }
  if (miss) atomicMin(bad, rec.index);
}

// The composed kinds (include/plonk_mi355x.h): what a row's six coefficients must be.  sel: all eleven selectors on H in the
// order of PM_PLONK_SELECTORS -- q_m q_l q_r q_o q_c q_4 q_arith, then the four widget selectors.
enum : u32 { CO_ZERO, CO_ONE, CO_NEG, CO_POW, CO_ANY };
PM_DEV void sel_words(const u32x4* sel, size_t n, u32 s, size_t row, u32 (&w)[8]) {
  const u32x4 lo = sel[2 * (n * s + row)], hi = sel[2 * (n * s + row) + 1];
  w[0] = lo.x, w[1] = lo.y, w[2] = lo.z, w[3] = lo.w, w[4] = hi.x, w[5] = hi.y, w[6] = hi.z, w[7] = hi.w;
}
__global__ void __launch_bounds__(256) composed_verify_kernel(const GadgetRec* recs, const u32x4* sel, size_t n, const u32* wire_vars,
                                                              u32x4* coef, u32x4* hcoef, u32* hids, u32* bad) {
  const GadgetRec rec = recs[blockIdx.x];
  if (rec.kind < PM_PLONK_COMPOSED_ARITH) return;
  const bool arith = rec.kind == PM_PLONK_COMPOSED_ARITH, bits = rec.kind == PM_PLONK_COMPOSED_BITS;
  const bool hades = rec.kind == PM_PLONK_PERMUTATION_HADES, vbase = rec.kind == PM_PLONK_GADGET_VAR_BASE;
  // HADES: H full rounds, rec.count - 2 H partial ones, H full ones; 30 rows a full round and 18 a partial one
  const u32 H = rec.param >> 1, rows_head = 30 * H, rows_mid = 18 * (rec.count - 2 * H);
  const u32 rows = arith ? rec.count : bits ? 2 * rec.count : hades ? 2 * rows_head + rows_mid : vbase ? 6 * rec.count : 3u;
  u32 one[8], neg[8];
  fe_canon_pack<FrP>(one, g_one_abi());
  fe_canon_pack<FrP>(neg, gneg(g_one_abi()));
  bool miss = false;
  for (u32 t = threadIdx.x; t < rows; t += 256) {
    const size_t row = (size_t)rec.first_row + t;
    u32 w[8];
    // an arithmetic row and nothing else; VAR_BASE: that on its select rows (2, 3 of six), q_variable_group_add on rows 0
    // and 4, and rows 1 and 5 carry results only: their selectors are not looked at
    const u32 pos = vbase ? t % 6 : 2u;
    sel_words(sel, n, 6, row, w);
    const bool no_arith = (w[0] | w[1] | w[2] | w[3] | w[4] | w[5] | w[6] | w[7]) == 0;
    u32 widget = 0, last = 0;
#pragma unroll
    for (u32 s = 7; s < 11; ++s) {
      sel_words(sel, n, s, row, w);
      last = w[0] | w[1] | w[2] | w[3] | w[4] | w[5] | w[6] | w[7];
      widget |= last;
    }
    if (pos == 2 || pos == 3) miss |= no_arith || widget != 0;
    else if (pos == 0 || pos == 4) miss |= last == 0;
    // q_m q_l q_r q_o q_c q_4
    u32 want[6] = {CO_ANY, CO_ANY, CO_ANY, CO_NEG, CO_ANY, CO_ANY};
    u32 pw[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const u32 va = wire_vars[row], vb = wire_vars[n + row], vc = wire_vars[2 * n + row];
    u32 slot[6] = {~0u, ~0u, ~0u, ~0u, ~0u, ~0u};   // HADES: where a selector's value goes in the round's 30 coefficients
    size_t round = 0;
    if (arith) {
      miss |= vc == PM_PLONK_NO_VAR;
    } else if (vbase) {
      const u32 vd = wire_vars[3 * n + row];
      const size_t r0 = rec.first_row, rb = row - pos;   // the gadget's and the round's first row
      const u32* const aw = wire_vars;
      const u32* const bw = wire_vars + n;
      const u32* const cw = wire_vars + 2 * n;
      want[3] = CO_ANY;
      if (pos == 0) {          // acc + acc; acc is what the round before wrote
        miss |= vc != va || vd != vb;
        if (rb != r0) miss |= va != aw[rb - 1] || vb != bw[rb - 1];
      } else if (pos == 1 || pos == 5) {   // a result row: x, y and the product are written
        miss |= va == PM_PLONK_NO_VAR || vb == PM_PLONK_NO_VAR || vd == PM_PLONK_NO_VAR;
      } else if (pos == 2) {   // sx = bit P.x
        want[0] = CO_ONE, want[3] = CO_NEG, want[1] = want[2] = want[4] = want[5] = CO_ZERO;
        miss |= vc == PM_PLONK_NO_VAR || vb != bw[r0 + 2];
      } else if (pos == 3) {   // sy = bit P.y - bit + 1
        want[0] = CO_ONE, want[1] = CO_NEG, want[3] = CO_NEG, want[4] = CO_ONE, want[2] = want[5] = CO_ZERO;
        miss |= vc == PM_PLONK_NO_VAR || va != aw[row - 1] || vb != bw[r0 + 3];
      } else {                 // dbl + (sx, sy)
        miss |= va != aw[rb + 1] || vb != bw[rb + 1] || vc != cw[rb + 2] || vd != cw[rb + 3];
      }
    } else if (hades) {
      // the round, whether it is full, and the row's place in it
      u32 rho, pos;
      bool full = true;
      if (t < rows_head) {
        rho = t / 30, pos = t % 30;
      } else if (t < rows_head + rows_mid) {
        rho = H + (t - rows_head) / 18, pos = (t - rows_head) % 18, full = false;
      } else {
        rho = rec.count - H + (t - rows_head - rows_mid) / 30, pos = (t - rows_head - rows_mid) % 30;
      }
      round = (size_t)rec.tab + rho;
      const size_t rb = row - pos;                   // the round's first row
      const u32* const cw = wire_vars + 2 * n;       // the c ids
      const u32 sbox_rows = full ? 15u : 3u;
      want[0] = want[1] = want[2] = want[4] = want[5] = CO_ZERO;
      miss |= vc == PM_PLONK_NO_VAR;
      u32 id_slot;
      if (pos < 5) {                                 // s'[j] = s[j] + q_c; s[j] is o_j of the round before
        want[1] = CO_ONE, want[4] = CO_ANY;
        slot[4] = 25 + pos;
        if (rho) miss |= va != cw[rb - 10 + 2 * pos + 1];
        id_slot = pos;
      } else if (pos < 5 + sbox_rows) {              // x2 = x x, x4 = x2 x2, x5 = x4 x
        const u32 u = pos - 5, j = full ? u / 3 : 4u, k = u % 3;
        const u32 x = cw[rb + j];
        want[0] = CO_ONE;
        miss |= va != (k ? cw[row - 1] : x) || vb != (k == 1 ? cw[row - 1] : x);
        id_slot = 5 * (k + 1) + j;
      } else {                                       // z_i = M_i0 v0 + M_i1 v1 + M_i2 v2, o_i = M_i3 v3 + M_i4 v4 + z_i
        const u32 u = pos - 5 - sbox_rows, i = u >> 1, k = u & 1u;
        u32 v[3];
#pragma unroll
        for (u32 e = 0; e < 3; ++e) {
          const u32 j = 3 * k + e;                   // j = 5 (k = 1, e = 2) is z_i
          v[e] = j == 5 ? cw[row - 1] : full ? cw[rb + 5 + 3 * j + 2] : j == 4 ? cw[rb + 7] : cw[rb + j];
        }
        want[1] = want[2] = CO_ANY, want[5] = k ? CO_ONE : CO_ANY;
        slot[1] = 5 * i + 3 * k, slot[2] = 5 * i + 3 * k + 1;
        if (!k) slot[5] = 5 * i + 2;
        miss |= va != v[0] || vb != v[1] || wire_vars[3 * n + row] != v[2];
        id_slot = 20 + u;
      }
      hids[30 * round + id_slot] = vc;
    } else if (bits) {
      const u32 k = t >> 1;
      if ((t & 1u) == 0) {   // the boolean row: bit * bit - bit
        want[0] = CO_ONE, want[1] = want[2] = want[4] = want[5] = CO_ZERO;
        miss |= va == PM_PLONK_NO_VAR || vb != va || vc != va;
      } else {               // 2^k bit + acc_(k-1) - acc_k
        want[0] = want[4] = want[5] = CO_ZERO, want[1] = CO_POW, want[2] = CO_ONE;
        u32 e[8];
#pragma unroll
        for (u32 i = 0; i < 8; ++i) e[i] = i == (k >> 5) ? 1u << (k & 31u) : 0u;
        fe_canon_pack<FrP>(pw, g_from_int(e));
        miss |= vc == PM_PLONK_NO_VAR || va != wire_vars[row - 1];
        if (k) miss |= vb != wire_vars[2 * n + row - 2];
      }
    } else {
      const size_t r0 = rec.first_row;
      const u32 u = wire_vars[2 * n + r0], y = wire_vars[2 * n + r0 + 1];
      if (t == 0) {          // a - b - u
        want[0] = want[4] = want[5] = CO_ZERO, want[1] = CO_ONE, want[2] = CO_NEG;
        miss |= vc == PM_PLONK_NO_VAR;
      } else if (t == 1) {   // 1 - z u - y
        want[0] = CO_NEG, want[4] = CO_ONE, want[1] = want[2] = want[5] = CO_ZERO;
        miss |= va == PM_PLONK_NO_VAR || vc == PM_PLONK_NO_VAR || vb != u;
      } else {               // y u
        want[0] = CO_ONE, want[1] = want[2] = want[3] = want[4] = want[5] = CO_ZERO;
        miss |= va != y || vb != u;
      }
    }
#pragma unroll
    for (u32 s = 0; s < 6; ++s) {
      sel_words(sel, n, s, row, w);
      u32 diff = 0;
#pragma unroll
      for (u32 i = 0; i < 8; ++i) {
        const u32 x = want[s] == CO_ONE ? one[i] : want[s] == CO_NEG ? neg[i] : want[s] == CO_POW ? pw[i] : 0u;
        diff |= w[i] ^ x;
      }
      miss |= want[s] != CO_ANY && diff != 0;
      if (arith && s != 3) {   // q_m q_l q_r q_c q_4 -> slots 0 1 2 4 3
        u32x4* o = coef + 10 * ((size_t)rec.tab + t) + 2 * (s < 3 ? s : s == 4 ? 4u : 3u);
        o[0] = u32x4{w[0], w[1], w[2], w[3]};
        o[1] = u32x4{w[4], w[5], w[6], w[7]};
      }
      if (slot[s] != ~0u) {
        u32x4* o = hcoef + 2 * (30 * round + slot[s]);
        o[0] = u32x4{w[0], w[1], w[2], w[3]};
        o[1] = u32x4{w[4], w[5], w[6], w[7]};
      }
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
// One thread per (gadget, proof).  The inversion votes across the wave (field_inv.hip.h), so no lane leaves early: a lane
// past the end works on the last gadget and writes nothing.
__global__ void __launch_bounds__(64) gadget_curve_add_kernel(const GadgetFill a, u32 first, u32 count) {
  const u32 g0 = blockIdx.x * 64 + threadIdx.x, proof = blockIdx.y;
  const bool live = g0 < count;
  const GadgetRec rec = a.recs[first + (live ? g0 : count - 1)];
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
__global__ void __launch_bounds__(64) gadget_bits_kernel(const GadgetFill a, u32 first) {
  const u32 k = blockIdx.x * 64 + threadIdx.x, proof = blockIdx.z;
  const GadgetRec rec = a.recs[first + blockIdx.y];
  if (k >= rec.count) return;
  u32x4* const vars = a.vars + 2 * a.var_stride * proof;
  const size_t row0 = rec.first_row;
  u32 v[8], m[8];
  g_to_int(ld_canon(vars, rec.in_var[0]), v);
#pragma unroll
  for (u32 w = 0; w < 8; ++w) {   // the low k + 1 bits
    const u32 lo = 32 * w, keep = k + 1;
    m[w] = v[w] & (lo + 32 <= keep ? 0xffffffffu : (lo >= keep ? 0u : ((1u << ((keep - lo) & 31u)) - 1u)));
  }
  const Fr acc = gadd(g_from_int(m), ld_var(vars, var_id(a, 1, row0 + 1)));
  st_var(vars, var_id(a, 0, row0 + 2 * (size_t)k), g_sel(bit_at<8>(v, k) != 0, g_one_abi(), fe_zero<FrP>()));
  st_var(vars, var_id(a, 2, row0 + 2 * (size_t)k + 1), acc);
}

// u = a - b, z = 1 / u or 0, y = 1 - u z = [u = 0].  One thread per (gadget, proof); the inversion votes across the wave, so
// (as in gadget_curve_add_kernel) a lane past the end works on the last gadget and writes nothing.
__global__ void __launch_bounds__(64) gadget_maybe_equal_kernel(const GadgetFill a, u32 first, u32 count) {
  const u32 g0 = blockIdx.x * 64 + threadIdx.x, proof = blockIdx.y;
  const bool live = g0 < count;
  const GadgetRec rec = a.recs[first + (live ? g0 : count - 1)];
  u32x4* const vars = a.vars + 2 * a.var_stride * proof;
  const size_t row = rec.first_row;
  const Fr u = gsub(ld_var(vars, var_id(a, 0, row)), ld_var(vars, var_id(a, 1, row)));
  const Fr inv = fe_inv_dev<FrP>(g_to_dev(u));         // 0 -> 0
  if (!live) return;
  st_var(vars, var_id(a, 2, row), u);
  st_var(vars, var_id(a, 0, row + 1), g_to_abi(inv));
  st_var(vars, var_id(a, 2, row + 1), g_sel(g_is_zero(u), g_one_abi(), fe_zero<FrP>()));
}

// ------------------------------------------------------------------ a Hades permutation of width 5
PM_DEV Fr fr_shfl(const Fr& v, u32 src) {
  Fr r;
#pragma unroll
  for (int i = 0; i < 9; ++i) r.l[i] = __shfl(v.l[i], (int)src);
  return r;
}
// One wave per (gadget, proof): blockIdx.x = the gadget within the launch, blockIdx.y = the proof.  Lane 5 i + j (i, j < 5) holds
// state word j and the matrix entry (i, j); lanes 25..63 leave at once and no cross-lane read names them: every source below is
// 5 i + e or 5 j with e < 5.  The loop and the kind of a round depend on the gadget only, so the 25 lanes stay together; which of
// x and x^5 a lane keeps is a select.  Every lane of row group i ends a round with z_i and o_i, every lane of column j with
// x, x^2, x^4, x^5 of word j, so the stores are spread: lane (k, j), k < 4, writes the k-th of the latter four, lanes (i, 0) and
// (i, 1) write z_i and o_i -- two stores a round and lane, their ids gathered at set time in exactly that order (NO_VAR where a
// partial round has no such row).  The next round's two coefficients and two ids are loaded before this round's arithmetic.
// Forms as in gadget_arith_kernel: the state is in the ABI form, one operand of each product goes through g_to_dev.
__global__ void __launch_bounds__(64) gadget_hades_kernel(const GadgetFill a, u32 first) {
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

// extended coordinates: x = X / Z, y = Y / Z, T = X Y / Z
struct EdPoint {
  Fr X, Y, Z, T;
};
// unified addition for a = -1 (Hisil, Wong, Carter, Dawson 2008): the projective form of the affine law above, with the same
// exceptional cases -- none on the curve.  9 products.
PM_DEV EdPoint ed_add(const EdPoint& p, const EdPoint& q, const Fr& d) {
  const Fr A = gmul(p.X, q.X), B = gmul(p.Y, q.Y), C = gmul(gmul(p.T, q.T), d), D = gmul(p.Z, q.Z);
  const Fr E = gsub(gsub(gmul(gadd(p.X, p.Y), gadd(q.X, q.Y)), A), B);
  const Fr F = gsub(D, C), G = gadd(D, C), H = gadd(B, A);
  return EdPoint{gmul(E, F), gmul(G, H), gmul(F, G), gmul(E, H)};
}
// the same with an affine second operand (x, y, t = x y): 8 products
PM_DEV EdPoint ed_madd(const EdPoint& p, const Fr& x, const Fr& y, const Fr& t, const Fr& d) {
  const Fr A = gmul(p.X, x), B = gmul(p.Y, y), C = gmul(gmul(p.T, t), d);
  const Fr E = gsub(gsub(gmul(gadd(p.X, p.Y), gadd(x, y)), A), B);
  const Fr F = gsub(p.Z, C), G = gadd(p.Z, C), H = gadd(B, A);
  return EdPoint{gmul(E, F), gmul(G, H), gmul(F, G), gmul(E, H)};
}
PM_DEV Fr fr_shfl_up(const Fr& v, u32 delta) {
  Fr r;
#pragma unroll
  for (int i = 0; i < 9; ++i) r.l[i] = __shfl_up(v.l[i], delta);
  return r;
}
PM_DEV EdPoint ed_shfl_up(const EdPoint& p, u32 delta) {
  return EdPoint{fr_shfl_up(p.X, delta), fr_shfl_up(p.Y, delta), fr_shfl_up(p.Z, delta), fr_shfl_up(p.T, delta)};
}
PM_DEV EdPoint ed_sel(bool c, const EdPoint& a, const EdPoint& b) {
  return EdPoint{g_sel(c, a.X, b.X), g_sel(c, a.Y, b.Y), g_sel(c, a.Z, b.Z), g_sel(c, a.T, b.T)};
}

constexpr u32 FB_RUN = PM_PLONK_GADGET_MAX_ROUNDS / 64;   // rounds a lane owns at most

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
__global__ void __launch_bounds__(64) gadget_fixed_base_kernel(const GadgetFill a, u32 first) {
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
  int bit[FB_RUN];
#pragma unroll
  for (u32 j = 0; j < FB_RUN; ++j) {
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
    for (u32 w = 0; w < 9; ++w) {   // the low R + 1 bits
      const u32 lo = 32 * w, keep = R + 1;
      const u32 m = lo + 32 <= keep ? 0xffffffffu : (lo >= keep ? 0u : ((1u << ((keep - lo) & 31u)) - 1u));
      xm[w] = x9[w] & m;
      sm[w] = s9[w] & m;
    }
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
    for (u32 j = 0; j < FB_RUN; ++j) {
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
  for (u32 j = 0; j < FB_RUN; ++j) {
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
  Fr PX[FB_RUN], PY[FB_RUN], PZ[FB_RUN], pre[FB_RUN];
  Fr prod = one;
#pragma unroll
  for (u32 j = 0; j < FB_RUN; ++j) {
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
  for (int j = FB_RUN - 1; j >= 0; --j) {
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
constexpr u32 VB_RUN = PM_PLONK_GADGET_MAX_ROUNDS / 64;   // rounds a lane owns at most
// One wave per (gadget, proof): blockIdx.x = the gadget within the launch, blockIdx.y = the proof.  Round k of the chain is
// dbl = acc + acc (the unified law: start and P may lie off the curve, so no formula that uses the curve equation) and
// new = dbl + (bit_k P.x, bit_k P.y - bit_k + 1), which for a bit of 0 is dbl itself.  The chain is R rounds deep whatever is
// done, so ALL 64 lanes walk ALL of it, in step: the loop, the bit of a round and the branch on it are wave-uniform.  What the
// lanes share out is the rest: lane l owns rounds l L .. (l + 1) L - 1, L = ceil(R / 64).  It reads the bits of its rounds
// (a ballot per slot turns them into wave-uniform masks), writes their select rows, keeps X, Y, Z of dbl and new when the
// chain passes through them, inverts the product of those <= 2 L values of Z once (all 64 lanes reach fe_inv_dev, which votes
// across the wave) and writes its rounds.  A lane without a round keeps Z = 1.  Some Z of the chain is zero exactly when a
// denominator of the affine law vanishes in that round, and the lane that owns the round sees it in its product.
__global__ void __launch_bounds__(64) gadget_var_base_kernel(const GadgetFill a, u32 first) {
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
  unsigned long long ones[VB_RUN];   // bit l of ones[j]: the bit of round l L + j is 1
  u32 mine = 0;
  bool wide = false;
#pragma unroll
  for (u32 j = 0; j < VB_RUN; ++j) {
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
  Fr DX[VB_RUN], DY[VB_RUN], DZ[VB_RUN], NX[VB_RUN], NY[VB_RUN], NZ[VB_RUN];
#pragma unroll
  for (u32 j = 0; j < VB_RUN; ++j) DX[j] = NX[j] = zero, DY[j] = NY[j] = DZ[j] = NZ[j] = one;
  u32 owner = 0, slot = 0;           // round k = owner L + slot
#pragma unroll 1
  for (u32 k = 0; k < R; ++k) {
    const unsigned long long m = slot == 0 ? ones[0] : slot == 1 ? ones[1] : slot == 2 ? ones[2] : ones[3];
    const EdPoint D = ed_add(Q, Q, d);
    Q = D;
    if ((m >> owner) & 1ull) Q = ed_madd(D, px, py, pt, d);
#pragma unroll
    for (u32 j = 0; j < VB_RUN; ++j) {
      const bool keep = owner == lane && slot == j;
      DX[j] = g_sel(keep, D.X, DX[j]), DY[j] = g_sel(keep, D.Y, DY[j]), DZ[j] = g_sel(keep, D.Z, DZ[j]);
      NX[j] = g_sel(keep, Q.X, NX[j]), NY[j] = g_sel(keep, Q.Y, NY[j]), NZ[j] = g_sel(keep, Q.Z, NZ[j]);
    }
    if (++slot == L) slot = 0, ++owner;
  }

  // ---- one inversion for the lane's <= 2 L points (Montgomery's trick), then its rows
  Fr pre[2 * VB_RUN];
  Fr prod = one;
#pragma unroll
  for (u32 j = 0; j < VB_RUN; ++j) {
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
  for (int j = VB_RUN - 1; j >= 0; --j) {
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

}  // namespace

int gadget_verify(pm_ctx* ctx, const void* d_recs, uint32_t count, size_t n, const void* d_sel, bool all11, const void* d_wire_vars,
                  void* d_tab, void* d_coef, void* d_hcoef, void* d_hids, size_t hades_rounds, uint32_t* d_bad, hipStream_t st) {
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (!st) st = ctx->stream;
  PM_HIP(ctx, hipSetDevice(ctx->device));
  PM_HIP(ctx, hipMemsetAsync(d_bad, 0xff, 4, st));
  if (hades_rounds) PM_HIP(ctx, hipMemsetAsync(d_hids, 0xff, hades_rounds * 120, st));   // PM_PLONK_NO_VAR where no row writes
  hipLaunchKernelGGL(gadget_verify_kernel, dim3(count), dim3(256), 0, st, (const GadgetRec*)d_recs, (const u32x4*)d_sel, n,
                     all11 ? 1u : 0u, all11 ? 7u : 2u, (u32x4*)d_tab, d_bad);
  if (all11)
    hipLaunchKernelGGL(composed_verify_kernel, dim3(count), dim3(256), 0, st, (const GadgetRec*)d_recs, (const u32x4*)d_sel, n,
                       (const u32*)d_wire_vars, (u32x4*)d_coef, (u32x4*)d_hcoef, (u32*)d_hids, d_bad);
  PM_HIP(ctx, hipGetLastError());
  return PM_OK;
}

int gadget_fill(pm_ctx* ctx, const void* d_recs, const GadgetGroup* groups, size_t n_groups, const void* d_wire_vars, size_t n,
                const void* d_tab, const void* d_coef, const void* d_hcoef, const void* d_hids, void* d_vars, size_t var_stride,
                uint32_t batch, void* d_rep, unsigned long long* rep_host, hipStream_t st) {
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (!st) st = ctx->stream;
  PM_HIP(ctx, hipSetDevice(ctx->device));
  GadgetFill a;
  a.recs = (const GadgetRec*)d_recs;
  a.wire_vars = (const u32*)d_wire_vars;
  a.tab = (const u32x4*)d_tab;
  a.coef = (const u32x4*)d_coef;
  a.hcoef = (const u32x4*)d_hcoef;
  a.hids = (const u32*)d_hids;
  a.vars = (u32x4*)d_vars;
  a.var_stride = var_stride;
  a.n = n;
  a.rep = (unsigned long long*)d_rep;
  {
    const host::Field<4>& F = host::FR();   // JubJub d = -(10240 / 10241)
    const HFr q = host::mul(host::from_u64(10240, F), host::inv(host::from_u64(10241, F), F), F);
    to_limbs29_shift(a.edwards_d, host::sub(host::zero<4>(), q, F), 1);
  }
  PM_HIP(ctx, hipMemsetAsync(d_rep, 0, (size_t)batch * 8, st));
  PM_HIP(ctx, hipMemsetAsync((char*)d_rep + (size_t)batch * 8, 0xff, (size_t)batch * 8, st));
  {
    ProfScope prof(ctx, st, "plonk_gadget_fill");
    for (size_t i = 0; i < n_groups; ++i) {
      const GadgetGroup& g = groups[i];
      const dim3 per_thread((g.count + 63) / 64, batch), per_wave(g.count, batch);
      switch (g.kind) {
        case PM_PLONK_GADGET_RANGE:
          hipLaunchKernelGGL(gadget_range_kernel, per_thread, dim3(64), 0, st, a, g.first, g.count);
          break;
        case PM_PLONK_GADGET_LOGIC:
          hipLaunchKernelGGL(gadget_logic_kernel, per_thread, dim3(64), 0, st, a, g.first, g.count);
          break;
        case PM_PLONK_GADGET_FIXED_BASE:
          hipLaunchKernelGGL(gadget_fixed_base_kernel, per_wave, dim3(64), 0, st, a, g.first);
          break;
        case PM_PLONK_GADGET_CURVE_ADD:
          hipLaunchKernelGGL(gadget_curve_add_kernel, per_thread, dim3(64), 0, st, a, g.first, g.count);
          break;
        case PM_PLONK_COMPOSED_ARITH:
          hipLaunchKernelGGL(gadget_arith_kernel, per_thread, dim3(64), 0, st, a, g.first, g.count);
          break;
        case PM_PLONK_COMPOSED_BITS:   // the gadgets along y, at most 65535 a launch
          for (u32 lo = 0; lo < g.count; lo += 65535u)
            hipLaunchKernelGGL(gadget_bits_kernel, dim3((g.span + 63) / 64, std::min(g.count - lo, 65535u), batch), dim3(64), 0, st, a,
                               g.first + lo);
          break;
        case PM_PLONK_COMPOSED_MAYBE_EQUAL:
          hipLaunchKernelGGL(gadget_maybe_equal_kernel, per_thread, dim3(64), 0, st, a, g.first, g.count);
          break;
        case PM_PLONK_PERMUTATION_HADES:   // the gadgets along x, at most 2^31 - 1 a launch
          hipLaunchKernelGGL(gadget_hades_kernel, per_wave, dim3(64), 0, st, a, g.first);
          break;
        default:                       // PM_PLONK_GADGET_VAR_BASE
          hipLaunchKernelGGL(gadget_var_base_kernel, per_wave, dim3(64), 0, st, a, g.first);
          break;
      }
    }
  }
  PM_HIP(ctx, hipGetLastError());
  if (rep_host) {
    PM_HIP(ctx, hipMemcpyAsync(rep_host, d_rep, (size_t)batch * 16, hipMemcpyDeviceToHost, st));
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
