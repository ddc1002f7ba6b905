// Radix-4 variant of the Stockham pass kernel (see ntt_kernels.hip.h for the algorithm): every
// thread keeps FOUR elements (36 VGPRs of data instead of 72) and a wave owns 9 KiB of the LDS
// tile instead of 18, so four waves per SIMD fit where the radix-8 kernel is limited to two by
// LDS.  Same passes, same tables for the inter-pass twiddles, its own step-twiddle tables.
//
// Every in-tile product has a table constant as its second factor, and the table stores it split for
// fe_mul_split (fields.hip.h): a step twiddle as two rows (data limbs 0-4 and 5-8, six reduction digits, 129 limb
// products instead of 153), w4 as nine rows (one per data limb, two digits, 97).  The results are of fe_mul's class,
// so the bounds written at BFLY / dft4 hold unchanged.  Only the inter-pass twiddles (36 B per element from HBM)
// keep the plain form.  The <10, 1> passes go one step further, "lazy split products" below: their table products leave
// a digit out, return values up to 37 r in normalised limbs and let the butterflies' constants carry the difference.
#pragma once
#include "ntt_kernels.hip.h"

namespace pm {

__host__ __device__ constexpr int step4_radix_log(int S, int s) { return (S - 2 * s) >= 2 ? 2 : 1; }
__host__ __device__ constexpr int num_steps4(int S) { return (S + 1) / 2; }
// passes of radix-4 steps only, two at least, that read the plain form (first and single passes): their exchanges are
// plane-major (below), the others keep Stockham's slots
__host__ __device__ constexpr bool step4_plane_major(int S, bool in_wide) { return !in_wide && S >= 4 && S % 2 == 0; }
__host__ __device__ constexpr int step4_tw_offset(int S, int s) {
  int off = 0;
  for (int i = 0; i < s; ++i) off += ((1 << step4_radix_log(S, i)) - 1) << (2 * i);
  return off;
}
__host__ __device__ constexpr int step4_tw_total(int S) { return step4_tw_offset(S, num_steps4(S)); }
__host__ __device__ constexpr size_t pass4_lds_bytes(int S, int LT) {
  return num_steps4(S) > 1 ? ((size_t)36 << (S + LT)) : 0;
}

// ---- step table of the radix-4 kernels: [head: seven wave-uniform constants | entries] ---------------------
// Head, seven blocks of 84 words: block 0 is w4 = w16^4, blocks 1..6 are w16^e for e = 1, 2, 3, 6, 9, 0 (w16 = wR^(R/16) of
// the table's direction; the first-layer step twiddles w16^(t m), see L1_UNIFORM below).  A block holds its constant for
// fe_mul_split<1, 2>, transposed: word 9 b + j = limb b of row_j = w 2^(29 (j - 7)) mod r, so the nine constants of
// column b are neighbours; words 81..83 are padding.  The head is read through the constant address space: wave-uniform
// addresses there are scalar loads, the limb is the scalar operand of its v_mad_u64_u32 and no VGPR holds it.
// Entries, 80 B each: limbs of row_0 = w 2^-87, then of row_1 = w 2^58 (fe_mul_split<5, 6>), two words of padding.
constexpr int STEP4_HEAD_CONSTS = 7;
constexpr int STEP4_HEAD_BLOCK = 84;                                   // words per head constant
constexpr int STEP4_HEAD = STEP4_HEAD_CONSTS * STEP4_HEAD_BLOCK / 4;   // u32x4 units in front of entry 0
constexpr int STEP4_ENTRY = 5;   // u32x4 units per entry
__host__ __device__ constexpr int step4_head_exp(int blk) { return blk == 0 ? 4 : blk == 4 ? 6 : blk == 5 ? 9 : blk == 6 ? 0 : blk; }
typedef const __attribute__((address_space(4))) u32* W4Rows;
PM_DEV W4Rows w4_rows(const u32x4* step_tw) {
  return (W4Rows)(reinterpret_cast<const u32*>(step_tw));
}
// head block of w16^e, e = t m with t in 1..3, m in 0..3: a nibble per exponent (0, 1, 2, 3, 4, 6, 9 -> 6, 1, 2, 3, 0, 4, 5)
PM_DEV W4Rows w16_rows(W4Rows head, u32 e) {
  return head + STEP4_HEAD_BLOCK * (u32)((0x5004003216ull >> (4 * e)) & 15u);
}
// x * w for a head constant (w4_rows / w16_rows): x (B < 6, any V the limbs allow) -> (1, <2), 97 limb products
PM_DEV Fr mul_head(const Fr& x, W4Rows rows) {
  return fe_mul_split<FrP, 1, 2>(x, [&](int j, int b) { return rows[9 * b + j]; });
}

// First-layer step twiddles applied by their producer.  Step 1 of a pass multiplies its input m by w16^(k' m), k' = u & 3:
// lane-varying there.  Step 0's thread u wrote that input as X[t] to slot 4u + t = m U + u' with k' = t, so the factor owed
// to X[t] is w16^(t m) with m = u >> (log2 U - 2): t is a compile-time index and m is the same for all of a wave when the
// wave's 64 >> LT values of u stay inside one aligned block of U/4.  Then step 0 applies it through the head's scalar
// rows (97 limb products, no VGPR, no vector load) and step 1 takes its inputs from the LDS as they are.  The waves with
// m = 0 multiply by w16^0 = 1 like the others: a branch around their products (fe_reduce_weak instead) measured slower,
// every wave of the workgroup meets the same barrier.  Step 0 is never u-fast when a second step follows it (u-fast
// belongs to a pass's last step).  Only passes that read the wide form (middle and last) take this path: the first and
// single passes, whose step 0 follows the loads from HBM directly, measured 1 - 2 us slower per launch with it; those of
// even S apply the same products on the consumer side of a plane-major exchange (below).
__host__ __device__ constexpr bool step4_l1_uniform(int S, int LT, bool in_wide) {
  return in_wide && num_steps4(S) >= 2 && step4_radix_log(S, 1) == 2 && (64 >> LT) <= ((1 << S) >> 4);
}

// ---- plane-major exchanges: first and single passes of even S >= 4 (radix-4 steps only) ------------------------------
// The passes that read the wide form keep the exchange and the producer-side products above.  On this one, with
// consumer-side products, the <10, 1> last pass lost its bank conflicts and measured 0.7 us slower per launch; with its
// producer-side products the 2^20 step measured 0.5 us behind: those launches are bound by VALU
// issue, not by the LDS, and the swizzles cost them instructions.
// Thread tau = tid >> LT of column c = tid & (T - 1) owns, at step s, the butterfly g_s(tau) = tau rotated left by 2 s
// inside its S - 2 bits: g_0 and g_last are the identity, so the HBM side of a pass is that of the Stockham map.  Its
// twiddle digit k' = g_s(tau) & (4^s - 1) is the top 2 s bits of tau.  After step s the thread writes X[t] to plane t at
// its own place, element t U T + tid of the tile: lane-contiguous stores, no index to compute.  Stockham puts that
// output at logical position (h : t : k'), g_s(tau) = (h : k'); step s + 1 reads logical positions m U + u'', so the
// reader of plane t is the thread (t : tau without the top two bits of h), whose four inputs m = 0..3 sit at its own tau
// with m put back where those two bits were: bits p + 1, p of the place inside the plane, p = S - 4 - 2 s.  A reader's
// lanes therefore see runs of 2^q consecutive elements, q = p + LT.  Runs under 32 elements would meet on the LDS banks, so
// both sides of such an exchange XOR a few higher bits of the element index into its low bits (XchgSwz: bits
// k .. k + w - 1 into bits j .. j + w - 1; disjoint fields, a bijection of the tile).  Writers stay conflict-free
// under it, an aligned group of lanes sees the XORed bits constant.  The last step of a u-fast pass (tid = c U + tau)
// strides its reads by 4 T elements and takes the low bits of tau into the bank bits instead.  The step-1 digit is
// tau >> (S - 4): the same for all of a wave when its 64 >> LT values of tau fit U/4, then step 1 multiplies through the
// head's scalar rows (step4_l1_consumer).  tests/test_ntt_plane_major.py walks these maps and a model of the banks
// through pm_test_ntt_exchange_map.
struct XchgSwz {
  int k, w, j;
};
// swizzle of exchange x (between steps x and x + 1); ufast: the pass's OUT_UFAST, it matters for the last exchange only
__host__ __device__ constexpr XchgSwz step4_xchg_swizzle(int S, int LT, bool ufast, int x) {
  const int q = S - 4 - 2 * x + LT;
  if (ufast && x == S / 2 - 2 && LT > 0) {
    // bits from LT + 2 up are tau; with U < 32 the wave's columns vary in bits 0 .. j - 1, which stay as they are
    const int k = LT + 2 > 4 ? LT + 2 : 4;
    int j = 0;
    while (((1 << (S - 2)) << j) < 32) ++j;
    int w = 5 - j;
    if (w > S + LT - k) w = S + LT - k;
    if (w > LT + 2 - j) w = LT + 2 - j;
    return XchgSwz{k, w, j};
  }
  if (q >= 5) return XchgSwz{0, 0, 0};
  return XchgSwz{q + 2 > 5 ? q + 2 : 5, 5 - q < 2 ? 5 - q : 2, q};
}
__host__ __device__ constexpr u32 step4_swizzled(XchgSwz z, u32 e) {
  return z.w == 0 ? e : e ^ (((e >> z.k) & ((1u << z.w) - 1u)) << z.j);
}
// (tau, c) of a thread at step s
__host__ __device__ constexpr u32 step4_pm_tau(int S, int LT, bool ufast, int s, u32 tid) {
  return ufast && s == S / 2 - 1 ? tid & ((1u << (S - 2)) - 1u) : tid >> LT;
}
__host__ __device__ constexpr u32 step4_pm_col(int S, int LT, bool ufast, int s, u32 tid) {
  return ufast && s == S / 2 - 1 ? tid >> (S - 2) : tid & ((1u << LT) - 1u);
}
__host__ __device__ constexpr u32 step4_pm_butterfly(int S, int s, u32 tau) {
  return ((tau << (2 * s)) & ((1u << (S - 2)) - 1u)) | (tau >> (S - 2 - 2 * s));
}
__host__ __device__ constexpr u32 step4_pm_digit(int S, int s, u32 tau) { return s == 0 ? 0u : tau >> (S - 2 - 2 * s); }
// element of the tile that step s < last writes X[t] to
__host__ __device__ constexpr u32 step4_pm_write(int S, int LT, bool ufast, int s, u32 tid, int t) {
  return step4_swizzled(step4_xchg_swizzle(S, LT, ufast, s), ((u32)t << (S - 2 + LT)) + tid);
}
// element of the tile that step s > 0 reads its input m from
__host__ __device__ constexpr u32 step4_pm_read(int S, int LT, bool ufast, int s, u32 tid, int m) {
  const u32 tau = step4_pm_tau(S, LT, ufast, s, tid), c = step4_pm_col(S, LT, ufast, s, tid);
  const int p = S - 2 - 2 * s;
  const u32 lo = tau & ((1u << (S - 4)) - 1u), t = tau >> (S - 4);
  const u32 place = ((lo >> p) << (p + 2)) | ((u32)m << p) | (lo & ((1u << p) - 1u));
  return step4_swizzled(step4_xchg_swizzle(S, LT, ufast, s - 1), ((((t << (S - 2)) | place)) << LT) + c);
}
// step 1 of a plane-major pass takes its twiddles from the head's scalar rows: its digit tau >> (S - 4) is wave-uniform
__host__ __device__ constexpr bool step4_l1_consumer(int S, int LT, bool ufast) {
  return step4_plane_major(S, false) && (64 >> LT) <= ((1 << S) >> 4) && !(ufast && S == 4);
}

// step s of a pass multiplies by per-lane table twiddles (vector loads) in a radix-4 step
__host__ __device__ constexpr bool step4_generic(int S, int LT, bool ufast, bool in_wide, int s) {
  return s > 0 && step4_radix_log(S, s) == 2 &&
         !(s == 1 && (step4_l1_uniform(S, LT, in_wide) || (step4_plane_major(S, in_wide) && step4_l1_consumer(S, LT, ufast))));
}

// Inter-pass twiddles applied by their producer (PASS_TW_OUT).  The pass that follows a wide store multiplies element idx
// by its table entry pass_tw[idx] before its first butterfly, so it cannot issue anything before both 36 B loads are back,
// and every workgroup of the launch is in that state at once.  The pass that writes element idx does the product
// instead, X[m] (<5, <40) times a canonical entry -> (1, <2) just before st_wide: the class the consumer's own product
// hands dft4s, and the consumer (PASS_TW_APPLIED) takes what it loads as it is.  The table, its layout and n^-1 folded into
// the last pass's table are unchanged; the multiply-adds only move from one launch to the one before.
// Where the producer issues the four loads decides whether it pays: vector loads return in order, so
// a step-twiddle load issued behind them waits for HBM with them, in every workgroup at once.  They go two and two behind
// the last twiddle load of the second-to-last and of the last step, each pair with that step's third product and dft4s in
// front of the next load.  All four ahead of the last exchange's barrier made the 2^20 step 5 us slower than consumer-side
// products.  The placement needs the last two steps to be radix-4 steps with table twiddles (even S >= 8).  Of those
// shapes the first passes of radix 2^10 are the producers: with them the 2^20 step is 2.7 - 3.6 us faster.  The radix-2^8 shapes
// keep the consumer side: as producers (first and middle pass of 2^24, first pass of 2^22) they measured no difference,
// the first pass paid what the last one gained (profiles/tw_producer_full_ab.txt), and the <8, 3> middle pass would need 130
// VGPRs.  A middle pass of radix 2^10 occurs in no plan that has direct tables.  ntt_run() asks through pass4_tw_producer().
__host__ __device__ constexpr bool step4_tw_producer(int S, int LT, bool ufast, bool in_wide) {
  return S == 10 && !in_wide && step4_generic(S, LT, ufast, in_wide, num_steps4(S) - 2) &&
         step4_generic(S, LT, ufast, in_wide, num_steps4(S) - 1);
}

struct FrSplit2 {
  u32 l[18];
};
PM_DEV FrSplit2 ld_tw2(const u32x4* ent, size_t idx) {
  const u32x4* p = ent + STEP4_ENTRY * idx;
  u32x4 a = p[0], b = p[1], c = p[2], d = p[3];
  const uint2 e = reinterpret_cast<const uint2*>(p + 4)[0];
  FrSplit2 r;
  r.l[0] = a.x; r.l[1] = a.y; r.l[2] = a.z; r.l[3] = a.w;
  r.l[4] = b.x; r.l[5] = b.y; r.l[6] = b.z; r.l[7] = b.w;
  r.l[8] = c.x; r.l[9] = c.y; r.l[10] = c.z; r.l[11] = c.w;
  r.l[12] = d.x; r.l[13] = d.y; r.l[14] = d.z; r.l[15] = d.w;
  r.l[16] = e.x; r.l[17] = e.y;
  return r;
}
// x * w for a table twiddle: x (B < 6, any V the limbs allow) -> (1, <2)
PM_DEV Fr mul_tw2(const Fr& x, const FrSplit2& w) {
  return fe_mul_split<FrP, 5, 6>(x, [&](int j, int b) { return w.l[9 * j + b]; });
}
// Wave priorities by step (PASS_STEP_PRIO, option ntt_step_prio).  The SIMD's issue arbiter compares the
// user priority before the age of a wave, and by age alone the older of a CU's two workgroups issues whenever it can: the
// younger one falls two to three steps behind and finishes alone, a quarter of the launch with half the waves
// (profiles/ntt_prio_timeline_parent.txt).  With the flag a wave enters the kernel at 3 and takes step4_prio() at the top of
// step s, behind the barrier that ends the exchange: of two co-resident workgroups the one a step behind is served first,
// so they alternate, and equal steps fall back to age.  The flag is the launch's: every test is a scalar branch around one
// s_setprio with a compile-time operand, at a place where a barrier bounds the compiler's scheduling already.  No result
// depends on it.  Not kept: priority 3 from a step's last product until the next step's LDS reads are issued, alone or on
// top of this rule (no gain, and its branches inside the steps cost every launch, flagged or not: 4 us of the 2^20 step).
// The passes of radix 2^10 take the flag.  Those of radix 2^8 measured slower with it (forward + inverse 2^24 3.27 -> 3.41 ms,
// coset 2^20 -> 2^22 449 -> 462 us, profiles/ntt_prio_headline_ab.txt): their kernels hold none of this code.
__host__ __device__ constexpr bool step4_has_prio(int S) { return S >= 10 && num_steps4(S) >= 2; }
__host__ __device__ constexpr int step4_prio(int S, int s) { return num_steps4(S) - 1 - s < 3 ? num_steps4(S) - 1 - s : 3; }

// ---- lazy split products (fe_mul_split with D = G, fields.hip.h): one reduction digit fewer per table product ---------------
// The products above return the class (1, <2) so that dft4's bounds hold as written; that costs one digit column and N - 1
// limb products each, and the butterflies do not need it.  A lazy product leaves the limbs normalised and the value below
// V r, V = 16.01 for a step twiddle in three rows (G = D = 3, 105 limb products instead of 129) and 37.01 for w4 in nine rows
// (G = D = 1, 89 instead of 97); dft4s_lazy carries V in its fe_sub constants, which are compile-time and free.  The weak
// reduction of x[0] at the top of every step and the products themselves (any value the limbs allow) bring each step's
// inputs back to the same classes, so nothing grows from step to step; the walk is in tests/test_fe_mul_split_lazy_model.py.
// The constants come from a table of their own, a.step_tw_lazy (the one above is unchanged and still serves the first-layer
// head constants, with D = 2):
//   head, 84 words: w4 for fe_mul_split<1, 1>, transposed as above: word 9 b + j = limb b of row_j = w4 2^(29 (j - 8)) mod r;
//   entries of the radix-4 steps s >= 2, in the order of the table above: ceil(9 / G) rows, row_j = w 2^(29 (j G + G - 9)) mod r,
//   canonical limbs, nine words a row, padded with zero words to a multiple of 16 B (G = 3: 27 words in 7 x 16 B).
// step4_lazy_form() is the G of a shape's step twiddles, 0 for a shape that keeps the code above instruction for
// instruction.  The <10, 1> passes of the 2^20 transform take it (profiles/lazy_split_headline_ab.txt):
// three rows where the pass reads the wide form (last and middle, 98 -> 112 VGPRs), two rows (G = D = 5, 121 limb products,
// value < 11.01 r, the registers of the parent's two rows) in the first pass, which holds the next pass's twiddles beside
// its own and needs 136 VGPRs with three rows, one wave per SIMD fewer.  Five rows (G = D = 2, 97 limb products, 124 VGPRs)
// in the last pass measured 2.4 us slower than three over the 2^20 step, with 98 VALU instructions per wave fewer: twelve
// 16-byte loads a twiddle instead of seven.  The other shapes were not measured with any of it and keep their code.
// Such a shape's generic steps all have s >= 2 (ntt_step4 asserts it).
__host__ __device__ constexpr int step4_lazy_form(int S, int LT, bool in_wide) {
  return S == 10 && LT == 1 ? (in_wide ? 3 : 5) : 0;
}
// A fixed-shape first pass (FIX != 0, below) has its addresses in 32-bit offsets, not in VGPR pairs, and holds three rows in
// 117 VGPRs without scratch (two rows: 102): 216 VALU instructions a wave fewer, 1.2 us a launch and 2.8 us of the 2^20 step
// (profiles/fixed_shape_headline_ab.txt).  PM_NTT_FIXED_FIRST_G is its G; A/B builds set the other one
// (make EXTRA=-DPM_NTT_FIXED_FIRST_G=5).  It reads the G = 3 table of the last pass, ntt_run() hands it over.  Its inputs and
// outputs are of the last pass's classes, step for step (tests/test_ntt_fixed_shape_lazy_model.py walks them).
#ifndef PM_NTT_FIXED_FIRST_G
#define PM_NTT_FIXED_FIRST_G 3
#endif
// G of the kernel ntt_pass4_fixed_kernel<.., FIX> (FIX = 0: of the generic kernel)
__host__ __device__ constexpr int step4_fixed_lazy_form(int S, int LT, bool in_wide, int FIX) {
  return FIX != 0 && !in_wide && step4_lazy_form(S, LT, in_wide) != 0 ? PM_NTT_FIXED_FIRST_G : step4_lazy_form(S, LT, in_wide);
}
constexpr int STEP4_LAZY_HEAD = STEP4_HEAD_BLOCK / 4;   // u32x4 units in front of the first entry
__host__ __device__ constexpr int step4_lazy_rows(int G) { return (9 + G - 1) / G; }
__host__ __device__ constexpr int step4_lazy_entry(int G) { return (9 * step4_lazy_rows(G) + 3) / 4; }   // u32x4 units per entry
__host__ __device__ constexpr bool step4_lazy_step(int S, int s) { return s >= 2 && s < num_steps4(S) && step4_radix_log(S, s) == 2; }
__host__ __device__ constexpr int step4_lazy_offset(int S, int s) {   // entries in front of step s
  int off = 0;
  for (int i = 2; i < s; ++i) off += step4_lazy_step(S, i) ? 3 << (2 * i) : 0;
  return off;
}
__host__ __device__ constexpr int step4_lazy_total(int S) { return step4_lazy_offset(S, num_steps4(S)); }

template <int G>
struct FrSplitLazy {
  u32 l[9 * step4_lazy_rows(G)];
};
template <int G>
PM_DEV FrSplitLazy<G> ld_tw_lazy(const u32x4* ent, size_t idx) {
  constexpr int WORDS = 9 * step4_lazy_rows(G), UNITS = step4_lazy_entry(G);
  const u32x4* p = ent + UNITS * idx;
  FrSplitLazy<G> r;
#pragma unroll
  for (int k = 0; k < UNITS; ++k) {
    if (WORDS - 4 * k == 2) {   // a row pair ends on half a unit
      const uint2 e = reinterpret_cast<const uint2*>(p + k)[0];
      r.l[4 * k] = e.x; r.l[4 * k + 1] = e.y;
    } else {
      const u32x4 v = p[k];
      r.l[4 * k] = v.x;
      if (4 * k + 1 < WORDS) r.l[4 * k + 1] = v.y;
      if (4 * k + 2 < WORDS) r.l[4 * k + 2] = v.z;
      if (4 * k + 3 < WORDS) r.l[4 * k + 3] = v.w;
    }
  }
  return r;
}
// x * w for a lazy table twiddle: x (B < 6 for G = 5, B <= 5 otherwise, any V the limbs allow) -> limbs < 2^29, value
// < (ceil(9 / G) B (1 + 2^-28) + 1) r: < 16.01 r for G = 3 and B = 5
template <int G>
PM_DEV Fr mul_tw_lazy(const Fr& x, const FrSplitLazy<G>& w) {
  return fe_mul_split<FrP, G, G>(x, [&](int j, int b) { return w.l[9 * j + b]; });
}
// x * w4 through the lazy head: x (B <= 4) -> limbs < 2^29, value < 37.01 r; 89 limb products
PM_DEV Fr mul_head_lazy(const Fr& x, W4Rows rows) {
  return fe_mul_split<FrP, 1, 1>(x, [&](int j, int b) { return rows[9 * b + j]; });
}

// Diagnostic build only (make EXTRA=-DPM_DEV_STAMPS, tools/ntt_phase_timeline.py): lane 0 of every wave leaves shader-clock
// and wall-clock stamps at its phase boundaries and its hardware placement in a buffer the host sets (ntt_stamps_arm in
// ntt4.hip), NTT_STAMP_WORDS words per wave: stamp k in words 2 k (s_memtime) and 2 k + 1 (s_memrealtime), k = 0 kernel entry,
// 1 entry loads returned, 2 + 3 s + {0, 1, 2} step s after its LDS reads / after its last product / after its second barrier,
// 2 + 3 NSTEPS after the last store is issued; word 36 = HW_ID | XCC_ID << 32, word 37 = blockIdx.x | wave << 32 |
// blockIdx.y << 48.  The product build has none of it.
#ifdef PM_DEV_STAMPS
constexpr int NTT_STAMP_WORDS = 40;
static __device__ unsigned long long* g_ntt_stamps = nullptr;
static __device__ unsigned long long g_ntt_stamp_waves = 0;   // waves the buffer has room for
PM_DEV unsigned long long* ntt_stamp_slot() {
  const unsigned long long w =
      ((unsigned long long)blockIdx.y * gridDim.x + blockIdx.x) * ((blockDim.x + 63u) >> 6) + (threadIdx.x >> 6);
  return (g_ntt_stamps && w < g_ntt_stamp_waves && (threadIdx.x & 63u) == 0) ? g_ntt_stamps + w * NTT_STAMP_WORDS : nullptr;
}
PM_DEV void ntt_stamp(int k) {
  __builtin_amdgcn_sched_barrier(0);
  unsigned long long t, r;
  asm volatile("s_memtime %0\n\ts_memrealtime %1\n\ts_waitcnt lgkmcnt(0)" : "=&s"(t), "=&s"(r) : : "memory");
  if (unsigned long long* p = ntt_stamp_slot()) {
    p[2 * k] = t;
    p[2 * k + 1] = r;
  }
  __builtin_amdgcn_sched_barrier(0);
}
PM_DEV void ntt_stamp_placement() {
  const unsigned long long hw = __builtin_amdgcn_s_getreg(4 | (31 << 11));     // HW_REG_HW_ID, 32 bits
  const unsigned long long xcc = __builtin_amdgcn_s_getreg(20 | (31 << 11));   // HW_REG_XCC_ID
  if (unsigned long long* p = ntt_stamp_slot()) {
    p[36] = hw | (xcc << 32);
    p[37] = (unsigned long long)blockIdx.x | ((unsigned long long)(threadIdx.x >> 6) << 32) | ((unsigned long long)blockIdx.y << 48);
  }
}
#define NTT_STAMP(k) ntt_stamp(k)
#define NTT_STAMP_LOADS(k)                          \
  do {                                              \
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); \
    ntt_stamp(k);                                   \
  } while (0)
#else
#define NTT_STAMP(k)
#define NTT_STAMP_LOADS(k)
#endif

// 4-point DIF as dft4 (ntt_kernels.hip.h), the product by w4 through its split rows: a3 enters it at (4, 5)
PM_DEV void dft4s(Fr& a0, Fr& a1, Fr& a2, Fr& a3, W4Rows w4) {
  BFLY(3, a0, a2);  // a0 (2+, <26)  a2 (4+, <27)
  BFLY(3, a1, a3);  // a1 (2, 4)     a3 (4, 5)
  a3 = mul_head(a3, w4);
  a2 = fe_norm<FrP>(a2);
  BFLY(5, a0, a1);  // a0 = X0, a1 = X2
  BFLY(3, a2, a3);  // a2 = X1, a3 = X3
  Fr t = a1;
  a1 = a2;
  a2 = t;
}

// dft4s with lazy inputs and a lazy w4 product: a0 (1, <2) (the weakly reduced or untwiddled input), a1..a3 (1, <16.01), what
// mul_tw_lazy<3> returns; the (1, <2) of step 0, of the first-layer products and of (5, 5) rows is inside it.  Every K is
// the least that fe_sub<K, 1> admits for its subtrahend, value < (K - 1) r.  Outputs (<5, <60): below the 2^261 = 68.6 r of
// fe_reduce_weak and fe_reduce_canon_pack, and limbs that fe_mul, fe_mul_split and the stores take.
PM_DEV void dft4s_lazy(Fr& a0, Fr& a1, Fr& a2, Fr& a3, W4Rows w4) {
  BFLY(18, a0, a2);  // a0 (2, <18.02)  a2 (4, <20.01)
  BFLY(18, a1, a3);  // a1 (2, <32.02)  a3 (4, <34.01)
  a3 = mul_head_lazy(a3, w4);  // (1, <37.01)
  a2 = fe_norm<FrP>(a2);
  BFLY(34, a0, a1);  // a0 = X0 (4, <50.04), a1 = X2 (5, <52.02)
  BFLY(39, a2, a3);  // a2 = X1 (2+, <57.02), a3 = X3 (4+, <59.01)
  Fr t = a1;
  a1 = a2;
  a2 = t;
}

// ---- fixed-shape variants (FIX = log_n, 0: the generic kernel; option ntt_fixed_shape) --------------
// The two <10, 1> passes of a plain 2^20 transform run with one geometry and one set of flags: log_n, log_ns, n_cols and the
// wide layout's blocking are constants there, the input is whole, nothing is multiplied in at the ends beside the inter-pass
// twiddles, and the priorities and the XCD tiling are on.  ntt_pass4_fixed_kernel<.., FIX> is that launch and nothing else
// (ntt_run() takes it only when pass4_fixed_match() holds, everything else launches ntt_pass4_kernel as before): the flag
// tests are decided at compile time, the other entries and exits do not exist, and every global address is a uniform
// 64-bit base (batch vector and tile, scalar arithmetic) plus a 32-bit byte offset of the lane (2^FIX x 36 B fits), the form
// a global load or store takes with its base in SGPRs.  The arithmetic, its order, the placement of the loads, the
// priorities and the LDS maps are those of the generic kernel, line for line.
constexpr u32 PASS4_FIX_GLOG = 2;   // blocking of the wide layout in a plan of <10, 1> passes (plan_wide_glog)
// the flags a launch must carry, all of them and no other: in_wide picks the last pass's set (first: false)
__host__ __device__ constexpr u32 pass4_fixed_flags(bool in_wide) {
  return (in_wide ? PASS_TW_APPLIED : PASS_TW_OUT) | PASS_STEP_PRIO | PASS_XCD_REMAP;
}
// may this launch take the fixed variant of (S, LT, in_wide) built for log_n = FIX: the geometry and the flags are the variant's,
// and the transform it belongs to is a plain one on a whole input (coset: PM_NTT_COSET; a coset transform's plain pass and
// the last pass behind a zero-padded input keep the generic kernel too: the variants were measured in the plain transform)
__host__ __device__ constexpr bool pass4_fixed_match(int FIX, int S, int LT, bool in_wide, u32 log_n, u32 log_ns, u32 wide_glog,
                                                     u32 flags, unsigned long long in_len, bool coset) {
  return FIX != 0 && log_n == (u32)FIX && log_ns == (in_wide ? (u32)(FIX - S) : 0u) && wide_glog == PASS4_FIX_GLOG &&
         flags == pass4_fixed_flags(in_wide) && in_len == (1ull << FIX) && !coset;
}
// A lane's byte offset, opaque to the compiler (no instruction): knowing its range, the compiler takes a constant summand out
// of it and adds it to the 64-bit address instead, lane by lane in VGPR pairs, which is the arithmetic these offsets replace.
PM_DEV u32 lane_off(u32 off) {
  asm("" : "+v"(off));
  return off;
}
// a wide vector seen from a uniform element i0: the lane adds an element offset i with (i0 & 3) + (i & 3) <= 3, so that the
// block and the place inside it split into a uniform and a lane part (the callers' i0 is a multiple of the tile width T <= 4
// and their i is a column below T plus a multiple of 4)
struct WideFix {
  char* q;    // limbs 0-3 of element i0; limbs 4-7 are 64 B further
  char* q8;   // limb 8 of element i0
};
PM_DEV WideFix wide_fix(const void* base, size_t i0) {
  char* b = reinterpret_cast<char*>(const_cast<void*>(base)) + 36 * 4 * (i0 >> PASS4_FIX_GLOG);
  const u32 e = (u32)i0 & 3u;
  return WideFix{b + 16 * e, b + 128 + 4 * e};
}
PM_DEV Fr ld_wide_fix(const WideFix& w, u32 i) {
  const u32 blk = 144u * (i >> PASS4_FIX_GLOG), e = i & 3u;
  const u32x4* q = reinterpret_cast<const u32x4*>(w.q + lane_off(blk + 16u * e));
  u32x4 a = q[0], b = q[4];
  u32 c = reinterpret_cast<const u32*>(w.q8 + lane_off(blk + 4u * e))[0];
  Fr r;
  r.l[0] = a.x; r.l[1] = a.y; r.l[2] = a.z; r.l[3] = a.w;
  r.l[4] = b.x; r.l[5] = b.y; r.l[6] = b.z; r.l[7] = b.w;
  r.l[8] = c;
  return r;
}
PM_DEV void st_wide_fix(const WideFix& w, u32 i, const Fr& v) {
  const u32 blk = 144u * (i >> PASS4_FIX_GLOG), e = i & 3u;
  u32x4* q = reinterpret_cast<u32x4*>(w.q + lane_off(blk + 16u * e));
  q[0] = u32x4{v.l[0], v.l[1], v.l[2], v.l[3]};
  q[4] = u32x4{v.l[4], v.l[5], v.l[6], v.l[7]};
  reinterpret_cast<u32*>(w.q8 + lane_off(blk + 4u * e))[0] = v.l[8];
}
// pass4_out_index of a fixed variant without its tile: the lane's element offset from output j0 R (first pass, log_ns = 0)
// or j0 (last pass, log_ns = FIX - S, where j < ns and k = j)
template <int S, int LT, bool OUT_UFAST, bool IN_WIDE, int FIX>
PM_DEV u32 pass4_fixed_out_lane(u32 tid, int m) {
  constexpr u32 U = (1u << S) / 4;
  const u32 c = OUT_UFAST ? tid / U : tid & ((1u << LT) - 1u);
  const u32 u = OUT_UFAST ? tid % U : tid >> LT;
  return IN_WIDE ? c + ((u + (u32)m * U) << (FIX - S)) : (c << S) + u + (u32)m * U;
}
// ld_tw_lazy with the entry's byte offset in 32 bits (a step's table is a few KB)
template <int G>
PM_DEV FrSplitLazy<G> ld_tw_lazy_fix(const u32x4* ent, u32 idx) {
  return ld_tw_lazy<G>(reinterpret_cast<const u32x4*>(reinterpret_cast<const char*>(ent) + lane_off(16u * step4_lazy_entry(G) * idx)), 0);
}

// Step twiddles kept in flight (PM_NTT_FIXED_TW_PREFETCH).  A lazy step twiddle is seven 16-byte loads
// that hit L2 (the step-4 table is 86 KB), and as the steps are written each of them is issued only behind the product by the
// one before it, a few instructions in front of the wait for it: nine round trips a wave that the wave itself covers nothing
// of.  With the macro at 1 the fixed last pass rotates two buffers: twiddle i + 1 of a step is issued in front of the product by
// twiddle i, and a step's first twiddle by the step before it, behind its butterflies and in front of the exchange's first
// barrier (the address is the lane's and the step's, nothing of the data).  Only the order of the loads changes.  0 is the order
// of the generic kernel (A/B builds: make EXTRA=-DPM_NTT_FIXED_TW_PREFETCH=0).  The first pass keeps the generic order: it
// stands at 117 VGPRs, a second buffer of 27 words fits only where the next pass's twiddles are not held yet (step 2), and that
// part with the carried first twiddles measured no faster (profiles/twiddle_prefetch_kernel_trace.txt).  The last pass:
// 34.2 -> 33.1 us a launch, 107 VGPRs, no scratch.
#ifndef PM_NTT_FIXED_TW_PREFETCH
#define PM_NTT_FIXED_TW_PREFETCH 1
#endif
__host__ __device__ constexpr bool step4_tw_prefetch(int S, int LT, bool in_wide, int FIX) {
  return PM_NTT_FIXED_TW_PREFETCH != 0 && FIX != 0 && in_wide && step4_fixed_lazy_form(S, LT, in_wide, FIX) != 0;
}
// the first twiddle of the next step on its way from one ntt_step4 to the next; G = 0: nothing is carried
template <int G>
struct Step4TwNext {
  FrSplitLazy<G> w;
};
template <>
struct Step4TwNext<0> {};
__host__ __device__ constexpr int step4_tw_next_form(int S, int LT, bool in_wide, int FIX) {
  return step4_tw_prefetch(S, LT, in_wide, FIX) ? step4_fixed_lazy_form(S, LT, in_wide, FIX) : 0;
}
// v behind dep for the compiler (no instruction).  With two twiddles loaded, two products of a step are ready at once, and
// the compiler weaves them into each other: 256 VGPRs and scratch in a kernel that holds 79 with the loads between them.
PM_DEV void fe_behind(Fr& v, const Fr& dep) {
  asm("" : "+v"(v.l[0]), "+v"(v.l[1]), "+v"(v.l[2]), "+v"(v.l[3]), "+v"(v.l[4]), "+v"(v.l[5]), "+v"(v.l[6]), "+v"(v.l[7]), "+v"(v.l[8])
      : "v"(dep.l[8]));
}
// twiddle t (0 .. 2, for x[t + 1]) of the lazy step STEP of a fixed variant, for this lane
template <int S, int LT, int STEP, bool OUT_UFAST, bool IN_WIDE, int FIX>
PM_DEV auto ld_step_lazy_fix(const NttPassArgs& a, u32 tid, u32 t) {
  constexpr int G = step4_fixed_lazy_form(S, LT, IN_WIDE, FIX);
  constexpr u32 U = (1u << S) / 4, nsp = 1u << (2 * STEP);
  constexpr bool ufast = OUT_UFAST && STEP == num_steps4(S) - 1;
  const u32 u = ufast ? tid % U : tid >> LT;
  const u32 kp = step4_plane_major(S, IN_WIDE) ? step4_pm_digit(S, STEP, u) : u & (nsp - 1);
  return ld_tw_lazy_fix<G>(a.step_tw_lazy + STEP4_LAZY_HEAD + step4_lazy_entry(G) * step4_lazy_offset(S, STEP), t * nsp + kp);
}

// element of the output vector (batch offset apart) that the last step of a pass stores its x[m] to
template <int S, int LT, bool OUT_UFAST>
PM_DEV size_t pass4_out_index(const NttPassArgs& a, u32 tid, size_t j0, int m) {
  constexpr int R = 1 << S;
  constexpr int U = R / 4;
  const u32 c = OUT_UFAST ? tid / U : tid & ((1u << LT) - 1u);
  const u32 u = OUT_UFAST ? tid % U : tid >> LT;
  const size_t j = j0 + c;
  const size_t ns = (size_t)1 << a.log_ns;
  const size_t k = j & (ns - 1);
  return (j - k) * R + k + (size_t)(u + m * U) * ns;
}

template <int S, int LT, int STEP, bool OUT_UFAST, bool IN_WIDE, bool OUT_WIDE, int FIX = 0>
PM_DEV void ntt_step4(Fr (&x)[4], Fr (&ptw)[4], const NttPassArgs& a, const NttConsts& kc, u32x4* lds0, u32x4* lds1,
                      u32* lds2, W4Rows w4, u32 tid, size_t j0,
                      Step4TwNext<step4_tw_next_form(S, LT, IN_WIDE, FIX)>* nx = nullptr) {
  constexpr int R = 1 << S;
  constexpr int T = 1 << LT;
  constexpr int U = R / 4;
  constexpr int NSTEPS = num_steps4(S);
  constexpr int LQ = step4_radix_log(S, STEP);
  constexpr u32 nsp = 1u << (2 * STEP);  // Ns'
  constexpr bool last = (STEP == NSTEPS - 1);
  constexpr bool ufast = OUT_UFAST && last;
  constexpr bool L1_UNIFORM = step4_l1_uniform(S, LT, IN_WIDE);
  constexpr bool PM = step4_plane_major(S, IN_WIDE);            // plane-major exchanges: u below is tau
  constexpr bool L1_CONSUMER = PM && step4_l1_consumer(S, LT, OUT_UFAST);
  constexpr bool TW_PRODUCER = OUT_WIDE && step4_tw_producer(S, LT, OUT_UFAST, IN_WIDE);
  constexpr int LAZY = step4_fixed_lazy_form(S, LT, IN_WIDE, FIX);  // G of the lazy step twiddles, 0: the (1, <2) products
  // step twiddles kept in flight (above): this step takes its first one from nx and leaves the next step's there
  constexpr bool PREFETCH = step4_tw_prefetch(S, LT, IN_WIDE, FIX);
  constexpr bool NEXT_PREFETCH = PREFETCH && !last && step4_generic(S, LT, OUT_UFAST, IN_WIDE, STEP + 1);
  static_assert(!PREFETCH || !TW_PRODUCER, "the next pass's twiddles have no place in the rotated order");
  static_assert(!(L1_UNIFORM && STEP == 0 && ufast), "the producer of the first-layer twiddles is in wave order");
  static_assert(!LAZY || !step4_generic(S, LT, OUT_UFAST, IN_WIDE, STEP) || step4_lazy_step(S, STEP), "the lazy table starts at step 2");
  const u32 c = ufast ? tid / U : tid & (T - 1);
  const u32 u = ufast ? tid % U : tid >> LT;
  constexpr int PRIO = step4_prio(S, STEP);   // PASS_STEP_PRIO: the further a wave has come, the lower (above step4_prio)
  if constexpr (step4_has_prio(S) && STEP > 0 && PRIO != step4_prio(S, STEP - 1)) {
    if constexpr (FIX != 0)
      __builtin_amdgcn_s_setprio(PRIO);
    else if (a.flags & PASS_STEP_PRIO)
      __builtin_amdgcn_s_setprio(PRIO);
  }
  if (STEP > 0) {
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const u32 e = PM ? step4_pm_read(S, LT, OUT_UFAST, STEP, tid, m) : (u + m * U) * T + c;
      u32x4 lo = lds0[e], hi = lds1[e];
      x[m].l[0] = lo.x; x[m].l[1] = lo.y; x[m].l[2] = lo.z; x[m].l[3] = lo.w;
      x[m].l[4] = hi.x; x[m].l[5] = hi.y; x[m].l[6] = hi.z; x[m].l[7] = hi.w;
      x[m].l[8] = lds2[e];
    }
  }
  NTT_STAMP(2 + 3 * STEP);
  const u32x4* stw = a.step_tw + STEP4_HEAD + STEP4_ENTRY * step4_tw_offset(S, STEP);
  // the step's twiddles and their product in the shape's form: lazy rows from a.step_tw_lazy, or the two rows of stw
  const auto ld_step = [&](size_t i) {
    if constexpr (LAZY != 0 && FIX != 0)
      return ld_tw_lazy_fix<LAZY>(a.step_tw_lazy + STEP4_LAZY_HEAD + step4_lazy_entry(LAZY) * step4_lazy_offset(S, STEP), (u32)i);
    else if constexpr (LAZY != 0)
      return ld_tw_lazy<LAZY>(a.step_tw_lazy + STEP4_LAZY_HEAD + step4_lazy_entry(LAZY) * step4_lazy_offset(S, STEP), i);
    else
      return ld_tw2(stw, i);
  };
  const auto mul_step = [](const Fr& v, const auto& w) {
    if constexpr (LAZY != 0)
      return mul_tw_lazy<LAZY>(v, w);
    else
      return mul_tw2(v, w);
  };
  if constexpr (LQ == 2) {
    const u32 kp = PM ? step4_pm_digit(S, STEP, u) : u & (nsp - 1);
    if constexpr (L1_CONSUMER && STEP == 1) {
      // k' is the wave's: X[0] (<5, <40) -> (1, <1.01), X[m] (<5, <40) times w16^(k' m) -> (1, <2) through the head's scalar
      // rows, each product's rows through an opaque pointer of its own (see below).  The waves with k' = 0 multiply by 1.
      const u32 ku = __builtin_amdgcn_readfirstlane(kp);
      x[0] = fe_reduce_weak<FrP>(x[0]);
#pragma unroll
      for (int m = 1; m < 4; ++m) {
        W4Rows rows = w16_rows(w4, ku * m);
        asm volatile("" : "+s"(rows));
        x[m] = mul_head(x[m], rows);
      }
    } else if constexpr (PREFETCH && STEP > 0 && !(L1_UNIFORM && STEP == 1)) {
      // twiddle 0 is on its way since the step before; 1 and 2 go out in front of the products by 0 and 1
      x[0] = fe_reduce_weak<FrP>(x[0]);
      __builtin_amdgcn_sched_barrier(0);
      const auto w2 = ld_step_lazy_fix<S, LT, STEP, OUT_UFAST, IN_WIDE, FIX>(a, tid, 1);
      __builtin_amdgcn_sched_barrier(0);
      x[1] = mul_step(x[1], nx->w);
      __builtin_amdgcn_sched_barrier(0);
      const auto w3 = ld_step_lazy_fix<S, LT, STEP, OUT_UFAST, IN_WIDE, FIX>(a, tid, 2);
      __builtin_amdgcn_sched_barrier(0);
      fe_behind(x[2], x[1]);
      x[2] = mul_step(x[2], w2);
      fe_behind(x[3], x[2]);
      x[3] = mul_step(x[3], w3);
    } else if (STEP > 0 && !(L1_UNIFORM && STEP == 1)) {
      x[0] = fe_reduce_weak<FrP>(x[0]);
      x[1] = mul_step(x[1], ld_step(0 * nsp + kp));
      x[2] = mul_step(x[2], ld_step(1 * nsp + kp));
      const auto w3 = ld_step(2 * nsp + kp);
      if constexpr (TW_PRODUCER && STEP >= NSTEPS - 2) {
        // the next pass's twiddles of outputs 0, 1 (second-to-last step) and 2, 3 (last step), issued behind the step's
        // own last twiddle load: loads return in order, so nothing this thread needs soon may queue behind them
        if constexpr (FIX != 0) {
          const WideFix wtw = wide_fix(a.pass_tw_out, j0 << S);
          constexpr int m0 = last ? 2 : 0;
          __builtin_amdgcn_sched_barrier(0);
          ptw[m0] = ld_wide_fix(wtw, pass4_fixed_out_lane<S, LT, OUT_UFAST, IN_WIDE, FIX>(tid, m0));
          ptw[m0 + 1] = ld_wide_fix(wtw, pass4_fixed_out_lane<S, LT, OUT_UFAST, IN_WIDE, FIX>(tid, m0 + 1));
          __builtin_amdgcn_sched_barrier(0);
        } else if (a.flags & PASS_TW_OUT) {
          const WidePtr wtw = wide_ptrs(const_cast<void*>(a.pass_tw_out), a.wide_glog);
          constexpr int m0 = last ? 2 : 0;
          __builtin_amdgcn_sched_barrier(0);
          ptw[m0] = ld_wide(wtw, pass4_out_index<S, LT, OUT_UFAST>(a, tid, j0, m0));
          ptw[m0 + 1] = ld_wide(wtw, pass4_out_index<S, LT, OUT_UFAST>(a, tid, j0, m0 + 1));
          __builtin_amdgcn_sched_barrier(0);
        }
      }
      x[3] = mul_step(x[3], w3);
    }
    // L1_UNIFORM, step 1: step 0 left x[0] at (1, <1.01) and x[1..3] at (1, <2), the classes dft4s takes
    // every step reads the w4 rows anew (scalar loads, a column at a time): an opaque copy of the pointer, or the
    // rows of step 0 stay in 81 SGPRs for the whole kernel and spill
    W4Rows w4s = LAZY != 0 ? w4_rows(a.step_tw_lazy) : w4;
    asm volatile("" : "+s"(w4s));
    if constexpr (LAZY != 0)
      dft4s_lazy(x[0], x[1], x[2], x[3], w4s);  // (<5, <60) where the comments below say (<5, <40)
    else
      dft4s(x[0], x[1], x[2], x[3], w4s);  // X[t] in x[t]
    if constexpr (L1_UNIFORM && STEP == 0) {
      // what step 1 owes its inputs, here: X[0] (<5, <40) -> (1, <1.01); X[t] (<5, <40) times w16^(t m) -> (1, <2).  The
      // rows of each product through an opaque pointer of its own, as above.
      const u32 m = __builtin_amdgcn_readfirstlane(u >> (S - 4));
      x[0] = fe_reduce_weak<FrP>(x[0]);
#pragma unroll
      for (int t = 1; t < 4; ++t) {
        W4Rows rows = w16_rows(w4, t * m);
        asm volatile("" : "+s"(rows));
        x[t] = mul_head(x[t], rows);
      }
    }
    NTT_STAMP(2 + 3 * STEP + 1);
    if constexpr (NEXT_PREFETCH) {   // the next step's first twiddle: the exchange covers its round trip
      __builtin_amdgcn_sched_barrier(0);
      nx->w = ld_step_lazy_fix<S, LT, STEP + 1, OUT_UFAST, IN_WIDE, FIX>(a, tid, 0);
      __builtin_amdgcn_sched_barrier(0);
    }
    if constexpr (!last) {
      __syncthreads();
      const u32 base = (u - kp) * 4 + kp;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const u32 e = PM ? step4_pm_write(S, LT, OUT_UFAST, STEP, tid, t) : (base + t * nsp) * T + c;
        lds0[e] = u32x4{x[t].l[0], x[t].l[1], x[t].l[2], x[t].l[3]};
        lds1[e] = u32x4{x[t].l[4], x[t].l[5], x[t].l[6], x[t].l[7]};
        lds2[e] = x[t].l[8];
      }
      __syncthreads();
      NTT_STAMP(2 + 3 * STEP + 2);
    }
    // last: Ns' = R/4, k' = u: X[t] belongs to row u + t U = x[t] already
  } else {  // radix 2, always the last step: Ns' = R/2, k' = v = u + i U, pairs (x[i], x[i+2])
    x[0] = fe_norm<FrP>(x[0]);
    x[1] = fe_norm<FrP>(x[1]);
    x[2] = mul_tw2(x[2], ld_tw2(stw, u));
    x[3] = mul_tw2(x[3], ld_tw2(stw, u + U));
    BFLY(3, x[0], x[2]);
    BFLY(3, x[1], x[3]);
    NTT_STAMP(2 + 3 * STEP + 1);
  }
  if constexpr (last) {
    const size_t n = (size_t)1 << a.log_n;
    if constexpr (FIX != 0 && OUT_WIDE) {
      static_assert(FIX == 0 || (TW_PRODUCER && !IN_WIDE), "the fixed first pass applies the next pass's twiddles");
      const WideFix wout = wide_fix(a.out, ((size_t)blockIdx.y << FIX) + (j0 << S));
      // The one flag test a fixed variant keeps (the launch has the flag, pass4_fixed_match): the branch ends the compiler's
      // scheduling region in front of the four products and behind them, as in the generic kernel.  As one region with the
      // last butterflies the products are woven into them and the kernel spills (256 VGPRs, 1.6 KB of scratch; fences of
      // sched_barrier do not end a region); with the branch it holds 102 VGPRs with two lazy rows, 117 with three, and no scratch.
      if (a.flags & PASS_TW_OUT) {
#pragma unroll
        for (int m = 0; m < 4; ++m) x[m] = fe_mul<FrP>(x[m], ptw[m]);  // (<5, <40) * canonical -> (1, <2)
      }
#pragma unroll
      for (int m = 0; m < 4; ++m) st_wide_fix(wout, pass4_fixed_out_lane<S, LT, OUT_UFAST, IN_WIDE, FIX>(tid, m), x[m]);
    } else if constexpr (FIX != 0) {
      static_assert(FIX == 0 || IN_WIDE, "the fixed last pass reads the wide form");
      char* gout = reinterpret_cast<char*>(a.out) + 32 * ((size_t)blockIdx.y * a.batch_stride_out + j0);
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        u32 w[8];   // one pair of stores behind the eight words, as below
        fe_reduce_canon_pack<FrP>(w, x[m]);  // (<5, <40)
        fe_store_words<FrP>(gout + lane_off(32u * pass4_fixed_out_lane<S, LT, OUT_UFAST, IN_WIDE, FIX>(tid, m)), w);
      }
    } else if constexpr (OUT_WIDE) {
      const WidePtr wout = wide_ptrs(a.out, a.wide_glog);
      const size_t boff = (size_t)blockIdx.y * n;
      if constexpr (TW_PRODUCER) {
        if (a.flags & PASS_TW_OUT) {
#pragma unroll
          for (int m = 0; m < 4; ++m) x[m] = fe_mul<FrP>(x[m], ptw[m]);  // (<5, <40) * canonical -> (1, <2)
        }
      }
#pragma unroll
      for (int m = 0; m < 4; ++m) st_wide(wout, boff + pass4_out_index<S, LT, OUT_UFAST>(a, tid, j0, m), x[m]);
    } else {
      const size_t j = j0 + c;
      const size_t ns = (size_t)1 << a.log_ns;
      const size_t k = j & (ns - 1);
      const size_t obase = (j - k) * R + k;
      u32x4* gout = reinterpret_cast<u32x4*>(a.out) + 2 * (size_t)blockIdx.y * a.batch_stride_out;
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        const size_t go = obase + (size_t)(u + m * U) * ns;
        // Both ends leave the eight words to ONE pair of stores behind them: with a store at the end of each, the compiler
        // merged what the two had in common into a 4-byte, a 16-byte and a 12-byte store, the wide ones off their
        // alignment, and the <10, 1> last pass measured 1 us slower per launch than with fe_store.
        u32 w[8];
        if (a.flags & (PASS_POST_SCALE | PASS_POST_COSET)) {
          // a product is anywhere below 2 r: its top limb reaches that of r in a large share of the elements and the vote of
          // fe_reduce_canon_pack would send nearly every wave down both paths
          Fr v = x[m];
          if (a.flags & PASS_POST_SCALE) v = fe_mul<FrP>(v, fr_limbs(kc.scale));
          if (a.flags & PASS_POST_COSET) v = fe_mul<FrP>(v, two_level(a.cs_hi, a.cs_lo, (u32)go, a.lh));
          fe_canon_pack<FrP>(w, v);
        } else {
          fe_reduce_canon_pack<FrP>(w, x[m]);  // (<5, <40); whole waves come here: the flags are the launch's
        }
        fe_store_words<FrP>(gout + 2 * go, w);
      }
    }
    NTT_STAMP(2 + 3 * NSTEPS);
  }
}

template <int S, int LT, bool OUT_UFAST, bool IN_WIDE, bool OUT_WIDE>
__global__ void __launch_bounds__((1 << (S + LT)) / 4 < 64 ? 64 : (1 << (S + LT)) / 4)
    ntt_pass4_kernel(const NttPassArgs a, const NttConsts kc) {
  constexpr int R = 1 << S;
  constexpr int T = 1 << LT;
  constexpr int U = R / 4;
  constexpr int NTHREADS = U * T;
  constexpr int NSTEPS = num_steps4(S);
  extern __shared__ u32x4 lds[];
  u32x4* lds0 = lds;
  u32x4* lds1 = lds + R * T;
  u32* lds2 = reinterpret_cast<u32*>(lds + 2 * R * T);

  const u32 tid = threadIdx.x;
  if (NTHREADS < 64 && tid >= NTHREADS) return;
#ifdef PM_DEV_STAMPS
  static_assert(2 + 3 * NSTEPS < 18, "stamp slots");
  ntt_stamp_placement();
#endif
  NTT_STAMP(0);
  if constexpr (step4_has_prio(S)) {   // the entry loads and step 0 run at 3
    if (a.flags & PASS_STEP_PRIO) __builtin_amdgcn_s_setprio(3);
  }
  const u32 log_n = a.log_n;
  const size_t n = (size_t)1 << log_n;
  const size_t n_cols = (size_t)1 << (log_n - S);
  const size_t j0 = (size_t)xcd_tile(blockIdx.x, gridDim.x, a.flags) * T;
  const W4Rows w4 = w4_rows(a.step_tw);

  Fr x[4], ptw[4];  // ptw: the next pass's twiddles (PASS_TW_OUT), loaded by the last two steps
  {
    constexpr bool ufast = OUT_UFAST && NSTEPS == 1;
    const u32 c = ufast ? tid / U : tid & (T - 1);
    const u32 u = ufast ? tid % U : tid >> LT;
    const size_t j = j0 + c;
    if constexpr (IN_WIDE) {
      const WidePtr win = wide_ptrs(const_cast<void*>(a.in), a.wide_glog);
      const size_t boff = (size_t)blockIdx.y * n;
      const u32 k = (u32)(j & (((size_t)1 << a.log_ns) - 1));
      const u32 tw_shift = log_n - a.log_ns - S;
      if (a.flags & PASS_TW_APPLIED) {  // (1, <2) products of the producing pass
#pragma unroll
        for (int m = 0; m < 4; ++m) x[m] = ld_wide(win, boff + j + (size_t)(u + m * U) * n_cols);
      } else if (a.flags & PASS_DIRECT_TW) {
        const WidePtr wtw = wide_ptrs(const_cast<void*>(a.pass_tw), a.wide_glog);
#pragma unroll
        for (int m = 0; m < 4; ++m) {
          const size_t idx = j + (size_t)(u + m * U) * n_cols;
          x[m] = fe_mul<FrP>(ld_wide(win, boff + idx), ld_wide(wtw, idx));
        }
      } else {
#pragma unroll
        for (int m = 0; m < 4; ++m) {
          const u32 row = u + m * U;
          Fr v = ld_wide(win, boff + j + (size_t)row * n_cols);
          x[m] = fe_mul<FrP>(v, fr_canon(two_level(a.tw_hi, a.tw_lo, (k * row) << tw_shift, a.lh)));
        }
      }
    } else {
      const u32x4* gin = reinterpret_cast<const u32x4*>(a.in) + 2 * (size_t)blockIdx.y * a.batch_stride_in;
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        const size_t gi = j + (size_t)(u + m * U) * n_cols;
        if (gi < a.in_len) {
          x[m] = fe_load<FrP>(gin + 2 * gi);
          if (a.flags & PASS_PRE_COSET)
            x[m] = fe_mul<FrP>(x[m], two_level(a.cs_hi, a.cs_lo, (u32)gi, a.lh));
        } else {
          x[m] = fe_zero<FrP>();
        }
      }
    }
  }
  NTT_STAMP_LOADS(1);
  ntt_step4<S, LT, 0, OUT_UFAST, IN_WIDE, OUT_WIDE>(x, ptw, a, kc, lds0, lds1, lds2, w4, tid, j0);
  if constexpr (NSTEPS > 1) ntt_step4<S, LT, 1, OUT_UFAST, IN_WIDE, OUT_WIDE>(x, ptw, a, kc, lds0, lds1, lds2, w4, tid, j0);
  if constexpr (NSTEPS > 2) ntt_step4<S, LT, 2, OUT_UFAST, IN_WIDE, OUT_WIDE>(x, ptw, a, kc, lds0, lds1, lds2, w4, tid, j0);
  if constexpr (NSTEPS > 3) ntt_step4<S, LT, 3, OUT_UFAST, IN_WIDE, OUT_WIDE>(x, ptw, a, kc, lds0, lds1, lds2, w4, tid, j0);
  if constexpr (NSTEPS > 4) ntt_step4<S, LT, 4, OUT_UFAST, IN_WIDE, OUT_WIDE>(x, ptw, a, kc, lds0, lds1, lds2, w4, tid, j0);
  if constexpr (NSTEPS > 5) ntt_step4<S, LT, 5, OUT_UFAST, IN_WIDE, OUT_WIDE>(x, ptw, a, kc, lds0, lds1, lds2, w4, tid, j0);
}

// The same pass for the one launch of pass4_fixed_match(FIX, ..): same arguments, same grid, same LDS.  A kernel of its own
// beside the generic one, which keeps its text and its instruction stream.
template <int S, int LT, bool OUT_UFAST, bool IN_WIDE, bool OUT_WIDE, int FIX>
__global__ void __launch_bounds__((1 << (S + LT)) / 4 < 64 ? 64 : (1 << (S + LT)) / 4)
    ntt_pass4_fixed_kernel(const NttPassArgs a, const NttConsts kc) {
  constexpr int R = 1 << S;
  constexpr int T = 1 << LT;
  constexpr int U = R / 4;
  constexpr int NSTEPS = num_steps4(S);
  static_assert(FIX > S + LT + 3 && FIX < 26 && T <= (1 << PASS4_FIX_GLOG) && U * T >= 64 && NSTEPS > 1 && NSTEPS <= 6 &&
                    step4_has_prio(S) && IN_WIDE != OUT_WIDE && OUT_UFAST == OUT_WIDE,
                "fixed variants: first and last passes with priorities, 36 B x 2^FIX in 32 bits, a tile inside a wide block");
  extern __shared__ u32x4 lds[];
  u32x4* lds0 = lds;
  u32x4* lds1 = lds + R * T;
  u32* lds2 = reinterpret_cast<u32*>(lds + 2 * R * T);

  const u32 tid = threadIdx.x;
  __builtin_amdgcn_s_setprio(3);   // the entry loads and step 0 run at 3
  // 2^(FIX - S - LT) tiles, a multiple of 8, dealt as xcd_tile() deals them under PASS_XCD_REMAP
  const size_t j0 = (size_t)((blockIdx.x & 7u) * ((1u << (FIX - S - LT)) >> 3) + (blockIdx.x >> 3)) * T;
  const W4Rows w4 = w4_rows(a.step_tw);

  Fr x[4], ptw[4];  // ptw: the next pass's twiddles, loaded by the last two steps
  {
    const u32 c = tid & (T - 1);
    const u32 u = tid >> LT;
    if constexpr (IN_WIDE) {   // (1, <2) products of the producing pass (PASS_TW_APPLIED)
      const WideFix win = wide_fix(a.in, ((size_t)blockIdx.y << FIX) + j0);
#pragma unroll
      for (int m = 0; m < 4; ++m) x[m] = ld_wide_fix(win, c + ((u + (u32)m * U) << (FIX - S)));
    } else {                   // the whole input is there (in_len = n), no coset
      const char* gin = reinterpret_cast<const char*>(a.in) + 32 * ((size_t)blockIdx.y * a.batch_stride_in + j0);
#pragma unroll
      for (int m = 0; m < 4; ++m) x[m] = fe_load<FrP>(gin + lane_off(32u * (c + ((u + (u32)m * U) << (FIX - S)))));
    }
  }
  Step4TwNext<step4_tw_next_form(S, LT, IN_WIDE, FIX)> nx;  // a step's first twiddle, issued by the step before it
  ntt_step4<S, LT, 0, OUT_UFAST, IN_WIDE, OUT_WIDE, FIX>(x, ptw, a, kc, lds0, lds1, lds2, w4, tid, j0, &nx);
  ntt_step4<S, LT, 1, OUT_UFAST, IN_WIDE, OUT_WIDE, FIX>(x, ptw, a, kc, lds0, lds1, lds2, w4, tid, j0, &nx);
  if constexpr (NSTEPS > 2) ntt_step4<S, LT, 2, OUT_UFAST, IN_WIDE, OUT_WIDE, FIX>(x, ptw, a, kc, lds0, lds1, lds2, w4, tid, j0, &nx);
  if constexpr (NSTEPS > 3) ntt_step4<S, LT, 3, OUT_UFAST, IN_WIDE, OUT_WIDE, FIX>(x, ptw, a, kc, lds0, lds1, lds2, w4, tid, j0, &nx);
  if constexpr (NSTEPS > 4) ntt_step4<S, LT, 4, OUT_UFAST, IN_WIDE, OUT_WIDE, FIX>(x, ptw, a, kc, lds0, lds1, lds2, w4, tid, j0, &nx);
  if constexpr (NSTEPS > 5) ntt_step4<S, LT, 5, OUT_UFAST, IN_WIDE, OUT_WIDE, FIX>(x, ptw, a, kc, lds0, lds1, lds2, w4, tid, j0, &nx);
}

// step twiddles of the radix-4 kernel: block s, entry [(t-1)*Ns' + k'] = wR^(k' t R/(Ns' q)), Ns' = 4^s, both rows
// of each (canonical limbs); the first 63 threads also write the head: nine rows each of w4 = c.w8[1] and of the six
// powers of w16 = c.w8[2].
// Multiplying by 2^e in Montgomery form (fe_pow2<261 + e>) is the shift by e: 261 - 87 = 174, 261 + 58 = 319.
static __global__ void step4_tw_kernel(u32x4* out, const NttConsts c, u32 S) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < 9 * STEP4_HEAD_CONSTS) {  // row_j = w 2^(29 (j - 7)): 2^(29 (j + 2)) in Montgomery form, walked up from 2^58
    const u32 blk = i / 9, j = i % 9;
    const Fr w = blk == 0 ? fr_limbs(c.w8[1]) : fr_pow(fr_limbs(c.w8[2]), (u32)step4_head_exp((int)blk), fr_limbs(c.one));
    Fr p = fe_pow2<FrP, 58>();
    for (u32 k = 0; k < j; ++k) p = fe_mul<FrP>(p, fe_pow2<FrP, 261 + 29>());
    const Fr row = fr_canon(fe_mul<FrP>(w, p));
    u32* head = reinterpret_cast<u32*>(out) + STEP4_HEAD_BLOCK * blk;
    for (u32 b = 0; b < 9; ++b) head[9 * b + j] = row.l[b];
    if (j < 3) head[81 + j] = 0u;
  }
  u32x4* ent = out + STEP4_HEAD;
  u32 off = 0;
  for (u32 s = 0; 2 * s < S; ++s) {
    const u32 lq = (S - 2 * s) >= 2 ? 2 : 1;
    const u32 nsp = 1u << (2 * s);
    const u32 cnt = ((1u << lq) - 1) * nsp;
    if (i >= off && i < off + cnt) {
      const u32 t = (i - off) / nsp + 1, kp = (i - off) % nsp;
      const u32 e = (kp * t) << (S - 2 * s - lq);
      const Fr w = fr_pow(fr_limbs(c.w8[0]), e, fr_limbs(c.one));
      const Fr r0 = fr_canon(fe_mul<FrP>(w, fe_pow2<FrP, 174>()));
      const Fr r1 = fr_canon(fe_mul<FrP>(w, fe_pow2<FrP, 319>()));
      u32x4* p = ent + STEP4_ENTRY * (size_t)i;
      p[0] = u32x4{r0.l[0], r0.l[1], r0.l[2], r0.l[3]};
      p[1] = u32x4{r0.l[4], r0.l[5], r0.l[6], r0.l[7]};
      p[2] = u32x4{r0.l[8], r1.l[0], r1.l[1], r1.l[2]};
      p[3] = u32x4{r1.l[3], r1.l[4], r1.l[5], r1.l[6]};
      p[4] = u32x4{r1.l[7], r1.l[8], 0u, 0u};
      return;
    }
    off += cnt;
  }
}

// the lazy table of radix 2^S in form G (layout above): the first nine threads also write the head, row j of w4 = c.w8[1].
// 2^(29 e) in Montgomery form is walked up from 2^29 by factors of 2^29 (fe_pow2<261 + 29>), e = j + 1 for the head's
// row_j and j G + G for an entry's.
static __global__ void step4_lazy_tw_kernel(u32x4* out, const NttConsts c, u32 S, u32 G) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  const auto pow29 = [](u32 e) {
    Fr p = fe_pow2<FrP, 29>();
    for (u32 k = 1; k < e; ++k) p = fe_mul<FrP>(p, fe_pow2<FrP, 261 + 29>());
    return p;
  };
  if (i < 9) {
    const Fr row = fr_canon(fe_mul<FrP>(fr_limbs(c.w8[1]), pow29(i + 1)));
    u32* head = reinterpret_cast<u32*>(out);
    for (u32 b = 0; b < 9; ++b) head[9 * b + i] = row.l[b];
    if (i < 3) head[81 + i] = 0u;
  }
  const u32 rows = (9 + G - 1) / G, units = (9 * rows + 3) / 4;
  u32 off = 0;
  for (u32 s = 2; 2 * s + 2 <= S; ++s) {   // the radix-4 steps from the third on
    const u32 nsp = 1u << (2 * s);
    const u32 cnt = 3 * nsp;
    if (i >= off && i < off + cnt) {
      const u32 t = (i - off) / nsp + 1, kp = (i - off) % nsp;
      const u32 e = (kp * t) << (S - 2 * s - 2);
      const Fr w = fr_pow(fr_limbs(c.w8[0]), e, fr_limbs(c.one));
      u32* p = reinterpret_cast<u32*>(out + STEP4_LAZY_HEAD + (size_t)units * i);
      for (u32 j = 0; j < rows; ++j) {
        const Fr row = fr_canon(fe_mul<FrP>(w, pow29(j * G + G)));
        for (u32 b = 0; b < 9; ++b) p[9 * j + b] = row.l[b];
      }
      for (u32 k = 9 * rows; k < 4 * units; ++k) p[k] = 0u;
      return;
    }
    off += cnt;
  }
}

}  // namespace pm
