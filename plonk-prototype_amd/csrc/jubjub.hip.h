// JubJub on the device, shared by gadgets.hip (the rows of the curve gadgets), jubjub.hip (the native calls, DESIGN.md section
// 7.2k), schnorr.hip (signatures, section 7.2l) and cipher.hip (note scanning, section 7.2o): the twisted Edwards curve -x^2 + y^2 = 1 + d x^2 y^2 over Fr, d = -(10240 / 10241), in extended coordinates, with the
// field helpers the group law is written in.  Everything here runs in the device form (x 2^261, poly_common.hip.h).
//
// Affine addends.  ed_madd takes its second operand as (x, y, t) with t = x y; (0, 1, 0) is the neutral addend, so a digit of 0
// selects it (g_sel) and the addition still runs: no branch depends on a digit.  -(x, y, t) = (-x, y, -t).
#pragma once
#include <algorithm>
#include <string>

#include "context.h"
#include "field_inv.hip.h"
#include "poly_common.hip.h"

struct pm_jubjub_base {
  int device = 0;
  uint64_t xy[8] = {0};     // the point, canonical Montgomery
  mutable int order_state = 0;   // schnorr.hip, under the context's mutex: 0 = the point's order is unknown, 1 = it is l, -1 = it is not
  void* d_tab = nullptr;    // JJ_WINDOWS x 8 entries of JJ_ENTRY_CHUNKS x 16 bytes (entry_limbs, jubjub.hip)
};

namespace pm {

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
// 2 p by the dedicated doubling for a = -1 (Hisil, Wong, Carter, Dawson 2008, section 3.3) with every output negated, which is
// the same point: A = X^2, B = Y^2, C = 2 Z^2, H = A + B, G = B - A, F = C - G, E = (X + Y)^2 - H, then (E F, G H, F G, E H).
// Four squarings and four products (three without T) where ed_add(p, p) takes nine products; no exceptional case on the curve,
// and p.T is not read, so a run of doublings needs T from its last one only.
template <bool WITH_T>
PM_DEV EdPoint ed_double(const EdPoint& p) {
  const Fr A = fe_sqr<FrP>(p.X), B = fe_sqr<FrP>(p.Y), zz = fe_sqr<FrP>(p.Z);
  const Fr H = gadd(A, B), G = gsub(B, A), F = gsub(gadd(zz, zz), G);
  const Fr E = gsub(fe_sqr<FrP>(gadd(p.X, p.Y)), H);
  return EdPoint{gmul(E, F), gmul(G, H), gmul(F, G), WITH_T ? gmul(E, H) : p.T};
}
PM_DEV EdPoint ed_sel(bool c, const EdPoint& a, const EdPoint& b) {
  return EdPoint{g_sel(c, a.X, b.X), g_sel(c, a.Y, b.Y), g_sel(c, a.Z, b.Z), g_sel(c, a.T, b.T)};
}

// ------------------------------------------------------------------ host: the Edwards d
// JubJub d = -(10240 / 10241), canonical Montgomery: the inversion once, not per call
inline const HFr& jubjub_d_host() {
  const host::Field<4>& F = host::FR();
  static const HFr edwards_d = host::sub(host::zero<4>(), host::mul(host::from_u64(10240, F), host::inv(host::from_u64(10241, F), F), F), F);
  return edwards_d;
}
// ... as the nine 29-bit limbs of the device form, what a kernel's arguments carry
inline void jubjub_d_limbs(u32 (&dst)[9]) { to_limbs29_shift(dst, jubjub_d_host(), 1); }

// ------------------------------------------------------------------ the native calls (jubjub.hip, schnorr.hip)
constexpr u32 JJ_WINDOWS = 64;       // signed base-16 digits of a scalar below 2^255
constexpr u32 JJ_ENTRY_CHUNKS = 7;   // fixed-base entry: x, y, t as 27 limbs and one word of padding, 112 bytes
constexpr u32 JJ_POINT_CHUNKS = 9;   // variable-base entry: X, Y, Z, T as 36 limbs, 144 bytes
constexpr size_t JJ_BASE_TABLE_BYTES = (size_t)JJ_WINDOWS * 8 * JJ_ENTRY_CHUNKS * 16;   // 57344
constexpr size_t JJ_MUL_TABLE_BYTES = 8 * (size_t)JJ_POINT_CHUNKS * 16;                 // per thread in flight: 1152

// ------------------------------------------------------------------ the affine law on the host (csrc/host_field.h)
struct HPoint {
  HFr x, y;
};
inline HPoint hpoint_load(const uint64_t* xy) { return HPoint{hfr_load(xy), hfr_load(xy + 4)}; }
inline void hpoint_store(uint64_t* xy, const HPoint& p) {
  memcpy(xy, p.x.l, 32);
  memcpy(xy + 4, p.y.l, 32);
}
inline HPoint hpoint_identity() { return HPoint{host::zero<4>(), host::one<4>(host::FR())}; }
inline bool hpoint_on_curve(const HPoint& p) {
  const host::Field<4>& F = host::FR();
  const HFr x2 = host::mul(p.x, p.x, F), y2 = host::mul(p.y, p.y, F);
  const HFr rhs = host::add(host::one<4>(F), host::mul(jubjub_d_host(), host::mul(x2, y2, F), F), F);
  return host::eq(host::sub(y2, x2, F), rhs);
}
// (x1, y1) + (x2, y2) = ((x1 y2 + y1 x2) / (1 + k), (y1 y2 + x1 x2) / (1 - k)), k = d x1 x2 y1 y2: complete on the curve
inline HPoint hpoint_add(const HPoint& p, const HPoint& q) {
  const host::Field<4>& F = host::FR();
  const HFr x1y2 = host::mul(p.x, q.y, F), y1x2 = host::mul(p.y, q.x, F), y1y2 = host::mul(p.y, q.y, F), x1x2 = host::mul(p.x, q.x, F);
  const HFr k = host::mul(jubjub_d_host(), host::mul(x1y2, y1x2, F), F), one = host::one<4>(F);
  const HFr inv = host::inv(host::mul(host::add(one, k, F), host::sub(one, k, F), F), F);   // one inversion for both denominators
  return HPoint{host::mul(host::mul(host::add(x1y2, y1x2, F), host::sub(one, k, F), F), inv, F),
                host::mul(host::mul(host::add(y1y2, x1x2, F), host::add(one, k, F), F), inv, F)};
}
// canonical or Montgomery scalar in memory -> the integer below r; false: not below r
inline bool scalar_to_int(const uint64_t* s, uint32_t form, uint64_t (&out)[4]) {
  if (!hfr_canonical(s)) return false;
  if (form == PM_SCALAR_CANONICAL) {
    memcpy(out, s, 32);
    return true;
  }
  HFr one_int = host::zero<4>();
  one_int.l[0] = 1;                                         // x R * 1 / R = x
  const HFr v = host::mul(hfr_load(s), one_int, host::FR());
  memcpy(out, v.l, 32);
  return true;
}
// plain double-and-add from the top bit: NOT the device's algorithm
inline HPoint hpoint_mul(const HPoint& p, const uint64_t (&k)[4]) {
  HPoint acc = hpoint_identity();
  for (int i = 254; i >= 0; --i) {
    acc = hpoint_add(acc, acc);
    if ((k[i / 64] >> (i % 64)) & 1) acc = hpoint_add(acc, p);
  }
  return acc;
}
inline bool point_fault(const uint64_t* xy) { return !hfr_canonical(xy) || !hfr_canonical(xy + 4) || !hpoint_on_curve(hpoint_load(xy)); }

// ------------------------------------------------------------------ device side
// the scalar at p as four 64-bit words of the integer below r
PM_DEV void jj_load_scalar(const u32x4* p, bool montgomery, u64 (&k)[4]) {
  Fr f;
  if (montgomery) {
    f = fe_zero<FrP>();
    f.l[0] = 32u;           // x 2^256 * 2^5 / 2^261 = x
  } else {
    f = fe_one<FrP>();
  }
  u32 w[8];
  fe_canon_pack<FrP>(w, fe_mul<FrP>(fe_load<FrP>(p), f));
#pragma unroll
  for (int i = 0; i < 4; ++i) k[i] = (u64)w[2 * i] | ((u64)w[2 * i + 1] << 32);
}
PM_DEV void jj_shr4(u64 (&k)[4]) {
#pragma unroll
  for (int i = 0; i < 3; ++i) k[i] = (k[i] >> 4) | (k[i + 1] << 60);
  k[3] >>= 4;
}
PM_DEV void jj_shl4(u64 (&k)[4]) {
#pragma unroll
  for (int i = 3; i > 0; --i) k[i] = (k[i] << 4) | (k[i - 1] >> 60);
  k[0] <<= 4;
}
// the signed digit of nibble `nib` with carry `c` in; c becomes the carry out (the file comment)
PM_DEV int jj_digit(u32 nib, u32& c) {
  const u32 v = nib + c;
  c = v > 8u ? 1u : 0u;
  return (int)v - (c ? 16 : 0);
}
// bit w = the carry INTO digit w, for the walk from the top digit down
PM_DEV u64 jj_carries(u64 (&k)[4]) {
  u64 t[4] = {k[0], k[1], k[2], k[3]}, m = 0;
  u32 c = 0;
#pragma unroll 1
  for (u32 w = 0; w < JJ_WINDOWS; ++w) {
    m |= (u64)c << w;
    (void)jj_digit((u32)t[0] & 15u, c);
    jj_shr4(t);
  }
  return m;
}
PM_DEV Fr jj_limbs(const u32x4& a, const u32x4& b, u32 c) {
  Fr r;
  r.l[0] = a.x, r.l[1] = a.y, r.l[2] = a.z, r.l[3] = a.w, r.l[4] = b.x, r.l[5] = b.y, r.l[6] = b.z, r.l[7] = b.w, r.l[8] = c;
  return r;
}
PM_DEV EdPoint jj_neutral() { return EdPoint{fe_zero<FrP>(), fe_one<FrP>(), fe_one<FrP>(), fe_zero<FrP>()}; }
// acc += d * (entry |d| of window w of tab): entry e of window w sits at chunk (8 w + e - 1) * 7
PM_DEV EdPoint jj_fixed_step(const EdPoint& acc, const u32x4* tab, u32 w, int d, const Fr& ed) {
  const u32 mag = (u32)(d < 0 ? -d : d), e = mag == 0 ? 1u : (mag > 8u ? 8u : mag);
  const u32x4* p = tab + (size_t)(8 * w + e - 1) * JJ_ENTRY_CHUNKS;
  const u32x4 c0 = p[0], c1 = p[1], c2 = p[2], c3 = p[3], c4 = p[4], c5 = p[5], c6 = p[6];
  const Fr x = jj_limbs(c0, c1, c2.x);
  const Fr y = jj_limbs(u32x4{c2.y, c2.z, c2.w, c3.x}, u32x4{c3.y, c3.z, c3.w, c4.x}, c4.y);
  const Fr t = jj_limbs(u32x4{c4.z, c4.w, c5.x, c5.y}, u32x4{c5.z, c5.w, c6.x, c6.y}, c6.z);
  const Fr zero = fe_zero<FrP>(), one = fe_one<FrP>();
  const Fr ax = g_sel(d == 0, zero, g_sel(d < 0, gneg(x), x));
  const Fr ay = g_sel(d == 0, one, y);
  const Fr at = g_sel(d == 0, zero, g_sel(d < 0, gneg(t), t));
  return ed_madd(acc, ax, ay, at, ed);
}
// k B from the window table of B, the digits from the bottom up (the order of a sum being free): 64 ed_madd.  Consumes k.
PM_DEV EdPoint jj_fixed_walk(const u32x4* tab, u64 (&k)[4], const Fr& ed) {
  u32 c = 0;
  EdPoint acc = jj_neutral();
#pragma unroll 1
  for (u32 w = 0; w < JJ_WINDOWS; ++w) {
    acc = jj_fixed_step(acc, tab, w, jj_digit((u32)k[0] & 15u, c), ed);
    jj_shr4(k);
  }
  return acc;
}
// (X / Z, Y / Z) to element i of out when live: one inversion, two products (and the change of form); Z = 0 gives (0, 0)
PM_DEV void jj_store_affine(u32x4* out, size_t i, bool live, const EdPoint& p) {
  const Fr zi = g_to_abi(fe_inv_dev<FrP>(p.Z));             // every lane of the wave is here
  if (!live) return;
  st_canon(out, 2 * i, gmul(p.X, zi));                      // device x ABI -> ABI
  st_canon(out, 2 * i + 1, gmul(p.Y, zi));
}
// v, hidden from the optimiser: what it derives from a loop-invariant operand of a product it otherwise keeps in registers
// across the whole loop (the table build below then needs all 512 registers of a lone wave and scratch on top)
PM_DEV void jj_opaque(Fr& v) {
#pragma unroll
  for (int i = 0; i < 9; ++i) asm volatile("" : "+v"(v.l[i]));
}

// variable base: one thread's table: chunk c of entry e (e P, e = 1..8, X Y Z T as 36 limbs) at base[((e - 1) * 9 + c) * stride],
// base = scratch + thread, stride = the threads of the grid: the lanes of a wave read and write consecutive 16-byte chunks when
// they share a digit and stay aligned when they do not.  A bounded grid walks n in strides (the table is per thread in flight);
// every wave runs the same number of rounds with its lanes clamped, and an element is read before the same thread writes it,
// so out may be the points.
PM_DEV void jj_table_store(u32x4* base, size_t stride, u32 e, const EdPoint& p) {
  u32 l[36];
#pragma unroll
  for (int j = 0; j < 9; ++j) l[j] = p.X.l[j], l[9 + j] = p.Y.l[j], l[18 + j] = p.Z.l[j], l[27 + j] = p.T.l[j];
  u32x4* q = base + (size_t)(e - 1) * JJ_POINT_CHUNKS * stride;
#pragma unroll
  for (int c = 0; c < 9; ++c) q[c * stride] = u32x4{l[4 * c], l[4 * c + 1], l[4 * c + 2], l[4 * c + 3]};
}
PM_DEV EdPoint jj_table_load(const u32x4* base, size_t stride, u32 e) {
  u32 l[36];
  const u32x4* q = base + (size_t)(e - 1) * JJ_POINT_CHUNKS * stride;
#pragma unroll
  for (int c = 0; c < 9; ++c) {
    const u32x4 v = q[c * stride];
    l[4 * c] = v.x, l[4 * c + 1] = v.y, l[4 * c + 2] = v.z, l[4 * c + 3] = v.w;
  }
  EdPoint p;
#pragma unroll
  for (int j = 0; j < 9; ++j) p.X.l[j] = l[j], p.Y.l[j] = l[9 + j], p.Z.l[j] = l[18 + j], p.T.l[j] = l[27 + j];
  return p;
}
// the table of (px, py): e P = (e - 1) P + P, e = 1 .. 8
PM_DEV void jj_table_build(u32x4* tbl, size_t T, const Fr& px, const Fr& py, const Fr& ed) {
  const Fr pt = gmul(px, py);
  EdPoint acc{px, py, fe_one<FrP>(), pt};
  jj_table_store(tbl, T, 1, acc);
#pragma unroll 1
  for (u32 e = 2; e <= 8; ++e) {
    Fr x = px, y = py, t = pt;
    jj_opaque(x), jj_opaque(y), jj_opaque(t);
    acc = ed_madd(acc, x, y, t, ed);
    jj_table_store(tbl, T, e, acc);
  }
}
// k P over that table from the top digit down: `windows` windows of four doublings and an addition.  The top digit is the top
// nibble of k and bit 63 of carries the carry into it (jj_carries); a caller with fewer than JJ_WINDOWS digits shifts both up
// first.  Consumes k.
PM_DEV EdPoint jj_ladder(const u32x4* tbl, size_t T, u64 (&k)[4], u64 carries, u32 windows, const Fr& ed) {
  EdPoint acc = jj_neutral();
#pragma unroll 1
  for (u32 w = 0; w < windows; ++w) {
#pragma unroll 1
    for (u32 j = 0; j < 4; ++j) acc = ed_add(acc, acc, ed);
    u32 c = (u32)(carries >> 63);
    const int d = jj_digit((u32)(k[3] >> 60), c);
    jj_shl4(k);
    carries <<= 1;
    const u32 mag = (u32)(d < 0 ? -d : d), e = mag == 0 ? 1u : (mag > 8u ? 8u : mag);
    const EdPoint q = jj_table_load(tbl, T, e);
    const EdPoint s{g_sel(d < 0, gneg(q.X), q.X), q.Y, q.Z, g_sel(d < 0, gneg(q.T), q.T)};
    acc = ed_add(acc, ed_sel(d == 0, jj_neutral(), s), ed);
  }
  return acc;
}
// ONE scalar for every thread of the grid (a viewing key in cipher.hip, the order l in jubjub_codec.hip): its 64 signed digits
// are recoded once on the host -- the recoding of jj_digit, the top digit first -- and travel by value in the kernel's
// arguments, four signed bytes a word from the low end: whole words, so that digit w arrives by a scalar load (a byte would
// take a vector one).
inline void recode_digits(const uint64_t (&k)[4], signed char (&out)[JJ_WINDOWS]) {
  uint32_t c = 0;
  for (u32 w = 0; w < JJ_WINDOWS; ++w) {
    const uint32_t v = (uint32_t)((k[w / 16] >> (4 * (w % 16))) & 15u) + c;
    c = v > 8u ? 1u : 0u;
    out[JJ_WINDOWS - 1 - w] = (signed char)((int)v - (c ? 16 : 0));
  }
}
inline void recode_digit_words(const uint64_t (&k)[4], u32 (&words)[JJ_WINDOWS / 4]) {
  signed char digits[JJ_WINDOWS];
  recode_digits(k, digits);
  for (u32 w = 0; w < JJ_WINDOWS / 4; ++w) words[w] = 0;
  for (u32 w = 0; w < JJ_WINDOWS; ++w) words[w >> 2] |= (u32)(unsigned char)digits[w] << (8 * (w & 3u));
}
// k P over the table of jj_table_build under those digits, from the top one down.  Digit w is read at a wave-uniform index, so
// it lives in a scalar register: its sign and the zero digit are uniform branches, and there is no per-lane recoding, no shift
// of a per-lane scalar and no word of carries.  The doublings by the dedicated formula, T from the last of four only.
PM_DEV EdPoint jj_ladder_uniform(const u32x4* tbl, size_t T, const u32 (&digits)[JJ_WINDOWS / 4], const Fr& ed) {
  EdPoint acc = jj_neutral();
#pragma unroll 1
  for (u32 w = 0; w < JJ_WINDOWS; ++w) {
#pragma unroll 1
    for (u32 j = 0; j < 3; ++j) acc = ed_double<false>(acc);
    acc = ed_double<true>(acc);                              // the addition reads T
    const int d = (int)(signed char)(digits[w >> 2] >> (8 * (w & 3u)));
    if (d != 0) {                                            // uniform: a zero digit adds nothing
      const u32 mag = (u32)(d < 0 ? -d : d), e = mag > 8u ? 8u : mag;
      EdPoint q = jj_table_load(tbl, T, e);
      if (d < 0) q.X = gneg(q.X), q.T = gneg(q.T);           // uniform
      acc = ed_add(acc, q, ed);
    }
  }
  return acc;
}
// MANY scalars into the same point (the viewing keys of pm_poseidon_cipher_scan_keys_dev): the window table pm_jubjub_base keeps
// for a fixed base, built per thread for its own point -- entry 8 w + e - 1 = e 16^w P, w = 0 .. 63, e = 1 .. 8, X Y Z T in the
// layout of jj_table_store -- so that a scalar costs additions only and the doublings are paid once.  A window by five doublings
// and three additions: an even entry e B = 2 (e / 2 B) from the entry the thread stored itself, an odd one (e - 1) B + B, then
// 16 B = 2 (8 B), the next window's B.  The entries are made in a rolled loop, one formula each turn under a uniform branch:
// written out, the eight of a window are independent enough for the scheduler to hold most of them at once (4628 bytes of
// scratch a lane).  B is invariant in that loop; it is read back from entry 1 each odd turn, which keeps it out of the
// registers and, as jj_opaque does for jj_table_build, out of the optimiser's sight.
PM_DEV void jj_window_table_build(u32x4* tbl, size_t T, const Fr& px, const Fr& py, const Fr& ed) {
  EdPoint b{px, py, fe_one<FrP>(), gmul(px, py)};
#pragma unroll 1
  for (u32 w = 0; w < JJ_WINDOWS; ++w) {
    u32x4* const win = tbl + (size_t)w * 8 * JJ_POINT_CHUNKS * T;
    jj_table_store(win, T, 1, b);
    EdPoint acc = b;
#pragma unroll 1
    for (u32 e = 2; e <= 8; ++e) {
      const EdPoint q = jj_table_load(win, T, (e & 1u) ? 1u : e >> 1);   // B or e / 2 B: no second copy of B in registers
      if (e & 1u)                                            // uniform
        acc = ed_add(acc, q, ed);
      else
        acc = ed_double<true>(q);
      jj_table_store(win, T, e, acc);
    }
    b = ed_double<true>(acc);
  }
}
// k P over that table: 64 additions at the most, no doubling.  `digits`: the words of recode_digit_words in device memory, read
// at an address that is the same in every lane of the workgroup, so a digit, its sign and the zero test stay scalar as in
// jj_ladder_uniform.  The top digit comes first there; the order of a sum is free and the walk goes from window 0 up.
PM_DEV EdPoint jj_window_walk(const u32x4* tbl, size_t T, const u32* __restrict__ digits, const Fr& ed) {
  EdPoint acc = jj_neutral();
#pragma unroll 1
  for (u32 w = 0; w < JJ_WINDOWS; ++w) {
    const u32 at = JJ_WINDOWS - 1 - w;
    const int d = (int)(signed char)(digits[at >> 2] >> (8 * (at & 3u)));
    if (d != 0) {                                            // uniform: a zero digit adds nothing
      const u32 mag = (u32)(d < 0 ? -d : d), e = mag > 8u ? 8u : mag;
      EdPoint q = jj_table_load(tbl + (size_t)w * 8 * JJ_POINT_CHUNKS * T, T, e);
      if (d < 0) q.X = gneg(q.X), q.T = gneg(q.T);           // uniform
      acc = ed_add(acc, q, ed);
    }
  }
  return acc;
}
// the words of r, most significant first
constexpr u32 JJ_R_WORDS[8] = {0x73eda753u, 0x299d7d48u, 0x3339d808u, 0x09a1d805u, 0x53bda402u, 0xfffe5bfeu, 0xffffffffu, 0x00000001u};
PM_DEV bool jj_below_r(const u32x4& lo, const u32x4& hi) {
  const u32 w[8] = {hi.w, hi.z, hi.y, hi.x, lo.w, lo.z, lo.y, lo.x};
  bool below = false, decided = false;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    below = (!decided && w[j] < JJ_R_WORDS[j]) ? true : below;
    decided = decided || w[j] != JJ_R_WORDS[j];
  }
  return below;
}
// the canonical value of v (normalised, below 2 r) is zero
PM_DEV bool jj_is_zero(const Fr& v) {
  u32 s[8], any = 0;
  fe_canon_pack<FrP>(s, v);
#pragma unroll
  for (int j = 0; j < 8; ++j) any |= s[j];
  return any == 0;
}
// the point at p (x | y): both coordinates below r and on the curve; x and y in the device form whatever the answer
PM_DEV bool jj_point_ok(const u32x4* p, const Fr& ed, Fr& x, Fr& y) {
  const bool canonical = jj_below_r(p[0], p[1]) && jj_below_r(p[2], p[3]);
  x = g_to_dev(ld_canon(p, 0)), y = g_to_dev(ld_canon(p, 1));
  const Fr x2 = gmul(x, x), y2 = gmul(y, y);
  const Fr rhs = gadd(fe_one<FrP>(), gmul(gmul(x2, y2), ed));
  const bool on_curve = jj_is_zero(gsub(gsub(y2, x2), rhs));   // not under `canonical &&`: no branch around the test
  return canonical && on_curve;
}

// ------------------------------------------------------------------ argument checks
inline int form_fault(pm_ctx* ctx, uint32_t scalar_form) {
  if (scalar_form != PM_SCALAR_MONTGOMERY && scalar_form != PM_SCALAR_CANONICAL)
    return set_err(ctx, PM_ERR_BAD_ARG, "scalar_form must be PM_SCALAR_MONTGOMERY or PM_SCALAR_CANONICAL");
  return PM_OK;
}
inline int base_fault(pm_ctx* ctx, const pm_jubjub_base* b) {
  if (!b) return set_err(ctx, PM_ERR_BAD_ARG, "null base");
  if (b->device != ctx->device) return set_err(ctx, PM_ERR_BAD_ARG, "the base belongs to another device");
  return PM_OK;
}

// ------------------------------------------------------------------ a slot per thread in flight
// The calls whose threads keep a window table in memory (pm_jubjub_mul_dev, pm_schnorr_verify_dev, pm_poseidon_cipher_scan_dev)
// bound their grid -- eight workgroups of 64 a CU at the most -- and walk n in strides of its threads.
inline size_t slot_blocks(const pm_ctx* ctx, size_t n) {
  return std::max<size_t>(std::min<size_t>((n + 63) / 64, (size_t)std::max(ctx->num_cus, 1) * 8), 1);
}
// ... and allocate, per call, the slots of that grid ([entry][chunk][thread of the grid]) with a tail of control words behind
// them.  finish_call (context.h) releases it once the launches are on the stream.
struct SlotScratch {
  size_t blocks, stride;    // the grid and its threads
  size_t slot_bytes = 0;
  char* base = nullptr;
  SlotScratch(const pm_ctx* ctx, size_t n) : blocks(slot_blocks(ctx, n)), stride(blocks * 64) {}
  hipError_t alloc(size_t bytes_per_thread, size_t tail_bytes) {
    slot_bytes = stride * bytes_per_thread;
    return hipMalloc((void**)&base, slot_bytes + tail_bytes);
  }
  u32x4* slots() const { return (u32x4*)base; }
  unsigned long long* tail() const { return (unsigned long long*)(base + slot_bytes); }
};

}  // namespace pm
