// Variable-base scalar multiplication in G1: k P for one point and one scalar per thread, by a signed fixed-window
// ladder, with or without the GLV endomorphism.  Shared by g1_mul.hip (pm_g1_scalar_mul_dev),
// ec_ntt.hip (the flagged Lagrange conversion) and test_hooks.hip.
//
// The split.  z = -0xd201000000010000 is the curve parameter, r = z^4 - z^2 + 1, and phi(x, y) = (beta x, y) with
// beta = 2^((p - 1) / 3) is multiplication by -z^2 on the order-r subgroup (g1_codec.hip tests membership with it).  So
// Q := (beta x, -y) = [z^2] P there, and because r - 1 = z^2 (z^2 - 1) exactly, a canonical k < r splits by a plain
// division:  k = k1 + k2 z^2  with  0 <= k1, k2 < z^2 < 2^128  and  k P = k1 P + k2 Q.  No lattice rounding, no signs.
// phi is a scalar multiplication ONLY on the subgroup: on any other curve point (the order-3 point (0, 2), say) the
// split gives a wrong answer, so callers choose xyzz_mul_glv only for points they know to be in the subgroup, and
// xyzz_mul_window (the same ladder over the whole 255-bit integer, valid for every curve point) otherwise.
//
// The ladder.  Window w = 4.  Adding 0x88..8 to the scalar turns its nibbles into signed digits: nibble_i(k + 0x88..8)
// - 8 is the digit d_i in [-8, 7], and the carry out of the top nibble is one more digit (0 or 1) above them -- the
// 33rd of a 128-bit half, the 65th of the 255-bit integer.  From the top digit down: four doublings, then add
// sign(d) T[|d|] (nothing for d = 0) for each half.  T[1..8] = P, 2P, .. 8P are built once per point.  A negative
// digit negates Y only (xyzz_neg); the Q-side entry is (beta X, -Y, ZZ, ZZZ) of the same table entry: one Fp product
// (beta is a reduced constant, the product is (1, <2): inside the X class) and the negation.
// GLV: 128 doublings and 2 x 33 digits (about 62 additions, 1/16 of the digits are zero) against 255 doublings and
// about 127 additions of the bitwise ladder; plain window: 256 doublings and about 61 additions.
//
// The table is NOT a register array (a runtime-indexed one goes to scratch): it is an explicit thread-private global
// buffer laid out [entry][16-byte chunk][thread], so the loads of a wave coalesce when its lanes share the digit (the
// uniform twiddles of the EC-NTT) and stay 16-byte aligned when they do not.  An entry is the 56 limbs of X, Y, ZZ, ZZZ
// in 14 chunks, the identity all zero (ZZ == 0, as in ld_xyzz):  8 entries x 224 bytes = 1792 bytes per point (per
// thread in flight: the kernels run a grid-stride loop over a bounded grid).
//
// Exceptional additions (acc == +-entry, identities) are the after-the-fact slow path of xyzz_add, as everywhere.  On
// subgroup points every partial sum a + b z^2 of the joint ladder lies in (0, r), so only identity operands occur; in
// the plain mode a point of small order meets P + P, P - P and identity table entries at almost every step.
#pragma once
#include "ec.hip.h"

namespace pm {

// ------------------------------------------------------------------ the split k = k1 + k2 z^2 (host and device)
struct GlvWords8 {
  u32 w[8];
};
struct GlvHalves {
  u32 k1[4], k2[4];
};
// z^2 and GLV_RECIP = floor(2^255 / z^2): the only constants of the division (checked below at compile time)
constexpr u32 GLV_Z2[4] = {0x00000000u, 0x00000001u, 0x0001a402u, 0xac45a401u};
constexpr u32 GLV_RECIP[4] = {0x7b67f717u, 0xb1fb7291u, 0xf00fd56eu, 0xbe35f678u};

// k < r as 8 saturated words -> (k mod z^2, floor(k / z^2)).  Barrett: q' = floor(k RECIP / 2^255) is q or q - 1
// (k RECIP / 2^255 lies in (k / z^2 - k / 2^255, k / z^2] and k < 2^255), so one conditional correction makes it exact.
// The remainder k - q' z^2 < 2 z^2 < 2^129 is computed modulo 2^160.
PM_HD GlvHalves glv_split_words(const GlvWords8& k) {
  u32 prod[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    u64 carry = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const u64 t = (u64)k.w[i] * GLV_RECIP[j] + prod[i + j] + carry;
      prod[i + j] = (u32)t;
      carry = t >> 32;
    }
    prod[i + 4] = (u32)carry;
  }
  u32 q[4] = {0, 0, 0, 0};
#pragma unroll
  for (int j = 0; j < 4; ++j) q[j] = (prod[7 + j] >> 31) | (prod[8 + j] << 1);
  // rem = k - q z^2 mod 2^160
  u32 t5[5] = {0, 0, 0, 0, 0};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    u64 carry = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (i + j < 5) {
        const u64 t = (u64)q[i] * GLV_Z2[j] + t5[i + j] + carry;
        t5[i + j] = (u32)t;
        carry = t >> 32;
      }
    }
    if (i == 0) t5[4] = (u32)carry;
  }
  u32 rem[5] = {0, 0, 0, 0, 0};
  u64 borrow = 0;
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    const u64 d = (u64)k.w[i] - t5[i] - borrow;
    rem[i] = (u32)d;
    borrow = (d >> 32) & 1u;
  }
  // rem >= z^2 ?  rem - z^2 over 5 words does not borrow
  u32 sub[5] = {0, 0, 0, 0, 0};
  borrow = 0;
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    const u64 d = (u64)rem[i] - (i < 4 ? GLV_Z2[i] : 0u) - borrow;
    sub[i] = (u32)d;
    borrow = (d >> 32) & 1u;
  }
  const bool fix = borrow == 0;
  GlvHalves h{};
  u64 inc = fix ? 1u : 0u;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    h.k1[i] = fix ? sub[i] : rem[i];
    const u64 s = (u64)q[i] + inc;
    h.k2[i] = (u32)s;
    inc = s >> 32;
  }
  return h;
}

namespace glv_check {
PM_HD bool halves_are(const GlvHalves& h, u32 a0, u32 a1, u32 a2, u32 a3, u32 b0, u32 b1, u32 b2, u32 b3) {
  return h.k1[0] == a0 && h.k1[1] == a1 && h.k1[2] == a2 && h.k1[3] == a3 && h.k2[0] == b0 && h.k2[1] == b1 && h.k2[2] == b2 &&
         h.k2[3] == b3;
}
// r - 1 = z^2 (z^2 - 1): the largest scalar gives k1 = 0, k2 = z^2 - 1 (this fails for a wrong z^2 or a wrong reciprocal)
constexpr GlvWords8 R_MINUS_1 = {{0x00000000u, 0xffffffffu, 0xfffe5bfeu, 0x53bda402u, 0x09a1d805u, 0x3339d808u, 0x299d7d48u, 0x73eda753u}};
static_assert(halves_are(glv_split_words(R_MINUS_1), 0, 0, 0, 0, GLV_Z2[0] - 1u, GLV_Z2[1] - 1u, GLV_Z2[2], GLV_Z2[3]), "r - 1 = z^2 (z^2 - 1)");
constexpr GlvWords8 Z2_AS_K = {{GLV_Z2[0], GLV_Z2[1], GLV_Z2[2], GLV_Z2[3], 0, 0, 0, 0}};
static_assert(halves_are(glv_split_words(Z2_AS_K), 0, 0, 0, 0, 1, 0, 0, 0), "z^2 = 0 + 1 z^2");
constexpr GlvWords8 Z2_MINUS_1 = {{0xffffffffu, 0x00000000u, GLV_Z2[2], GLV_Z2[3], 0, 0, 0, 0}};
static_assert(halves_are(glv_split_words(Z2_MINUS_1), 0xffffffffu, 0, GLV_Z2[2], GLV_Z2[3], 0, 0, 0, 0), "z^2 - 1 stays whole");
}  // namespace glv_check

// ------------------------------------------------------------------ device
PM_DEV void fr_glv_split(const u32 (&k)[8], u32 (&k1)[4], u32 (&k2)[4]) {
  GlvWords8 in;
#pragma unroll
  for (int i = 0; i < 8; ++i) in.w[i] = k[i];
  const GlvHalves h = glv_split_words(in);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    k1[i] = h.k1[i];
    k2[i] = h.k2[i];
  }
}

// scalar in memory (ABI Montgomery, R = 2^256, or the plain integer; below r) -> the canonical integer, 8 saturated words
PM_DEV void fr_load_canon(const u32x4* p, bool montgomery, u32 (&w)[8]) {
  Fr f;
  if (montgomery) {
    f = fe_zero<FrP>();
    f.l[0] = 32u;   // x 2^256 * 2^5 / 2^261 = x
  } else {
    f = fe_one<FrP>();
  }
  fe_canon_pack<FrP>(w, fe_mul<FrP>(fe_load<FrP>(p), f));
}

// -p with Y reduced first: Y (1+, <5) -> product (1, <2) -> 3p - Y (3, <3) -> normalised (1+, <3), in class
PM_DEV Xyzz xyzz_neg(const Xyzz& p) {
  Xyzz r = p;
  r.y = fe_norm<FpP>(fe_sub<FpP, 3, 1>(fe_zero<FpP>(), fe_mul<FpP>(p.y, fe_one<FpP>())));
  return r;
}

// beta = 2^((p - 1) / 3) (G1_BETA of g1_codec.hip) in the device form, beta 2^392 mod p, as 14 x 28-bit limbs
PM_DEV Fp glv_beta() {
  constexpr u32 B[14] = {0xa75929au, 0x681b798u, 0x22a3e9du, 0xabc02bfu, 0x4e5bb45u, 0x55e6e7eu, 0x4814117u,
                         0x6d04f1bu, 0xae3387du, 0x54acb0cu, 0x0a4c74bu, 0x56138b5u, 0xb64e066u, 0x00076f2u};
  Fp r;
#pragma unroll
  for (int i = 0; i < 14; ++i) r.l[i] = B[i];
  return r;
}

constexpr int MUL_WINDOW = 4;                      // bits per digit
constexpr int MUL_TABLE_ENTRIES = 1 << (MUL_WINDOW - 1);   // T[1..8]
constexpr int MUL_ENTRY_CHUNKS = 14;               // 56 limbs as 16-byte chunks
constexpr size_t MUL_TABLE_BYTES = (size_t)MUL_TABLE_ENTRIES * MUL_ENTRY_CHUNKS * 16;   // per thread: 1792

// One thread's view of the table buffer: chunk c of entry e is at base[(e * 14 + c) * stride], base = buffer + thread,
// stride = threads of the grid.
struct MulTable {
  u32x4* base;
  size_t stride;
};

PM_DEV void mul_table_store(const MulTable& t, u32 e, const Xyzz& v) {
  u32x4* p = t.base + (size_t)e * MUL_ENTRY_CHUNKS * t.stride;
  if (v.inf) {
    const u32x4 z = u32x4{0u, 0u, 0u, 0u};
#pragma unroll
    for (int c = 0; c < MUL_ENTRY_CHUNKS; ++c) p[c * t.stride] = z;
    return;
  }
  u32 l[56];
#pragma unroll
  for (int i = 0; i < 14; ++i) {
    l[i] = v.x.l[i];
    l[14 + i] = v.y.l[i];
    l[28 + i] = v.zz.l[i];
    l[42 + i] = v.zzz.l[i];
  }
#pragma unroll
  for (int c = 0; c < MUL_ENTRY_CHUNKS; ++c) p[c * t.stride] = u32x4{l[4 * c], l[4 * c + 1], l[4 * c + 2], l[4 * c + 3]};
}
PM_DEV Xyzz mul_table_load(const MulTable& t, u32 e) {
  const u32x4* p = t.base + (size_t)e * MUL_ENTRY_CHUNKS * t.stride;
  u32 l[56];
#pragma unroll
  for (int c = 0; c < MUL_ENTRY_CHUNKS; ++c) {
    const u32x4 v = p[c * t.stride];
    l[4 * c] = v.x;
    l[4 * c + 1] = v.y;
    l[4 * c + 2] = v.z;
    l[4 * c + 3] = v.w;
  }
  Xyzz r;
  u32 z = 0;
#pragma unroll
  for (int i = 0; i < 14; ++i) {
    r.x.l[i] = l[i];
    r.y.l[i] = l[14 + i];
    r.zz.l[i] = l[28 + i];
    r.zzz.l[i] = l[42 + i];
    z |= l[28 + i];
  }
  r.inf = (z == 0);
  return r;
}

// k += 0x88..8 over NW words: nibble i of the sum minus 8 is the signed digit d_i in [-8, 7]; returns the carry, the
// digit above the top nibble (0 or 1)
template <int NW>
PM_DEV u32 mul_recode(u32 (&k)[NW]) {
  u64 c = 0;
#pragma unroll
  for (int i = 0; i < NW; ++i) {
    const u64 s = (u64)k[i] + 0x88888888u + c;
    k[i] = (u32)s;
    c = s >> 32;
  }
  return (u32)c;
}

// The ladder over recoded digits: a (carry ca) multiplies P, and with GLV b (carry cb) multiplies Q = (beta x, -y).
// One site each for the doubling and for the addition (the digit loop and the two sides are rolled): the code is the size
// of the bitwise ladder's.  a and b are consumed (shifted out from the top).
template <int NW, bool GLV>
PM_DEV Xyzz xyzz_mul_digits(const Xyzz& p, u32 (&a)[NW], u32 ca, u32 (&b)[NW], u32 cb, const MulTable& t) {
  Xyzz acc = xyzz_identity();
  if (p.inf) return acc;
  {
    mul_table_store(t, 0, p);
    Xyzz cur = xyzz_double(p);
    mul_table_store(t, 1, cur);
#pragma unroll 1
    for (u32 e = 2; e < (u32)MUL_TABLE_ENTRIES; ++e) {
      cur = xyzz_add(cur, p);   // P + P, P - P for points of order 2, 3: the slow path
      mul_table_store(t, e, cur);
    }
  }
  constexpr int NDIG = NW * 32 / MUL_WINDOW;
#pragma unroll 1
  for (int step = 0; step <= NDIG; ++step) {   // step 0: the carry digits, nothing to double yet
#pragma unroll 1
    for (int i = 0; i < MUL_WINDOW; ++i) acc = xyzz_double(acc);
#pragma unroll 1
    for (int side = 0; side < (GLV ? 2 : 1); ++side) {
      int d;
      if (step == 0)
        d = (int)(side ? cb : ca);
      else
        d = (int)((side ? b[NW - 1] : a[NW - 1]) >> (32 - MUL_WINDOW)) - (1 << (MUL_WINDOW - 1));
      if (d != 0) {   // digit 0 adds nothing
        const u32 m = (u32)(d < 0 ? -d : d);
        Xyzz e = mul_table_load(t, m - 1);
        if (side) e.x = fe_mul<FpP>(e.x, glv_beta());   // X (1+, <10) x beta (1, <1) -> (1, <2)
        if ((d < 0) != (side != 0)) e = xyzz_neg(e);     // -|d| P, or +|d| Q = (beta X, -Y)
        acc = xyzz_add(acc, e);
      }
    }
    if (step) {
#pragma unroll
      for (int i = NW - 1; i > 0; --i) {
        a[i] = (a[i] << MUL_WINDOW) | (a[i - 1] >> (32 - MUL_WINDOW));
        if (GLV) b[i] = (b[i] << MUL_WINDOW) | (b[i - 1] >> (32 - MUL_WINDOW));
      }
      a[0] <<= MUL_WINDOW;
      if (GLV) b[0] <<= MUL_WINDOW;
    }
  }
  return acc;
}

// k1 P + k2 Q, Q = (beta x, -y) = [z^2] P: k P for k = k1 + k2 z^2 and P IN THE ORDER-r SUBGROUP (or the identity);
// undefined for any other point.  k1, k2 < 2^128 from fr_glv_split.
PM_DEV Xyzz xyzz_mul_glv(const Xyzz& p, const u32 (&k1)[4], const u32 (&k2)[4], const MulTable& t) {
  u32 a[4], b[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    a[i] = k1[i];
    b[i] = k2[i];
  }
  const u32 ca = mul_recode<4>(a), cb = mul_recode<4>(b);
  return xyzz_mul_digits<4, true>(p, a, ca, b, cb, t);
}

// k P for any curve point P and k < 2^256 (8 saturated words)
PM_DEV Xyzz xyzz_mul_window(const Xyzz& p, const u32 (&k)[8], const MulTable& t) {
  u32 a[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) a[i] = k[i];
  const u32 ca = mul_recode<8>(a);
  return xyzz_mul_digits<8, false>(p, a, ca, a, 0u, t);
}

// the routine the kernels are templates on
template <bool GLV>
PM_DEV Xyzz xyzz_mul_table(const Xyzz& p, const u32 (&k)[8], const MulTable& t) {
  if constexpr (GLV) {
    u32 k1[4], k2[4];
    fr_glv_split(k, k1, k2);
    return xyzz_mul_glv(p, k1, k2, t);
  } else {
    return xyzz_mul_window(p, k, t);
  }
}
}  // namespace pm
