// Integers modulo l, the order of JubJub's prime subgroup, on the device: what u = k - c sk of a Schnorr signature lives in
// (schnorr.hip).  Plain 64-bit C++ on four words, one value per lane, NOT a third parameter set of
// fields.hip.h: a signature needs three products modulo l against some 520 modulo r, so the carry-free 29-bit form would buy
// nothing and its Consts<> would be instantiated for one call site.
//
// scl_mont(a, b) = a b / 2^256 mod l (coarsely integrated operand scanning, as host::mul).  Bound: a b < l 2^256, then
// (a b + q l) / 2^256 < 2 l < 2^253 fits four words and ONE conditional subtraction makes it canonical (< l).  The callers:
//   scl_reduce(a)        a < r < 2^255:       a (2^256 mod l) < 2^255 l                     -> a mod l
//   scl_mulsub(a, b, c)  b < 2^255, c < 2^250: b c < 2^505 < l 2^256 (l > 2^251), then t < l times 2^512 mod l < l
//                                                                                           -> (a - b c) mod l, a < r
// The host restatement (host_field.h, mod_l / mulsub_l) is long division; tests/test_schnorr_host.py and
// tests/test_gpu_schnorr.py hold both against Python's %.
#pragma once
#include "fields.hip.h"

namespace pm {

constexpr u64 SCL_L[4] = {0xd0970e5ed6f72cb7ull, 0xa6682093ccc81082ull, 0x06673b0101343b00ull, 0x0e7db4ea6533afa9ull};
constexpr u64 SCL_R1[4] = {0x25f80bb3b99607d9ull, 0xf315d62f66b6e750ull, 0x932514eeeb8814f4ull, 0x09a6fc6f479155c6ull};   // 2^256 mod l
constexpr u64 SCL_R2[4] = {0x67719aa495e57731ull, 0x51b0cef09ce3fc26ull, 0x69dab7fac026e9a5ull, 0x04f6547b8d127688ull};   // 2^512 mod l
constexpr u64 SCL_NINV = 0x1ba3a358ef788ef9ull;                                                                             // -1 / l mod 2^64

// a b + t + c as (low word, hi): at most (2^64 - 1)^2 + 2 (2^64 - 1) = 2^128 - 1
PM_DEV u64 scl_mac(u64 a, u64 b, u64 t, u64 c, u64& hi) {
  u64 lo = a * b;
  hi = __umul64hi(a, b);
  lo += t;
  hi += lo < t ? 1u : 0u;
  lo += c;
  hi += lo < c ? 1u : 0u;
  return lo;
}
// a - b, the borrow out
PM_DEV u64 scl_sub(u64 (&r)[4], const u64 (&a)[4], const u64 (&b)[4]) {
  u64 bw = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const u64 d = a[i] - b[i], e = d - bw;
    bw = (a[i] < b[i] || d < bw) ? 1u : 0u;
    r[i] = e;
  }
  return bw;
}
PM_DEV bool scl_below_l(const u64 (&a)[4]) {
  u64 d[4];
  const u64 l[4] = {SCL_L[0], SCL_L[1], SCL_L[2], SCL_L[3]};
  return scl_sub(d, a, l) != 0;
}
// a b / 2^256 mod l, canonical; a b < l 2^256 (the file comment)
PM_DEV void scl_mont(u64 (&r)[4], const u64 (&a)[4], const u64 (&b)[4]) {
  u64 t[6] = {0, 0, 0, 0, 0, 0};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    u64 c = 0, hi;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      t[j] = scl_mac(a[j], b[i], t[j], c, hi);
      c = hi;
    }
    u64 s = t[4] + c;
    t[5] = s < c ? 1u : 0u;
    t[4] = s;
    const u64 q = t[0] * SCL_NINV;
    (void)scl_mac(q, SCL_L[0], t[0], 0, hi);
    c = hi;
#pragma unroll
    for (int j = 1; j < 4; ++j) {
      t[j - 1] = scl_mac(q, SCL_L[j], t[j], c, hi);
      c = hi;
    }
    s = t[4] + c;
    t[3] = s;
    t[4] = t[5] + (s < c ? 1u : 0u);
  }
  const u64 v[4] = {t[0], t[1], t[2], t[3]}, l[4] = {SCL_L[0], SCL_L[1], SCL_L[2], SCL_L[3]};
  u64 d[4];
  const bool below = scl_sub(d, v, l) != 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) r[i] = below ? v[i] : d[i];
}
// a mod l for a < 2^255
PM_DEV void scl_reduce(u64 (&r)[4], const u64 (&a)[4]) {
  const u64 r1[4] = {SCL_R1[0], SCL_R1[1], SCL_R1[2], SCL_R1[3]};
  scl_mont(r, a, r1);
}
// (a - b c) mod l for a, b < 2^255 and c < 2^250
PM_DEV void scl_mulsub(u64 (&r)[4], const u64 (&a)[4], const u64 (&b)[4], const u64 (&c)[4]) {
  const u64 r2[4] = {SCL_R2[0], SCL_R2[1], SCL_R2[2], SCL_R2[3]}, l[4] = {SCL_L[0], SCL_L[1], SCL_L[2], SCL_L[3]};
  u64 t[4], p[4], ar[4], d[4], e[4];
  scl_mont(t, b, c);        // b c / 2^256
  scl_mont(p, t, r2);       // b c mod l
  scl_reduce(ar, a);
  const bool borrow = scl_sub(d, ar, p) != 0;
  // d + l when a mod l < b c mod l: the sum wraps past 2^256 back to the difference in [0, l)
  u64 cy = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const u64 s = d[i] + l[i], s2 = s + cy;
    cy = (s < d[i] || s2 < s) ? 1u : 0u;
    e[i] = s2;
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) r[i] = borrow ? e[i] : d[i];
}

}  // namespace pm
