// Plain host C++, no HIP calls: everything pm_jubjub_msm_dev (jubjub_msm.hip) decides before it
// launches -- the window width, the windows of a 256-bit word at that width, the buckets, the bounds every count and cursor
// is held to, and the workspace layout -- and the signed-window recoding itself, which the kernels and the host hook
// pm_test_jubjub_msm_digits compile from the same lines.
//
// Digits.  A scalar is any 256-bit word k.  Window w holds bits [c w, c w + c) (zero past bit 255); with the carry in,
// v = window + carry <= 2^c; v > 2^(c-1) gives the digit v - 2^c and carry 1, anything else the digit v and carry 0.  So
// |d| <= 2^(c-1), sum d_w 2^(c w) = k as integers, and with windows = ceil(257 / c) the top window holds at most c - 1 bits
// of k: its v is at most 2^(c-1) and nothing carries out of it -- for EVERY word, those >= r included.  A digit d != 0 lands
// in bucket |d| - 1 < 2^(c-1) of its window.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/plonk_mi355x.h"

#ifdef __HIPCC__
#define PM_JMSM_HD __host__ __device__ inline
#else
#define PM_JMSM_HD inline
#endif

namespace pm {

constexpr uint32_t JMSM_MIN_C = 4, JMSM_MAX_C = 16;   // what "jubjub_msm_window_bits" may force
constexpr uint32_t JMSM_SEG = 32;                     // (digit, point) pairs one thread of the accumulate sums
constexpr uint32_t JMSM_HEAVY = 16;                   // a bucket of more segments than this is summed by a whole wave
constexpr uint32_t JMSM_SCAN_TILE = 2048;             // buckets per workgroup of the scan: 256 threads x 8
constexpr uint32_t JMSM_RED_THREADS = 256;            // threads that share one window's running sums
constexpr uint32_t JMSM_POINT_BYTES = 144;            // X Y Z T, 36 limbs

// the rule: c = log2(n) - 1 between JMSM_MIN_C and 15, and 16 from 2^21 points on.  Every bucket is a thread of the accumulate
// and a window's running sums are split over JMSM_RED_THREADS, so wide windows cost parallel work, not a serial tail: up to
// 2^16 points the call is bound by latency (one ladder's worth of doublings in the final kernel, then the longest segment),
// and more, emptier buckets shorten the longest chain; from there on c = 15 keeps a bucket at 16 pairs or fewer for 2^18
// points and 64 for 2^20 (two segments).  Past that the pairs per bucket double with n and c = 16 halves them again: reasoned,
// not measured.  DESIGN.md section 7.2m has the sweep this rests on.
static inline uint32_t jubjub_msm_window_bits(size_t n, long opt_c) {
  if (opt_c) return (uint32_t)opt_c;
  uint32_t lg = 0;
  while (((size_t)1 << (lg + 1)) <= (n > 1 ? n : 1)) ++lg;
  if (lg >= 21) return JMSM_MAX_C;
  const long c = (long)lg - 1;
  return (uint32_t)(c < (long)JMSM_MIN_C ? JMSM_MIN_C : (c > 15 ? 15 : c));
}
// 256 bits and the carry out of bit 255
static inline uint32_t jubjub_msm_windows(uint32_t c) { return (257 + c - 1) / c; }

struct JubjubMsmPlan {
  uint32_t c, windows, buckets;    // window bits, windows of a scalar, buckets of a window: 2^(c-1)
  uint32_t batch, rows;            // rows = batch x windows bucket sets
  uint32_t total_buckets;          // rows x buckets
  uint32_t seg_buckets;            // buckets a thread of the window kernel walks
  uint32_t tiles;                  // workgroups of the scan
  uint64_t max_pairs;              // n x windows x batch: every digit non-zero
  uint64_t max_items;              // segments at most: max_pairs / JMSM_SEG + total_buckets
  // the workspace, byte offsets (every one a multiple of 16)
  size_t off_count, off_cursor, off_pair_off, off_item_off, off_tile_sums, off_pairs, off_partials, off_wsums, bytes;
};

inline size_t jmsm_round16(size_t v) { return (v + 15) / 16 * 16; }

// PM_OK, PM_ERR_BAD_ARG (batch = 0, a forced width outside JMSM_MIN_C .. JMSM_MAX_C) or PM_ERR_LENGTH: n > 2^31 - 1, more
// than 2^32 - 1 pairs or segments, or more than 2^28 buckets -- what the 32-bit offsets and the pairs' 31-bit point index
// cannot hold
static inline int jubjub_msm_plan(size_t n, uint32_t batch, long opt_c, JubjubMsmPlan* p) {
  if (batch == 0 || (opt_c != 0 && (opt_c < (long)JMSM_MIN_C || opt_c > (long)JMSM_MAX_C))) return PM_ERR_BAD_ARG;
  if (n > 0x7fffffffu) return PM_ERR_LENGTH;
  JubjubMsmPlan g{};
  g.c = jubjub_msm_window_bits(n, opt_c);
  g.windows = jubjub_msm_windows(g.c);
  g.buckets = 1u << (g.c - 1);
  g.batch = batch;
  const uint64_t rows = (uint64_t)batch * g.windows, total = rows * g.buckets;
  g.max_pairs = (uint64_t)n * rows;
  g.max_items = g.max_pairs / JMSM_SEG + total;
  if (total > (1ull << 28) || g.max_pairs > 0xffffffffull || g.max_items > 0xffffffffull) return PM_ERR_LENGTH;
  g.rows = (uint32_t)rows, g.total_buckets = (uint32_t)total;
  g.seg_buckets = g.buckets > JMSM_RED_THREADS ? g.buckets / JMSM_RED_THREADS : 1;
  g.tiles = (g.total_buckets + JMSM_SCAN_TILE - 1) / JMSM_SCAN_TILE;
  size_t at = 0;
  const auto take = [&at](size_t bytes) {
    const size_t o = at;
    at += jmsm_round16(bytes);
    return o;
  };
  g.off_count = take(4 * (size_t)total);               // count and cursor are adjacent: one memset
  g.off_cursor = take(4 * (size_t)total);
  g.off_pair_off = take(4 * ((size_t)total + 1));
  g.off_item_off = take(4 * ((size_t)total + 1));
  g.off_tile_sums = take(8 * (size_t)g.tiles);
  g.off_pairs = take(4 * (size_t)g.max_pairs);
  g.off_partials = take((size_t)JMSM_POINT_BYTES * (size_t)g.max_items);
  g.off_wsums = take((size_t)JMSM_POINT_BYTES * (size_t)rows);
  g.bytes = at;
  *p = g;
  return PM_OK;
}

// ------------------------------------------------------------------ the recoding (host and device)
template <class W>
PM_JMSM_HD void jmsm_shr(W (&k)[4], uint32_t c) {   // 0 < c < 64
  k[0] = (k[0] >> c) | (k[1] << (64 - c));
  k[1] = (k[1] >> c) | (k[2] << (64 - c));
  k[2] = (k[2] >> c) | (k[3] << (64 - c));
  k[3] >>= c;
}
// the digit of the low c bits of k with carry `cy` in; cy becomes the carry out
template <class W>
PM_JMSM_HD int32_t jmsm_digit(const W (&k)[4], uint32_t c, uint32_t& cy) {
  const uint32_t v = ((uint32_t)k[0] & ((1u << c) - 1)) + cy;
  cy = v > (1u << (c - 1)) ? 1u : 0u;
  return (int32_t)v - (cy ? (int32_t)(1u << c) : 0);
}
// emit(w, d) for the `windows` digits of k from the bottom up; returns the carry out of the last (0 at the plan's windows).
// W: a 64-bit unsigned word (the device's and the host's typedefs differ)
template <class W, class F>
PM_JMSM_HD uint32_t jmsm_for_each_digit(const W (&k)[4], uint32_t c, uint32_t windows, F&& emit) {
  W t[4] = {k[0], k[1], k[2], k[3]};
  uint32_t cy = 0;
  for (uint32_t w = 0; w < windows; ++w) {
    emit(w, jmsm_digit(t, c, cy));
    jmsm_shr(t, c);
  }
  return cy;
}

}  // namespace pm
