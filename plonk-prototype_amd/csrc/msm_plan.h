// Plain host C++, no HIP calls: everything the MSM driver decides before it launches -- the bucket-fill geometry
// (MsmGeom, shared with the kernels of msm_sort.hip.h, which take it by value), the accumulate levels and the level-1
// chunk, the bucket-reduction levels, who applies the weights, the launch geometry that follows from these and the
// workspace layout.  msm_run (msm.hip) builds an MsmPlan per piece shape and sizes its buffers from it; msm_enqueue
// launches from it and takes no decision of its own.  pm_test_msm_plan / pm_test_msm_sizing show the plan to CPU tests.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "../../include/plonk_mi355x.h"

#ifdef __HIPCC__
#define PM_PLAN_HD __host__ __device__
#else
#define PM_PLAN_HD
#endif

namespace pm {

typedef uint32_t u32;

#ifndef SORT_T1
#define SORT_T1 1024
#endif
static constexpr u32 SORT_THREADS1 = SORT_T1;    // scatter kernel: threads = scalars per tile at most
static constexpr u32 SORT_TILE1_PAIRS = 14 * SORT_THREADS1;   // scatter kernel: pairs staged per tile (8 B each in LDS)
static constexpr u32 SORT_MAX_BINS = 4096;       // partitions one MSM of a batch may have (LDS histogram of a tile)
static constexpr u32 SORT_MAX_RBITS = 12;        // local bins: 2^R counters + 2^R cursors in LDS

// the bucket reduction's shape (msm_bucket_reduce_kernel and its followers in msm.hip)
static constexpr u32 GROUP = 32;                 // items per wave in the reduction: one per lane PAIR (ec.hip.h, struct Half)
static constexpr u32 PLANES = 5;                 // log2 GROUP: bit planes one butterfly leaves
static constexpr u32 RED_WAVES = 4;              // waves per workgroup in level 1: one per SIMD of the CU

struct MsmGeom {
  u32 c;         // window bits
  u32 nwin;      // digit windows
  u32 nsets;     // bucket sets per MSM: nwin, or 1 when the bases carry a table of 2^(c w) P
  u32 batch;     // MSMs sharing the bases in this launch sequence (their sets are laid side by side)
  u32 bbits;     // c - 1: bits of the bucket field
  u32 nbuckets;  // 1 << bbits per set
  u32 trash;     // first key that is not a bucket (nsets * batch << bbits)
  u32 row_stride;  // table mode: points per table row (value = window * row_stride + index)
  // the sort plan
  u32 pbits;     // P: bits of the bucket index that select the partition
  u32 rbits;     // R = bbits - P: bits left for the local sort
  u32 sa;        // table mode: the buckets below a_size (the short TOP window's digits land there, on top of every
  u32 a_size;    //   other window's share) are cut into partitions 2^sa times narrower; 0 = one width everywhere
  u32 na;        // partitions below a_size
  u32 na_off;    // na - (a_size >> R): what the narrow region adds to the partition index of the rest
  u32 pps;       // partitions per bucket set: (1 << P) + na_off
  u32 bins;      // partitions per MSM of the batch: nsets * pps
  u32 np;        // partitions in all: batch * bins
  u32 ts;        // scalars per tile of the histogram / scatter kernels
  u32 tiles;     // tiles per MSM of the batch
  u32 ctl_cap;   // partitions the control block is laid out for (>= np; fixed per allocation, set by the caller)
};

// window bits of an MSM over n points (the option's, by size, or the table's: fixed when the table was built), and the
// digit windows of a 256-bit scalar at that width
static inline u32 msm_window_bits(size_t n, long opt_c, u32 table_c) {
  u32 lg = 0;
  while (((size_t)1 << (lg + 1)) <= (n > 1 ? n : 1)) ++lg;
  long c = opt_c ? opt_c : (lg < 9 ? 5 : (lg > 20 ? 16 : (long)lg - 4));
  if (table_c) c = table_c;  // fixed when the table was built
  return (u32)c;
}
static inline u32 msm_windows(u32 c) { return (256 + c - 1) / c; }

static inline MsmGeom make_geom(size_t n, long opt_c, u32 table_c, size_t table_stride, u32 batch) {
  MsmGeom g;
  g.c = msm_window_bits(n, opt_c, table_c);
  g.nwin = msm_windows(g.c);
  g.nsets = table_c ? 1u : g.nwin;
  g.batch = batch;
  g.bbits = g.c - 1;
  g.nbuckets = 1u << g.bbits;
  g.trash = (g.nsets * batch) << g.bbits;
  g.row_stride = (u32)table_stride;
  // partitions of ~13 K pairs (one tile of the local sort with room for the spread of uniform digits), as long as a
  // tile of the scatter kernel still writes runs of several pairs per partition
  const size_t per_set = table_c ? n * g.nwin : n;
  u32 p = 0;
  while (p < g.bbits && (per_set >> p) > 13500) ++p;
  const u32 p_min = g.bbits > SORT_MAX_RBITS ? g.bbits - SORT_MAX_RBITS : 0u;
  u32 p_max = 10;
  while (p_max > p_min && (g.nsets << p_max) > SORT_MAX_BINS) --p_max;
  if (p > p_max) p = p_max;
  if (p < p_min) p = p_min;
  g.pbits = p;
  g.rbits = g.bbits - p;
  // With the window table every window feeds ONE bucket set, and the top window is short (c = 20: 16 bits, digits
  // below 2^15 of 2^19 buckets): the low buckets carry (windows - 1) / 2^bbits + 1 / 2^tb of the pairs each instead
  // of (windows - 1) / 2^bbits -- 2.3 times the others for c = 20, 24 times for c = 22.  Partitions of equal width
  // would make 64 (c = 22: 8) workgroups of the local sort run two (ten) tiles while the rest run one; the low
  // region is cut 2^sa times finer instead, so that every partition holds about the same number of pairs.
  g.sa = g.a_size = g.na = g.na_off = 0;
  if (table_c && g.nwin > 1 && p >= 1) {
    const u32 tbits = 256 - g.c * (g.nwin - 1);   // bits of the top window; the scalar is below 2^255
    if (tbits < g.c && tbits >= 2 && tbits - 1 >= g.rbits) {
      const u32 tb = tbits - 1;
      const double ratio = 1.0 + (double)(1u << (g.bbits - tb)) / (double)(g.nwin - 1);
      u32 sa = 0;
      while (ratio / (double)(1u << sa) > 1.18 && sa < g.rbits) ++sa;
      if (sa) {
        g.sa = sa;
        g.a_size = 1u << tb;
        g.na = g.a_size >> (g.rbits - sa);
        g.na_off = g.na - (g.a_size >> g.rbits);
      }
    }
  }
  g.pps = (1u << p) + g.na_off;
  g.bins = g.nsets * g.pps;
  g.np = batch * g.bins;
  g.ts = SORT_TILE1_PAIRS / g.nwin < SORT_THREADS1 ? SORT_TILE1_PAIRS / g.nwin : SORT_THREADS1;
  g.tiles = (u32)((n + g.ts - 1) / g.ts);
  g.ctl_cap = g.np;
  return g;
}

// partition of a bucket inside its set, and back: first bucket and bucket-index bits of a partition
PM_PLAN_HD inline u32 part_of(const MsmGeom& g, u32 bucket) {
  return bucket < g.a_size ? bucket >> (g.rbits - g.sa) : g.na_off + (bucket >> g.rbits);
}
PM_PLAN_HD inline void part_range(const MsmGeom& g, u32 pl, u32& first_bucket, u32& bits) {
  if (pl < g.na) {
    bits = g.rbits - g.sa;
    first_bucket = pl << bits;
  } else {
    bits = g.rbits;
    first_bucket = (pl - g.na_off) << bits;
  }
}

// ------------------------------------------------------------------ the plan of one piece
// what the plan reads from the context: the options "msm_window_bits", "msm_chunk", "msm_lb" (0 = the library's choice)
// and the device's compute units
struct MsmTune {
  long window_bits, chunk, lb;
  unsigned num_cus;
};

// Every accumulate level shrinks its list to two slots per 64 entries, so a pair count that fits a size_t is down to one
// wave after thirteen levels; the bucket reduction has at most three follow-up levels (msm_plan refuses more of either).
static constexpr u32 MSM_MAX_LEVELS = 16, MSM_MAX_RED_LEVELS = 3;

// byte offsets into the device workspace of one piece (each aligned to 256)
struct MsmLayout {
  // bucket fill: integer scalars + per-tile count rows (histogram -> scatter), partitioned pairs, sorted keys / values
  size_t canon, rows, pairs, keys1, vals1;
  size_t buckets;
  size_t pkeys[MSM_MAX_LEVELS], ppts[MSM_MAX_LEVELS];   // the partial list accumulate level i reads (i >= 1)
  size_t heads;                                         // level 1's parked heads, one slot per thread
  // level 1 writes 7 sequences of one record per wave, every further level 5 sequences more of one record per group;
  // the last one writes to win (sequence-major: nsets_all x host_items records per sequence), which the host reads
  size_t l1, lvl[MSM_MAX_RED_LEVELS], win;
  size_t fin;                                           // msm_reduce_finish_kernel's one record per set
};

struct MsmPlan {
  size_t n;          // points per MSM
  MsmGeom g;         // (g.batch: the MSMs of the piece)
  size_t m;          // (key, value) pairs at most: one per non-zero digit
  u32 nsets_all;     // bucket sets of the piece: g.nsets * batch
  // bucket fill
  u32 tiles_per_wg, wgs_per_msm;   // histogram kernel: batch * wgs_per_msm workgroups
  u32 scatter_wgs;
  // accumulate: lv[0] is level 1 (sorted pairs, `chunk` entries per thread), the rest read partial lists
  struct Level {
    size_t len;   // entries read at this level
    u32 chunk, offset;
    u32 blocks, threads;   // the launch
  };
  Level lv[MSM_MAX_LEVELS];
  u32 n_levels;
  size_t l1_threads;     // threads level 1 is sized for (every digit non-zero)
  u32 chunk_lo;          // the shortest chunk the histogram kernel may choose for a sparse input
  u32 chunk_arg;         // what the histogram kernel is handed: the option's chunk, else chunk_lo
  size_t place_lds;      // level 1: LDS request that places one (81 KB) or two (54 KB) waves per SIMD; 0 = plain grid
  // bucket reduction
  u32 lb, log_lb;        // buckets per lane pair in level 1
  u32 n1;                // waves per set in level 1
  u32 n_dev;             // follow-up levels, groups[k] groups per set each
  u32 groups[MSM_MAX_RED_LEVELS];
  u32 host_items;        // items per set and sequence that are left for the fold
  u32 n_seq_host;        // sequences the fold receives: 7 + 5 n_dev
  u32 nplanes;           // bit planes among them: 5 (n_dev + 1)
  bool use_finish;       // the device applies the weights (msm_reduce_finish_kernel) and the host gets one record per set
  MsmLayout at;
  size_t ws_bytes, pinned_bytes;
};

static inline size_t msm_align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// The plan of one piece: `batch` MSMs of n points over bases that carry a table of width table_c (0: none; bases_n points
// per table row).  PM_OK, or PM_ERR_BAD_ARG with *why set (then *out holds the geometry and nothing else).
static inline int msm_plan(size_t n, size_t bases_n, unsigned batch, unsigned table_c, const MsmTune& tune, MsmPlan* out,
                           const char** why) {
  MsmPlan& P = *out;
  P = MsmPlan();
  P.n = n;
  const MsmGeom g = P.g = make_geom(n, tune.window_bits, table_c, bases_n, batch);
  auto refuse = [&](const char* text) {   // the geometry stays: it says which shape was refused
    P = MsmPlan();
    P.n = n, P.g = g;
    *why = text;
    return PM_ERR_BAD_ARG;
  };
  if (g.bins > SORT_MAX_BINS || g.rbits > SORT_MAX_RBITS || g.ts == 0)
    return refuse("window width outside what the bucket fill is laid out for");
  const size_t m = P.m = n * batch * g.nwin;  // (key, value) pairs at most: one per non-zero digit
  const u32 nsets_all = P.nsets_all = g.nsets * batch;
  // Entries per thread in the big kernel (measured, profiles/r01_msm_sweep.txt, r02_msm_sweep.txt): about
  // four times the mean run length m / #buckets when the grid allows it (then a run is split over at
  // most two neighbouring lanes and the in-wave join costs one addition), at least 128, and never so
  // long that the grid drops below 2^17 threads; small inputs end up with chunks shorter than a run
  // and pay up to six additions per wave in the segmented scan instead.
  // The kernel holds two waves per SIMD, i.e. `slots` threads at a time, and every thread does the same work: a grid
  // of 3.25 x slots threads (a batch of four MSMs with 128-entry chunks) runs as four rounds, the last one a quarter
  // full.  So the grid is a whole number of rounds and the chunk follows from it (batch of four: 104 entries, as for
  // a single MSM; measured: 2.55 -> 2.3 ms of accumulate per MSM in a batch).
  const size_t avg_run = std::max<size_t>(1, m / ((size_t)g.nbuckets * nsets_all));
  const size_t slots = (size_t)tune.num_cus * 4 * 2 * 64;
  const size_t want = std::max<size_t>(128, 4 * avg_run);
  const size_t rounds = std::max<size_t>(1, (m + slots * want - 1) / (slots * want));
  // Small inputs (the commit rounds of a 2^10 .. 2^14-gate circuit) fill a fraction of one round and the kernel's time is
  // the length of one thread's chain: the chunk goes down to 12 entries, and to 4 where the runs are that short -- below
  // ~0.6 of a run the in-wave join pays for what the chain saves (profiles/r03_small_msm.txt: batch of four at 2^14,
  // accumulate 434 -> 365 us; at 2^10, 185 -> 108 us)
  u32 chunk_lo = (u32)std::min<size_t>(12, std::max<size_t>(4, (6 * avg_run + 9) / 10));
  u32 L1 = tune.chunk ? (u32)tune.chunk : (u32)std::max<size_t>(chunk_lo, (m + rounds * slots - 1) / (rounds * slots));
  // r05: while the whole grid fits ONE wave per SIMD -- placed exactly, below -- a thread's time is its chain: chunk mixed
  // additions at a lone wave's ~11.8 us each, then the in-wave join, one general addition (~16.5 us) per doubling of the lanes
  // a run is spread over.  The chunk that minimises that sum (profiles/r05_small_msm.txt: 2^12 points, one vector: 12 -> 5
  // entries, accumulate 174 -> 131 us)
  const size_t lone_waves = (size_t)tune.num_cus * 4;
  if (!tune.chunk) {
    double best = 1e30;
    for (u32 L = 2; L <= 16; ++L) {
      const size_t waves = ((m + L - 1) / L + 63) / 64;
      if (waves > lone_waves) continue;
      const double span = (double)avg_run / L + 1.0;
      const double cost = 11.8 * L + 16.5 * std::ceil(std::log2(span));
      if (cost < best) {
        best = cost;
        L1 = L;
        chunk_lo = std::min<u32>(chunk_lo, L);
      }
    }
  }
  // Partial lists: every level leaves two slots per WAVE; the deeper levels take one slot per lane, so
  // the list shrinks by 32 per level and ends in a single wave (final level).
  u32& n_levels = P.n_levels;
  P.lv[n_levels++] = {m, L1, 0, 0, 0};
  {
    size_t nthr = (m + L1 - 1) / L1;
    while (nthr > 1) {
      if (n_levels == MSM_MAX_LEVELS) return refuse("internal: more accumulate levels than the plan holds");
      const size_t len = 2 * ((nthr + 63) / 64);
      P.lv[n_levels++] = {len, 1, 1, 0, 0};
      nthr = len + 1;            // one lane per slot, shifted by one
      if (nthr <= 64) break;     // a single wave: final
    }
  }
  P.chunk_lo = chunk_lo;
  P.chunk_arg = tune.chunk ? L1 : chunk_lo;
  const size_t l1_threads = P.l1_threads = (m + L1 - 1) / L1;
  const size_t total_buckets = (size_t)g.nbuckets * nsets_all;
  // Buckets per lane pair in level 1 of the reduction (a power of two).  A pair does 2 LB + 5 group operations and the
  // kernel runs ONE wave per SIMD (section 4 of msm.hip): waves beyond 4 per CU queue for a second round.  Every further
  // level is a launch of ~5 dependent operations, and the host fold pays per sequence and item it receives.  LB is the
  // candidate with the smallest estimate of the three together (us; the constants are measured: profiles/r04_small_msm.txt
  // -- 2^19 buckets: 16, a batch of four: 64, an 8-way shard's 2^15: 1, four sets of 2^12: 4).
  // The host takes over when at most HOST_ITEMS items per set are left: a launch that folds two or three items is a
  // ~55 us chain on one wave, the same fold is a handful of additions (~1 us each) in the host fold (msm_fold).
  constexpr u32 HOST_ITEMS = 4;
  struct RedPlan {
    u32 lb, n1, host_items;
    std::vector<u32> groups;
    double est;
  };
  auto red_plan = [&](u32 lb) {
    RedPlan p;
    p.lb = lb;
    p.n1 = (g.nbuckets / lb + GROUP - 1) / GROUP;   // waves per set in level 1
    p.host_items = p.n1;
    while (p.host_items > HOST_ITEMS) {
      p.host_items = (p.host_items + GROUP - 1) / GROUP;
      p.groups.push_back(p.host_items);
    }
    const double waves = (double)p.n1 * nsets_all, slots = (double)tune.num_cus * RED_WAVES;
    const double rounds = std::ceil(waves / slots), n_seq = (PLANES + 2) + PLANES * (double)p.groups.size();
    p.est = rounds * (2.0 * lb + 6.0) * 9.0 + 65.0 * (double)p.groups.size() +
            (double)nsets_all * n_seq * (0.35 * p.host_items + 0.7 * (p.host_items - 1));
    return p;
  };
  RedPlan plan = red_plan(1);
  if (tune.lb) {
    plan = red_plan(std::min<u32>((u32)tune.lb, g.nbuckets));
  } else {
    for (u32 lb = 2; lb <= 256 && lb <= g.nbuckets; lb *= 2) {
      RedPlan p = red_plan(lb);
      if (p.est < plan.est) plan = p;
    }
  }
  const u32 LB = P.lb = plan.lb;
  u32& log_lb = P.log_lb;
  while ((1u << log_lb) < LB) ++log_lb;
  const u32 n1 = P.n1 = plan.n1, host_items = P.host_items = plan.host_items;
  const std::vector<u32>& lvl_groups = plan.groups;   // group counts of the follow-up levels
  const u32 n_dev = (u32)lvl_groups.size();   // follow-up launches
  if (n_dev > MSM_MAX_RED_LEVELS) return refuse("internal: bucket reduction deeper than four levels");
  P.n_dev = n_dev;
  std::copy(lvl_groups.begin(), lvl_groups.end(), P.groups);
  // what the host receives: 7 + 5 n_dev sequences (Tt, five planes per level, W) of host_items entries per set
  const u32 n_seq_host = P.n_seq_host = (PLANES + 2) + PLANES * n_dev;

  // workspace layout
  size_t off = 0;
  auto take = [&](size_t bytes) {
    size_t o = off;
    off = msm_align_up(off + bytes, 256);
    return o;
  };
  MsmLayout& at = P.at;
  at.canon = take((size_t)n * batch * 32), at.rows = take((size_t)batch * g.tiles * g.bins * 2);
  at.pairs = take(m * 8), at.keys1 = take(m * 4 + 4), at.vals1 = take(m * 4 + 4);
  at.buckets = take(total_buckets * 256);
  for (u32 i = 1; i < n_levels; ++i) {
    at.pkeys[i] = take(P.lv[i].len * 4);
    at.ppts[i] = take(P.lv[i].len * 256);
  }
  at.heads = take(n_levels > 1 ? l1_threads * 256 : 0);
  at.l1 = take((size_t)(PLANES + 2) * nsets_all * n1 * 256);
  for (u32 k = 0; k < n_dev; ++k) at.lvl[k] = take((size_t)((PLANES + 2) + PLANES * (k + 1)) * nsets_all * lvl_groups[k] * 256);
  at.win = take((size_t)n_seq_host * nsets_all * host_items * 256);
  // Who applies the weights: the host fold (~1 us per addition, ~0.65 us per doubling, per set) or one more launch
  // (msm_reduce_finish_kernel: a fixed chain whatever the number of sets).  One or a few sets: the host.
  const u32 nplanes = P.nplanes = PLANES * (n_dev + 1);
  const double fold_host_us = (double)nsets_all * (n_seq_host * (0.3 * host_items + 1.0 * (host_items - 1)) + 1.65 * nplanes);
  const double fold_dev_us = (host_items + 0.72 * (log_lb + nplanes + 1) + 5.0) * 9.0 + 20.0 + 0.5 * nsets_all;
  const bool use_finish = P.use_finish = fold_host_us > fold_dev_us;
  at.fin = take(use_finish ? (size_t)nsets_all * 256 : 0);
  P.ws_bytes = off;
  P.pinned_bytes = use_finish ? (size_t)nsets_all * 256 : (size_t)n_seq_host * nsets_all * host_items * 256;

  // the launches that follow from it
  // bucket fill
  // at most ~2 K workgroups: the partition totals cost one atomic per (workgroup-tile, partition)
  u32& tiles_per_wg = P.tiles_per_wg = 1;
  while ((size_t)batch * ((g.tiles + tiles_per_wg - 1) / tiles_per_wg) > 2048) ++tiles_per_wg;
  P.wgs_per_msm = (g.tiles + tiles_per_wg - 1) / tiles_per_wg;
  P.scatter_wgs = std::min<u32>(batch * g.tiles, (u32)tune.num_cus);
  // accumulate
  for (u32 lvl = 0; lvl < n_levels; ++lvl) {
    MsmPlan::Level& l = P.lv[lvl];
    const bool last = (lvl + 1 == n_levels);
    const size_t nthr = lvl == 0 ? l1_threads : (l.len + l.offset + l.chunk - 1) / l.chunk;
    const unsigned blocks = (unsigned)((nthr + 127) / 128);
    if (lvl > 0 && last && nthr > 64) return refuse("internal: final MSM level wider than a wave");
    l.blocks = blocks, l.threads = 128;
    if (lvl == 0) {
      // Two waves that share a SIMD run one after the other (oldest first, section 4 of DESIGN.md), and two-wave workgroups
      // are not spread evenly: a grid of at most one (two) waves per SIMD is launched as four-wave workgroups -- a wave per
      // SIMD of a CU -- with an LDS request that keeps a second (third) workgroup off the CU.  The kernel uses no LDS.
      const size_t waves = (nthr + 63) / 64;
      size_t place_lds = 0;
      // (just over a half / a third of the CU's 160 KB: what is left -- 79 KB / 52 KB -- still takes the workgroups of the
      // prover's side stream, the coset transforms that run beside the commitments of rounds 1 and 2; with 96 / 72 KB those
      // kept accumulate workgroups waiting for a CU: 2^16-gate proofs took 4.13 ms or 4.47 ms, at random)
      if (waves <= lone_waves) place_lds = 81 * 1024;
      else if (waves <= 2 * lone_waves) place_lds = 54 * 1024;
      if (place_lds) l.blocks = (unsigned)((nthr + 255) / 256), l.threads = 256;
      P.place_lds = place_lds;
    }
  }
  return PM_OK;
}

}  // namespace pm
