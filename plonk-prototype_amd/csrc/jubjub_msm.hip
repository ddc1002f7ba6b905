// Native JubJub MSM: sum s_i P_i on the embedded curve by the bucket method over signed c-bit windows,
// with the group law of jubjub.hip.h and the plan and the recoding of jubjub_msm_plan.h.  `batch` scalar vectors share the
// points; vector b and window w own the bucket set ("row") b windows + w, and every kernel below works on all rows at once.
//
//   count     one thread per (vector, point): the digits of its scalar, one atomic per non-zero digit on the bucket's counter
//             (one per wave for the lanes that share a bucket with the wave's first or last pending lane: skewed scalars).
//   scan      exclusive sums over all buckets of the pairs and of the SEGMENTS (JMSM_SEG pairs at most, never across a bucket):
//             tile sums, one workgroup over the tiles, then the tiles again.
//   scatter   the count kernel again, now writing (point index | sign << 31) at the bucket's cursor.
//   partial   one thread per segment: the sum of its pairs, each point read as it came in (affine, one product for t = x y),
//             into an extended point of its own.  A bucket of one segment is then complete.
//   bucket    one thread per bucket adds the segments of a bucket that has several; a bucket of more than JMSM_HEAVY is taken
//             by the whole wave instead, lanes striding over its segments and folding with six butterfly steps.  Under total
//             skew (every scalar the same) the partial kernel still runs n / JMSM_SEG threads wide and one wave a window folds
//             them: slow, not serial.
//   window    one workgroup per row: thread t walks seg_buckets buckets from the top with the usual two running sums, which
//             leaves sum m B_(t G + m) and S_t = sum B; it adds (t G) S_t by double-and-add (t G < 2^15) and the workgroup
//             folds its threads through LDS.
//   final     one thread per vector: Horner over the windows (c doublings each), ONE inversion, the affine point.
//
// The order in which atomics land decides the order of the pairs inside a bucket and nothing else; the law is exact and the
// point leaves in affine form, so the bytes do not depend on it, on c or on the batch.
//
// Bounds, for any 256-bit scalar word.  A digit's magnitude is clamped to 1 .. buckets although the recoding never exceeds it
// (jubjub_msm_plan.h).  The scatter writes pair p only for p below the end of its bucket, which the SAME digits counted; a
// point index read back from a pair is clamped below n; segments past the scanned total leave at once.  Nothing else is
// addressed by data.
//
// fe_inv_dev votes across the wave: every lane of the final kernel reaches it (a lane past the batch works on the last vector
// and stores nothing).  NOT hardened against side channels: addresses depend on the scalars.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "context.h"
#include "field_inv.hip.h"
#include "jubjub.hip.h"
#include "jubjub_msm_plan.h"

namespace pm {
namespace {

struct JmsmArgs {
  const u32x4* points;      // n x (x | y)
  const u32x4* scalars;     // batch vectors at scalar_stride elements
  u32x4* out;               // batch x (x | y)
  u32* count;               // [total_buckets] pairs of a bucket
  u32* cursor;              // [total_buckets] the scatter's
  u32* pair_off;            // [total_buckets + 1]
  u32* item_off;            // [total_buckets + 1] segments before a bucket
  u32* tile_sums;           // [tiles][2]
  u32* pairs;               // [max_pairs]
  u32x4* partials;          // [max_items] x 9 chunks
  u32x4* wsums;             // [rows] x 9 chunks
  size_t n, scalar_stride;
  u32 batch, c, windows, buckets, total_buckets, tiles, seg_buckets, montgomery;
  u32 max_items;
  u32 edwards_d[9];         // device form
};

PM_DEV void jm_store(u32x4* base, size_t at, const EdPoint& p) { jj_table_store(base + at * JJ_POINT_CHUNKS, 1, 1, p); }
PM_DEV EdPoint jm_load(const u32x4* base, size_t at) { return jj_table_load(base + at * JJ_POINT_CHUNKS, 1, 1); }
PM_DEV u32 jm_segments(u32 count) { return (count + JMSM_SEG - 1) / JMSM_SEG; }

// ---- count (SCATTER = false) and scatter (true): thread g = vector * n + point
template <bool SCATTER>
__global__ void __launch_bounds__(256) jmsm_digits_kernel(const JmsmArgs a) {
  const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= a.n * a.batch) return;
  const u32 b = (u32)(g / a.n);
  const size_t i = g - (size_t)b * a.n;
  u64 k[4];
  jj_load_scalar(a.scalars + 2 * ((size_t)b * a.scalar_stride + i), a.montgomery != 0, k);
  const u32 lane = threadIdx.x & 63u;
  u32 cy = 0;
#pragma unroll 1
  for (u32 w = 0; w < a.windows; ++w) {                     // the same trip count in every lane: the votes below are whole
    const int d = jmsm_digit(k, a.c, cy);
    jmsm_shr(k, a.c);
    bool pending = d != 0;
    u32 mag = (u32)(d < 0 ? -d : d);
    mag = mag > a.buckets ? a.buckets : (mag ? mag : 1u);
    const u32 bucket = (b * a.windows + w) * a.buckets + (mag - 1);
    const u32 entry = (u32)i | (d < 0 ? 0x80000000u : 0u);
    // Skew: the lanes that share a bucket with the first pending lane (then with the last) go in with ONE atomic, so a bucket
    // most scalars hit -- the carry into the window above a run of small witnesses -- costs a wave one atomic, not 64 on one address.
#pragma unroll 1
    for (int round = 0; round < 2; ++round) {
      const unsigned long long act = __ballot(pending);
      if (!act) break;
      const int leader = round == 0 ? __ffsll((long long)act) - 1 : 63 - __clzll((long long)act);
      const u32 lb = __shfl(bucket, leader);
      const bool mine = pending && bucket == lb;
      const unsigned long long same = __ballot(mine);
      const u32 cnt = (u32)__popcll(same);
      if (cnt < 2) continue;                                 // wave-uniform
      u32 base = 0;
      if (lane == (u32)leader) base = atomicAdd((SCATTER ? a.cursor : a.count) + lb, cnt);
      if (SCATTER) {
        base = __shfl(base, leader);
        const u32 p = a.pair_off[lb] + base + (u32)__popcll(same & ((1ull << lane) - 1ull));
        if (mine && p < a.pair_off[lb + 1]) a.pairs[p] = entry;
      }
      pending = pending && !mine;
    }
    if (!pending) continue;
    if (!SCATTER) {
      atomicAdd(a.count + bucket, 1u);
    } else {
      const u32 p = a.pair_off[bucket] + atomicAdd(a.cursor + bucket, 1u);
      if (p < a.pair_off[bucket + 1]) a.pairs[p] = entry;
    }
  }
}

// ---- scan: tile sums / the tiles' exclusive sums / offsets.  A thread owns 8 consecutive buckets of its tile.
PM_DEV void jm_block_exclusive(u32 (&s)[2][256], u32 t, u32& x, u32& y) {   // in: a thread's sums; out: the sums of the threads before it
  s[0][t] = x, s[1][t] = y;
  __syncthreads();
  for (u32 d = 1; d < 256; d <<= 1) {
    const u32 px = t >= d ? s[0][t - d] : 0u, py = t >= d ? s[1][t - d] : 0u;
    __syncthreads();
    s[0][t] += px, s[1][t] += py;
    __syncthreads();
  }
  const u32 ix = s[0][t], iy = s[1][t];
  x = ix - x, y = iy - y;
}
__global__ void __launch_bounds__(256) jmsm_tile_sums_kernel(const JmsmArgs a) {
  __shared__ u32 s[2][256];
  const u32 t = threadIdx.x, first = blockIdx.x * JMSM_SCAN_TILE + t * 8;
  u32 x = 0, y = 0;
  for (u32 j = first; j < first + 8 && j < a.total_buckets; ++j) x += a.count[j], y += jm_segments(a.count[j]);
  u32 ex = x, ey = y;
  jm_block_exclusive(s, t, ex, ey);
  if (t == 255) a.tile_sums[2 * blockIdx.x] = ex + x, a.tile_sums[2 * blockIdx.x + 1] = ey + y;
}
__global__ void __launch_bounds__(256) jmsm_tile_scan_kernel(const JmsmArgs a) {   // one workgroup
  __shared__ u32 s[2][256];
  const u32 t = threadIdx.x, per = (a.tiles + 255) / 256, first = t * per;
  u32 x = 0, y = 0;
  for (u32 j = first; j < first + per && j < a.tiles; ++j) x += a.tile_sums[2 * j], y += a.tile_sums[2 * j + 1];
  jm_block_exclusive(s, t, x, y);
  for (u32 j = first; j < first + per && j < a.tiles; ++j) {
    const u32 cx = a.tile_sums[2 * j], cyy = a.tile_sums[2 * j + 1];
    a.tile_sums[2 * j] = x, a.tile_sums[2 * j + 1] = y;
    x += cx, y += cyy;
  }
}
__global__ void __launch_bounds__(256) jmsm_offsets_kernel(const JmsmArgs a) {
  __shared__ u32 s[2][256];
  const u32 t = threadIdx.x, first = blockIdx.x * JMSM_SCAN_TILE + t * 8;
  u32 x = 0, y = 0;
  for (u32 j = first; j < first + 8 && j < a.total_buckets; ++j) x += a.count[j], y += jm_segments(a.count[j]);
  jm_block_exclusive(s, t, x, y);
  x += a.tile_sums[2 * blockIdx.x], y += a.tile_sums[2 * blockIdx.x + 1];
  for (u32 j = first; j < first + 8 && j < a.total_buckets; ++j) {
    a.pair_off[j] = x, a.item_off[j] = y;
    x += a.count[j], y += jm_segments(a.count[j]);
    if (j + 1 == a.total_buckets) a.pair_off[j + 1] = x, a.item_off[j + 1] = y;
  }
}

// ---- partial: thread = segment
__global__ void __launch_bounds__(64) jmsm_partial_kernel(const JmsmArgs a) {
  const u32 item = blockIdx.x * 64 + threadIdx.x;
  if (item >= a.item_off[a.total_buckets] || item >= a.max_items) return;
  // the last bucket whose first segment is not after this one: it is not empty, its successors up to the next are
  u32 lo = 0, hi = a.total_buckets;                          // item_off[lo] <= item < item_off[hi]
  while (hi - lo > 1) {
    const u32 mid = lo + (hi - lo) / 2;
    if (a.item_off[mid] <= item) lo = mid; else hi = mid;
  }
  const u32 end_b = a.pair_off[lo + 1];
  u32 p = a.pair_off[lo] + (item - a.item_off[lo]) * JMSM_SEG;
  const u32 end = p >= end_b ? p : (end_b - p > JMSM_SEG ? p + JMSM_SEG : end_b);
  const Fr ed = fr_limbs(a.edwards_d);
  EdPoint acc = jj_neutral();
#pragma unroll 1
  for (; p < end; ++p) {
    const u32 e = a.pairs[p];
    size_t i = e & 0x7fffffffu;
    i = i < a.n ? i : a.n - 1;
    const Fr x = g_to_dev(ld_canon(a.points, 2 * i)), y = g_to_dev(ld_canon(a.points, 2 * i + 1)), t = gmul(x, y);
    const bool neg = (e >> 31) != 0;
    acc = ed_madd(acc, g_sel(neg, gneg(x), x), y, g_sel(neg, gneg(t), t), ed);
  }
  jm_store(a.partials, item, acc);
}

// ---- bucket: thread = bucket; the sum of a bucket's segments lands in its first
PM_DEV EdPoint jm_shfl_xor(const EdPoint& p, int m) {
  EdPoint r;
#pragma unroll
  for (int j = 0; j < 9; ++j) {
    r.X.l[j] = __shfl_xor(p.X.l[j], m), r.Y.l[j] = __shfl_xor(p.Y.l[j], m);
    r.Z.l[j] = __shfl_xor(p.Z.l[j], m), r.T.l[j] = __shfl_xor(p.T.l[j], m);
  }
  return r;
}
__global__ void __launch_bounds__(64) jmsm_bucket_kernel(const JmsmArgs a) {
  const u32 j = blockIdx.x * 64 + threadIdx.x;
  const bool live = j < a.total_buckets;
  const u32 first = live ? a.item_off[j] : 0u, segs = live ? a.item_off[j + 1] - first : 0u;
  const Fr ed = fr_limbs(a.edwards_d);
  if (segs > 1 && segs <= JMSM_HEAVY) {
    EdPoint acc = jm_load(a.partials, first);
#pragma unroll 1
    for (u32 s = 1; s < segs; ++s) acc = ed_add(acc, jm_load(a.partials, first + s), ed);
    jm_store(a.partials, first, acc);
  }
  unsigned long long heavy = __ballot(segs > JMSM_HEAVY);
#pragma unroll 1
  while (heavy) {                                            // wave-uniform
    const int lane = __ffsll((long long)heavy) - 1;
    heavy &= heavy - 1;
    const u32 hf = __shfl(first, lane), hs = __shfl(segs, lane);
    EdPoint acc = jj_neutral();
#pragma unroll 1
    for (u32 s = threadIdx.x; s < hs; s += 64) acc = ed_add(acc, jm_load(a.partials, hf + s), ed);
#pragma unroll 1
    for (int m = 32; m >= 1; m >>= 1) acc = ed_add(acc, jm_shfl_xor(acc, m), ed);
    if (threadIdx.x == 0) jm_store(a.partials, hf, acc);    // every lane has read its segments: the butterfly depends on them
  }
}

// ---- window: workgroup = row
__global__ void __launch_bounds__(256) jmsm_window_kernel(const JmsmArgs a) {
  __shared__ u32 lds[36][JMSM_RED_THREADS];
  const u32 t = threadIdx.x, row = blockIdx.x, G = a.seg_buckets, segs = a.buckets / G;
  const Fr ed = fr_limbs(a.edwards_d);
  EdPoint tot = jj_neutral();
  if (t < segs) {
    EdPoint run = jj_neutral();
    const u32 base = row * a.buckets + t * G;               // bucket index of magnitude t G + 1
#pragma unroll 1
    for (u32 m = G; m >= 1; --m) {
      const u32 j = base + m - 1;
      if (a.count[j]) run = ed_add(run, jm_load(a.partials, a.item_off[j]), ed);
      tot = ed_add(tot, run, ed);
    }
    // + (t G) S_t, from the top bit of t G
    const u32 k = t * G;
    if (k) {
      EdPoint mul = jj_neutral();
#pragma unroll 1
      for (int bit = 31 - __clz((int)k); bit >= 0; --bit) {
        mul = ed_add(mul, mul, ed);
        if ((k >> bit) & 1u) mul = ed_add(mul, run, ed);
      }
      tot = ed_add(tot, mul, ed);
    }
  }
#pragma unroll 1
  for (u32 s = JMSM_RED_THREADS / 2; s >= 1; s >>= 1) {
    if (t >= s && t < 2 * s) {
#pragma unroll
      for (int q = 0; q < 9; ++q) lds[q][t] = tot.X.l[q], lds[9 + q][t] = tot.Y.l[q], lds[18 + q][t] = tot.Z.l[q], lds[27 + q][t] = tot.T.l[q];
    }
    __syncthreads();
    if (t < s) {
      EdPoint o;
#pragma unroll
      for (int q = 0; q < 9; ++q) o.X.l[q] = lds[q][t + s], o.Y.l[q] = lds[9 + q][t + s], o.Z.l[q] = lds[18 + q][t + s], o.T.l[q] = lds[27 + q][t + s];
      tot = ed_add(tot, o, ed);
    }
    __syncthreads();
  }
  if (t == 0) jm_store(a.wsums, row, tot);
}

// ---- final: thread = vector
__global__ void __launch_bounds__(64) jmsm_final_kernel(const JmsmArgs a) {
  const u32 g = blockIdx.x * 64 + threadIdx.x;
  const bool live = g < a.batch;
  const u32 b = live ? g : a.batch - 1;
  const Fr ed = fr_limbs(a.edwards_d);
  EdPoint acc = jj_neutral();
#pragma unroll 1
  for (u32 w = a.windows; w-- > 0;) {
#pragma unroll 1
    for (u32 j = 0; j < a.c; ++j) acc = ed_add(acc, acc, ed);
    acc = ed_add(acc, jm_load(a.wsums, (size_t)b * a.windows + w), ed);
  }
  jj_store_affine(a.out, b, live, acc);
}

}  // namespace

// context.h: the launches of one MSM on st, arguments already checked; the caller holds the context's mutex and has selected
// the device.  The workspace is the context's (jj_msm_ws): grown here, ordered across streams, released by pm_trim.
int jubjub_msm_enqueue(pm_ctx* ctx, const void* d_points_xy, const void* d_scalars, size_t n, size_t scalar_stride, uint32_t batch,
                       bool montgomery, void* d_out_xy, hipStream_t st) {
  JubjubMsmPlan p;
  if (int rc = jubjub_msm_plan(n, batch, ctx->opt_jubjub_msm_window_bits, &p))
    return set_err(ctx, rc, rc == PM_ERR_LENGTH ? "pm_jubjub_msm_dev: n x windows x batch exceeds what the plan indexes (jubjub_msm_plan.h)"
                                                : "pm_jubjub_msm_dev: batch = 0");
  JmsmArgs a{};
  a.points = (const u32x4*)d_points_xy, a.scalars = (const u32x4*)d_scalars, a.out = (u32x4*)d_out_xy;
  a.n = n, a.scalar_stride = scalar_stride, a.batch = batch, a.montgomery = montgomery ? 1u : 0u;
  jubjub_d_limbs(a.edwards_d);
  ProfScope prof(ctx, st, "jubjub_msm");
  const unsigned final_blocks = (batch + 63) / 64;
  if (n == 0) {                                              // no window: the neutral element through the same store
    a.windows = 0, a.c = p.c;
    hipLaunchKernelGGL(jmsm_final_kernel, dim3(final_blocks), dim3(64), 0, st, a);
    PM_HIP(ctx, hipGetLastError());
    return PM_OK;
  }
  OrderScope order_scope(ctx, ctx->ord_jj_msm, st);
  if (order_scope.rc) return order_scope.rc;
  if (int rc = ensure_buffer(ctx, ctx->jj_msm_ws, p.bytes)) return rc;
  char* const ws = (char*)ctx->jj_msm_ws.ptr;
  a.count = (u32*)(ws + p.off_count), a.cursor = (u32*)(ws + p.off_cursor), a.pair_off = (u32*)(ws + p.off_pair_off);
  a.item_off = (u32*)(ws + p.off_item_off), a.tile_sums = (u32*)(ws + p.off_tile_sums), a.pairs = (u32*)(ws + p.off_pairs);
  a.partials = (u32x4*)(ws + p.off_partials), a.wsums = (u32x4*)(ws + p.off_wsums);
  a.c = p.c, a.windows = p.windows, a.buckets = p.buckets, a.total_buckets = p.total_buckets, a.tiles = p.tiles;
  a.seg_buckets = p.seg_buckets, a.max_items = (u32)p.max_items;
  PM_HIP(ctx, hipMemsetAsync(a.count, 0, p.off_pair_off - p.off_count, st));   // count and cursor
  const unsigned digit_blocks = (unsigned)((n * batch + 255) / 256);
  hipLaunchKernelGGL((jmsm_digits_kernel<false>), dim3(digit_blocks), dim3(256), 0, st, a);
  hipLaunchKernelGGL(jmsm_tile_sums_kernel, dim3(p.tiles), dim3(256), 0, st, a);
  hipLaunchKernelGGL(jmsm_tile_scan_kernel, dim3(1), dim3(256), 0, st, a);
  hipLaunchKernelGGL(jmsm_offsets_kernel, dim3(p.tiles), dim3(256), 0, st, a);
  hipLaunchKernelGGL((jmsm_digits_kernel<true>), dim3(digit_blocks), dim3(256), 0, st, a);
  hipLaunchKernelGGL(jmsm_partial_kernel, dim3((unsigned)((p.max_items + 63) / 64)), dim3(64), 0, st, a);
  hipLaunchKernelGGL(jmsm_bucket_kernel, dim3((p.total_buckets + 63) / 64), dim3(64), 0, st, a);
  hipLaunchKernelGGL(jmsm_window_kernel, dim3(p.rows), dim3(JMSM_RED_THREADS), 0, st, a);
  hipLaunchKernelGGL(jmsm_final_kernel, dim3(final_blocks), dim3(64), 0, st, a);
  PM_HIP(ctx, hipGetLastError());
  return PM_OK;
}

}  // namespace pm

using namespace pm;

extern "C" int pm_jubjub_msm_dev(pm_ctx* ctx, const void* d_points_xy, const void* d_scalars, size_t n, size_t scalar_stride,
                                 uint32_t batch, uint32_t scalar_form, void* d_out_xy, void* hip_stream) {
  if (!ctx) return PM_ERR_BAD_ARG;
  if (int rc = form_fault(ctx, scalar_form)) return rc;
  if (int rc = pointer_fault(ctx, {d_out_xy}, unaligned({d_points_xy, d_scalars}) || (n != 0 && (!d_points_xy || !d_scalars)))) return rc;
  if (batch == 0) return set_err(ctx, PM_ERR_BAD_ARG, "pm_jubjub_msm_dev: batch = 0");
  if (scalar_stride < n) return set_err(ctx, PM_ERR_BAD_ARG, "pm_jubjub_msm_dev: scalar_stride < n");
  if (n > 0x7fffffffu || scalar_stride > ((size_t)1 << 40)) return set_err(ctx, PM_ERR_LENGTH, "pm_jubjub_msm_dev: n > 2^31 - 1 or scalar_stride > 2^40");
  std::lock_guard<std::mutex> lk(ctx->mu);
  JubjubMsmPlan p;                                           // what the plan cannot index is refused before the ranges are compared
  if (jubjub_msm_plan(n, batch, ctx->opt_jubjub_msm_window_bits, &p) == PM_ERR_LENGTH)
    return set_err(ctx, PM_ERR_LENGTH, "pm_jubjub_msm_dev: n x windows x batch exceeds what the plan indexes (jubjub_msm_plan.h)");
  const size_t out_bytes = 64 * (size_t)batch, scalar_bytes = n ? 32 * ((size_t)(batch - 1) * scalar_stride + n) : 0;
  if (overlap(d_out_xy, out_bytes, d_points_xy, 64 * n) || overlap(d_out_xy, out_bytes, d_scalars, scalar_bytes))   // n = 0: empty ranges
    return set_err(ctx, PM_ERR_BAD_ARG, "pm_jubjub_msm_dev: d_out_xy overlaps an input");
  PM_DEVICE_STREAM(ctx, hip_stream, st);
  return jubjub_msm_enqueue(ctx, d_points_xy, d_scalars, n, scalar_stride, batch, scalar_form == PM_SCALAR_MONTGOMERY, d_out_xy, st);
}

extern "C" int pm_jubjub_msm_host(const uint64_t* points_xy, const uint64_t* scalars, size_t n, uint32_t scalar_form,
                                  uint64_t out_xy[8]) {
  if (!out_xy || (n != 0 && (!points_xy || !scalars))) return PM_ERR_BAD_ARG;
  if (scalar_form != PM_SCALAR_MONTGOMERY && scalar_form != PM_SCALAR_CANONICAL) return PM_ERR_BAD_ARG;
  HPoint acc = hpoint_identity();
  for (size_t i = 0; i < n; ++i) {
    uint64_t k[4];
    if (point_fault(points_xy + 8 * i) || !scalar_to_int(scalars + 4 * i, scalar_form, k)) return PM_ERR_BAD_ARG;
    acc = hpoint_add(acc, hpoint_mul(hpoint_load(points_xy + 8 * i), k));
  }
  hpoint_store(out_xy, acc);
  return PM_OK;
}

extern "C" int pm_test_jubjub_msm_plan(size_t n, uint32_t batch, long window_bits, uint32_t num_cus, uint64_t out[8]) {
  if (!out) return PM_ERR_BAD_ARG;
  (void)num_cus;                                             // the plan does not depend on the machine
  JubjubMsmPlan p;
  memset(out, 0, 64);
  if (int rc = jubjub_msm_plan(n, batch, window_bits, &p)) return rc;
  out[0] = p.c, out[1] = p.windows, out[2] = p.buckets, out[3] = p.max_pairs, out[4] = p.bytes, out[5] = p.rows;
  out[6] = p.max_items, out[7] = p.seg_buckets;
  return PM_OK;
}

extern "C" int pm_test_jubjub_msm_digits(const uint64_t scalar[4], uint32_t c, int32_t* digits, uint32_t* n_digits) {
  if (!scalar || !digits || !n_digits || c < JMSM_MIN_C || c > JMSM_MAX_C) return PM_ERR_BAD_ARG;
  const uint64_t k[4] = {scalar[0], scalar[1], scalar[2], scalar[3]};
  const uint32_t windows = jubjub_msm_windows(c);
  const uint32_t carry = jmsm_for_each_digit(k, c, windows, [&](uint32_t w, int32_t d) { digits[w] = d; });
  if (carry) digits[windows] = (int32_t)carry;               // never, by the plan's window count: shown, not hidden, if it were
  *n_digits = windows + carry;
  return PM_OK;
}
