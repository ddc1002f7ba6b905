// Composer-form circuits: the copy permutation from wire variables (pm_plonk_sigma_from_wires*) and
// the witness from variable assignments (the gather behind pm_plonk_witness_from_vars_dev).
//
// sigma_index from wire_vars[4n] (position j n + i = the variable at wire j of gate i): the positions of a variable, ordered by
// rank r = 4 i + j (gate first, then a b c d: the order in which dusk's Permutation pushes them), form one cycle.  That is a
// stable sort of the (id, position) pairs by id, fed in rank order, and one link pass over the sorted array:
//
//   per 8-bit digit, least significant first, ceil(bits(num_vars - 1) / 8) passes:
//     wire_hist_kernel     per-tile digit counts (counts[digit][tile]) and per-digit totals
//     wire_scan_kernel     exclusive scan of counts in (digit, tile) order: where each tile's run of a digit starts
//     wire_scatter_kernel  every pair to  start + its rank among the tile's earlier pairs of the same digit
//   wire_link_kernel       sorted[k] -> sorted[k + 1] when the ids agree, else -> the first pair of its id
//
// The in-tile ranks come from a wave-level multi-split: a wave walks its contiguous quarter of the tile 64 pairs at a time,
// eight __ballot masks give every lane the set of lanes with its digit, and the lanes below it in that set are the pairs in
// front of it.  No rank comes from an atomic, so the output is a pure function of the input (counts do: sums do not depend on
// order).  The first pass reads wire_vars itself; PM_PLONK_NO_VAR positions (and ids out of range, which fail the call) are
// left out of the sort there and map to themselves, so the later passes sort m <= 4n pairs, m read from device memory.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <type_traits>

#include "context.h"

namespace pm {
namespace {

typedef unsigned int u32;
typedef unsigned long long u64;

constexpr u32 WS_THREADS = 256;
constexpr u32 WS_WAVES = WS_THREADS / 64;
constexpr u32 WS_IPT = 16;                         // pairs per thread
constexpr u32 WS_TILE = WS_THREADS * WS_IPT;       // 4096 pairs per tile
constexpr u32 WS_CHUNK = WS_TILE / WS_WAVES;       // a wave's contiguous share of a tile
constexpr u32 WS_DIGITS = 256;
constexpr u32 WS_MAX_PASSES = 4;

// control words (u32) behind the per-pass digit totals
constexpr u32 CTL_TOTALS = 0;                                  // [WS_MAX_PASSES][256]
constexpr u32 CTL_COUNT = WS_MAX_PASSES * WS_DIGITS;           // m: pairs in the sort
constexpr u32 CTL_BAD = CTL_COUNT + 1;                         // lowest position with an id out of range, ~0 = none
constexpr u32 CTL_WORDS = CTL_BAD + 1;

struct WirePlan {
  u32 passes, tiles;
  size_t total;            // 4n
  size_t pair_bytes;       // one pair buffer
  size_t counts_bytes;     // counts[256][tiles]
  size_t scratch_bytes;    // 2 pair buffers + counts + control
};

int wire_sort_plan(size_t n, size_t num_vars, WirePlan& p) {
  if (n < 4 || (n & (n - 1)) || n > ((size_t)1 << 29)) return PM_ERR_LENGTH;   // positions and tile starts stay below 2^31
  if (num_vars > 0xffffffffull) return PM_ERR_BAD_ARG;                          // ids are 32 bit, PM_PLONK_NO_VAR is no id
  u32 bits = 0;
  for (size_t top = num_vars > 1 ? num_vars - 1 : 0; top; top >>= 1) ++bits;
  p.passes = std::max<u32>(1, (bits + 7) / 8);
  p.total = 4 * n;
  p.tiles = (u32)((p.total + WS_TILE - 1) / WS_TILE);
  p.pair_bytes = p.total * 8;
  p.counts_bytes = (size_t)WS_DIGITS * p.tiles * 4;
  p.scratch_bytes = 2 * p.pair_bytes + p.counts_bytes + CTL_WORDS * 4;
  return PM_OK;
}

// Element e of tile `tile`, pass 0: the pair of rank e from the wire map.  valid = it takes part in the sort.
struct FromWires {
  const u32* wire_vars;
  u32 n, total, num_vars;
  __device__ u32 count() const { return total; }
  __device__ u64 load(u32 e, bool& valid, u32& pos) const {
    pos = (e & 3u) * n + (e >> 2);
    const u32 id = wire_vars[pos];
    valid = id < num_vars;          // PM_PLONK_NO_VAR >= every num_vars
    return ((u64)id << 32) | pos;
  }
};
struct FromPairs {
  const u64* src;
  const u32* ctl;
  __device__ u32 count() const { return ctl[CTL_COUNT]; }
  __device__ u64 load(u32 e, bool& valid, u32& pos) const {
    valid = true;
    const u64 pr = src[e];
    pos = (u32)pr;
    return pr;
  }
};

// the lanes of the wave that are valid and hold digit d (d: 8 bits)
__device__ __forceinline__ u64 match_digit(u32 d, bool valid) {
  u64 peers = __ballot(valid);
#pragma unroll
  for (u32 b = 0; b < 8; ++b) {
    const bool bit = (d >> b) & 1u;
    const u64 m = __ballot(bit);
    peers &= bit ? m : ~m;
  }
  return peers;
}
__device__ __forceinline__ u32 lanes_below(u64 mask) {
  return __builtin_amdgcn_mbcnt_hi((u32)(mask >> 32), __builtin_amdgcn_mbcnt_lo((u32)mask, 0u));
}

template <class Src>
__global__ __launch_bounds__(WS_THREADS) void wire_hist_kernel(Src src, u32 shift, u32 tiles, u32* counts, u32* ctl, u32 pass,
                                                               long long* sigma) {
  __shared__ u32 hist[WS_DIGITS];
  const u32 tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, tile = blockIdx.x;
  const u32 m = src.count();
  hist[tid] = 0;
  __syncthreads();
  const u32 base = tile * WS_TILE + wave * WS_CHUNK;
  u32 bad = 0xffffffffu;
  for (u32 r = 0; r < WS_CHUNK / 64; ++r) {
    const u32 e = base + r * 64 + lane;
    bool valid = false;
    u32 pos = 0;
    u64 pr = 0;
    if (e < m) pr = src.load(e, valid, pos);
    if constexpr (std::is_same<Src, FromWires>::value) {
      // left out of the sort: sigma fixes the position; an id that is neither below num_vars nor PM_PLONK_NO_VAR fails the call
      if (e < m && !valid) {
        sigma[pos] = (long long)pos;
        if ((u32)(pr >> 32) != PM_PLONK_NO_VAR) bad = min(bad, pos);
      }
    }
    const u32 d = (u32)(pr >> (32 + shift)) & 255u;
    const u64 peers = match_digit(d, valid);
    if (valid && lanes_below(peers) == 0) atomicAdd(&hist[d], (u32)__popcll(peers));   // a count: the order of the adds is free
  }
  if constexpr (std::is_same<Src, FromWires>::value) {
    if (bad != 0xffffffffu) atomicMin(&ctl[CTL_BAD], bad);
  }
  __syncthreads();
  const u32 c = hist[tid];
  counts[(size_t)tid * tiles + tile] = c;
  if (c) atomicAdd(&ctl[CTL_TOTALS + pass * WS_DIGITS + tid], c);
}

// counts[d][t] -> the first output index of tile t's pairs with digit d.  One workgroup per digit.
__global__ __launch_bounds__(WS_THREADS) void wire_scan_kernel(u32 tiles, u32* counts, u32* ctl, u32 pass) {
  __shared__ u32 tot[WS_DIGITS];
  __shared__ u32 wsum[WS_WAVES];
  __shared__ u32 carry_s;
  const u32 tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, d = blockIdx.x;
  tot[tid] = ctl[CTL_TOTALS + pass * WS_DIGITS + tid];
  __syncthreads();
  if (tid == 0) {
    u32 below = 0, all = 0;
    for (u32 k = 0; k < WS_DIGITS; ++k) {
      if (k < d) below += tot[k];
      all += tot[k];
    }
    carry_s = below;
    if (d == 0 && pass == 0) ctl[CTL_COUNT] = all;
  }
  __syncthreads();
  u32* row = counts + (size_t)d * tiles;
  for (u32 t0 = 0; t0 < tiles; t0 += WS_THREADS * 4) {
    const u32 b0 = t0 + tid * 4;
    u32 v[4], s = 0;
#pragma unroll
    for (u32 i = 0; i < 4; ++i) {
      v[i] = s;
      if (b0 + i < tiles) s += row[b0 + i];
    }
    u32 inc = s;
#pragma unroll
    for (int k = 1; k < 64; k <<= 1) {
      const u32 t = __shfl_up(inc, k);
      if ((int)lane >= k) inc += t;
    }
    if (lane == 63u) wsum[wave] = inc;
    const u32 carry = carry_s;
    __syncthreads();
    u32 wp = 0, total = 0;
#pragma unroll
    for (u32 w = 0; w < WS_WAVES; ++w) {
      const u32 t = wsum[w];
      if (w < wave) wp += t;
      total += t;
    }
    const u32 start = carry + wp + inc - s;
#pragma unroll
    for (u32 i = 0; i < 4; ++i)
      if (b0 + i < tiles) row[b0 + i] = start + v[i];
    __syncthreads();
    if (tid == 0) carry_s = carry + total;
    __syncthreads();
  }
}

template <class Src>
__global__ __launch_bounds__(WS_THREADS) void wire_scatter_kernel(Src src, u32 shift, u32 tiles, const u32* counts, u64* dst) {
  __shared__ u32 wcnt[WS_WAVES][WS_DIGITS];   // pairs of each digit the wave has passed; then where the wave's run starts
  const u32 tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, tile = blockIdx.x;
  const u32 m = src.count();
#pragma unroll
  for (u32 w = 0; w < WS_WAVES; ++w) wcnt[w][tid] = 0;
  __syncthreads();
  const u32 base = tile * WS_TILE + wave * WS_CHUNK;
  u64 pr[WS_IPT];
  u32 rank[WS_IPT];       // among the wave's earlier pairs of the digit; ~0 = not in the sort
#pragma unroll
  for (u32 r = 0; r < WS_IPT; ++r) {
    const u32 e = base + r * 64 + lane;
    bool valid = false;
    u32 pos = 0;
    pr[r] = 0;
    if (e < m) pr[r] = src.load(e, valid, pos);
    const u32 d = (u32)(pr[r] >> (32 + shift)) & 255u;
    const u64 peers = match_digit(d, valid);
    const u32 below = lanes_below(peers);
    rank[r] = valid ? wcnt[wave][d] + below : 0xffffffffu;
    __builtin_amdgcn_wave_barrier();                       // every lane has read the count before the set's first lane moves it
    if (valid && below == 0) wcnt[wave][d] += (u32)__popcll(peers);
    __builtin_amdgcn_wave_barrier();
  }
  __syncthreads();
  {
    // digit tid: the tile's run starts at counts[tid][tile]; wave w's share of it after the shares of the waves before
    u32 at = counts[(size_t)tid * tiles + tile];
#pragma unroll
    for (u32 w = 0; w < WS_WAVES; ++w) {
      const u32 c = wcnt[w][tid];
      wcnt[w][tid] = at;
      at += c;
    }
  }
  __syncthreads();
#pragma unroll
  for (u32 r = 0; r < WS_IPT; ++r)
    if (rank[r] != 0xffffffffu) {
      const u32 d = (u32)(pr[r] >> (32 + shift)) & 255u;
      dst[wcnt[wave][d] + rank[r]] = pr[r];
    }
}

// sorted[k] = (id, position): the position's successor is the next pair's position while the id lasts, and the position of the
// id's first pair at the end of the run -- found by galloping back over the run, then a binary search for its lower bound.
__global__ __launch_bounds__(WS_THREADS) void wire_link_kernel(const u64* sorted, const u32* ctl, long long* sigma) {
  const u32 m = ctl[CTL_COUNT];
  for (u32 k = blockIdx.x * WS_THREADS + threadIdx.x; k < m; k += gridDim.x * WS_THREADS) {
    const u64 pr = sorted[k];
    const u32 id = (u32)(pr >> 32);
    u32 next;
    if (k + 1 < m && (u32)(sorted[k + 1] >> 32) == id) {
      next = (u32)sorted[k + 1];
    } else {
      u32 lo = k, step = 1;
      while (lo >= step && (u32)(sorted[lo - step] >> 32) == id) {
        lo -= step;
        step <<= 1;
      }
      u32 lb = lo >= step ? lo - step + 1 : 0, ub = lo;     // the first pair of the id is in [lb, ub]
      while (lb < ub) {
        const u32 mid = lb + (ub - lb) / 2;
        if ((u32)(sorted[mid] >> 32) == id) ub = mid;
        else lb = mid + 1;
      }
      next = (u32)sorted[lb];
    }
    sigma[(u32)pr] = (long long)next;
  }
}

// out[b][p] = vars[b][wire_vars[p]], 32-byte elements as two 16-byte halves; PM_PLONK_NO_VAR -> 0
__global__ __launch_bounds__(256) void witness_gather_kernel(const u32* wire_vars, size_t total, const uint4* vars, size_t var_stride,
                                                             uint4* out) {
  const size_t b = blockIdx.y;
  const uint4* v = vars + 2 * var_stride * b;
  uint4* o = out + 2 * total * b;
  for (size_t t = (size_t)blockIdx.x * 256 + threadIdx.x; t < 2 * total; t += (size_t)gridDim.x * 256) {
    const u32 id = wire_vars[t >> 1];
    o[t] = id == PM_PLONK_NO_VAR ? make_uint4(0, 0, 0, 0) : v[2 * (size_t)id + (t & 1)];
  }
}

}  // namespace

int sigma_index_from_wires(pm_ctx* ctx, const void* d_wire_vars, size_t num_vars, size_t n, void* d_sigma_index, hipStream_t st) {
  if (!ctx || !d_wire_vars || !d_sigma_index) return PM_ERR_BAD_ARG;
  WirePlan p;
  const int prc = wire_sort_plan(n, num_vars, p);
  if (prc == PM_ERR_LENGTH) return set_err(ctx, prc, "n must be a power of two in 4..2^29");
  if (prc != PM_OK) return set_err(ctx, prc, "num_vars must be below 2^32");
  void* scratch = nullptr;
  int rc = pm_dev_alloc(ctx, p.scratch_bytes, &scratch);
  if (rc != PM_OK) return rc;
  u32 ctl_host[2] = {0, 0xffffffffu};   // CTL_COUNT, CTL_BAD
  auto run = [&]() -> int {
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (!st) st = ctx->stream;
    PM_HIP(ctx, hipSetDevice(ctx->device));
    u64* buf[2] = {(u64*)scratch, (u64*)((char*)scratch + p.pair_bytes)};
    u32* counts = (u32*)((char*)scratch + 2 * p.pair_bytes);
    u32* ctl = counts + (size_t)WS_DIGITS * p.tiles;
    long long* sigma = (long long*)d_sigma_index;
    PM_HIP(ctx, hipMemsetAsync(ctl, 0, CTL_COUNT * 4 + 4, st));
    PM_HIP(ctx, hipMemsetAsync(ctl + CTL_BAD, 0xff, 4, st));
    const FromWires fw{(const u32*)d_wire_vars, (u32)n, (u32)p.total, (u32)num_vars};
    {
      ProfScope prof(ctx, st, "plonk_wire_sort");
      for (u32 pass = 0; pass < p.passes; ++pass) {
        const u32 shift = 8 * pass;
        u64* out = buf[pass & 1];
        if (pass == 0) {
          hipLaunchKernelGGL(wire_hist_kernel<FromWires>, dim3(p.tiles), dim3(WS_THREADS), 0, st, fw, shift, p.tiles, counts, ctl,
                             pass, sigma);
        } else {
          const FromPairs fp{buf[(pass - 1) & 1], ctl};
          hipLaunchKernelGGL(wire_hist_kernel<FromPairs>, dim3(p.tiles), dim3(WS_THREADS), 0, st, fp, shift, p.tiles, counts, ctl,
                             pass, sigma);
        }
        hipLaunchKernelGGL(wire_scan_kernel, dim3(WS_DIGITS), dim3(WS_THREADS), 0, st, p.tiles, counts, ctl, pass);
        if (pass == 0) {
          hipLaunchKernelGGL(wire_scatter_kernel<FromWires>, dim3(p.tiles), dim3(WS_THREADS), 0, st, fw, shift, p.tiles, counts, out);
        } else {
          const FromPairs fp{buf[(pass - 1) & 1], ctl};
          hipLaunchKernelGGL(wire_scatter_kernel<FromPairs>, dim3(p.tiles), dim3(WS_THREADS), 0, st, fp, shift, p.tiles, counts, out);
        }
      }
    }
    {
      ProfScope prof(ctx, st, "plonk_wire_link");
      const unsigned blocks = (unsigned)std::min<size_t>((p.total + WS_THREADS - 1) / WS_THREADS, (size_t)ctx->num_cus * 16);
      hipLaunchKernelGGL(wire_link_kernel, dim3(blocks), dim3(WS_THREADS), 0, st, buf[(p.passes - 1) & 1], ctl, sigma);
    }
    PM_HIP(ctx, hipGetLastError());
    PM_HIP(ctx, hipMemcpyAsync(ctl_host, ctl + CTL_COUNT, 8, hipMemcpyDeviceToHost, st));
    PM_HIP(ctx, hipStreamSynchronize(st));   // the verdict on the ids; the scratch is free to go
    return PM_OK;
  };
  rc = run();
  (void)pm_dev_free(ctx, scratch);
  if (rc != PM_OK) return rc;
  if (ctl_host[1] != 0xffffffffu)
    return set_err(ctx, PM_ERR_BAD_ARG, "wire_vars: the id at position " + std::to_string(ctl_host[1]) +
                                            " is neither below num_vars nor PM_PLONK_NO_VAR");
  return PM_OK;
}

int witness_from_vars(pm_ctx* ctx, const void* d_wire_vars, size_t n, const void* d_vars, size_t var_stride, uint32_t batch,
                      void* d_out, hipStream_t st) {
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (!st) st = ctx->stream;
  PM_HIP(ctx, hipSetDevice(ctx->device));
  ProfScope prof(ctx, st, "plonk_witness_gather");
  const unsigned blocks = (unsigned)std::min<size_t>((8 * n + 255) / 256, (size_t)ctx->num_cus * 16);
  hipLaunchKernelGGL(witness_gather_kernel, dim3(blocks, batch), dim3(256), 0, st, (const u32*)d_wire_vars, 4 * n,
                     (const uint4*)d_vars, var_stride, (uint4*)d_out);
  PM_HIP(ctx, hipGetLastError());
  return PM_OK;
}

}  // namespace pm

using namespace pm;

extern "C" int pm_plonk_sigma_from_wires_dev(pm_ctx* ctx, const void* d_wire_vars, size_t num_vars, size_t n,
                                             void* d_sigma_index_out, void* stream) {
  return sigma_index_from_wires(ctx, d_wire_vars, num_vars, n, d_sigma_index_out, (hipStream_t)stream);
}

extern "C" int pm_plonk_sigma_from_wires(pm_ctx* ctx, const uint32_t* wire_vars, size_t num_vars, size_t n,
                                         int64_t* sigma_index_out) {
  if (!ctx || !wire_vars || !sigma_index_out) return PM_ERR_BAD_ARG;
  WirePlan p;
  const int prc = wire_sort_plan(n, num_vars, p);
  if (prc == PM_ERR_LENGTH) return set_err(ctx, prc, "n must be a power of two in 4..2^29");
  if (prc != PM_OK) return set_err(ctx, prc, "num_vars must be below 2^32");
  void *d_wires = nullptr, *d_sigma = nullptr;
  int rc = pm_dev_alloc(ctx, 4 * n * 4, &d_wires);
  if (!rc) rc = pm_dev_alloc(ctx, 4 * n * 8, &d_sigma);
  if (!rc) rc = pm_dev_upload(ctx, d_wires, wire_vars, 4 * n * 4);
  if (!rc) rc = sigma_index_from_wires(ctx, d_wires, num_vars, n, d_sigma, nullptr);
  if (!rc) rc = pm_dev_download(ctx, sigma_index_out, d_sigma, 4 * n * 8);
  if (d_wires) (void)pm_dev_free(ctx, d_wires);
  if (d_sigma) (void)pm_dev_free(ctx, d_sigma);
  return rc;
}

extern "C" int pm_test_wire_sort_plan(size_t n, size_t num_vars, uint32_t* passes, uint32_t* tiles, size_t* scratch_bytes) {
  WirePlan p;
  const int rc = wire_sort_plan(n, num_vars, p);
  if (rc != PM_OK) return rc;
  if (passes) *passes = p.passes;
  if (tiles) *tiles = p.tiles;
  if (scratch_bytes) *scratch_bytes = p.scratch_bytes;
  return PM_OK;
}
