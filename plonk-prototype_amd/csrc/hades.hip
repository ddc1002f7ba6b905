// Native Poseidon: the Hades permutation of width 5 outside a circuit, the modelled sponge on top of it,
// an arity-4 Merkle tree and the sibling paths of its leaves.  gadgets.hip fills the ROWS of one permutation (25 lanes of a wave,
// every intermediate stored); here only the final state leaves the kernel, in two forms that produce the same bytes:
//
//   THREAD  one permutation per lane, the five words in registers in the device form (x 2^261).  Round keys and matrices are
//           wave-uniform: they sit in one device table in the constant address space, every index is uniform, so they arrive by
//           scalar loads and enter the multiply-adds as scalar operands -- no vector register and no LDS holds a constant.  A row
//           of the matrix is ONE reduction: the five products of a row go into the same column accumulators (45 limb products a
//           column set, 9 * 5 + 8 = 53 < 64 in units of 2^58: within the bound of fe_mont_cols for normalised operands), and the
//           next round's key is added at the columns above the radix, (T + key 2^261) / 2^261 = T / 2^261 + key.  A round is
//           5 x (405 + 72) limb products for the matrix and 117 + 117 + 153 for each s-box instead of 28 (or 40) x 153.
//           Values: state words are normalised limbs below 2.1 r throughout (5 * 2.1 r * r / 2^261 + r + key).
//   WAVE    lanes cooperate: lane 5 i + j of a half-wave holds word j and matrix entry (i, j) as in gadget_hades_kernel; two
//           permutations a wave (lanes 0..24 and 32..56).  Four dependent products a round instead of 28; lane (i, j) takes its
//           next word straight from the five products of row j (45 cross-lane reads a round, no second exchange).
//
// Both keep the sponge's state in registers across chunks; a tree level is the sponge on messages of four (no padding).  What is
// stored goes through fe_store: canonical whatever representative the form arrived at.
//
// Section 7.2n adds the tree in place: an update of k leaves that hashes only their ancestors (the two hash kernels again, with
// an argument block that takes slot i's node from a worklist in device memory; the worklists come from a compaction a level)
// and the verification of paths, `height` dependent permutations a path from the same rounds.
//
// Section 7.2r adds the append-only tree of ledger height (pm_poseidon_ledger): only the filled prefix of a level is stored, what
// lies to its right is the empty subtree of the level.  An append hashes the contiguous dirty range of every level (the two hash
// kernels with a third argument block, whose children beyond a stored prefix are that constant), the levels of one node included,
// up to the root, a launch a level; a truncate is that walk alone.
#include <hip/hip_runtime.h>

#include <string>
#include <type_traits>
#include <vector>

#include "context.h"
#include "hades.hip.h"
#include "poly_common.hip.h"

namespace pm {
namespace {

using host::HFr;

// ------------------------------------------------------------------ device side
struct HadesIo {
  u32x4* states;              // permute: n x 5 elements, in place
  const u32x4* msgs;          // hash: message i at element i * msg_stride
  u32x4* out;                 // hash: one element a message
  size_t n, msg_stride;
  u32 msg_len;
  u32 capacity[9];            // device form
};
// what an incremental tree update keeps in the caller's work area (section 7.2n): the verdict on the indices, the
// permutations run, and the length of every level's worklist
struct MerkleCtl {
  u64 bad;                    // the lowest offending position, ~0 = none
  u64 hashed;
  u32 cnt[PM_POSEIDON_MERKLE_MAX_HEIGHT + 1];
};
constexpr u64 MERKLE_NONE = ~0ull;
// the INDEXED hash: slot i hashes the four children of node ids[i] of one level.  n bounds the launch; the number of slots
// is ctl->cnt[level], nothing runs after a bad verdict.  msgs = the level below, out = the level itself.
struct HadesNodeIo : HadesIo {
  const u32* ids;
  const MerkleCtl* ctl;
  u32 level;
};
// the RANGE hash with defaults (section 7.2r): slot i hashes node first + i of one level of an append-only tree.  Child
// 4 (first + i) + c is read from the level below (msgs) when it is inside that level's stored prefix of `below` nodes and is
// the empty subtree of that level, *z, otherwise.  out = the level itself.  Nothing is materialised: what lies beyond a
// stored prefix is never read.
struct HadesRangeIo : HadesIo {
  u64 first, below;
  const u32x4* z;             // one canonical element: Z of the level below
};
PM_DEV size_t h_slots(const HadesIo& io) { return io.n; }
PM_DEV size_t h_slots(const HadesNodeIo& io) {
  const size_t have = io.ctl->bad == MERKLE_NONE ? io.ctl->cnt[io.level] : 0;
  return have < io.n ? have : io.n;
}
// slot -> its message; out_at = the element of its output
PM_DEV const u32x4* h_place(const HadesIo& io, size_t slot, size_t& out_at) {
  out_at = slot;
  return io.msgs + 2 * io.msg_stride * slot;
}
PM_DEV const u32x4* h_place(const HadesNodeIo& io, size_t slot, size_t& out_at) {
  out_at = io.ids[slot];
  return io.msgs + 8 * out_at;                               // the four children of the node
}
PM_DEV const u32x4* h_place(const HadesRangeIo& io, size_t slot, size_t& out_at) {
  out_at = io.first + slot;
  return io.msgs;                                            // the level below from its node 0: h_word indexes it by child
}
// word t (0..3) of the chunk at element `at` of slot's message (`left` elements to go); node = the slot's out_at
PM_DEV Fr h_word(const HadesIo&, const u32x4* msg, size_t, size_t at, u32 left, u32 t) { return h_chunk_word(msg, at, left, t); }
PM_DEV Fr h_word(const HadesRangeIo& io, const u32x4* msg, size_t node, size_t, u32, u32 t) {
  const u64 child = 4 * (u64)node + t;
  const bool stored = child < io.below;
  return h_to_dev(ld_canon(stored ? msg : io.z, stored ? child : 0));
}

template <bool HASH, class Io = HadesIo>
__global__ void __launch_bounds__(64) hades_thread_kernel(const HadesTab tab, const Io io) {
  const size_t idx = (size_t)blockIdx.x * 64 + threadIdx.x;
  if (idx >= h_slots(io)) return;
  Fr s[5];
  if (!HASH) {
    u32x4* const p = io.states + 10 * idx;
#pragma unroll
    for (int j = 0; j < 5; ++j) s[j] = h_absorb(h_to_dev(ld_canon(p, j)), fe_zero<FrP>(), tab.ark + 9 * j);
    h_rounds_thread(s, tab);
#pragma unroll
    for (int j = 0; j < 5; ++j) st_canon(p, j, h_to_abi(s[j]));
  } else {
    size_t out_at;
    const u32x4* const msg = h_place(io, idx, out_at);
#pragma unroll
    for (int i = 0; i < 9; ++i) s[0].l[i] = io.capacity[i];
#pragma unroll
    for (int j = 1; j < 5; ++j) s[j] = fe_zero<FrP>();
#pragma unroll 1
    for (u32 at = 0; at < io.msg_len; at += 4) {
      s[0] = h_absorb(s[0], fe_zero<FrP>(), tab.ark);
#pragma unroll
      for (int j = 1; j < 5; ++j) s[j] = h_absorb(s[j], h_word(io, msg, out_at, at, io.msg_len - at, j - 1), tab.ark + 9 * j);
      h_rounds_thread(s, tab);
    }
    st_canon(io.out, out_at, h_to_abi(s[1]));
  }
}

PM_DEV Fr h_shfl(const Fr& v, u32 src) {
  Fr r;
#pragma unroll
  for (int i = 0; i < 9; ++i) r.l[i] = __shfl(v.l[i], (int)src);
  return r;
}
PM_DEV Fr h_sel(bool c, const Fr& a, const Fr& b) {
  Fr r;
#pragma unroll
  for (int i = 0; i < 9; ++i) r.l[i] = c ? a.l[i] : b.l[i];
  return r;
}
PM_DEV Fr h_lane_const(const u32* p) {
  Fr r;
#pragma unroll
  for (int i = 0; i < 9; ++i) r.l[i] = p[i];
  return r;
}
// the rounds with lane (i, j) of a half-wave holding word j (keys of round 0 added) and entry (i, j); base = the half's lane 0.
// Every lane of the wave runs every round: the loop and the kind of a round depend on the parameters only.
PM_DEV Fr h_rounds_wave(Fr s, const u32* mds, const u32* ark, const HadesTab& tab, u32 base, u32 i, u32 j) {
  Fr m = h_lane_const(mds + 9 * (5 * i + j)), key = h_lane_const(ark + 45 + 9 * j);
#pragma unroll 1
  for (u32 rho = 0; rho < tab.rounds; ++rho) {
    const u32 nx = rho + 1 < tab.rounds ? rho + 1 : rho;   // the last round loads its own again
    const Fr m_n = h_lane_const(mds + (size_t)tab.mds_stride * nx + 9 * (5 * i + j));
    const Fr key_n = h_lane_const(ark + 45 * (size_t)(nx + 1) + 9 * j);
    const bool full = rho < tab.half_full || rho >= tab.rounds - tab.half_full;
    const Fr x5 = h_sbox(s);
    const Fr p = fe_mul<FrP>(m, h_sel(full || j == 4, x5, s));
    Fr sum = fe_add<FrP>(h_shfl(p, base + 5 * j), key);    // row j: the word this lane holds next
#pragma unroll
    for (u32 e = 1; e < 5; ++e) sum = fe_add<FrP>(sum, h_shfl(p, base + 5 * j + e));
    s = fe_reduce_weak<FrP>(sum);                          // limbs below 6 * 2^29, value below 6.1 r
    m = m_n, key = key_n;
  }
  return s;
}

template <bool HASH, class Io = HadesIo>
__global__ void __launch_bounds__(64) hades_wave_kernel(const HadesTab tab, const Io io) {
  const u32 lane = threadIdx.x, base = lane & 32u, l = (lane & 31u) < 25u ? (lane & 31u) : 24u;   // lanes 25..31 shadow lane 24
  const bool owner = (lane & 31u) < 25u;
  const u32 i = l / 5, j = l - 5 * i;
  size_t idx = 2 * (size_t)blockIdx.x + (base >> 5);
  const size_t n = h_slots(io);
  if (!std::is_same<Io, HadesIo>::value && 2 * (size_t)blockIdx.x >= n) return;   // a surplus wave: the whole wave leaves
  const bool live = idx < n;                               // an odd n: the last wave's second half repeats the first
  if (!live) idx = n - 1;
  const u32* const mds = (const u32*)tab.mds;
  const u32* const ark = (const u32*)tab.ark;
  const Fr key0 = h_lane_const(ark + 9 * j);
  if (!HASH) {
    u32x4* const p = io.states + 10 * idx;
    Fr s = fe_reduce_weak<FrP>(fe_add<FrP>(h_to_dev(ld_canon(p, j)), key0));
    s = h_rounds_wave(s, mds, ark, tab, base, i, j);
    if (live && owner && i == 0) st_canon(p, j, h_to_abi(s));
  } else {
    size_t out_at;
    const u32x4* const msg = h_place(io, idx, out_at);
    Fr s = fe_zero<FrP>();
    if (j == 0) {
#pragma unroll
      for (int k = 0; k < 9; ++k) s.l[k] = io.capacity[k];
    }
#pragma unroll 1
    for (u32 at = 0; at < io.msg_len; at += 4) {
      const Fr add = j == 0 ? fe_zero<FrP>() : h_word(io, msg, out_at, at, io.msg_len - at, j - 1);
      s = fe_reduce_weak<FrP>(fe_add<FrP>(fe_add<FrP>(s, add), key0));
      s = h_rounds_wave(s, mds, ark, tab, base, i, j);
    }
    if (live && owner && l == 1) st_canon(io.out, out_at, h_to_abi(s));
  }
}

// out[j][l][c] = child c of the level-(l + 1) ancestor of leaf idx[j]: node ((i >> 2l) & ~3) + c of level l (level 0 = the leaves)
__global__ void __launch_bounds__(256) merkle_paths_kernel(const u32x4* leaves, const u32x4* tree, u32 h, const u64* idx, size_t k,
                                                           u32x4* out) {
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;   // one thread a node: (j, l, c)
  if (t >= k * h * 4) return;
  const u32 c = (u32)(t & 3u), l = (u32)((t >> 2) % h);
  const size_t j = (t >> 2) / h;
  const u64 leaf = idx[j];
  if (leaf >> (2 * h)) return;                               // refused by the host after the call; nothing is read for it
  const u64 node = ((leaf >> (2 * l)) & ~3ull) + c;
  const u32x4* src = leaves;
  if (l) {
    u64 off = 0;                                             // levels 1..l-1 come before level l in the tree
    for (u32 q = 1; q < l; ++q) off += 1ull << (2 * (h - q));
    src = tree + 2 * off;
  }
  out[2 * t] = src[2 * node];
  out[2 * t + 1] = src[2 * node + 1];
}
__global__ void __launch_bounds__(256) merkle_index_check_kernel(const u64* idx, size_t k, u32 h, unsigned long long* bad) {
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (t < k && (idx[t] >> (2 * h))) atomicMin(bad, (unsigned long long)t);
}

// ---- incremental update (section 7.2n).  The worklist of level l holds the distinct node ids of that level, ascending; the
// list of level l + 1 is its heads -- the entries whose id >> 2 differs from the left neighbour's -- shifted and compacted in
// order.  Every kernel after the validation reads the verdict first and does nothing when it is bad.
constexpr u32 MERKLE_TILE = 128;   // worklist entries a workgroup of the compaction, one a thread: two waves

// the first position whose index is not below 4^h or not above its predecessor
__global__ void __launch_bounds__(256) merkle_update_check_kernel(const u64* idx, size_t k, u32 h, MerkleCtl* ctl) {
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= k) return;
  const u64 i = idx[t];
  if ((i >> (2 * h)) || (t && i <= idx[t - 1])) atomicMin((unsigned long long*)&ctl->bad, (unsigned long long)t);
}
// leaves[idx[t]] = values[t]; the worklist of level 0 is the indices themselves
__global__ void __launch_bounds__(256) merkle_update_scatter_kernel(const u64* idx, const u32x4* values, size_t k, u32x4* leaves,
                                                                    const MerkleCtl* ctl, u32* list) {
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (ctl->bad != MERKLE_NONE || t >= k) return;
  const u64 i = idx[t];                                      // below 4^h <= 2^30: the verdict is good
  leaves[2 * i] = values[2 * t];
  leaves[2 * i + 1] = values[2 * t + 1];
  list[t] = (u32)i;
}
PM_DEV u32 merkle_head(const u32* list, u32 t, u32 n) { return t < n && (t == 0 || (list[t] >> 2) != (list[t - 1] >> 2)) ? 1u : 0u; }
// exclusive prefix of v over the MERKLE_TILE threads of a workgroup, and the sum
PM_DEV u32 merkle_block_exclusive(u32 v, u32& total) {
  __shared__ u32 wsum[MERKLE_TILE / 64];
  const u32 lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  u32 inc = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const u32 t = __shfl_up(inc, d);
    if ((int)lane >= d) inc += t;
  }
  if (lane == 63u) wsum[wave] = inc;
  __syncthreads();
  u32 before = 0;
  total = 0;
#pragma unroll
  for (u32 w = 0; w < MERKLE_TILE / 64; ++w) {
    const u32 t = wsum[w];
    if (w < wave) before += t;
    total += t;
  }
  __syncthreads();                                           // wsum may be written again
  return before + inc - v;
}
// sums[tile] = the heads of one tile of the level's worklist; a tile past the list's end writes 0
__global__ void __launch_bounds__(MERKLE_TILE) merkle_heads_kernel(const MerkleCtl* ctl, u32 level, const u32* list, u32* sums) {
  if (ctl->bad != MERKLE_NONE) return;
  u32 total;
  merkle_block_exclusive(merkle_head(list, blockIdx.x * MERKLE_TILE + threadIdx.x, ctl->cnt[level]), total);
  if (threadIdx.x == 0) sums[blockIdx.x] = total;
}
// one workgroup: sums -> their exclusive prefixes; the total is the length of the next level's list and what that level hashes
__global__ void __launch_bounds__(MERKLE_TILE) merkle_tile_scan_kernel(MerkleCtl* ctl, u32 level, u32* sums, u32 tiles) {
  if (ctl->bad != MERKLE_NONE) return;
  const u32 per = (tiles + MERKLE_TILE - 1) / MERKLE_TILE, first = threadIdx.x * per;
  u32 mine = 0, total;
  for (u32 j = first; j < first + per && j < tiles; ++j) mine += sums[j];
  u32 at = merkle_block_exclusive(mine, total);
  for (u32 j = first; j < first + per && j < tiles; ++j) {
    const u32 c = sums[j];
    sums[j] = at;
    at += c;
  }
  if (threadIdx.x == 0) ctl->cnt[level + 1] = total, ctl->hashed += total;
}
// next[sums[tile] + rank] = list[t] >> 2 for every head t.  ALONE: the launch is this one tile; it keeps the count itself.
template <bool ALONE>
__global__ void __launch_bounds__(MERKLE_TILE) merkle_compact_kernel(MerkleCtl* ctl, u32 level, const u32* list, const u32* sums,
                                                                     u32* next) {
  if (ctl->bad != MERKLE_NONE) return;
  const u32 t = blockIdx.x * MERKLE_TILE + threadIdx.x;
  const u32 head = merkle_head(list, t, ctl->cnt[level]);
  u32 total;
  const u32 rank = merkle_block_exclusive(head, total);
  if (head) next[(ALONE ? 0u : sums[blockIdx.x]) + rank] = list[t] >> 2;
  if (ALONE && threadIdx.x == 0) ctl->cnt[level + 1] = total, ctl->hashed += total;
}

// ---- path verification (section 7.2n): `h` dependent permutations a path; the hash of a level stays in registers and is
// compared, canonical, with the child the next level holds at the path's position (the root after the last level)
struct MerkleVerifyIo {
  const u32x4* paths;         // [k][h][4]
  const u64* idx;
  const u32x4* root;
  u32* status;
  size_t k;
  u32 h;
  u32 capacity[9];            // device form
};
PM_DEV bool merkle_same(const Fr& hash, const u32x4* want) {
  u32 s[8];
  fe_canon_pack<FrP>(s, h_to_abi(hash));
  const u32x4 a = want[0], b = want[1];
  return s[0] == a.x && s[1] == a.y && s[2] == a.z && s[3] == a.w && s[4] == b.x && s[5] == b.y && s[6] == b.z && s[7] == b.w;
}
// the element the hash of path level l must equal
PM_DEV const u32x4* merkle_successor(const MerkleVerifyIo& io, const u32x4* path, u64 leaf, u32 l) {
  return l + 1 < io.h ? path + 2 * (4 * (size_t)(l + 1) + ((leaf >> (2 * (l + 1))) & 3u)) : io.root;
}

__global__ void __launch_bounds__(64) merkle_verify_thread_kernel(const HadesTab tab, const MerkleVerifyIo io) {
  const size_t p = (size_t)blockIdx.x * 64 + threadIdx.x;
  if (p >= io.k) return;
  const u64 leaf = io.idx[p];
  if (leaf >> (2 * io.h)) {
    io.status[p] = PM_MERKLE_PATH_INDEX;                     // nothing of the path is read
    return;
  }
  const u32x4* const path = io.paths + 8 * (size_t)io.h * p;
  u32 status = PM_MERKLE_PATH_OK;
  Fr s[5];
#pragma unroll 1
  for (u32 l = 0; l < io.h; ++l) {
#pragma unroll
    for (int i = 0; i < 9; ++i) s[0].l[i] = io.capacity[i];
    s[0] = h_absorb(s[0], fe_zero<FrP>(), tab.ark);
#pragma unroll
    for (int j = 1; j < 5; ++j) s[j] = h_absorb(fe_zero<FrP>(), h_to_dev(ld_canon(path, 4 * (size_t)l + j - 1)), tab.ark + 9 * j);
    h_rounds_thread(s, tab);
    if (!merkle_same(s[1], merkle_successor(io, path, leaf, l))) {
      status = PM_MERKLE_PATH_LINK + l;                      // the lowest failing level
      break;
    }
  }
  io.status[p] = status;
}

__global__ void __launch_bounds__(64) merkle_verify_wave_kernel(const HadesTab tab, const MerkleVerifyIo io) {
  const u32 lane = threadIdx.x, base = lane & 32u, l = (lane & 31u) < 25u ? (lane & 31u) : 24u;   // as in hades_wave_kernel
  const bool owner = (lane & 31u) < 25u;
  const u32 i = l / 5, j = l - 5 * i;
  size_t p = 2 * (size_t)blockIdx.x + (base >> 5);
  const bool live = p < io.k;
  if (!live) p = io.k - 1;
  const u32* const mds = (const u32*)tab.mds;
  const u32* const ark = (const u32*)tab.ark;
  const Fr key0 = h_lane_const(ark + 9 * j);
  const u64 leaf = io.idx[p];
  const bool readable = !(leaf >> (2 * io.h));               // an index out of range: its half runs the rounds on zeros
  const u32x4* const path = io.paths + 8 * (size_t)io.h * p;
  u32 status = readable ? PM_MERKLE_PATH_OK : PM_MERKLE_PATH_INDEX;
#pragma unroll 1
  for (u32 lv = 0; lv < io.h; ++lv) {
    Fr s = fe_zero<FrP>();
    if (j == 0) {
#pragma unroll
      for (int k = 0; k < 9; ++k) s.l[k] = io.capacity[k];
    } else if (readable) {
      s = h_to_dev(ld_canon(path, 4 * (size_t)lv + j - 1));
    }
    s = fe_reduce_weak<FrP>(fe_add<FrP>(s, key0));
    s = h_rounds_wave(s, mds, ark, tab, base, i, j);
    if (readable && l == 1 && status == PM_MERKLE_PATH_OK && !merkle_same(s, merkle_successor(io, path, leaf, lv)))
      status = PM_MERKLE_PATH_LINK + lv;
  }
  if (live && owner && l == 1) io.status[p] = status;
}

// ---- the append-only tree (section 7.2r).  The slab holds level l at element ledger_offset(reserve, l): the levels one after
// the other, level q with room for ceil(reserve / 4^q) nodes; level l stores the nodes below ledger_width(count, l).
__host__ __device__ inline u64 ledger_width(u64 leaves, u32 l) { return (leaves + ((1ull << (2 * l)) - 1)) >> (2 * l); }
__host__ __device__ inline u64 ledger_offset(u64 reserve, u32 l) {
  u64 off = 0;
  for (u32 q = 0; q < l; ++q) off += ledger_width(reserve, q);
  return off;
}
struct LedgerView {
  const u32x4* slab;
  const u32x4* z;             // Z_0 .. Z_h, canonical
  u64 count, reserve;
  u32 h;
};
// merkle_paths_kernel with defaults: a node at or beyond its level's stored prefix is that level's Z
__global__ void __launch_bounds__(256) ledger_paths_kernel(const LedgerView v, const u64* idx, size_t k, u32x4* out) {
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;   // one thread a node: (j, l, c)
  if (t >= k * v.h * 4) return;
  const u32 c = (u32)(t & 3u), l = (u32)((t >> 2) % v.h);
  const size_t j = (t >> 2) / v.h;
  const u64 leaf = idx[j];
  if (leaf >= v.count) return;                               // refused by the host after the call; nothing is read for it
  const u64 node = ((leaf >> (2 * l)) & ~3ull) + c;
  const u32x4* const src = node < ledger_width(v.count, l) ? v.slab + 2 * (ledger_offset(v.reserve, l) + node) : v.z + 2 * l;
  out[2 * t] = src[0];
  out[2 * t + 1] = src[1];
}
__global__ void __launch_bounds__(256) ledger_index_check_kernel(const u64* idx, size_t k, u64 count, unsigned long long* bad) {
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (t < k && idx[t] >= count) atomicMin(bad, (unsigned long long)t);
}

// ------------------------------------------------------------------ launches
// AUTO: the WAVE form below this many permutations, the THREAD form from it on.  Measured at (67, 8), DESIGN.md section 7.2j:
// THREAD takes 0.48 ms for anything up to one wave a SIMD, WAVE grows by 0.054 ms a 1024 permutations and meets it at 8192.
constexpr size_t HADES_AUTO_CROSSOVER = 8192;

bool use_wave(size_t n, uint32_t flags) { return flags == PM_HADES_FORM_WAVE || (flags == PM_HADES_FORM_AUTO && n < HADES_AUTO_CROSSOVER); }

template <bool HASH, class Io>
hipError_t launch(const pm_hades_params* p, const Io& io, uint32_t flags, hipStream_t st) {
  const HadesTab tab = tab_of(p);
  if (use_wave(io.n, flags))
    hipLaunchKernelGGL((hades_wave_kernel<HASH, Io>), dim3((unsigned)((io.n + 1) / 2)), dim3(64), 0, st, tab, io);
  else
    hipLaunchKernelGGL((hades_thread_kernel<HASH, Io>), dim3((unsigned)((io.n + 63) / 64)), dim3(64), 0, st, tab, io);
  return hipGetLastError();
}

int common_fault(pm_ctx* ctx, const pm_hades_params* p, uint32_t flags) {
  if (int rc = params_fault(ctx, p)) return rc;
  if (flags > PM_HADES_FORM_WAVE) return set_err(ctx, PM_ERR_BAD_ARG, "flags must be PM_HADES_FORM_AUTO, _THREAD or _WAVE");
  return PM_OK;
}

// ark [R][5], mds [n_mds][5][5] (validated) -> the handle with its device table
int params_build(pm_ctx* ctx, uint32_t R, uint32_t F, const uint64_t* ark, const uint64_t* mds, uint32_t n_mds, pm_hades_params** out) {
  std::vector<u32> tab(225 * (size_t)n_mds + 45 * ((size_t)R + 1), 0u);
  for (size_t k = 0; k < 25 * (size_t)n_mds; ++k) to_limbs29(&tab[9 * k], hfr_load(mds + 4 * k));
  u32* const a = &tab[225 * (size_t)n_mds];
  for (size_t k = 0; k < 5 * (size_t)R; ++k) to_limbs29(a + 9 * k, hfr_load(ark + 4 * k));
  std::lock_guard<std::mutex> lk(ctx->mu);
  PM_HIP(ctx, hipSetDevice(ctx->device));
  void* d = nullptr;
  PM_HIP(ctx, hipMalloc(&d, tab.size() * 4));
  const hipError_t e = hipMemcpy(d, tab.data(), tab.size() * 4, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    (void)hipFree(d);
    return set_err(ctx, PM_ERR_HIP, std::string("hipMemcpy: ") + hipGetErrorString(e));
  }
  pm_hades_params* p = new pm_hades_params();
  p->device = ctx->device, p->rounds = R, p->full = F, p->n_mds = n_mds, p->d_tab = d;
  p->ark.assign(ark, ark + 20 * (size_t)R), p->mds.assign(mds, mds + 100 * (size_t)n_mds);
  *out = p;
  return PM_OK;
}

}  // namespace

// context.h: the rounds gathered for a HADES gadget (GadgetTables::hcoef at its offset: R x 30 canonical coefficients, 25 matrix
// entries then 5 round keys) -> a handle with a matrix a round.  Waits for the context's stream.
int hades_params_from_rounds(pm_ctx* ctx, const void* d_rounds, uint32_t R, uint32_t F, pm_hades_params** out) {
  std::vector<uint64_t> raw(120 * (size_t)R), ark(20 * (size_t)R), mds(100 * (size_t)R);
  {
    std::lock_guard<std::mutex> lk(ctx->mu);
    PM_HIP(ctx, hipSetDevice(ctx->device));
    PM_HIP(ctx, hipStreamSynchronize(ctx->stream));
    PM_HIP(ctx, hipMemcpy(raw.data(), d_rounds, raw.size() * 8, hipMemcpyDeviceToHost));
  }
  for (size_t rho = 0; rho < R; ++rho) {
    memcpy(&mds[100 * rho], &raw[120 * rho], 800);
    memcpy(&ark[20 * rho], &raw[120 * rho + 100], 160);
  }
  const std::string why = params_fault(R, F, ark.data(), mds.data(), R);
  if (!why.empty()) return set_err(ctx, PM_ERR_BAD_ARG, "pm_hades_params_from_key: " + why);
  return params_build(ctx, R, F, ark.data(), mds.data(), R, out);
}

}  // namespace pm

using namespace pm;

extern "C" int pm_hades_params_create(pm_ctx* ctx, uint32_t rounds, uint32_t full_rounds, const uint64_t* ark, const uint64_t* mds,
                                      uint32_t n_mds, pm_hades_params** out) {
  if (!ctx || !out) return PM_ERR_BAD_ARG;
  const std::string why = params_fault(rounds, full_rounds, ark, mds, n_mds);
  if (!why.empty()) return set_err(ctx, PM_ERR_BAD_ARG, "pm_hades_params_create: " + why);
  return params_build(ctx, rounds, full_rounds, ark, mds, n_mds, out);
}

extern "C" int pm_hades_params_info(const pm_hades_params* params, uint32_t* rounds, uint32_t* full_rounds, uint32_t* n_mds) {
  if (!params) return PM_ERR_BAD_ARG;
  if (rounds) *rounds = params->rounds;
  if (full_rounds) *full_rounds = params->full;
  if (n_mds) *n_mds = params->n_mds;
  return PM_OK;
}

extern "C" void pm_hades_params_free(pm_ctx* ctx, pm_hades_params* params) {
  if (!params) return;
  if (ctx) {
    std::lock_guard<std::mutex> lk(ctx->mu);
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    if (params->d_tab) (void)hipFree(params->d_tab);   // hipFree waits for the device: launches on caller streams included
  }
  delete params;
}

extern "C" int pm_hades_permute_dev(pm_ctx* ctx, const pm_hades_params* params, void* d_states, size_t n, uint32_t flags,
                                    void* hip_stream) {
  if (!ctx) return PM_ERR_BAD_ARG;
  if (int rc = common_fault(ctx, params, flags)) return rc;
  if (n == 0) return PM_OK;
  if (int rc = pointer_fault(ctx, {d_states})) return rc;
  if (int rc = count_fault(ctx, n)) return rc;
  PM_ENTER(ctx, hip_stream, st);
  HadesIo io{};
  io.states = (u32x4*)d_states, io.n = n;
  ProfScope prof(ctx, st, "hades_permute");
  PM_HIP(ctx, launch<false>(params, io, flags, st));
  return PM_OK;
}

extern "C" int pm_poseidon_hash_dev(pm_ctx* ctx, const pm_hades_params* params, const uint64_t capacity[4], const void* d_msgs,
                                    size_t msg_len, size_t msg_stride, size_t n, void* d_out, uint32_t flags, void* hip_stream) {
  if (!ctx) return PM_ERR_BAD_ARG;
  if (int rc = common_fault(ctx, params, flags)) return rc;
  HadesIo io{};
  if (int rc = capacity_to_dev(ctx, capacity, io.capacity)) return rc;
  if (msg_len == 0 || msg_len > 0xffffffffull) return set_err(ctx, PM_ERR_BAD_ARG, "msg_len must be in 1 .. 2^32 - 1");
  if (msg_stride < msg_len) return set_err(ctx, PM_ERR_BAD_ARG, "msg_stride is below msg_len");
  if (n == 0) return PM_OK;
  if (int rc = pointer_fault(ctx, {d_msgs, d_out})) return rc;
  if (int rc = count_fault(ctx, n)) return rc;
  if (overlap(d_msgs, ((n - 1) * msg_stride + msg_len) * 32, d_out, n * 32)) return set_err(ctx, PM_ERR_BAD_ARG, "d_out overlaps d_msgs");
  PM_ENTER(ctx, hip_stream, st);
  io.msgs = (const u32x4*)d_msgs, io.out = (u32x4*)d_out, io.n = n, io.msg_stride = msg_stride, io.msg_len = (u32)msg_len;
  ProfScope prof(ctx, st, "poseidon_hash");
  PM_HIP(ctx, launch<true>(params, io, flags, st));
  return PM_OK;
}

extern "C" int pm_poseidon_merkle_dev(pm_ctx* ctx, const pm_hades_params* params, const uint64_t capacity[4], const void* d_leaves,
                                      uint32_t height, void* d_tree, uint32_t flags, void* hip_stream) {
  if (!ctx) return PM_ERR_BAD_ARG;
  if (int rc = common_fault(ctx, params, flags)) return rc;
  HadesIo io{};
  if (int rc = capacity_to_dev(ctx, capacity, io.capacity)) return rc;
  if (height < 1 || height > PM_POSEIDON_MERKLE_MAX_HEIGHT) return set_err(ctx, PM_ERR_BAD_ARG, "height must be in 1 .. 15");
  if (int rc = pointer_fault(ctx, {d_leaves, d_tree})) return rc;
  const size_t leaves = (size_t)1 << (2 * height);
  if (overlap(d_leaves, leaves * 32, d_tree, (leaves - 1) / 3 * 32)) return set_err(ctx, PM_ERR_BAD_ARG, "d_tree overlaps d_leaves");
  PM_ENTER(ctx, hip_stream, st);
  ProfScope prof(ctx, st, "poseidon_merkle");
  const u32x4* below = (const u32x4*)d_leaves;
  u32x4* level = (u32x4*)d_tree;
  io.msg_len = 4, io.msg_stride = 4;
  for (uint32_t l = 1; l <= height; ++l) {                   // a launch a level: level l reads level l - 1
    io.n = (size_t)1 << (2 * (height - l));
    io.msgs = below, io.out = level;
    PM_HIP(ctx, launch<true>(params, io, flags, st));
    below = level, level += 2 * io.n;
  }
  return PM_OK;
}

extern "C" int pm_poseidon_merkle_paths_dev(pm_ctx* ctx, const void* d_leaves, const void* d_tree, uint32_t height,
                                            const void* d_indices, size_t k, void* d_out, void* hip_stream) {
  if (!ctx) return PM_ERR_BAD_ARG;
  if (height < 1 || height > PM_POSEIDON_MERKLE_MAX_HEIGHT) return set_err(ctx, PM_ERR_BAD_ARG, "height must be in 1 .. 15");
  if (k == 0) return PM_OK;
  if (int rc = pointer_fault(ctx, {d_leaves, d_tree, d_out}, !d_indices || ((uintptr_t)d_indices & 7u))) return rc;
  if (k > 0x7fffffffu / (4 * height)) return set_err(ctx, PM_ERR_LENGTH, "too many paths for one call");
  PM_ENTER(ctx, hip_stream, st);
  unsigned long long* d_bad = nullptr;
  unsigned long long bad = ~0ull;
  PM_HIP(ctx, hipMalloc((void**)&d_bad, 8));
  hipError_t e = hipMemcpyAsync(d_bad, &bad, 8, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(merkle_index_check_kernel, dim3((unsigned)((k + 255) / 256)), dim3(256), 0, st, (const u64*)d_indices, k,
                       height, d_bad);
    const size_t nodes = k * height * 4;
    hipLaunchKernelGGL(merkle_paths_kernel, dim3((unsigned)((nodes + 255) / 256)), dim3(256), 0, st, (const u32x4*)d_leaves,
                       (const u32x4*)d_tree, height, (const u64*)d_indices, k, (u32x4*)d_out);
    e = hipGetLastError();
  }
  if (int rc = finish_call(ctx, e, st, &bad, d_bad, 8, d_bad, "pm_poseidon_merkle_paths_dev")) return rc;
  if (bad != ~0ull) return set_err(ctx, PM_ERR_BAD_ARG, "index " + std::to_string(bad) + " is not below 4^height");
  return PM_OK;
}

namespace {
// the caller's work area of an update: the control block, a sum a tile of the compaction, the worklists of two levels
struct MerkleWork {
  size_t sums, list0, list1, bytes;
};
MerkleWork merkle_work(size_t k) {
  const auto a16 = [](size_t x) { return (x + 15) & ~(size_t)15; };
  MerkleWork w{};
  if (k == 0) return w;
  static_assert(sizeof(MerkleCtl) <= 128, "the control block has 128 bytes");
  w.sums = 128;
  w.list0 = w.sums + a16(4 * ((k + MERKLE_TILE - 1) / MERKLE_TILE));
  w.list1 = w.list0 + a16(4 * k);
  w.bytes = w.list1 + a16(4 * k);
  return w;
}
}  // namespace

extern "C" size_t pm_poseidon_merkle_update_work_bytes(size_t k) { return merkle_work(k).bytes; }

extern "C" int pm_poseidon_merkle_update_dev(pm_ctx* ctx, const pm_hades_params* params, const uint64_t capacity[4], void* d_leaves,
                                             void* d_tree, uint32_t height, const void* d_indices, const void* d_values, size_t k,
                                             void* d_work, uint32_t flags, uint64_t* hashed, void* hip_stream) {
  if (!ctx) return PM_ERR_BAD_ARG;
  if (int rc = common_fault(ctx, params, flags)) return rc;
  HadesNodeIo io{};
  if (int rc = capacity_to_dev(ctx, capacity, io.capacity)) return rc;
  if (height < 1 || height > PM_POSEIDON_MERKLE_MAX_HEIGHT) return set_err(ctx, PM_ERR_BAD_ARG, "height must be in 1 .. 15");
  if (hashed) *hashed = 0;
  if (k == 0) return PM_OK;
  if (int rc = pointer_fault(ctx, {d_leaves, d_tree, d_values, d_work}, !d_indices || ((uintptr_t)d_indices & 7u))) return rc;
  const size_t leaves = (size_t)1 << (2 * height), nodes = (leaves - 1) / 3;
  if (k > leaves) return set_err(ctx, PM_ERR_BAD_ARG, "more indices than leaves: they cannot be strictly ascending");
  const MerkleWork w = merkle_work(k);
  if (overlap(d_leaves, leaves * 32, d_tree, nodes * 32)) return set_err(ctx, PM_ERR_BAD_ARG, "d_tree overlaps d_leaves");
  const struct { const void* p; size_t bytes; const char* name; } ins[3] = {{d_values, k * 32, "d_values"}, {d_work, w.bytes, "d_work"},
                                                                          {d_indices, k * 8, "d_indices"}};
  for (const auto& in : ins)
    if (overlap(in.p, in.bytes, d_leaves, leaves * 32) || overlap(in.p, in.bytes, d_tree, nodes * 32))
      return set_err(ctx, PM_ERR_BAD_ARG, std::string(in.name) + " overlaps the leaves or the tree");
  PM_ENTER(ctx, hip_stream, st);
  ProfScope prof(ctx, st, "poseidon_merkle_update");
  MerkleCtl* const ctl = (MerkleCtl*)d_work;
  u32* const sums = (u32*)((char*)d_work + w.sums);
  u32* const list[2] = {(u32*)((char*)d_work + w.list0), (u32*)((char*)d_work + w.list1)};
  MerkleCtl start{};
  start.bad = MERKLE_NONE, start.cnt[0] = (u32)k;
  hipError_t e = hipMemcpyAsync(ctl, &start, sizeof start, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) {
    const unsigned blocks = (unsigned)((k + 255) / 256);
    hipLaunchKernelGGL(merkle_update_check_kernel, dim3(blocks), dim3(256), 0, st, (const u64*)d_indices, k, height, ctl);
    hipLaunchKernelGGL(merkle_update_scatter_kernel, dim3(blocks), dim3(256), 0, st, (const u64*)d_indices, (const u32x4*)d_values, k,
                       (u32x4*)d_leaves, ctl, list[0]);
    e = hipGetLastError();
  }
  const u32x4* below = (const u32x4*)d_leaves;
  u32x4* level = (u32x4*)d_tree;
  io.msg_len = 4, io.msg_stride = 4, io.ctl = ctl;
  size_t bound = k;                                          // of the list of level l - 1: min(k, 4^(height - l + 1))
  for (uint32_t l = 1; l <= height && e == hipSuccess; ++l) {
    const u32 tiles = (u32)((bound + MERKLE_TILE - 1) / MERKLE_TILE);
    const u32* const from = list[(l - 1) & 1];
    u32* const to = list[l & 1];
    if (tiles == 1) {
      hipLaunchKernelGGL(merkle_compact_kernel<true>, dim3(1), dim3(MERKLE_TILE), 0, st, ctl, l - 1, from, (const u32*)sums, to);
    } else {
      hipLaunchKernelGGL(merkle_heads_kernel, dim3(tiles), dim3(MERKLE_TILE), 0, st, (const MerkleCtl*)ctl, l - 1, from, sums);
      hipLaunchKernelGGL(merkle_tile_scan_kernel, dim3(1), dim3(MERKLE_TILE), 0, st, ctl, l - 1, sums, tiles);
      hipLaunchKernelGGL(merkle_compact_kernel<false>, dim3(tiles), dim3(MERKLE_TILE), 0, st, ctl, l - 1, from, (const u32*)sums, to);
    }
    const size_t width = (size_t)1 << (2 * (height - l));
    bound = k < width ? k : width;
    io.n = bound, io.ids = to, io.level = l, io.msgs = below, io.out = level;
    e = launch<true>(params, io, flags, st);
    below = level, level += 2 * width;
  }
  u64 verdict[2] = {0, 0};                                   // MerkleCtl::bad, ::hashed: one copy, one wait
  if (e == hipSuccess) e = hipMemcpyAsync(verdict, ctl, sizeof verdict, hipMemcpyDeviceToHost, st);
  const hipError_t waited = hipStreamSynchronize(st);
  if (e == hipSuccess) e = waited;
  if (e != hipSuccess) return set_err(ctx, PM_ERR_HIP, std::string("pm_poseidon_merkle_update_dev: ") + hipGetErrorString(e));
  if (verdict[0] != MERKLE_NONE)
    return set_err(ctx, PM_ERR_BAD_ARG, "index " + std::to_string(verdict[0]) + " is not below 4^height or not above its predecessor");
  if (hashed) *hashed = verdict[1];
  return PM_OK;
}

namespace {
// the two verification entries: the dense tree's, which refuses what its tree cannot be (height > 15), and the ledger tree's
int merkle_verify(pm_ctx* ctx, const pm_hades_params* params, const uint64_t capacity[4], const void* d_paths, const void* d_indices,
                  size_t k, uint32_t height, uint32_t max_height, const void* d_root, void* d_status, uint32_t flags, void* hip_stream) {
  if (!ctx) return PM_ERR_BAD_ARG;
  if (int rc = common_fault(ctx, params, flags)) return rc;
  MerkleVerifyIo io{};
  if (int rc = capacity_to_dev(ctx, capacity, io.capacity)) return rc;
  if (height < 1 || height > max_height) return set_err(ctx, PM_ERR_BAD_ARG, "height must be in 1 .. " + std::to_string(max_height));
  if (k == 0) return PM_OK;
  if (int rc = pointer_fault(ctx, {d_paths, d_root}, !d_indices || !d_status || ((uintptr_t)d_indices & 7u) || ((uintptr_t)d_status & 3u)))
    return rc;
  if (k > 0x7fffffffu) return set_err(ctx, PM_ERR_LENGTH, "k > 2^31");
  if (overlap(d_status, k * 4, d_paths, k * height * 128) || overlap(d_status, k * 4, d_indices, k * 8) ||
      overlap(d_status, k * 4, d_root, 32))
    return set_err(ctx, PM_ERR_BAD_ARG, "d_status overlaps an input");
  PM_ENTER(ctx, hip_stream, st);
  io.paths = (const u32x4*)d_paths, io.idx = (const u64*)d_indices, io.root = (const u32x4*)d_root, io.status = (u32*)d_status;
  io.k = k, io.h = height;
  const HadesTab tab = tab_of(params);
  ProfScope prof(ctx, st, "poseidon_merkle_verify");
  if (use_wave(k, flags))
    hipLaunchKernelGGL(merkle_verify_wave_kernel, dim3((unsigned)((k + 1) / 2)), dim3(64), 0, st, tab, io);
  else
    hipLaunchKernelGGL(merkle_verify_thread_kernel, dim3((unsigned)((k + 63) / 64)), dim3(64), 0, st, tab, io);
  PM_HIP(ctx, hipGetLastError());
  return PM_OK;
}
}  // namespace

extern "C" int pm_poseidon_merkle_verify_dev(pm_ctx* ctx, const pm_hades_params* params, const uint64_t capacity[4],
                                             const void* d_paths, const void* d_indices, size_t k, uint32_t height, const void* d_root,
                                             void* d_status, uint32_t flags, void* hip_stream) {
  return merkle_verify(ctx, params, capacity, d_paths, d_indices, k, height, PM_POSEIDON_MERKLE_MAX_HEIGHT, d_root, d_status, flags,
                       hip_stream);
}

extern "C" int pm_poseidon_ledger_verify_dev(pm_ctx* ctx, const pm_hades_params* params, const uint64_t capacity[4],
                                             const void* d_paths, const void* d_indices, size_t k, uint32_t height, const void* d_root,
                                             void* d_status, uint32_t flags, void* hip_stream) {
  return merkle_verify(ctx, params, capacity, d_paths, d_indices, k, height, PM_POSEIDON_LEDGER_MAX_HEIGHT, d_root, d_status, flags,
                       hip_stream);
}

// ------------------------------------------------------------------ the append-only tree
struct pm_poseidon_ledger {
  int device = 0;
  uint32_t height = 0;
  uint64_t count = 0, reserve = 0;        // filled leaves; leaves the slab has room for
  pm_hades_params own;                    // a copy of the constants with its own device table
  u32 capacity[9] = {};                   // device form
  std::vector<uint64_t> z;                // Z_0 .. Z_height, canonical: the host's copy of d_z
  void* d_slab = nullptr;                 // level l at element ledger_offset(reserve, l)
  void* d_z = nullptr;
  void* d_root = nullptr;                 // one element, current after every call
  void* d_bad = nullptr;                  // one u64: the verdict of a paths call's index check
};

namespace {
// What an append of k leaves at `count` hashes (the definitions of section 7.2r); index l, 1 <= l <= height.
struct LedgerPlan {
  u64 first[PM_POSEIDON_LEDGER_MAX_HEIGHT + 1], nodes[PM_POSEIDON_LEDGER_MAX_HEIGHT + 1], below[PM_POSEIDON_LEDGER_MAX_HEIGHT + 1];
  u32 chain_from;                         // the first level whose range is one node (one node a level from there on); 0 for k = 0
  u64 hashed;
};
u64 ledger_positions(u32 height) { return 1ull << (2 * height); }
size_t table_bytes(const pm_hades_params& p) { return (225 * (size_t)p.n_mds + 45 * ((size_t)p.rounds + 1)) * 4; }
int ledger_plan(u32 height, u64 count, u64 k, LedgerPlan* p) {
  *p = LedgerPlan{};
  if (height < 1 || height > PM_POSEIDON_LEDGER_MAX_HEIGHT || count > ledger_positions(height)) return PM_ERR_BAD_ARG;
  if (k > 0x7fffffffu || k > ledger_positions(height) - count) return PM_ERR_LENGTH;
  if (k == 0) return PM_OK;
  const u64 last = count + k - 1;
  for (u32 l = 1; l <= height; ++l) {
    p->first[l] = count >> (2 * l);
    p->nodes[l] = (last >> (2 * l)) - p->first[l] + 1;
    p->below[l] = ledger_width(count + k, l - 1);
    p->hashed += p->nodes[l];
    if (!p->chain_from && p->nodes[l] == 1) p->chain_from = l;
  }
  return PM_OK;
}

int ledger_fault(pm_ctx* ctx, const pm_poseidon_ledger* t) {
  if (!t) return set_err(ctx, PM_ERR_BAD_ARG, "null ledger");
  if (t->device != ctx->device) return set_err(ctx, PM_ERR_BAD_ARG, "the ledger belongs to another device");
  return PM_OK;
}
// [p, p + bytes) shares a byte with device memory the handle owns
bool ledger_owns(const pm_poseidon_ledger* t, const void* p, size_t bytes) {
  return overlap(p, bytes, t->d_slab, pm_poseidon_ledger_bytes(t->height, t->reserve)) ||
         overlap(p, bytes, t->d_z, 32 * ((size_t)t->height + 1)) || overlap(p, bytes, t->d_root, 32) || overlap(p, bytes, t->d_bad, 8);
}
u32x4* ledger_level_ptr(const pm_poseidon_ledger* t, u32 l) { return (u32x4*)t->d_slab + 2 * ledger_offset(t->reserve, l); }

// The levels of the plan on the stream, a range launch each, and a copy of the root to the handle's own element.  One launch
// that walks the single-node levels with the hash in registers was built and measured: 1.4 to 1.7 % of a one-leaf append,
// inside the spread at one of four points, so it was not kept.
hipError_t ledger_hash(pm_poseidon_ledger* t, const LedgerPlan& plan, uint32_t flags, hipStream_t st) {
  const u32 H = t->height;
  HadesRangeIo io{};
  memcpy(io.capacity, t->capacity, sizeof io.capacity);
  io.msg_len = 4, io.msg_stride = 4;
  for (u32 l = 1; l <= H; ++l) {
    io.n = (size_t)plan.nodes[l], io.first = plan.first[l], io.below = plan.below[l];
    io.msgs = ledger_level_ptr(t, l - 1), io.out = ledger_level_ptr(t, l), io.z = (const u32x4*)t->d_z + 2 * (l - 1);
    if (hipError_t e = launch<true>(&t->own, io, flags, st)) return e;
  }
  return hipMemcpyAsync(t->d_root, ledger_level_ptr(t, H), 32, hipMemcpyDeviceToDevice, st);
}

// a slab with room for `reserve` leaves that holds the stored prefixes of the current one; waits for the stream
int ledger_grow(pm_ctx* ctx, pm_poseidon_ledger* t, u64 reserve, hipStream_t st) {
  const size_t bytes = pm_poseidon_ledger_bytes(t->height, reserve);
  void* d = nullptr;
  PM_HIP(ctx, hipMalloc(&d, bytes));
  hipError_t e = hipSuccess;
  for (u32 l = 0; l <= t->height && e == hipSuccess && t->count; ++l)
    e = hipMemcpyAsync((u32x4*)d + 2 * ledger_offset(reserve, l), ledger_level_ptr(t, l), 32 * (size_t)ledger_width(t->count, l),
                       hipMemcpyDeviceToDevice, st);
  const hipError_t waited = hipStreamSynchronize(st);
  if (e == hipSuccess) e = waited;
  if (e != hipSuccess) {
    (void)hipFree(d);
    return set_err(ctx, PM_ERR_HIP, std::string("pm_poseidon_ledger_append_dev: ") + hipGetErrorString(e));
  }
  if (t->d_slab) (void)hipFree(t->d_slab);
  t->d_slab = d, t->reserve = reserve;
  return PM_OK;
}

void ledger_release(pm_poseidon_ledger* t) {
  for (void* p : {t->d_slab, t->d_z, t->d_root, t->d_bad, t->own.d_tab})
    if (p) (void)hipFree(p);
  delete t;
}
}  // namespace

extern "C" size_t pm_poseidon_ledger_bytes(uint32_t height, uint64_t reserve_leaves) {
  if (height < 1 || height > PM_POSEIDON_LEDGER_MAX_HEIGHT || reserve_leaves > ledger_positions(height)) return 0;
  const u64 elements = ledger_offset(reserve_leaves, height + 1);      // below 2^63
  return elements > SIZE_MAX / 32 ? SIZE_MAX : 32 * (size_t)elements;  // more than an address space: no allocation succeeds
}

extern "C" int pm_poseidon_ledger_create(pm_ctx* ctx, const pm_hades_params* params, const uint64_t capacity[4], uint32_t height,
                                         const uint64_t empty_leaf[4], uint64_t reserve_leaves, pm_poseidon_ledger** out) {
  if (!ctx || !out) return PM_ERR_BAD_ARG;
  if (int rc = params_fault(ctx, params)) return rc;
  u32 cap[9];
  if (int rc = capacity_to_dev(ctx, capacity, cap)) return rc;
  if (height < 1 || height > PM_POSEIDON_LEDGER_MAX_HEIGHT) return set_err(ctx, PM_ERR_BAD_ARG, "height must be in 1 .. 31");
  if (!empty_leaf || !hfr_canonical(empty_leaf)) return set_err(ctx, PM_ERR_BAD_ARG, "empty_leaf is null or not canonical");
  if (reserve_leaves > ledger_positions(height)) return set_err(ctx, PM_ERR_BAD_ARG, "reserve_leaves exceeds 4^height");
  pm_poseidon_ledger* t = new pm_poseidon_ledger();
  t->device = ctx->device, t->height = height, t->reserve = reserve_leaves;
  t->own.device = params->device, t->own.rounds = params->rounds, t->own.full = params->full, t->own.n_mds = params->n_mds;
  t->own.ark = params->ark, t->own.mds = params->mds;
  memcpy(t->capacity, cap, sizeof cap);
  t->z.assign(4 * ((size_t)height + 1), 0);
  memcpy(t->z.data(), empty_leaf, 32);
  for (u32 l = 0; l < height; ++l) {                         // Z_(l+1) = word 1 of the permutation of (capacity, Z_l x 4)
    const HFr zl = hfr_load(&t->z[4 * l]);
    HFr s[5] = {hfr_load(capacity), zl, zl, zl, zl};
    host_permute(params->rounds, params->full, params->ark.data(), params->mds.data(), params->n_mds, s);
    memcpy(&t->z[4 * (l + 1)], s[1].l, 32);
  }
  std::lock_guard<std::mutex> lk(ctx->mu);
  hipError_t e = hipSetDevice(ctx->device);
  const size_t slab = pm_poseidon_ledger_bytes(height, reserve_leaves), zb = 32 * ((size_t)height + 1);
  if (e == hipSuccess) e = hipMalloc(&t->own.d_tab, table_bytes(*params));
  if (e == hipSuccess) e = hipMalloc(&t->d_z, zb);
  if (e == hipSuccess) e = hipMalloc(&t->d_root, 32);
  if (e == hipSuccess) e = hipMalloc(&t->d_bad, 8);
  if (e == hipSuccess && slab) e = hipMalloc(&t->d_slab, slab);
  if (e == hipSuccess) e = hipMemcpy(t->own.d_tab, params->d_tab, table_bytes(*params), hipMemcpyDeviceToDevice);
  if (e == hipSuccess) e = hipMemcpy(t->d_z, t->z.data(), zb, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(t->d_root, &t->z[4 * height], 32, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipDeviceSynchronize();           // the copy of the table: `params` may be freed after this call
  if (e != hipSuccess) {
    ledger_release(t);
    return set_err(ctx, e == hipErrorOutOfMemory ? PM_ERR_OOM : PM_ERR_HIP, std::string("pm_poseidon_ledger_create: ") + hipGetErrorString(e));
  }
  *out = t;
  return PM_OK;
}

extern "C" void pm_poseidon_ledger_free(pm_ctx* ctx, pm_poseidon_ledger* ledger) {
  if (!ledger) return;
  if (ctx) {
    std::lock_guard<std::mutex> lk(ctx->mu);
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    ledger_release(ledger);                                  // hipFree waits for the device: launches on caller streams included
    return;
  }
  delete ledger;
}

extern "C" int pm_poseidon_ledger_info(const pm_poseidon_ledger* ledger, uint32_t* height, uint64_t* count, uint64_t* reserve_leaves,
                                       size_t* device_bytes) {
  if (!ledger) return PM_ERR_BAD_ARG;
  if (height) *height = ledger->height;
  if (count) *count = ledger->count;
  if (reserve_leaves) *reserve_leaves = ledger->reserve;
  if (device_bytes)
    *device_bytes = pm_poseidon_ledger_bytes(ledger->height, ledger->reserve) + 32 * ((size_t)ledger->height + 2) + table_bytes(ledger->own);
  return PM_OK;
}

extern "C" int pm_poseidon_ledger_empty_roots(const pm_poseidon_ledger* ledger, uint64_t* out) {
  if (!ledger || !out) return PM_ERR_BAD_ARG;
  memcpy(out, ledger->z.data(), ledger->z.size() * 8);
  return PM_OK;
}

extern "C" int pm_poseidon_ledger_level(const pm_poseidon_ledger* ledger, uint32_t level, void** d_ptr, uint64_t* nodes) {
  if (!ledger || level > ledger->height) return PM_ERR_BAD_ARG;
  if (d_ptr) *d_ptr = ledger->d_slab ? (void*)ledger_level_ptr(ledger, level) : nullptr;
  if (nodes) *nodes = ledger_width(ledger->count, level);
  return PM_OK;
}

extern "C" int pm_poseidon_ledger_append_dev(pm_ctx* ctx, pm_poseidon_ledger* ledger, const void* d_values, size_t k, uint32_t flags,
                                             uint64_t* hashed, void* hip_stream) {
  if (!ctx) return PM_ERR_BAD_ARG;
  if (int rc = ledger_fault(ctx, ledger)) return rc;
  if (flags > PM_HADES_FORM_WAVE) return set_err(ctx, PM_ERR_BAD_ARG, "flags must be PM_HADES_FORM_AUTO, _THREAD or _WAVE");
  if (hashed) *hashed = 0;
  if (k == 0) return PM_OK;
  if (int rc = pointer_fault(ctx, {d_values})) return rc;
  LedgerPlan plan;
  if (int rc = ledger_plan(ledger->height, ledger->count, k, &plan))
    return set_err(ctx, rc, "the tree cannot hold count + k leaves, or k > 2^31 - 1");
  if (ledger_owns(ledger, d_values, k * 32)) return set_err(ctx, PM_ERR_BAD_ARG, "d_values overlaps the ledger's own memory");
  PM_ENTER(ctx, hip_stream, st);
  const u64 leaves = ledger->count + k;
  if (leaves > ledger->reserve) {
    const u64 twice = 2 * ledger->reserve, most = ledger_positions(ledger->height);
    const u64 want = twice > leaves ? twice : leaves;
    if (int rc = ledger_grow(ctx, ledger, want < most ? want : most, st)) return rc;
  }
  ProfScope prof(ctx, st, "poseidon_ledger_append");
  PM_HIP(ctx, hipMemcpyAsync(ledger_level_ptr(ledger, 0) + 2 * ledger->count, d_values, k * 32, hipMemcpyDeviceToDevice, st));
  PM_HIP(ctx, ledger_hash(ledger, plan, flags, st));
  ledger->count = leaves;
  if (hashed) *hashed = plan.hashed;
  return PM_OK;
}

extern "C" int pm_poseidon_ledger_truncate_dev(pm_ctx* ctx, pm_poseidon_ledger* ledger, uint64_t new_count, uint32_t flags,
                                               uint64_t* hashed, void* hip_stream) {
  if (!ctx) return PM_ERR_BAD_ARG;
  if (int rc = ledger_fault(ctx, ledger)) return rc;
  if (flags > PM_HADES_FORM_WAVE) return set_err(ctx, PM_ERR_BAD_ARG, "flags must be PM_HADES_FORM_AUTO, _THREAD or _WAVE");
  if (new_count > ledger->count) return set_err(ctx, PM_ERR_BAD_ARG, "new_count is above the count: a truncate cannot append");
  if (hashed) *hashed = 0;
  if (new_count == ledger->count) return PM_OK;
  PM_ENTER(ctx, hip_stream, st);
  ProfScope prof(ctx, st, "poseidon_ledger_truncate");
  if (new_count == 0) {
    PM_HIP(ctx, hipMemcpyAsync(ledger->d_root, (const u32x4*)ledger->d_z + 2 * ledger->height, 32, hipMemcpyDeviceToDevice, st));
  } else {
    LedgerPlan plan;                                         // the ancestors of leaf new_count - 1: its append to new_count - 1 leaves
    if (int rc = ledger_plan(ledger->height, new_count - 1, 1, &plan)) return set_err(ctx, rc, "pm_poseidon_ledger_truncate_dev: no plan");
    PM_HIP(ctx, ledger_hash(ledger, plan, flags, st));
    if (hashed) *hashed = plan.hashed;
  }
  ledger->count = new_count;
  return PM_OK;
}

extern "C" int pm_poseidon_ledger_root_dev(pm_ctx* ctx, const pm_poseidon_ledger* ledger, void* d_root, void* hip_stream) {
  if (!ctx) return PM_ERR_BAD_ARG;
  if (int rc = ledger_fault(ctx, ledger)) return rc;
  if (int rc = pointer_fault(ctx, {d_root})) return rc;
  if (ledger_owns(ledger, d_root, 32)) return set_err(ctx, PM_ERR_BAD_ARG, "d_root overlaps the ledger's own memory");
  PM_ENTER(ctx, hip_stream, st);
  PM_HIP(ctx, hipMemcpyAsync(d_root, ledger->d_root, 32, hipMemcpyDeviceToDevice, st));
  return PM_OK;
}

extern "C" int pm_poseidon_ledger_root(pm_ctx* ctx, const pm_poseidon_ledger* ledger, uint64_t out[4], void* hip_stream) {
  if (!ctx) return PM_ERR_BAD_ARG;
  if (int rc = ledger_fault(ctx, ledger)) return rc;
  if (!out) return set_err(ctx, PM_ERR_BAD_ARG, "null out");
  PM_ENTER(ctx, hip_stream, st);
  return finish_call(ctx, hipSuccess, st, out, ledger->d_root, 32, nullptr, "pm_poseidon_ledger_root");
}

extern "C" int pm_poseidon_ledger_paths_dev(pm_ctx* ctx, const pm_poseidon_ledger* ledger, const void* d_indices, size_t k, void* d_out,
                                            void* hip_stream) {
  if (!ctx) return PM_ERR_BAD_ARG;
  if (int rc = ledger_fault(ctx, ledger)) return rc;
  if (k == 0) return PM_OK;
  if (int rc = pointer_fault(ctx, {d_out}, !d_indices || ((uintptr_t)d_indices & 7u))) return rc;
  if (k > 0x7fffffffu / (4 * ledger->height)) return set_err(ctx, PM_ERR_LENGTH, "too many paths for one call");
  if (ledger_owns(ledger, d_out, k * ledger->height * 128)) return set_err(ctx, PM_ERR_BAD_ARG, "d_out overlaps the ledger's own memory");
  PM_ENTER(ctx, hip_stream, st);
  unsigned long long* const d_bad = (unsigned long long*)ledger->d_bad;   // the handle's: no allocation a call
  unsigned long long bad = ~0ull;
  hipError_t e = hipMemcpyAsync(d_bad, &bad, 8, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) {
    const LedgerView v{(const u32x4*)ledger->d_slab, (const u32x4*)ledger->d_z, ledger->count, ledger->reserve, ledger->height};
    hipLaunchKernelGGL(ledger_index_check_kernel, dim3((unsigned)((k + 255) / 256)), dim3(256), 0, st, (const u64*)d_indices, k,
                       ledger->count, d_bad);
    const size_t nodes = k * ledger->height * 4;
    hipLaunchKernelGGL(ledger_paths_kernel, dim3((unsigned)((nodes + 255) / 256)), dim3(256), 0, st, v, (const u64*)d_indices, k,
                       (u32x4*)d_out);
    e = hipGetLastError();
  }
  if (int rc = finish_call(ctx, e, st, &bad, d_bad, 8, nullptr, "pm_poseidon_ledger_paths_dev")) return rc;
  if (bad != ~0ull) return set_err(ctx, PM_ERR_BAD_ARG, "index " + std::to_string(bad) + " is not below the count");
  return PM_OK;
}

extern "C" int pm_test_ledger_plan(uint32_t height, uint64_t count, uint64_t k, uint64_t* first, uint64_t* nodes, uint64_t* below,
                                   uint32_t* chain_from, uint64_t* hashed) {
  LedgerPlan plan;
  const int rc = ledger_plan(height, count, k, &plan);
  if (rc != PM_OK) return rc;
  for (u32 l = 1; l <= height; ++l) {
    if (first) first[l - 1] = plan.first[l];
    if (nodes) nodes[l - 1] = plan.nodes[l];
    if (below) below[l - 1] = plan.below[l];
  }
  if (chain_from) *chain_from = plan.chain_from;
  if (hashed) *hashed = plan.hashed;
  return PM_OK;
}

extern "C" int pm_hades_permute_host(uint32_t rounds, uint32_t full_rounds, const uint64_t* ark, const uint64_t* mds, uint32_t n_mds,
                                     uint64_t state[20]) {
  if (!state || !params_fault(rounds, full_rounds, ark, mds, n_mds).empty()) return PM_ERR_BAD_ARG;
  HFr s[5];
  for (int j = 0; j < 5; ++j) {
    if (!hfr_canonical(state + 4 * j)) return PM_ERR_BAD_ARG;
    s[j] = hfr_load(state + 4 * j);
  }
  host_permute(rounds, full_rounds, ark, mds, n_mds, s);
  memcpy(state, s, 160);
  return PM_OK;
}

extern "C" int pm_poseidon_hash_host(uint32_t rounds, uint32_t full_rounds, const uint64_t* ark, const uint64_t* mds, uint32_t n_mds,
                                     const uint64_t capacity[4], const uint64_t* msg, size_t msg_len, uint64_t out[4]) {
  if (!capacity || !msg || !out || msg_len == 0 || !params_fault(rounds, full_rounds, ark, mds, n_mds).empty()) return PM_ERR_BAD_ARG;
  if (!hfr_canonical(capacity)) return PM_ERR_BAD_ARG;
  for (size_t k = 0; k < msg_len; ++k)
    if (!hfr_canonical(msg + 4 * k)) return PM_ERR_BAD_ARG;
  const host::Field<4>& Fq = host::FR();
  HFr s[5] = {hfr_load(capacity), host::zero<4>(), host::zero<4>(), host::zero<4>(), host::zero<4>()};
  for (size_t at = 0; at < msg_len; at += 4) {
    const size_t left = msg_len - at < 4 ? msg_len - at : 4;
    for (size_t t = 0; t < left; ++t) s[1 + t] = host::add(s[1 + t], hfr_load(msg + 4 * (at + t)), Fq);
    if (left < 4) s[1 + left] = host::add(s[1 + left], host::one<4>(Fq), Fq);
    host_permute(rounds, full_rounds, ark, mds, n_mds, s);
  }
  memcpy(out, s[1].l, 32);
  return PM_OK;
}
