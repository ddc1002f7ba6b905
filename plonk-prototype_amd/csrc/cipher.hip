// The Poseidon cipher on JubJub keys: encrypting a note to its recipient, decrypting it under a shared
// secret, and SCANNING -- trial-decrypting every note of a ledger under one viewing key to find the recipient's own.  One
// thread per note, over the routines of hades.hip.h (one permutation on a lane's own state) and jubjub.hip.h (the group law,
// the window tables).  P = the Hades permutation of a pm_hades_params handle, L = the message capacity (1 .. 4), S = (S.x, S.y)
// the shared secret, a JubJub point:
//
//   init     the state [2^32, L, S.x, S.y, nonce]
//   encrypt  s = P(init); s[1 + i] += m[i], c[i] = s[1 + i] for i < L; s = P(s); c[L] = s[1].  L + 1 elements.
//   decrypt  s = P(init); m[i] = c[i] - s[1 + i], s[1 + i] = c[i]; s = P(s); accepted when c[L] = s[1].
//   scan     a note is (R, nonce, c) with R = e G and S = e PK, PK = vk G; the recipient recovers S = vk R.  Two kernels on the
//            stream.  Ladder: a thread's table 1 R .. 8 R in the scratch buffer, vk R by a signed 4-bit ladder over it (the
//            windows and the table of jubjub_var_kernel, its doublings by the dedicated formula, T from the last of four
//            only), ONE inversion -- S is hashed, so it has to be affine -- and S into the thread's slot.  Then the decrypt
//            kernel with S from the slot and its point test on R.  The ladder keeps the register budget jubjub_var_kernel
//            has (two waves a SIMD) and the permutations their own.
//   scan under K keys (section 7.2q, further down): the window table e 16^w R of a note built once, a walk of at most 64
//            additions and one inversion per (note, key), the same decryption, a mask of K bits a note.
//
// Every thread of a scan multiplies by the SAME scalar: the 64 signed digits of vk are recoded once on the host and travel by
// value in the kernel's arguments, top first.  Digit w is read at a wave-uniform index, so it lives in a scalar register: its
// sign and the zero digit are uniform branches, and there is no per-lane recoding, no shift of a per-lane scalar and no word
// of carries.
//
// Every lane runs everything: a lane past n works on element n - 1 and stores nothing (fe_inv_dev votes across the wave), and
// a failed early test selects the status, it does not branch around the work.  Nothing is read or written at an address that
// depends on an input except the table entries, whose index is clamped to 1 .. 8.  For any status but PM_CIPHER_OK the
// message words written are zero: a wrong key's garbage never leaves the device.
//
// The scheme is the shape of dusk-poseidon's PoseidonCipher as remembered: prior knowledge, pinned by nothing here.
// NOT hardened against side channels: the scan reads its table at addresses that depend on the viewing key.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "cipher_scan_plan.h"
#include "context.h"
#include "field_inv.hip.h"
#include "hades.hip.h"
#include "jubjub.hip.h"

namespace pm {
namespace {

using host::HFr;

constexpr u32 CPH_MAX_LEN = 4;                              // message words: the rate of the width-5 permutation
constexpr size_t CPH_SLOT_BYTES = JJ_MUL_TABLE_BYTES + 64;  // a thread's scratch: 1 R .. 8 R, then S (x | y): 1216 in flight

// ------------------------------------------------------------------ the host forms (csrc/host_field.h)
void host_init(HFr (&s)[5], const HPoint& secret, const uint64_t* nonce, uint32_t len) {
  const host::Field<4>& Fq = host::FR();
  s[0] = host::from_u64(1ull << 32, Fq), s[1] = host::from_u64(len, Fq);
  s[2] = secret.x, s[3] = secret.y, s[4] = hfr_load(nonce);
}
bool host_consts_fault(uint32_t R, uint32_t F, const uint64_t* ark, const uint64_t* mds, uint32_t n_mds, uint32_t len) {
  return len < 1 || len > CPH_MAX_LEN || !params_fault(R, F, ark, mds, n_mds).empty();
}

// ------------------------------------------------------------------ device side
struct CipherIo {
  const u32x4* secrets;     // n x (x | y)
  const u32x4* tested;      // decrypt: the points its test judges -- the secrets, or a scan's ephemeral keys
  const u32x4* nonces;      // n elements
  const u32x4* in;          // encrypt: n x len messages; decrypt: n x (len + 1) cipher words
  u32x4* out;               // encrypt: n x (len + 1); decrypt: n x len
  u32* status;              // decrypt: n, or null
  unsigned long long* n_ok; // decrypt: the count of status 0, or null
  size_t n;
  u32 len;
  u32 domain[9], len_word[9];   // 2^32 and L, device form
  u32 edwards_d[9];         // device form
};
struct CipherScanIo {
  const u32x4* points;      // n x (x | y): the ephemeral keys
  u32x4* scratch;           // the tables: [entry][chunk][thread of the grid]
  u32x4* secrets;           // a secret (x | y) a thread of the grid: behind the tables, or a key's row of slots (scan_keys)
  size_t n;
  u32 edwards_d[9];         // device form
  u32 digits[JJ_WINDOWS / 4];       // of the viewing key: recode_digit_words (jubjub.hip.h)
};

// s = init with the keys of round 0 added.  x, y, nonce in the device form, normalised, below 2 r: with the round key a word
// stays below the 4.2 r h_absorb reduces from.
PM_DEV void cph_init(Fr (&s)[5], const Fr& x, const Fr& y, const Fr& nonce, const CipherIo& a, const HadesTab& tab) {
  const Fr zero = fe_zero<FrP>();
  s[0] = h_absorb(fr_limbs(a.domain), zero, tab.ark);
  s[1] = h_absorb(fr_limbs(a.len_word), zero, tab.ark + 9);
  s[2] = h_absorb(zero, x, tab.ark + 18);
  s[3] = h_absorb(zero, y, tab.ark + 27);
  s[4] = h_absorb(zero, nonce, tab.ark + 36);
}

__global__ void __launch_bounds__(64) cipher_encrypt_kernel(const HadesTab tab, const CipherIo a) {
  const size_t g = (size_t)blockIdx.x * 64 + threadIdx.x;
  const bool live = g < a.n;
  const size_t i = live ? g : a.n - 1;
  const Fr zero = fe_zero<FrP>();
  Fr s[5];
  cph_init(s, g_to_dev(ld_canon(a.secrets, 2 * i)), g_to_dev(ld_canon(a.secrets, 2 * i + 1)), g_to_dev(ld_canon(a.nonces, i)), a, tab);
  h_rounds_thread(s, tab);
  // a state word leaves the rounds below 2.1 r with its top limb open; the sum with a message is reduced before the round key
  // joins it, so h_absorb sees a normalised word below 2 r
  s[0] = h_absorb(s[0], zero, tab.ark);
#pragma unroll
  for (u32 j = 0; j < CPH_MAX_LEN; ++j) {
    if (j < a.len) {                                         // uniform
      const Fr c = gadd(s[1 + j], g_to_dev(ld_canon(a.in, a.len * i + j)));
      if (live) st_canon(a.out, (a.len + 1) * i + j, g_to_abi(c));
      s[1 + j] = h_absorb(c, zero, tab.ark + 9 * (1 + j));
    } else {
      s[1 + j] = h_absorb(s[1 + j], zero, tab.ark + 9 * (1 + j));
    }
  }
  h_rounds_thread(s, tab);
  if (live) st_canon(a.out, (a.len + 1) * i + a.len, g_to_abi(s[1]));
}

// the nonce and the len + 1 cipher words at ct are below r
PM_DEV bool cph_range_ok(const u32x4* nonce, const u32x4* ct, u32 len) {
  bool ok = jj_below_r(nonce[0], nonce[1]);
#pragma unroll
  for (u32 j = 0; j <= CPH_MAX_LEN; ++j)
    if (j <= len) ok = ok && jj_below_r(ct[2 * j], ct[2 * j + 1]);   // uniform
  return ok;
}
// The decryption of note i: the messages, packed, into m -- as computed, whatever the verdict -- and the status returned.
// SCAN: the secret is the (x | y) at `secret`, what a ladder or a walk left in a slot, and the point test judges the ephemeral
// key at a.tested; otherwise the secret is that point itself.
template <bool SCAN>
PM_DEV u32 cph_open(const HadesTab& tab, const CipherIo& a, size_t i, const u32x4* secret, u32 (&m)[CPH_MAX_LEN][8]) {
  const Fr zero = fe_zero<FrP>();
  const u32x4* const ct = a.in + 2 * (size_t)(a.len + 1) * i;
  Fr s[5];
  bool point_ok;
  {
    Fr x, y;
    point_ok = jj_point_ok(a.tested + 4 * i, fr_limbs(a.edwards_d), x, y);
    if (SCAN) x = g_to_dev(ld_canon(secret, 0)), y = g_to_dev(ld_canon(secret, 1));
    cph_init(s, x, y, g_to_dev(ld_canon(a.nonces, i)), a, tab);
  }
  const bool range_ok = cph_range_ok(a.nonces + 2 * i, ct, a.len);
  h_rounds_thread(s, tab);
  // the messages wait, packed, for the verdict of the tag
  s[0] = h_absorb(s[0], zero, tab.ark);
#pragma unroll
  for (u32 j = 0; j < CPH_MAX_LEN; ++j) {
    if (j < a.len) {                                         // uniform
      const Fr c = g_to_dev(ld_canon(ct, j));
      fe_canon_pack<FrP>(m[j], g_to_abi(gsub(c, fe_reduce_weak<FrP>(s[1 + j]))));   // gsub takes a normalised subtrahend
      s[1 + j] = h_absorb(c, zero, tab.ark + 9 * (1 + j));
    } else {
#pragma unroll
      for (int k = 0; k < 8; ++k) m[j][k] = 0;
      s[1 + j] = h_absorb(s[1 + j], zero, tab.ark + 9 * (1 + j));
    }
  }
  h_rounds_thread(s, tab);
  const u32x4 t0 = ct[2 * a.len], t1 = ct[2 * a.len + 1];
  u32 tag[8];
  fe_canon_pack<FrP>(tag, g_to_abi(s[1]));
  const u32 diff = (tag[0] ^ t0.x) | (tag[1] ^ t0.y) | (tag[2] ^ t0.z) | (tag[3] ^ t0.w) | (tag[4] ^ t1.x) | (tag[5] ^ t1.y) |
                   (tag[6] ^ t1.z) | (tag[7] ^ t1.w);
  return !point_ok ? PM_CIPHER_POINT : !range_ok ? PM_CIPHER_RANGE : diff != 0 ? PM_CIPHER_TAG : PM_CIPHER_OK;
}

// SCAN: the secret is what the ladder left in the thread's slot and the point test judges the ephemeral key
template <bool SCAN>
__global__ void __launch_bounds__(64) cipher_decrypt_kernel(const HadesTab tab, const CipherIo a) {
  const size_t g = (size_t)blockIdx.x * 64 + threadIdx.x;
  const bool live = g < a.n;
  const size_t i = live ? g : a.n - 1;
  u32 m[CPH_MAX_LEN][8];
  const u32 status = cph_open<SCAN>(tab, a, i, a.secrets + 4 * i, m);
  const u32 keep = status == PM_CIPHER_OK ? ~0u : 0u;       // a mask, not a select between vectors (that one goes through scratch)
  if (a.n_ok) {
    const unsigned long long hits = __ballot(live && status == PM_CIPHER_OK);
    if (threadIdx.x == 0 && hits) atomicAdd(a.n_ok, (unsigned long long)__popcll(hits));
  }
  if (!live) return;
#pragma unroll
  for (u32 j = 0; j < CPH_MAX_LEN; ++j) {
    if (j < a.len) {
      u32x4* const q = a.out + 2 * ((size_t)a.len * i + j);
      q[0] = u32x4{m[j][0] & keep, m[j][1] & keep, m[j][2] & keep, m[j][3] & keep};
      q[1] = u32x4{m[j][4] & keep, m[j][5] & keep, m[j][6] & keep, m[j][7] & keep};
    }
  }
  if (a.status) a.status[i] = status;
}

// vk R_i for one stride of notes: a thread's table, the ladder under the uniform digits, one inversion, S into the slot.
// Two waves a SIMD: the ladder's register budget, as jubjub_var_kernel.
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 2))) cipher_scan_ladder_kernel(const CipherScanIo a) {
  const size_t T = (size_t)gridDim.x * 64, tid = (size_t)blockIdx.x * 64 + threadIdx.x;
  u32x4* const tbl = a.scratch + tid;
  const size_t i = tid < a.n ? tid : a.n - 1;
  const Fr ed = fr_limbs(a.edwards_d);
  // ---- the table of R
  jj_table_build(tbl, T, g_to_dev(ld_canon(a.points, 2 * i)), g_to_dev(ld_canon(a.points, 2 * i + 1)), ed);
  // ---- the ladder from the top digit down; a digit is the same in every lane of the grid
  const EdPoint acc = jj_ladder_uniform(tbl, T, a.digits, ed);
  // ---- S = (X / Z, Y / Z) into the slot of this thread, live or not: the slots are per thread of the grid
  const Fr zi = g_to_abi(fe_inv_dev<FrP>(acc.Z));           // every lane of the wave is here
  u32x4* const out = a.secrets + 4 * tid;
  st_canon(out, 0, gmul(acc.X, zi));                         // device x ABI -> ABI
  st_canon(out, 1, gmul(acc.Y, zi));
}

// ------------------------------------------------------------------ many viewing keys in one scan
// Per stride of notes in flight: BUILD, a thread a note, writes the window table e 16^w R_i of jj_window_table_build; WALK, the
// grid over (notes of the stride) x keys with one key a workgroup, adds at most 64 of its entries under the key's digits, inverts
// once and leaves S = vk_k R_i, canonical, in the slot [key][thread]; OPEN, the same grid, decrypts (note, key) with cph_open
// and, on a hit, sets bit `key` of the note's mask and leaves the message in the staging slot [key][thread][L]; EMIT, a thread a
// note, writes the status, the lowest set key's message or zeros, and adds the hits.  Below `cipher_scan_keys_table_min` keys
// the ladder kernel above fills the slots key by key in place of BUILD and WALK; OPEN and EMIT are the same.
struct CipherKeysIo {
  const u32x4* points;      // the stride's ephemeral keys
  u32x4* table;             // [entry 8 w + e - 1][chunk][thread of the stride]
  u32x4* secrets;           // [key][thread] x (x | y)
  u32x4* staging;           // [key][thread][len] messages of the hits
  const u32* digits;        // [key][JJ_WINDOWS / 4]: recode_digit_words
  unsigned long long* masks;   // the stride's
  u32x4* out;               // the stride's messages, or null
  u32* status;              // the stride's, or null
  unsigned long long* n_hits;  // or null
  size_t n, T;              // notes of this stride; the notes in flight, what the scratch is laid out for
  u32 edwards_d[9];         // device form
};

// Two waves a SIMD: 512 registers hold B, 2 B, 4 B and the point in the making without scratch
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 2))) cipher_keys_build_kernel(const CipherKeysIo a) {
  const size_t T = a.T, tid = (size_t)blockIdx.x * 64 + threadIdx.x;
  const size_t i = tid < a.n ? tid : a.n - 1;
  jj_window_table_build(a.table + tid, T, g_to_dev(ld_canon(a.points, 2 * i)), g_to_dev(ld_canon(a.points, 2 * i + 1)),
                        fr_limbs(a.edwards_d));
}

// blockIdx.y = the key.  Two waves a SIMD: the inversion's register budget, as the ladder.
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 2))) cipher_keys_walk_kernel(const CipherKeysIo a) {
  const size_t T = a.T, tid = (size_t)blockIdx.x * 64 + threadIdx.x;
  const u32 key = blockIdx.y;
  const EdPoint acc = jj_window_walk(a.table + tid, T, a.digits + (size_t)key * (JJ_WINDOWS / 4), fr_limbs(a.edwards_d));
  const Fr zi = g_to_abi(fe_inv_dev<FrP>(acc.Z));           // every lane of the wave is here
  u32x4* const out = a.secrets + 4 * ((size_t)key * T + tid);
  st_canon(out, 0, gmul(acc.X, zi));                         // device x ABI -> ABI
  st_canon(out, 1, gmul(acc.Y, zi));
}

// blockIdx.y = the key; c.tested, c.nonces and c.in are the stride's.  A hit sets its bit by an atomic OR, whose result does not
// depend on the order of the keys, and nothing else is written per key but the message of a hit.
__global__ void __launch_bounds__(64) cipher_keys_open_kernel(const HadesTab tab, const CipherIo c, const CipherKeysIo a) {
  const size_t T = a.T, tid = (size_t)blockIdx.x * 64 + threadIdx.x;
  const u32 key = blockIdx.y;
  const bool live = tid < a.n;
  const size_t i = live ? tid : a.n - 1, slot = (size_t)key * T + tid;
  u32 m[CPH_MAX_LEN][8];
  const u32 status = cph_open<true>(tab, c, i, a.secrets + 4 * slot, m);
  if (!live || status != PM_CIPHER_OK) return;
  atomicOr(a.masks + i, 1ull << key);
#pragma unroll
  for (u32 j = 0; j < CPH_MAX_LEN; ++j) {
    if (j < c.len) {
      u32x4* const q = a.staging + 2 * (slot * c.len + j);
      q[0] = u32x4{m[j][0], m[j][1], m[j][2], m[j][3]};
      q[1] = u32x4{m[j][4], m[j][5], m[j][6], m[j][7]};
    }
  }
}

// a thread a note: what depends on the note alone (the point test of R, the ranges), the mask, the lowest key's message
__global__ void __launch_bounds__(64) cipher_keys_emit_kernel(const CipherIo c, const CipherKeysIo a) {
  const size_t T = a.T, tid = (size_t)blockIdx.x * 64 + threadIdx.x;
  const bool live = tid < a.n;
  const size_t i = live ? tid : a.n - 1;
  Fr x, y;
  const bool point_ok = jj_point_ok(c.tested + 4 * i, fr_limbs(a.edwards_d), x, y);
  const bool range_ok = cph_range_ok(c.nonces + 2 * i, c.in + 2 * (size_t)(c.len + 1) * i, c.len);
  const unsigned long long mask = live ? a.masks[i] : 0ull;
  if (a.n_hits) {
    u32 hits = (u32)__popcll(mask);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) hits += __shfl_xor(hits, off);
    if (threadIdx.x == 0 && hits) atomicAdd(a.n_hits, (unsigned long long)hits);
  }
  if (!live) return;
  if (a.status) a.status[i] = !point_ok ? PM_CIPHER_POINT : !range_ok ? PM_CIPHER_RANGE : mask ? PM_CIPHER_OK : PM_CIPHER_TAG;
  if (!a.out) return;
  const u32 key = mask ? (u32)__ffsll((long long)mask) - 1 : 0;
  const u32x4* const from = a.staging + 2 * (((size_t)key * T + tid) * c.len);
  const u32 keep = mask ? ~0u : 0u;                          // a mask, not a select between vectors, as in the decryption
#pragma unroll
  for (u32 j = 0; j < 2 * CPH_MAX_LEN; ++j) {
    if (j < 2 * c.len) {
      const u32x4 v = from[j];
      a.out[2 * (size_t)c.len * i + j] = u32x4{v.x & keep, v.y & keep, v.z & keep, v.w & keep};
    }
  }
}

// ------------------------------------------------------------------ launches
int common_fault(pm_ctx* ctx, const pm_hades_params* params, uint32_t msg_len) {
  if (int rc = params_fault(ctx, params)) return rc;
  if (msg_len < 1 || msg_len > CPH_MAX_LEN) return set_err(ctx, PM_ERR_BAD_ARG, "msg_len must be 1 .. 4");
  return PM_OK;
}
void io_consts(CipherIo& a, uint32_t msg_len) {
  const host::Field<4>& Fq = host::FR();
  a.len = msg_len;
  to_limbs29(a.domain, host::from_u64(1ull << 32, Fq));
  to_limbs29(a.len_word, host::from_u64(msg_len, Fq));
  jubjub_d_limbs(a.edwards_d);
}
// what decrypt and scan do once their kernels are on the stream: the count back when it is wanted, the buffer released
int finish(pm_ctx* ctx, hipError_t e, hipStream_t st, void* buf, const unsigned long long* d_ok, size_t* n_ok, const char* who) {
  unsigned long long ok = 0;
  if (int rc = finish_call(ctx, e, st, n_ok ? &ok : nullptr, d_ok, 8, buf, who)) return rc;
  if (n_ok) *n_ok = (size_t)ok;
  return PM_OK;
}

}  // namespace
}  // namespace pm

using namespace pm;

extern "C" int pm_poseidon_cipher_encrypt_dev(pm_ctx* ctx, const pm_hades_params* params, const void* d_secrets_xy,
                                              const void* d_nonces, const void* d_msgs, uint32_t msg_len, size_t n,
                                              void* d_ciphers, void* hip_stream) {
  if (!ctx) return PM_ERR_BAD_ARG;
  if (int rc = common_fault(ctx, params, msg_len)) return rc;
  if (int rc = pointer_fault(ctx, {d_secrets_xy, d_nonces, d_msgs, d_ciphers})) return rc;
  if (int rc = count_fault(ctx, n)) return rc;
  if (n == 0) return PM_OK;
  PM_ENTER(ctx, hip_stream, st);
  CipherIo a{};
  a.secrets = (const u32x4*)d_secrets_xy, a.nonces = (const u32x4*)d_nonces, a.in = (const u32x4*)d_msgs, a.out = (u32x4*)d_ciphers;
  a.n = n;
  io_consts(a, msg_len);
  ProfScope prof(ctx, st, "poseidon_cipher_encrypt");
  hipLaunchKernelGGL(cipher_encrypt_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, tab_of(params), a);
  PM_HIP(ctx, hipGetLastError());
  return PM_OK;
}

extern "C" int pm_poseidon_cipher_decrypt_dev(pm_ctx* ctx, const pm_hades_params* params, const void* d_secrets_xy,
                                              const void* d_nonces, const void* d_ciphers, uint32_t msg_len, size_t n,
                                              void* d_msgs_out, void* d_status, size_t* n_ok, void* hip_stream) {
  if (!ctx) return PM_ERR_BAD_ARG;
  if (int rc = common_fault(ctx, params, msg_len)) return rc;
  if (int rc = pointer_fault(ctx, {d_secrets_xy, d_nonces, d_ciphers, d_msgs_out}, ((uintptr_t)d_status & 3u) != 0)) return rc;
  if (int rc = count_fault(ctx, n)) return rc;
  if (n_ok) *n_ok = 0;
  if (n == 0) return PM_OK;
  PM_ENTER(ctx, hip_stream, st);
  unsigned long long* d_ok = nullptr;
  if (n_ok) PM_HIP(ctx, hipMalloc((void**)&d_ok, 16));
  CipherIo a{};
  a.secrets = a.tested = (const u32x4*)d_secrets_xy, a.nonces = (const u32x4*)d_nonces, a.in = (const u32x4*)d_ciphers;
  a.out = (u32x4*)d_msgs_out, a.status = (u32*)d_status, a.n_ok = d_ok, a.n = n;
  io_consts(a, msg_len);
  hipError_t e = n_ok ? hipMemsetAsync(d_ok, 0, 16, st) : hipSuccess;
  if (e == hipSuccess) {
    ProfScope prof(ctx, st, "poseidon_cipher_decrypt");
    hipLaunchKernelGGL(cipher_decrypt_kernel<false>, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, tab_of(params), a);
    e = hipGetLastError();
  }
  return finish(ctx, e, st, d_ok, d_ok, n_ok, "pm_poseidon_cipher_decrypt_dev");
}

extern "C" int pm_poseidon_cipher_scan_dev(pm_ctx* ctx, const pm_hades_params* params, const uint64_t view_key[4],
                                           uint32_t scalar_form, const void* d_ephemeral_xy, const void* d_nonces,
                                           const void* d_ciphers, uint32_t msg_len, size_t n, void* d_msgs_out, void* d_status,
                                           size_t* n_ok, void* hip_stream) {
  if (!ctx) return PM_ERR_BAD_ARG;
  if (int rc = common_fault(ctx, params, msg_len)) return rc;
  if (int rc = form_fault(ctx, scalar_form)) return rc;
  uint64_t vk[4];
  if (!view_key || !scalar_to_int(view_key, scalar_form, vk)) return set_err(ctx, PM_ERR_BAD_ARG, "the viewing key is null or not below r");
  if (int rc = pointer_fault(ctx, {d_ephemeral_xy, d_nonces, d_ciphers, d_msgs_out}, ((uintptr_t)d_status & 3u) != 0)) return rc;
  if (int rc = count_fault(ctx, n)) return rc;
  if (n_ok) *n_ok = 0;
  if (n == 0) return PM_OK;
  PM_ENTER(ctx, hip_stream, st);
  // the slots of the threads in flight, and the count of hits
  SlotScratch scratch(ctx, n);
  PM_HIP(ctx, scratch.alloc(CPH_SLOT_BYTES, 16));
  const size_t stride = scratch.stride;
  unsigned long long* const d_ok = scratch.tail();
  CipherScanIo l{};
  l.scratch = scratch.slots();
  l.secrets = l.scratch + (size_t)8 * JJ_POINT_CHUNKS * stride;
  jubjub_d_limbs(l.edwards_d);
  recode_digit_words(vk, l.digits);
  CipherIo a{};
  a.secrets = l.secrets, a.n_ok = n_ok ? d_ok : nullptr;
  io_consts(a, msg_len);
  const HadesTab tab = tab_of(params);
  hipError_t e = n_ok ? hipMemsetAsync(d_ok, 0, 16, st) : hipSuccess;
  if (e == hipSuccess) {
    ProfScope prof(ctx, st, "poseidon_cipher_scan");
    for (size_t off = 0; off < n && e == hipSuccess; off += stride) {   // a stride is decrypted before the next ladder reuses the slots
      l.n = a.n = std::min(stride, n - off);
      l.points = a.tested = (const u32x4*)d_ephemeral_xy + 4 * off;
      a.nonces = (const u32x4*)d_nonces + 2 * off, a.in = (const u32x4*)d_ciphers + 2 * (size_t)(msg_len + 1) * off;
      a.out = (u32x4*)d_msgs_out + 2 * (size_t)msg_len * off, a.status = d_status ? (u32*)d_status + off : nullptr;
      hipLaunchKernelGGL(cipher_scan_ladder_kernel, dim3((unsigned)scratch.blocks), dim3(64), 0, st, l);
      hipLaunchKernelGGL(cipher_decrypt_kernel<true>, dim3((unsigned)((a.n + 63) / 64)), dim3(64), 0, st, tab, a);
      e = hipGetLastError();
    }
  }
  return finish(ctx, e, st, scratch.base, d_ok, n_ok, "pm_poseidon_cipher_scan_dev");
}

// the plan of a scan under n_keys keys with the context's options: the full table from cipher_scan_keys_table_min keys on
static int scan_keys_plan(const pm_ctx* ctx, uint32_t n_keys, uint32_t msg_len, size_t n, bool* full_table, CipherScanKeysPlan* p) {
  const long table_min = ctx->opt_cipher_scan_keys_table_min ? ctx->opt_cipher_scan_keys_table_min : PM_CIPHER_SCAN_KEYS_TABLE_MIN;
  *full_table = (long)n_keys >= table_min;
  return cipher_scan_keys_plan(ctx->num_cus, n_keys, msg_len, n, ctx->opt_cipher_scan_table_mb, *full_table, p);
}

extern "C" size_t pm_poseidon_cipher_scan_keys_work_bytes(pm_ctx* ctx, uint32_t n_keys, uint32_t msg_len, size_t n) {
  if (!ctx || n > 0x7fffffffu) return 0;
  std::lock_guard<std::mutex> lk(ctx->mu);
  bool full_table;
  CipherScanKeysPlan plan{};
  return scan_keys_plan(ctx, n_keys, msg_len, n, &full_table, &plan) == PM_OK ? plan.bytes : 0;
}

extern "C" int pm_poseidon_cipher_scan_keys_dev(pm_ctx* ctx, const pm_hades_params* params, const uint64_t* view_keys,
                                                uint32_t n_keys, uint32_t scalar_form, const void* d_ephemeral_xy,
                                                const void* d_nonces, const void* d_ciphers, uint32_t msg_len, size_t n,
                                                void* d_masks, void* d_msgs_out, void* d_status, size_t* n_hits, void* hip_stream) {
  if (!ctx) return PM_ERR_BAD_ARG;
  if (int rc = common_fault(ctx, params, msg_len)) return rc;
  if (int rc = form_fault(ctx, scalar_form)) return rc;
  if (n_keys < 1 || n_keys > PM_CIPHER_SCAN_MAX_KEYS) return set_err(ctx, PM_ERR_BAD_ARG, "n_keys must be 1 .. 64");
  if (!view_keys) return set_err(ctx, PM_ERR_BAD_ARG, "the viewing keys are null");
  u32 digits[PM_CIPHER_SCAN_MAX_KEYS][JJ_WINDOWS / 4];      // lives until finish() has waited for the device
  for (uint32_t k = 0; k < n_keys; ++k) {
    uint64_t vk[4];
    if (!scalar_to_int(view_keys + 4 * k, scalar_form, vk)) return set_err(ctx, PM_ERR_BAD_ARG, "a viewing key is not below r");
    recode_digit_words(vk, digits[k]);
  }
  if (int rc = pointer_fault(ctx, {d_ephemeral_xy, d_nonces, d_ciphers, d_masks}, unaligned({d_msgs_out}) || ((uintptr_t)d_status & 3u) != 0))
    return rc;
  if (int rc = count_fault(ctx, n)) return rc;
  if (n_hits) *n_hits = 0;
  if (n == 0) return PM_OK;
  PM_ENTER(ctx, hip_stream, st);
  bool full_table;
  CipherScanKeysPlan plan{};
  if (int rc = scan_keys_plan(ctx, n_keys, msg_len, n, &full_table, &plan)) return set_err(ctx, rc, "pm_poseidon_cipher_scan_keys_dev: no plan");
  char* base = nullptr;
  PM_HIP(ctx, hipMalloc((void**)&base, plan.bytes));         // PM_ERR_OOM before an output byte is written
  const size_t stride = plan.stride;
  CipherKeysIo k{};
  k.table = (u32x4*)base, k.secrets = (u32x4*)(base + plan.off_secrets), k.staging = (u32x4*)(base + plan.off_staging);
  k.digits = (const u32*)(base + plan.off_digits), k.T = stride;
  unsigned long long* const d_hits = (unsigned long long*)(base + plan.off_count);
  k.n_hits = n_hits ? d_hits : nullptr;
  jubjub_d_limbs(k.edwards_d);
  CipherScanIo l{};                                          // the per-key path: one table 1 R .. 8 R a thread, shared by the keys in turn
  l.scratch = k.table;
  jubjub_d_limbs(l.edwards_d);
  CipherIo a{};
  io_consts(a, msg_len);
  const HadesTab tab = tab_of(params);
  hipError_t e = hipMemcpyAsync(base + plan.off_digits, digits, CSK_DIGIT_BYTES * n_keys, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemsetAsync(d_hits, 0, CSK_COUNT_BYTES, st);
  if (e == hipSuccess) e = hipMemsetAsync(d_masks, 0, 8 * n, st);
  for (size_t off = 0; off < n && e == hipSuccess; off += stride) {   // a stride is emitted before the next one reuses the scratch
    k.n = l.n = a.n = std::min(stride, n - off);
    const dim3 notes((unsigned)((k.n + 63) / 64)), pairs(notes.x, n_keys);
    k.points = l.points = a.tested = (const u32x4*)d_ephemeral_xy + 4 * off;
    a.nonces = (const u32x4*)d_nonces + 2 * off, a.in = (const u32x4*)d_ciphers + 2 * (size_t)(msg_len + 1) * off;
    k.masks = (unsigned long long*)d_masks + off;
    k.out = d_msgs_out ? (u32x4*)d_msgs_out + 2 * (size_t)msg_len * off : nullptr;
    k.status = d_status ? (u32*)d_status + off : nullptr;
    if (full_table) {
      {
        ProfScope prof(ctx, st, "poseidon_cipher_scan_keys_build");
        hipLaunchKernelGGL(cipher_keys_build_kernel, notes, dim3(64), 0, st, k);
      }
      ProfScope prof(ctx, st, "poseidon_cipher_scan_keys_walk");
      hipLaunchKernelGGL(cipher_keys_walk_kernel, pairs, dim3(64), 0, st, k);
    } else {
      ProfScope prof(ctx, st, "poseidon_cipher_scan_keys_ladder");
      for (uint32_t j = 0; j < n_keys; ++j) {                // the ladder's table layout follows ITS grid: every launch the stride's
        l.secrets = k.secrets + 4 * (size_t)j * stride;
        memcpy(l.digits, digits[j], sizeof l.digits);
        hipLaunchKernelGGL(cipher_scan_ladder_kernel, dim3((unsigned)plan.blocks), dim3(64), 0, st, l);
      }
    }
    {
      ProfScope prof(ctx, st, "poseidon_cipher_scan_keys_open");
      hipLaunchKernelGGL(cipher_keys_open_kernel, pairs, dim3(64), 0, st, tab, a, k);
    }
    ProfScope prof(ctx, st, "poseidon_cipher_scan_keys_emit");
    hipLaunchKernelGGL(cipher_keys_emit_kernel, notes, dim3(64), 0, st, a, k);
    e = hipGetLastError();
  }
  return finish(ctx, e, st, base, d_hits, n_hits, "pm_poseidon_cipher_scan_keys_dev");
}

extern "C" int pm_test_cipher_scan_keys_plan(uint32_t num_cus, uint32_t n_keys, uint32_t msg_len, size_t n, long table_mb,
                                             size_t* stride, size_t* bytes) {
  if (!stride || !bytes) return PM_ERR_BAD_ARG;
  CipherScanKeysPlan plan{};
  *stride = *bytes = 0;
  if (int rc = cipher_scan_keys_plan((int)num_cus, n_keys, msg_len, n, table_mb, true, &plan)) return rc;
  *stride = plan.stride, *bytes = plan.bytes;
  return PM_OK;
}

extern "C" int pm_poseidon_cipher_encrypt_host(uint32_t rounds, uint32_t full_rounds, const uint64_t* ark, const uint64_t* mds,
                                               uint32_t n_mds, const uint64_t secret_xy[8], const uint64_t nonce[4],
                                               const uint64_t* msg, uint32_t msg_len, uint64_t* cipher_out) {
  if (!secret_xy || !nonce || !msg || !cipher_out || host_consts_fault(rounds, full_rounds, ark, mds, n_mds, msg_len)) return PM_ERR_BAD_ARG;
  if (point_fault(secret_xy) || !hfr_canonical(nonce)) return PM_ERR_BAD_ARG;
  for (uint32_t j = 0; j < msg_len; ++j)
    if (!hfr_canonical(msg + 4 * j)) return PM_ERR_BAD_ARG;
  const host::Field<4>& Fq = host::FR();
  HFr s[5];
  host_init(s, hpoint_load(secret_xy), nonce, msg_len);
  host_permute(rounds, full_rounds, ark, mds, n_mds, s);
  for (uint32_t j = 0; j < msg_len; ++j) {
    s[1 + j] = host::add(s[1 + j], hfr_load(msg + 4 * j), Fq);
    memcpy(cipher_out + 4 * j, s[1 + j].l, 32);
  }
  host_permute(rounds, full_rounds, ark, mds, n_mds, s);
  memcpy(cipher_out + 4 * msg_len, s[1].l, 32);
  return PM_OK;
}

extern "C" int pm_poseidon_cipher_decrypt_host(uint32_t rounds, uint32_t full_rounds, const uint64_t* ark, const uint64_t* mds,
                                               uint32_t n_mds, const uint64_t secret_xy[8], const uint64_t nonce[4],
                                               const uint64_t* cipher, uint32_t msg_len, uint64_t* msg_out, uint32_t* status) {
  if (!secret_xy || !nonce || !cipher || !msg_out || !status || host_consts_fault(rounds, full_rounds, ark, mds, n_mds, msg_len))
    return PM_ERR_BAD_ARG;
  memset(msg_out, 0, 32 * (size_t)msg_len);
  bool in_range = hfr_canonical(nonce);
  for (uint32_t j = 0; j <= msg_len; ++j) in_range = in_range && hfr_canonical(cipher + 4 * j);
  if (point_fault(secret_xy)) {
    *status = PM_CIPHER_POINT;
  } else if (!in_range) {
    *status = PM_CIPHER_RANGE;
  } else {
    const host::Field<4>& Fq = host::FR();
    HFr s[5], m[CPH_MAX_LEN];
    host_init(s, hpoint_load(secret_xy), nonce, msg_len);
    host_permute(rounds, full_rounds, ark, mds, n_mds, s);
    for (uint32_t j = 0; j < msg_len; ++j) {
      const HFr c = hfr_load(cipher + 4 * j);
      m[j] = host::sub(c, s[1 + j], Fq);
      s[1 + j] = c;
    }
    host_permute(rounds, full_rounds, ark, mds, n_mds, s);
    *status = host::eq(s[1], hfr_load(cipher + 4 * msg_len)) ? PM_CIPHER_OK : PM_CIPHER_TAG;
    if (*status == PM_CIPHER_OK)
      for (uint32_t j = 0; j < msg_len; ++j) memcpy(msg_out + 4 * j, m[j].l, 32);
  }
  return PM_OK;
}

extern "C" int pm_test_cipher_stride(pm_ctx* ctx, size_t* stride) {
  if (!ctx || !stride) return PM_ERR_BAD_ARG;
  *stride = slot_blocks(ctx, ~(size_t)0 >> 1) * 64;
  return PM_OK;
}

extern "C" int pm_test_cipher_digits(const uint64_t view_key[4], uint32_t scalar_form, int8_t digits[64]) {
  uint64_t vk[4];
  if (!view_key || !digits || (scalar_form != PM_SCALAR_MONTGOMERY && scalar_form != PM_SCALAR_CANONICAL)) return PM_ERR_BAD_ARG;
  if (!scalar_to_int(view_key, scalar_form, vk)) return PM_ERR_BAD_ARG;
  signed char d[JJ_WINDOWS];
  recode_digits(vk, d);
  for (u32 w = 0; w < JJ_WINDOWS; ++w) digits[w] = d[w];
  return PM_OK;
}
