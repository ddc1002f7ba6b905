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
  u32x4* scratch;           // [entry][chunk][thread of the grid], then a secret (x | y) a thread
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

// SCAN: the secret is what the ladder left in the thread's slot and the point test judges the ephemeral key
template <bool SCAN>
__global__ void __launch_bounds__(64) cipher_decrypt_kernel(const HadesTab tab, const CipherIo a) {
  const size_t g = (size_t)blockIdx.x * 64 + threadIdx.x;
  const bool live = g < a.n;
  const size_t i = live ? g : a.n - 1;
  const Fr zero = fe_zero<FrP>();
  const u32x4* const ct = a.in + 2 * (size_t)(a.len + 1) * i;
  Fr s[5];
  bool point_ok, range_ok;
  {
    Fr x, y;
    point_ok = jj_point_ok(a.tested + 4 * i, fr_limbs(a.edwards_d), x, y);
    if (SCAN) x = g_to_dev(ld_canon(a.secrets, 2 * i)), y = g_to_dev(ld_canon(a.secrets, 2 * i + 1));
    range_ok = jj_below_r(a.nonces[2 * i], a.nonces[2 * i + 1]);
    cph_init(s, x, y, g_to_dev(ld_canon(a.nonces, i)), a, tab);
  }
  h_rounds_thread(s, tab);
  // the messages wait, packed, for the verdict of the tag
  u32 m[CPH_MAX_LEN][8];
  s[0] = h_absorb(s[0], zero, tab.ark);
#pragma unroll
  for (u32 j = 0; j < CPH_MAX_LEN; ++j) {
    if (j < a.len) {                                         // uniform
      range_ok = range_ok && jj_below_r(ct[2 * j], ct[2 * j + 1]);
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
  range_ok = range_ok && jj_below_r(t0, t1);
  u32 tag[8];
  fe_canon_pack<FrP>(tag, g_to_abi(s[1]));
  const u32 diff = (tag[0] ^ t0.x) | (tag[1] ^ t0.y) | (tag[2] ^ t0.z) | (tag[3] ^ t0.w) | (tag[4] ^ t1.x) | (tag[5] ^ t1.y) |
                   (tag[6] ^ t1.z) | (tag[7] ^ t1.w);
  const u32 status = !point_ok ? PM_CIPHER_POINT : !range_ok ? PM_CIPHER_RANGE : diff != 0 ? PM_CIPHER_TAG : PM_CIPHER_OK;
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
  u32x4* const out = a.scratch + (size_t)8 * JJ_POINT_CHUNKS * T + 4 * tid;
  st_canon(out, 0, gmul(acc.X, zi));                         // device x ABI -> ABI
  st_canon(out, 1, gmul(acc.Y, zi));
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
  jubjub_d_limbs(l.edwards_d);
  recode_digit_words(vk, l.digits);
  CipherIo a{};
  a.secrets = l.scratch + (size_t)8 * JJ_POINT_CHUNKS * stride, a.n_ok = n_ok ? d_ok : nullptr;
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
