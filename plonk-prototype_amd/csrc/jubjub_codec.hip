// The JubJub wire format: a point as 32 bytes -- the canonical y, little-endian, with the least
// significant bit of the canonical x in bit 255 -- decoded and encoded in bulk on the device, one thread a point, over the square
// root of fr_sqrt.hip.h; and that root on its own (pm_fr_sqrt_dev).
//
//   decode    clear the sign bit, require y < r; u = y^2 - 1, v = 1 + d y^2 (never zero: -1 / d is a non-square); x = sqrt(u / v)
//             by the ratio form, one exponentiation and no inversion; x negated when its parity differs from the sign bit; x = 0
//             with the sign bit set is refused, so the accepted bytes are exactly the image of the encoder.
//   subgroup  only with PM_JUBJUB_CHECK_SUBGROUP, a second kernel over the decoded points: [l] P by the wave-uniform ladder of
//             the scan (jj_ladder_uniform, the digits of l recoded once on the host) and one inversion for the
//             identity test on the affine result.  A whole ladder a point: off by default.
//   encode    y and the parity of x out of the Montgomery form; nothing is validated.
//
// Every lane runs everything: a lane past n works on element n - 1 and stores nothing, and a failed test selects the status, it
// does not branch around the work.  A refused point is written as (0, 0), off the curve.  Records are addressed by a stride in
// bytes and only the record itself is read or written, so a strided call touches nothing in between.
//
// The encoding is the shape of JubJubAffine::to_bytes / from_bytes as remembered: prior knowledge, pinned by nothing here.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "context.h"
#include "fr_sqrt.hip.h"
#include "jubjub.hip.h"

namespace pm {
namespace {

using host::HFr;

constexpr size_t CODEC_BYTES = 32, CODEC_POINT_BYTES = 64;

// ------------------------------------------------------------------ the host forms (csrc/host_field.h)
// the canonical integer of a Montgomery element: x R * 1 / R
HFr host_plain(const HFr& v) {
  HFr one_int = host::zero<4>();
  one_int.l[0] = 1;
  return host::mul(v, one_int, host::FR());
}
HFr host_from_plain(const HFr& v) {
  HFr r2;
  memcpy(r2.l, host::FR().r2, 32);
  return host::mul(v, r2, host::FR());
}
// The even root of a (Montgomery, canonical) by the textbook Tonelli-Shanks loop: NOT the device's algorithm.  false: a is no
// square (root is then zero).
bool host_sqrt(const HFr& a, HFr& root) {
  const host::Field<4>& F = host::FR();
  const HFr one = host::one<4>(F);
  root = host::zero<4>();
  if (host::is_zero(a)) return true;
  // r - 1 = 2^32 t, t odd; e = (t - 1) / 2 = t >> 1
  uint64_t e[4];
  for (int i = 0; i < 4; ++i) e[i] = F.m[i];
  e[0] -= 1;
  for (int i = 0; i < 4; ++i) e[i] = (e[i] >> 33) | (i < 3 ? e[i + 1] << 31 : 0);
  const HFr w = host::pow(a, e, 4, F);
  HFr x = host::mul(a, w, F), b = host::mul(x, w, F), z = host::fr_root_of_unity();
  unsigned m = host::FR_TWO_ADICITY;
  while (!host::eq(b, one)) {
    unsigned i = 0;
    for (HFr s = b; !host::eq(s, one) && i < m; ++i) s = host::mul(s, s, F);
    if (i == m) return false;                                // the order of b is 2^m: no root
    HFr c = z;
    for (unsigned j = 0; j + i + 1 < m; ++j) c = host::mul(c, c, F);
    x = host::mul(x, c, F), z = host::mul(c, c, F), b = host::mul(b, z, F), m = i;
  }
  root = (host_plain(x).l[0] & 1) ? host::sub(host::zero<4>(), x, F) : x;
  return true;
}
uint32_t host_decode(const uint8_t* in, uint32_t flags, HPoint& p) {
  const host::Field<4>& F = host::FR();
  p = HPoint{host::zero<4>(), host::zero<4>()};
  uint64_t w[4];
  memcpy(w, in, 32);
  const bool sign = (w[3] >> 63) != 0;
  w[3] &= ~(1ull << 63);
  if (!hfr_canonical(w)) return PM_JUBJUB_BAD_RANGE;
  const HFr y = host_from_plain(hfr_load(w)), y2 = host::mul(y, y, F), one = host::one<4>(F);
  const HFr u = host::sub(y2, one, F), v = host::add(one, host::mul(jubjub_d_host(), y2, F), F);
  HFr x;
  if (!host_sqrt(host::mul(u, host::inv(v, F), F), x)) return PM_JUBJUB_BAD_NOT_ON_CURVE;
  if (host::is_zero(x) && sign) return PM_JUBJUB_BAD_SIGN;
  if (((host_plain(x).l[0] & 1) != 0) != sign) x = host::sub(host::zero<4>(), x, F);
  const HPoint q{x, y};
  if (flags & PM_JUBJUB_CHECK_SUBGROUP) {
    uint64_t l[4];
    memcpy(l, host::JUBJUB_L(), 32);
    const HPoint t = hpoint_mul(q, l), id = hpoint_identity();
    if (!host::eq(t.x, id.x) || !host::eq(t.y, id.y)) return PM_JUBJUB_BAD_NOT_IN_SUBGROUP;
  }
  p = q;
  return PM_JUBJUB_OK;
}

// ------------------------------------------------------------------ the tables of the root (fr_sqrt.hip.h)
// entry j of table i = g^(-j 2^(8 i)) as device limbs in 48 bytes, then the keys: limb 0 of h^j, h = g^(2^24), which is entry
// (256 - j) mod 256 of table 3.  Empty: two keys coincide (they do not; the constants are fixed).
std::vector<u32> sqrt_table_host() {
  const host::Field<4>& F = host::FR();
  std::vector<u32> t(FR_SQRT_TABLE_BYTES / 4, 0u);
  HFr step = host::inv(host::fr_root_of_unity(), F);
  for (u32 i = 0; i < FR_SQRT_WINDOWS; ++i) {
    HFr acc = host::one<4>(F);
    for (u32 j = 0; j < FR_SQRT_ENTRIES; ++j) {
      to_limbs29(&t[(size_t)4 * FR_SQRT_ENTRY_CHUNKS * (FR_SQRT_ENTRIES * i + j)], acc);
      acc = host::mul(acc, step, F);
    }
    step = acc;                                              // step^256
  }
  u32* const keys = &t[FR_SQRT_KEYS_OFFSET / 4];
  const size_t last = (size_t)4 * FR_SQRT_ENTRY_CHUNKS * FR_SQRT_ENTRIES * (FR_SQRT_WINDOWS - 1);
  for (u32 j = 0; j < FR_SQRT_ENTRIES; ++j) keys[j] = t[last + (size_t)4 * FR_SQRT_ENTRY_CHUNKS * ((FR_SQRT_ENTRIES - j) % FR_SQRT_ENTRIES)];
  std::vector<u32> sorted(keys, keys + FR_SQRT_ENTRIES);
  std::sort(sorted.begin(), sorted.end());
  if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end()) t.clear();
  return t;
}
// the context's copy, built at the first call; the caller holds the context's mutex and has selected the device
int sqrt_consts(pm_ctx* ctx, bool ratio, FrSqrtConsts& c) {
  if (!ctx->fr_sqrt_tab.ptr) {
    const std::vector<u32> t = sqrt_table_host();
    if (t.empty()) return set_err(ctx, PM_ERR_BAD_ARG, "the keys of the square-root tables coincide");
    void* d = nullptr;
    PM_HIP(ctx, hipMalloc(&d, FR_SQRT_TABLE_BYTES));
    const hipError_t e = hipMemcpy(d, t.data(), FR_SQRT_TABLE_BYTES, hipMemcpyHostToDevice);   // returns when the table is there
    if (e != hipSuccess) {
      (void)hipFree(d);
      PM_HIP(ctx, e);
    }
    ctx->fr_sqrt_tab.ptr = d, ctx->fr_sqrt_tab.bytes = FR_SQRT_TABLE_BYTES;
  }
  c.tab = (const u32x4*)ctx->fr_sqrt_tab.ptr;
  c.keys = (const PM_KCONST u32*)((const char*)ctx->fr_sqrt_tab.ptr + FR_SQRT_KEYS_OFFSET);
  fr_sqrt_exponent(c, ratio);
  return PM_OK;
}

// ------------------------------------------------------------------ device side
struct SqrtIo {
  const u32x4* in;
  u32x4* out;
  u32* flags;               // n, or null
  unsigned long long* count;   // of flag 1, or null
  size_t n;
};
struct DecodeIo {
  const char* in;           // record i at in + i in_stride
  char* out;                // point i at out + i out_stride
  size_t in_stride, out_stride;
  u32* status;              // n, or null
  unsigned long long* n_ok; // the count of status 0, or null (and null when the subgroup kernel counts)
  size_t n;
  u32 edwards_d[9];         // device form
};
struct SubgroupIo {
  char* points;             // point i at points + i stride
  size_t stride;
  u32x4* scratch;           // [entry][chunk][thread of the grid]
  u32* status;
  unsigned long long* n_ok;
  size_t n;
  u32 edwards_d[9];
  u32 digits[JJ_WINDOWS / 4];   // of l: recode_digit_words (jubjub.hip.h)
};
struct EncodeIo {
  const u32x4* in;
  u32x4* out;
  size_t n;
};

// the canonical integer of v (device form) as eight words: x 2^261 * 1 / 2^261
PM_DEV void codec_plain(u32 (&w)[8], const Fr& v) {
  Fr one_int = fe_zero<FrP>();
  one_int.l[0] = 1u;
  fe_canon_pack<FrP>(w, fe_mul<FrP>(v, one_int));
}

__global__ void __launch_bounds__(64) fr_sqrt_kernel(const FrSqrtConsts c, const SqrtIo a) {
  const size_t g = (size_t)blockIdx.x * 64 + threadIdx.x;
  const bool live = g < a.n;
  const size_t i = live ? g : a.n - 1;
  u32x4 lo = a.in[2 * i], hi = a.in[2 * i + 1];
  const bool below = jj_below_r(lo, hi);
  const u32 m = below ? ~0u : 0u;                            // an input that is not below r is worked on as zero
  const u32 s[8] = {lo.x & m, lo.y & m, lo.z & m, lo.w & m, hi.x & m, hi.y & m, hi.z & m, hi.w & m};
  bool square;
  const Fr root = fr_sqrt_dev(g_to_dev(fe_unpack<FrP>(s)), c, square);
  square = square && below;
  u32 w[8];
  fe_canon_pack<FrP>(w, g_to_abi(root));
  const u32 keep = square ? ~0u : 0u;
  if (a.count) {
    const unsigned long long hits = __ballot(live && square);
    if (threadIdx.x == 0 && hits) atomicAdd(a.count, (unsigned long long)__popcll(hits));
  }
  if (!live) return;
  a.out[2 * i] = u32x4{w[0] & keep, w[1] & keep, w[2] & keep, w[3] & keep};
  a.out[2 * i + 1] = u32x4{w[4] & keep, w[5] & keep, w[6] & keep, w[7] & keep};
  if (a.flags) a.flags[i] = square ? 1u : 0u;
}

__global__ void __launch_bounds__(64) jubjub_decode_kernel(const FrSqrtConsts c, const DecodeIo a) {
  const size_t g = (size_t)blockIdx.x * 64 + threadIdx.x;
  const bool live = g < a.n;
  const size_t i = live ? g : a.n - 1;
  const u32x4* const rec = (const u32x4*)(a.in + i * a.in_stride);
  u32x4 lo = rec[0], hi = rec[1];
  const bool sign = (hi.w >> 31) != 0;
  hi.w &= 0x7fffffffu;
  const bool below = jj_below_r(lo, hi);
  const u32 m = below ? ~0u : 0u;                            // a y that is not below r is worked on as zero
  const u32 s[8] = {lo.x & m, lo.y & m, lo.z & m, lo.w & m, hi.x & m, hi.y & m, hi.z & m, hi.w & m};
  const Fr y = fe_mul<FrP>(fe_unpack<FrP>(s), fe_pow2<FrP, 2 * FrP::W * FrP::N>());   // the integer y * 2^522 / 2^261
  const Fr y2 = fe_sqr<FrP>(y), one = fe_one<FrP>();
  const Fr u = gsub(y2, one), v = gadd(one, gmul(y2, fr_limbs(a.edwards_d)));
  bool square;
  Fr x = fr_sqrt_ratio_dev(u, v, c, square);
  u32 px[8];
  codec_plain(px, x);
  const bool x_zero = (px[0] | px[1] | px[2] | px[3] | px[4] | px[5] | px[6] | px[7]) == 0;
  x = g_sel(((px[0] & 1u) != 0) != sign, gneg(x), x);
  const u32 status = !below ? PM_JUBJUB_BAD_RANGE : !square ? PM_JUBJUB_BAD_NOT_ON_CURVE : (x_zero && sign) ? PM_JUBJUB_BAD_SIGN : PM_JUBJUB_OK;
  const u32 keep = status == PM_JUBJUB_OK ? ~0u : 0u;       // a mask, not a select between vectors
  u32 wx[8], wy[8];
  fe_canon_pack<FrP>(wx, g_to_abi(x));
  fe_canon_pack<FrP>(wy, g_to_abi(y));
  if (a.n_ok) {
    const unsigned long long hits = __ballot(live && status == PM_JUBJUB_OK);
    if (threadIdx.x == 0 && hits) atomicAdd(a.n_ok, (unsigned long long)__popcll(hits));
  }
  if (!live) return;
  u32x4* const q = (u32x4*)(a.out + i * a.out_stride);
  q[0] = u32x4{wx[0] & keep, wx[1] & keep, wx[2] & keep, wx[3] & keep};
  q[1] = u32x4{wx[4] & keep, wx[5] & keep, wx[6] & keep, wx[7] & keep};
  q[2] = u32x4{wy[0] & keep, wy[1] & keep, wy[2] & keep, wy[3] & keep};
  q[3] = u32x4{wy[4] & keep, wy[5] & keep, wy[6] & keep, wy[7] & keep};
  if (a.status) a.status[i] = status;
}

// [l] P for one stride of decoded points; (0, 0) is a point the decoding refused and stays what it is.  Two waves a SIMD: the
// ladder's register budget, as cipher_scan_ladder_kernel.
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 2))) jubjub_subgroup_kernel(const SubgroupIo a) {
  const size_t T = (size_t)gridDim.x * 64, tid = (size_t)blockIdx.x * 64 + threadIdx.x;
  const bool live = tid < a.n;
  const size_t i = live ? tid : a.n - 1;
  u32x4* const p = (u32x4*)(a.points + i * a.stride);
  const Fr ed = fr_limbs(a.edwards_d);
  u32x4* const tbl = a.scratch + tid;
  jj_table_build(tbl, T, g_to_dev(ld_canon(p, 0)), g_to_dev(ld_canon(p, 1)), ed);
  const EdPoint acc = jj_ladder_uniform(tbl, T, a.digits, ed);
  // the identity is (0, 1).  The affine test, with the inversion of the scan's ladder kernel (3 % of the ladder): under the
  // projective one, X = 0 and Y = Z, the compiler stretches the ladder over all 256 registers of the budget and spills four
  const Fr zi = fe_inv_dev<FrP>(acc.Z);                      // every lane of the wave is here
  const bool x_zero = jj_is_zero(gmul(acc.X, zi));
  const bool identity = jj_is_zero(gsub(gmul(acc.Y, zi), fe_one<FrP>())) && x_zero;
  // read again, after the ladder: sixteen words are not carried through it
  const u32x4 c0 = p[0], c1 = p[1], c2 = p[2], c3 = p[3];
  const bool refused = (c0.x | c0.y | c0.z | c0.w | c1.x | c1.y | c1.z | c1.w | c2.x | c2.y | c2.z | c2.w | c3.x | c3.y | c3.z | c3.w) == 0;
  const bool ok = !refused && identity;
  if (a.n_ok) {
    const unsigned long long hits = __ballot(live && ok);
    if (threadIdx.x == 0 && hits) atomicAdd(a.n_ok, (unsigned long long)__popcll(hits));
  }
  if (!live || refused || identity) return;
  const u32x4 zero{0u, 0u, 0u, 0u};
  p[0] = zero, p[1] = zero, p[2] = zero, p[3] = zero;
  if (a.status) a.status[i] = PM_JUBJUB_BAD_NOT_IN_SUBGROUP;
}

__global__ void __launch_bounds__(64) jubjub_encode_kernel(const EncodeIo a) {
  const size_t g = (size_t)blockIdx.x * 64 + threadIdx.x;
  if (g >= a.n) return;
  // ABI form x 2^5 / 2^261: the integer itself, as jj_load_scalar takes a Montgomery scalar
  Fr f = fe_zero<FrP>();
  f.l[0] = 32u;
  u32 wx[8], wy[8];
  fe_canon_pack<FrP>(wx, fe_mul<FrP>(ld_canon(a.in, 2 * g), f));
  fe_canon_pack<FrP>(wy, fe_mul<FrP>(ld_canon(a.in, 2 * g + 1), f));
  a.out[2 * g] = u32x4{wy[0], wy[1], wy[2], wy[3]};
  a.out[2 * g + 1] = u32x4{wy[4], wy[5], wy[6], (wy[7] & 0x7fffffffu) | (wx[0] << 31)};
}

// 0 means packed; otherwise a multiple of 16 that is at least the packed size
bool stride_fault(size_t& stride, size_t packed) {
  if (stride == 0) stride = packed;
  return stride % 16 != 0 || stride < packed;
}
int finish(pm_ctx* ctx, hipError_t e, hipStream_t st, void* buf, const unsigned long long* d_count, size_t* count, const char* who) {
  unsigned long long got = 0;
  if (int rc = finish_call(ctx, e, st, count ? &got : nullptr, d_count, 8, buf, who)) return rc;
  if (count) *count = (size_t)got;
  return PM_OK;
}

}  // namespace
}  // namespace pm

using namespace pm;

extern "C" int pm_fr_sqrt_dev(pm_ctx* ctx, const void* d_in, size_t n, void* d_out, void* d_is_square, size_t* n_square,
                              void* hip_stream) {
  if (!ctx) return PM_ERR_BAD_ARG;
  if (int rc = pointer_fault(ctx, {d_in, d_out}, ((uintptr_t)d_is_square & 3u) != 0)) return rc;
  if (int rc = count_fault(ctx, n)) return rc;
  if (n_square) *n_square = 0;
  if (n == 0) return PM_OK;
  PM_ENTER(ctx, hip_stream, st);
  FrSqrtConsts c{};
  if (int rc = sqrt_consts(ctx, false, c)) return rc;
  unsigned long long* d_count = nullptr;
  if (n_square) PM_HIP(ctx, hipMalloc((void**)&d_count, 16));
  const SqrtIo a{(const u32x4*)d_in, (u32x4*)d_out, (u32*)d_is_square, d_count, n};
  hipError_t e = n_square ? hipMemsetAsync(d_count, 0, 16, st) : hipSuccess;
  if (e == hipSuccess) {
    ProfScope prof(ctx, st, "fr_sqrt");
    hipLaunchKernelGGL(fr_sqrt_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, c, a);
    e = hipGetLastError();
  }
  return finish(ctx, e, st, d_count, d_count, n_square, "pm_fr_sqrt_dev");
}

extern "C" int pm_jubjub_decompress_dev(pm_ctx* ctx, const void* d_bytes, size_t in_stride_bytes, size_t n, uint32_t flags,
                                        void* d_out_xy, size_t out_stride_bytes, void* d_status, size_t* n_ok, void* hip_stream) {
  if (!ctx) return PM_ERR_BAD_ARG;
  if (flags & ~PM_JUBJUB_CHECK_SUBGROUP) return set_err(ctx, PM_ERR_BAD_ARG, "unknown flag bits");
  if (stride_fault(in_stride_bytes, CODEC_BYTES) || stride_fault(out_stride_bytes, CODEC_POINT_BYTES))
    return set_err(ctx, PM_ERR_BAD_ARG, "a stride is 0 (packed) or a multiple of 16 that is at least the packed size");
  if (int rc = pointer_fault(ctx, {d_bytes, d_out_xy}, ((uintptr_t)d_status & 3u) != 0)) return rc;
  if (int rc = count_fault(ctx, n)) return rc;
  if (n_ok) *n_ok = 0;
  if (n == 0) return PM_OK;
  PM_ENTER(ctx, hip_stream, st);
  FrSqrtConsts c{};
  if (int rc = sqrt_consts(ctx, true, c)) return rc;
  const bool subgroup = (flags & PM_JUBJUB_CHECK_SUBGROUP) != 0;
  // the tables of the ladder's threads in flight when the subgroup is checked, and the count when it is wanted
  SlotScratch scratch(ctx, n);
  void* buf = nullptr;
  unsigned long long* d_ok = nullptr;
  if (subgroup) {
    PM_HIP(ctx, scratch.alloc(JJ_MUL_TABLE_BYTES, 16));
    buf = scratch.base, d_ok = n_ok ? scratch.tail() : nullptr;
  } else if (n_ok) {
    PM_HIP(ctx, hipMalloc(&buf, 16));
    d_ok = (unsigned long long*)buf;
  }
  DecodeIo a{};
  a.in = (const char*)d_bytes, a.out = (char*)d_out_xy, a.in_stride = in_stride_bytes, a.out_stride = out_stride_bytes;
  a.status = (u32*)d_status, a.n_ok = subgroup ? nullptr : d_ok, a.n = n;
  jubjub_d_limbs(a.edwards_d);
  hipError_t e = d_ok ? hipMemsetAsync(d_ok, 0, 16, st) : hipSuccess;
  if (e == hipSuccess) {
    ProfScope prof(ctx, st, "jubjub_decompress");
    hipLaunchKernelGGL(jubjub_decode_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, c, a);
    e = hipGetLastError();
    if (subgroup && e == hipSuccess) {
      SubgroupIo l{};
      l.stride = out_stride_bytes, l.scratch = scratch.slots(), l.n_ok = d_ok;
      jubjub_d_limbs(l.edwards_d);
      uint64_t order[4];
      memcpy(order, host::JUBJUB_L(), 32);
      recode_digit_words(order, l.digits);
      for (size_t off = 0; off < n && e == hipSuccess; off += scratch.stride) {   // a stride at a time: the tables are per thread in flight
        l.n = std::min(scratch.stride, n - off);
        l.points = (char*)d_out_xy + off * out_stride_bytes, l.status = d_status ? (u32*)d_status + off : nullptr;
        hipLaunchKernelGGL(jubjub_subgroup_kernel, dim3((unsigned)scratch.blocks), dim3(64), 0, st, l);
        e = hipGetLastError();
      }
    }
  }
  return finish(ctx, e, st, buf, d_ok, n_ok, "pm_jubjub_decompress_dev");
}

extern "C" int pm_jubjub_compress_dev(pm_ctx* ctx, const void* d_xy, size_t n, void* d_bytes_out, void* hip_stream) {
  if (!ctx) return PM_ERR_BAD_ARG;
  if (int rc = pointer_fault(ctx, {d_xy, d_bytes_out})) return rc;
  if (int rc = count_fault(ctx, n)) return rc;
  if (n == 0) return PM_OK;
  PM_ENTER(ctx, hip_stream, st);
  const EncodeIo a{(const u32x4*)d_xy, (u32x4*)d_bytes_out, n};
  ProfScope prof(ctx, st, "jubjub_compress");
  hipLaunchKernelGGL(jubjub_encode_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, a);
  PM_HIP(ctx, hipGetLastError());
  return PM_OK;
}

extern "C" int pm_fr_sqrt_host(const uint64_t a[4], uint64_t out[4], uint32_t* is_square) {
  if (!a || !out || !is_square) return PM_ERR_BAD_ARG;
  HFr root = host::zero<4>();
  *is_square = hfr_canonical(a) && host_sqrt(hfr_load(a), root) ? 1u : 0u;
  memcpy(out, root.l, 32);
  return PM_OK;
}

extern "C" int pm_jubjub_compress(const uint64_t xy[8], uint8_t out[32]) {
  if (!xy || !out || point_fault(xy)) return PM_ERR_BAD_ARG;
  const HPoint p = hpoint_load(xy);
  HFr y = host_plain(p.y);
  y.l[3] |= (host_plain(p.x).l[0] & 1) << 63;
  memcpy(out, y.l, 32);
  return PM_OK;
}

extern "C" int pm_jubjub_decompress(const uint8_t in[32], uint32_t flags, uint64_t xy[8], uint32_t* status) {
  if (!in || !xy || !status || (flags & ~PM_JUBJUB_CHECK_SUBGROUP)) return PM_ERR_BAD_ARG;
  HPoint p;
  *status = host_decode(in, flags, p);
  hpoint_store(xy, p);
  return PM_OK;
}
