// Checked commit-key loading: the 48-byte zcash encoding of G1 (G1Affine::{to_compressed, from_compressed}; n of them
// back to back are dusk-plonk's CommitKey::to_var_bytes / from_slice) and the on-curve / subgroup checks, on the device.
// One thread per point, four kernels:
//
//   g1_decompress_kernel    x -> y = (x^3 + 4)^((p + 1) / 4), the root picked by the sign bit; y^2 = x^3 + 4 decides
//                           "on the curve".  The exponent is a constant (379 bits, 229 set): the whole ladder is a fixed
//                           schedule read with wave-uniform indices -- a sliding window of 4 bits over a table of the 8
//                           odd powers (112 VGPRs; the 16 entries of a fixed window would be 224), 379 squarings + 79
//                           products + 8 for the table.  Lanes with a malformed input run the same stream on x = 0.
//   g1_curve_check_kernel   points already affine: coordinates below p, y^2 = x^3 + 4 or the pair (0, 0).
//   g1_subgroup_kernel      phi(P) = [-z^2] P with phi(x, y) = (beta x, y), beta = 2^((p - 1) / 3), z = -0xd201000000010000
//                           the curve parameter (M. Scott, "A note on group membership tests for G1, G2 and GT on BLS
//                           pairing-friendly curves", 2021): two multiplications by the sparse 64-bit |z| (63 doublings and
//                           5 additions each) instead of 255 doublings and ~130 additions by r.  A kernel of its own: the
//                           decompression waves do not carry a point accumulator.  Every wave takes the same branches (the
//                           scalar is a constant); only the after-the-fact special cases of xyzz_add diverge.
//   g1_compress_kernel      the inverse of the decoder, the device twin of Transcript::g1_compress.
//
// Verdict: one 64-bit word, (index << 2 | reason), updated with atomicMin -- the lowest failing index and, for that
// point, the lowest reason, whatever the order the waves run in.  The output is always written in full; a rejected
// point becomes (0, 0).
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>

#include "context.h"
#include "ec.hip.h"
#include "host_field.h"
#include "prover_transcript.h"

namespace pm {

enum { FORM_ABI = 0, FORM_DEV = 1 };   // coordinates x R mod p with R = 2^384 (the ABI) or 2^392 (resident bases)

constexpr u32 G1_HALF[12] = {0xffffd555u, 0xdcff7fffu, 0x58a9ffffu, 0x0f55ffffu, 0x7b587b12u, 0xb3986950u,
                             0x79c2895fu, 0xb23ba5c2u, 0x21a5d66bu, 0x258dd3dbu, 0x1cbff34du, 0x0d0088f5u};   // (p - 1) / 2
constexpr u32 G1_SQRT_EXP[12] = {0xffffeaabu, 0xee7fbfffu, 0xac54ffffu, 0x07aaffffu, 0x3dac3d89u, 0xd9cc34a8u,
                                 0x3ce144afu, 0xd91dd2e1u, 0x90d2eb35u, 0x92c6e9edu, 0x8e5ff9a6u, 0x0680447au};   // (p + 1) / 4
constexpr int G1_SQRT_BITS = 379;
constexpr u32 G1_BETA[12] = {0xfffefffeu, 0x2e01ffffu, 0x620a0002u, 0xde17d813u, 0xe6f89688u, 0xddb3a93bu,
                             0x6a0f77eau, 0xba69c607u, 0xdf76ce51u, 0x5f19672fu, 0x00000000u, 0x00000000u};   // 2^((p-1)/3) mod p
constexpr unsigned long long G1_Z_ABS = 0xd201000000010000ull;

// The ladder of t^((p + 1) / 4) as one entry per squaring, most significant bit first: 0 = square only, k + 1 = square,
// then multiply by the table's entry k = t^(2k + 1).  A window opens at a set bit and ends at the last set bit among the
// WIN bits from there; the product is due after the squaring of the window's last bit.
template <int WIN>
struct SqrtSchedule {
  u32 op[G1_SQRT_BITS];
};
constexpr u32 sqrt_exp_bit(int i) { return (G1_SQRT_EXP[i >> 5] >> (i & 31)) & 1u; }
template <int WIN>
constexpr SqrtSchedule<WIN> make_sqrt_schedule() {
  SqrtSchedule<WIN> s{};
  int i = G1_SQRT_BITS - 1;
  while (i >= 0) {
    if (!sqrt_exp_bit(i)) {
      --i;
      continue;
    }
    int j = i - WIN + 1 < 0 ? 0 : i - WIN + 1;
    while (!sqrt_exp_bit(j)) ++j;
    u32 val = 0;
    for (int b = i; b >= j; --b) val = 2 * val + sqrt_exp_bit(b);
    s.op[G1_SQRT_BITS - 1 - j] = (val >> 1) + 1;
    i = j - 1;
  }
  return s;
}
constexpr int G1_SQRT_WIN = 4;
__constant__ SqrtSchedule<G1_SQRT_WIN> g1_sqrt_schedule = make_sqrt_schedule<G1_SQRT_WIN>();

// t^((p + 1) / 4): a square root of t when t is a square (p = 3 mod 4).  t and the result: products, (1, <2)
PM_DEV Fp fp_sqrt_candidate(const Fp& t) {
  constexpr int NT = 1 << (G1_SQRT_WIN - 1);
  Fp T[NT];
  T[0] = t;
  const Fp t2 = fe_sqr<FpP>(t);
#pragma unroll
  for (int k = 1; k < NT; ++k) T[k] = fe_mul<FpP>(T[k - 1], t2);
  Fp acc = fe_one<FpP>();
#pragma unroll 1
  for (int s = 0; s < G1_SQRT_BITS; ++s) {
    acc = fe_sqr<FpP>(acc);
    const u32 op = g1_sqrt_schedule.op[s];   // the same for every lane of every wave
    if (op) {
      Fp m = T[0];
#pragma unroll
      for (int k = 1; k < NT; ++k) m = fp_select(op == (u32)(k + 1), T[k], m);
      acc = fe_mul<FpP>(acc, m);
    }
  }
  return acc;
}

PM_DEV void report_bad(unsigned long long* verdict, size_t i, u32 reason) {
  atomicMin(verdict, ((unsigned long long)i << 2) | reason);
}
PM_DEV bool words_below_p(const u32 (&s)[12]) {
  bool lt = false, eq = true;
#pragma unroll
  for (int i = 11; i >= 0; --i) {
    lt = lt || (eq && s[i] < FpP::SAT[i]);
    eq = eq && s[i] == FpP::SAT[i];
  }
  return lt;
}
PM_DEV bool words_above_half(const u32 (&s)[12]) {
  bool gt = false, eq = true;
#pragma unroll
  for (int i = 11; i >= 0; --i) {
    gt = gt || (eq && s[i] > G1_HALF[i]);
    eq = eq && s[i] == G1_HALF[i];
  }
  return gt;
}
PM_DEV void load_words12(const u32x4* p, u32 (&s)[12]) {
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const u32x4 v = p[i];
    s[4 * i] = v.x;
    s[4 * i + 1] = v.y;
    s[4 * i + 2] = v.z;
    s[4 * i + 3] = v.w;
  }
}
PM_DEV void store_words12(u32x4* p, const u32 (&s)[12]) {
#pragma unroll
  for (int i = 0; i < 3; ++i) p[i] = u32x4{s[4 * i], s[4 * i + 1], s[4 * i + 2], s[4 * i + 3]};
}
// x^3 + 4 for x in the device form, reduced through a product: (1, <2)
PM_DEV Fp curve_rhs(const Fp& X) {
  const Fp x3 = fe_mul<FpP>(fe_sqr<FpP>(X), X);
  return fe_mul<FpP>(fe_add<FpP>(x3, fe_pow2<FpP, FpP::W * FpP::N + 2>()), fe_one<FpP>());
}
// a == b mod p for two products
PM_DEV bool fp_equal_products(const Fp& a, const Fp& b) { return fp_is_zero_lazy(fe_sub<FpP, 3, 1>(a, b)); }
// coordinate in memory -> the plain integer below p as saturated words
template <int FORM>
PM_DEV void coord_to_integer(const Fp& a, u32 (&w)[12]) {
  fe_canon_pack<FpP>(w, fe_mul_limb<FpP>(a, FORM == FORM_ABI ? 256u : 1u));   // x 2^384 * 2^8 / 2^392
}

__global__ void __launch_bounds__(128) g1_decompress_kernel(const u32x4* in, size_t n, u32x4* out, unsigned long long* verdict) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  u32 w[12], s[12];
  load_words12(in + 3 * i, w);
#pragma unroll
  for (int k = 0; k < 12; ++k) s[k] = __builtin_bswap32(w[11 - k]);   // big-endian bytes -> little-endian words
  const u32 top = s[11] >> 29;
  s[11] &= 0x1fffffffu;
  const bool compressed = top & 4u, inf = top & 2u, big = top & 1u;
  u32 nz = 0;
#pragma unroll
  for (int k = 0; k < 12; ++k) nz |= s[k];
  const bool malformed = !compressed || (inf && (big || nz)) || (!inf && !words_below_p(s));
  if (malformed || inf) {   // the dummy: x = 0, a point of the curve
#pragma unroll
    for (int k = 0; k < 12; ++k) s[k] = 0;
  }
  const Fp X = fe_mul<FpP>(fe_unpack<FpP>(s), fe_pow2<FpP, 2 * FpP::W * FpP::N>());   // x 2^392
  const Fp t = curve_rhs(X);
  const Fp y = fp_sqrt_candidate(t);
  const bool on_curve = fp_equal_products(fe_sqr<FpP>(y), t);
  u32 yw[12];
  coord_to_integer<FORM_DEV>(y, yw);
  const bool flip = words_above_half(yw) != big;
  const Fp ysel = fp_select(flip, fe_sub<FpP, 3, 1>(fe_zero<FpP>(), y), y);
  const Fp to_abi = fe_pow2<FpP, 384>();
  const u32 reason = malformed ? PM_G1_BAD_ENCODING : ((!inf && !on_curve) ? PM_G1_BAD_NOT_ON_CURVE : 0u);
  if (reason) report_bad(verdict, i, reason);
  const bool keep = !reason && !inf;
  u32 ox[12], oy[12];
  fe_canon_pack<FpP>(ox, fe_mul<FpP>(X, to_abi));
  fe_canon_pack<FpP>(oy, fe_mul<FpP>(ysel, to_abi));
#pragma unroll
  for (int k = 0; k < 12; ++k) {
    ox[k] = keep ? ox[k] : 0u;
    oy[k] = keep ? oy[k] : 0u;
  }
  store_words12(out + 6 * i, ox);
  store_words12(out + 6 * i + 3, oy);
}

template <int FORM>
__global__ void __launch_bounds__(128) g1_compress_kernel(const u32x4* in, size_t n, u32x4* out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  u32 xs[12], ys[12], xw[12], yw[12];
  load_words12(in + 6 * i, xs);
  load_words12(in + 6 * i + 3, ys);
  u32 nz = 0;
#pragma unroll
  for (int k = 0; k < 12; ++k) nz |= xs[k] | ys[k];
  coord_to_integer<FORM>(fe_unpack<FpP>(xs), xw);
  coord_to_integer<FORM>(fe_unpack<FpP>(ys), yw);
  const bool big = words_above_half(yw);
  if (!nz) {
#pragma unroll
    for (int k = 0; k < 12; ++k) xw[k] = 0;
  }
  xw[11] |= nz ? (big ? 0xa0000000u : 0x80000000u) : 0xc0000000u;
  u32 o[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) o[k] = __builtin_bswap32(xw[11 - k]);
  store_words12(out + 3 * i, o);
}

template <int FORM>
__global__ void __launch_bounds__(128) g1_curve_check_kernel(const u32x4* in, size_t n, unsigned long long* verdict) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  u32 xs[12], ys[12];
  load_words12(in + 6 * i, xs);
  load_words12(in + 6 * i + 3, ys);
  u32 nz = 0;
#pragma unroll
  for (int k = 0; k < 12; ++k) nz |= xs[k] | ys[k];
  const bool canonical = words_below_p(xs) && words_below_p(ys);
  Fp X = fe_unpack<FpP>(xs), Y = fe_unpack<FpP>(ys);
  if (FORM == FORM_ABI) {
    X = fe_abi_to_dev<FpP>(X);
    Y = fe_abi_to_dev<FpP>(Y);
  }
  const bool on_curve = fp_equal_products(fe_sqr<FpP>(Y), curve_rhs(X));
  if (!canonical)
    report_bad(verdict, i, PM_G1_BAD_ENCODING);
  else if (nz && !on_curve)
    report_bad(verdict, i, PM_G1_BAD_NOT_ON_CURVE);
}

// [|z|] p: left-to-right double-and-add from the bit below the top one; the scalar is a constant
PM_DEV Xyzz xyzz_mul_z(const Xyzz& p) {
  Xyzz r = p;
#pragma unroll 1
  for (int bit = 62; bit >= 0; --bit) {
    r = xyzz_double(r);
    if ((G1_Z_ABS >> bit) & 1ull) r = xyzz_add(r, p);
  }
  return r;
}

// zero_out (may be null): the ABI affine array a rejected point is cleared in (the decoder's output)
template <int FORM>
__global__ void __launch_bounds__(128) g1_subgroup_kernel(const u32x4* in, size_t n, unsigned long long* verdict, u32x4* zero_out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  Fp x = fe_load<FpP>(in + 6 * i), y = fe_load<FpP>(in + 6 * i + 3);
  u32 nz = 0;
#pragma unroll
  for (int k = 0; k < 14; ++k) nz |= x.l[k] | y.l[k];
  if (FORM == FORM_ABI) {
    x = fe_abi_to_dev<FpP>(x);
    y = fe_abi_to_dev<FpP>(y);
  }
  Xyzz p;
  p.x = x;
  p.y = y;
  p.zz = fe_one<FpP>();
  p.zzz = fe_one<FpP>();
  p.inf = nz == 0;
  const Xyzz q = xyzz_mul_z(xyzz_mul_z(p));   // [z^2] P
  // phi(P) = -Q:  beta x ZZ = X_Q  and  y ZZZ = -Y_Q
  u32 bw[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) bw[k] = G1_BETA[k];
  const Fp beta = fe_mul<FpP>(fe_unpack<FpP>(bw), fe_pow2<FpP, 2 * FpP::W * FpP::N>());
  const Fp lx = fe_mul<FpP>(fe_mul<FpP>(beta, x), q.zz);
  const Fp ly = fe_mul<FpP>(y, q.zzz);
  const bool same_x = fp_is_zero_lazy(fe_sub<FpP, 11, 1>(lx, q.x));
  const bool neg_y = fp_is_zero_lazy(fe_add<FpP>(ly, q.y));
  const bool ok = p.inf || (!q.inf && same_x && neg_y);
  if (!ok) {
    report_bad(verdict, i, PM_G1_BAD_NOT_IN_SUBGROUP);
    if (zero_out) {
      const u32x4 z = u32x4{0u, 0u, 0u, 0u};
#pragma unroll
      for (int k = 0; k < 6; ++k) zero_out[6 * i + k] = z;
    }
  }
}

namespace {

struct DevScratch {   // freed on every path
  void* p = nullptr;
  ~DevScratch() {
    if (p) (void)hipFree(p);
  }
};
inline dim3 grid_for(size_t n) { return dim3((unsigned)((n + 127) / 128)); }
inline bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

int finish_verdict(pm_ctx* ctx, const void* d_verdict, hipStream_t st, uint64_t* bad_index, uint32_t* bad_reason, const char* what) {
  unsigned long long v = ~0ull;
  PM_HIP(ctx, hipMemcpyAsync(&v, d_verdict, 8, hipMemcpyDeviceToHost, st));
  PM_HIP(ctx, hipStreamSynchronize(st));
  if (v == ~0ull) return PM_OK;
  static const char* const why[4] = {"", "malformed encoding or non-canonical coordinate", "not on the curve", "not in the subgroup"};
  if (bad_index) *bad_index = v >> 2;
  if (bad_reason) *bad_reason = (uint32_t)(v & 3u);
  return set_err(ctx, PM_ERR_POINT, std::string(what) + ": point " + std::to_string(v >> 2) + " " + why[v & 3u] + " (reason " +
                                        std::to_string(v & 3u) + ")");
}

// the caller holds ctx->mu and has set the device
int decompress_locked(pm_ctx* ctx, const void* d_bytes, size_t n, uint32_t flags, void* d_out_xy, uint64_t* bad_index,
                      uint32_t* bad_reason, hipStream_t st) {
  DevScratch verdict;
  PM_HIP(ctx, hipMalloc(&verdict.p, 8));
  PM_HIP(ctx, hipMemsetAsync(verdict.p, 0xff, 8, st));
  {
    ProfScope prof(ctx, st, "g1_decompress");
    hipLaunchKernelGGL(g1_decompress_kernel, grid_for(n), dim3(128), 0, st, (const u32x4*)d_bytes, n, (u32x4*)d_out_xy,
                       (unsigned long long*)verdict.p);
  }
  if (flags & PM_G1_CHECK_SUBGROUP) {
    ProfScope prof(ctx, st, "g1_subgroup_check");
    hipLaunchKernelGGL((g1_subgroup_kernel<FORM_ABI>), grid_for(n), dim3(128), 0, st, (const u32x4*)d_out_xy, n,
                       (unsigned long long*)verdict.p, (u32x4*)d_out_xy);
  }
  PM_HIP(ctx, hipGetLastError());
  return finish_verdict(ctx, verdict.p, st, bad_index, bad_reason, "g1 decompress");
}

template <int FORM>
int check_locked(pm_ctx* ctx, const void* d_xy, size_t n, uint32_t flags, uint64_t* bad_index, uint32_t* bad_reason, hipStream_t st) {
  DevScratch verdict;
  PM_HIP(ctx, hipMalloc(&verdict.p, 8));
  PM_HIP(ctx, hipMemsetAsync(verdict.p, 0xff, 8, st));
  {
    ProfScope prof(ctx, st, "g1_curve_check");
    hipLaunchKernelGGL((g1_curve_check_kernel<FORM>), grid_for(n), dim3(128), 0, st, (const u32x4*)d_xy, n,
                       (unsigned long long*)verdict.p);
  }
  if (flags & PM_G1_CHECK_SUBGROUP) {
    ProfScope prof(ctx, st, "g1_subgroup_check");
    hipLaunchKernelGGL((g1_subgroup_kernel<FORM>), grid_for(n), dim3(128), 0, st, (const u32x4*)d_xy, n,
                       (unsigned long long*)verdict.p, (u32x4*)nullptr);
  }
  PM_HIP(ctx, hipGetLastError());
  return finish_verdict(ctx, verdict.p, st, bad_index, bad_reason, "g1 check");
}

template <int FORM>
int compress_locked(pm_ctx* ctx, const void* d_xy, size_t n, void* d_bytes_out, hipStream_t st) {
  ProfScope prof(ctx, st, "g1_compress");
  hipLaunchKernelGGL((g1_compress_kernel<FORM>), grid_for(n), dim3(128), 0, st, (const u32x4*)d_xy, n, (u32x4*)d_bytes_out);
  PM_HIP(ctx, hipGetLastError());
  return PM_OK;
}

constexpr size_t G1_MAX_POINTS = 0x7fffffffu;

}  // namespace
}  // namespace pm

// ------------------------------------------------------------------ host, one point
extern "C" int pm_g1_compress(const uint64_t xy[12], uint8_t out[48]) {
  if (!xy || !out) return PM_ERR_BAD_ARG;
  Transcript::g1_compress(out, xy);
  return PM_OK;
}

extern "C" int pm_g1_decompress(const uint8_t in[48], uint32_t flags, uint64_t xy[12], uint32_t* bad_reason) {
  if (!in || !xy || (flags & ~PM_G1_CHECK_SUBGROUP)) return PM_ERR_BAD_ARG;
  using namespace pm::host;
  const Field<6>& F = FP();
  memset(xy, 0, 96);
  auto fail = [&](uint32_t reason) {
    if (bad_reason) *bad_reason = reason;
    return (int)PM_ERR_POINT;
  };
  const bool compressed = in[0] & 0x80, inf = in[0] & 0x40, big = in[0] & 0x20;
  HFp xi = zero<6>();
  for (int i = 0; i < 48; ++i) xi.l[(47 - i) / 8] |= (uint64_t)(i ? in[i] : (in[0] & 0x1f)) << (8 * ((47 - i) % 8));
  if (!compressed) return fail(PM_G1_BAD_ENCODING);
  if (inf) return (big || !is_zero(xi)) ? fail(PM_G1_BAD_ENCODING) : (int)PM_OK;
  if (geq<6>(xi.l, F.m)) return fail(PM_G1_BAD_ENCODING);
  HFp r2, raw1 = zero<6>();
  memcpy(r2.l, F.r2, 48);
  raw1.l[0] = 1;
  const HFp x = mul(xi, r2, F);
  const HFp t = add(mul(mul(x, x, F), x, F), from_u64(4, F), F);
  static const uint64_t e[6] = {0xee7fbfffffffeaabULL, 0x07aaffffac54ffffULL, 0xd9cc34a83dac3d89ULL,
                                0xd91dd2e13ce144afULL, 0x92c6e9ed90d2eb35ULL, 0x0680447a8e5ff9a6ULL};   // (p + 1) / 4
  HFp y = pow(t, e, 6, F);
  if (!eq(mul(y, y, F), t)) return fail(PM_G1_BAD_NOT_ON_CURVE);
  const HFp yc = mul(y, raw1, F), nyc = sub(zero<6>(), yc, F);   // canonical y and p - y
  const bool is_big = geq<6>(yc.l, nyc.l) && !eq(yc, nyc);
  if (is_big != big) y = sub(zero<6>(), y, F);
  if (flags & PM_G1_CHECK_SUBGROUP) {   // [r] P by double-and-add over the group law behind pm_g1_fold
    XYZZ p, acc = xyzz_identity();
    p.x = x;
    p.y = y;
    p.zz = one(F);
    p.zzz = one(F);
    for (int bit = 254; bit >= 0; --bit) {
      acc = xyzz_double(acc);
      if ((FR().m[bit / 64] >> (bit % 64)) & 1) acc = xyzz_add(acc, p);
    }
    if (!is_zero(acc.zz)) return fail(PM_G1_BAD_NOT_IN_SUBGROUP);
  }
  memcpy(xy, x.l, 48);
  memcpy(xy + 6, y.l, 48);
  return PM_OK;
}

// ------------------------------------------------------------------ device buffers
extern "C" int pm_g1_decompress_dev(pm_ctx* ctx, const void* d_bytes, size_t n, uint32_t flags, void* d_out_xy,
                                    uint64_t* bad_index, uint32_t* bad_reason, void* hip_stream) {
  if (!ctx) return PM_ERR_BAD_ARG;
  if (flags & ~PM_G1_CHECK_SUBGROUP) return pm::set_err(ctx, PM_ERR_BAD_ARG, "unknown flag bits");
  if (n == 0) return PM_OK;
  if (!d_bytes || !d_out_xy) return pm::set_err(ctx, PM_ERR_BAD_ARG, "null device pointer");
  if (!pm::aligned16(d_bytes) || !pm::aligned16(d_out_xy)) return pm::set_err(ctx, PM_ERR_BAD_ARG, "device pointers must be 16-byte aligned");
  if (n > pm::G1_MAX_POINTS) return pm::set_err(ctx, PM_ERR_LENGTH, "n > 2^31");
  std::lock_guard<std::mutex> lk(ctx->mu);
  PM_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t st = hip_stream ? (hipStream_t)hip_stream : ctx->stream;
  return pm::decompress_locked(ctx, d_bytes, n, flags, d_out_xy, bad_index, bad_reason, st);
}

extern "C" int pm_g1_check_dev(pm_ctx* ctx, const void* d_xy, size_t n, uint32_t flags, uint64_t* bad_index,
                               uint32_t* bad_reason, void* hip_stream) {
  if (!ctx) return PM_ERR_BAD_ARG;
  if (flags & ~PM_G1_CHECK_SUBGROUP) return pm::set_err(ctx, PM_ERR_BAD_ARG, "unknown flag bits");
  if (n == 0) return PM_OK;
  if (!d_xy) return pm::set_err(ctx, PM_ERR_BAD_ARG, "null device pointer");
  if (!pm::aligned16(d_xy)) return pm::set_err(ctx, PM_ERR_BAD_ARG, "device pointers must be 16-byte aligned");
  if (n > pm::G1_MAX_POINTS) return pm::set_err(ctx, PM_ERR_LENGTH, "n > 2^31");
  std::lock_guard<std::mutex> lk(ctx->mu);
  PM_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t st = hip_stream ? (hipStream_t)hip_stream : ctx->stream;
  return pm::check_locked<pm::FORM_ABI>(ctx, d_xy, n, flags, bad_index, bad_reason, st);
}

extern "C" int pm_g1_compress_dev(pm_ctx* ctx, const void* d_xy, size_t n, void* d_bytes_out, void* hip_stream) {
  if (!ctx) return PM_ERR_BAD_ARG;
  if (n == 0) return PM_OK;
  if (!d_xy || !d_bytes_out) return pm::set_err(ctx, PM_ERR_BAD_ARG, "null device pointer");
  if (!pm::aligned16(d_xy) || !pm::aligned16(d_bytes_out)) return pm::set_err(ctx, PM_ERR_BAD_ARG, "device pointers must be 16-byte aligned");
  if (n > pm::G1_MAX_POINTS) return pm::set_err(ctx, PM_ERR_LENGTH, "n > 2^31");
  std::lock_guard<std::mutex> lk(ctx->mu);
  PM_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t st = hip_stream ? (hipStream_t)hip_stream : ctx->stream;
  return pm::compress_locked<pm::FORM_ABI>(ctx, d_xy, n, d_bytes_out, st);
}

// ------------------------------------------------------------------ conveniences
extern "C" int pm_g1_bases_check(pm_ctx* ctx, const pm_bases* bases, uint32_t flags, uint64_t* bad_index, uint32_t* bad_reason) {
  if (!ctx) return PM_ERR_BAD_ARG;
  if (!bases) return pm::set_err(ctx, PM_ERR_BAD_ARG, "null bases");
  if (flags & ~PM_G1_CHECK_SUBGROUP) return pm::set_err(ctx, PM_ERR_BAD_ARG, "unknown flag bits");
  if (bases->n == 0) return PM_OK;
  std::lock_guard<std::mutex> lk(ctx->mu);
  PM_HIP(ctx, hipSetDevice(ctx->device));
  return pm::check_locked<pm::FORM_DEV>(ctx, bases->d_xy, bases->n, flags, bad_index, bad_reason, ctx->stream);
}

extern "C" int pm_g1_bases_from_compressed(pm_ctx* ctx, const uint8_t* bytes, size_t n, uint32_t flags, pm_bases** out,
                                           uint64_t* bad_index, uint32_t* bad_reason) {
  if (!ctx || !out) return PM_ERR_BAD_ARG;
  *out = nullptr;
  if (flags & ~PM_G1_CHECK_SUBGROUP) return pm::set_err(ctx, PM_ERR_BAD_ARG, "unknown flag bits");
  if (!bytes && n) return pm::set_err(ctx, PM_ERR_BAD_ARG, "null bytes");
  if (n > pm::G1_MAX_POINTS) return pm::set_err(ctx, PM_ERR_LENGTH, "n > 2^31");
  if (n == 0) return pm_g1_bases_from_dev(ctx, nullptr, 0, out);
  pm::DevScratch d_bytes, d_xy;
  {
    std::lock_guard<std::mutex> lk(ctx->mu);
    PM_HIP(ctx, hipSetDevice(ctx->device));
    PM_HIP(ctx, hipMalloc(&d_bytes.p, n * 48));
    PM_HIP(ctx, hipMalloc(&d_xy.p, n * 96));
    PM_HIP(ctx, hipMemcpyAsync(d_bytes.p, bytes, n * 48, hipMemcpyHostToDevice, ctx->stream));
    const int rc = pm::decompress_locked(ctx, d_bytes.p, n, flags, d_xy.p, bad_index, bad_reason, ctx->stream);
    if (rc) return rc;
  }
  return pm_g1_bases_from_dev(ctx, d_xy.p, n, out);   // takes the lock itself; returns with its copy complete
}

extern "C" int pm_g1_bases_to_compressed(pm_ctx* ctx, const pm_bases* bases, uint8_t* bytes_out) {
  if (!ctx) return PM_ERR_BAD_ARG;
  if (!bases) return pm::set_err(ctx, PM_ERR_BAD_ARG, "null bases");
  if (bases->n == 0) return PM_OK;
  if (!bytes_out) return pm::set_err(ctx, PM_ERR_BAD_ARG, "null output");
  std::lock_guard<std::mutex> lk(ctx->mu);
  PM_HIP(ctx, hipSetDevice(ctx->device));
  pm::DevScratch d_bytes;
  PM_HIP(ctx, hipMalloc(&d_bytes.p, bases->n * 48));
  const int rc = pm::compress_locked<pm::FORM_DEV>(ctx, bases->d_xy, bases->n, d_bytes.p, ctx->stream);
  if (rc) return rc;
  PM_HIP(ctx, hipMemcpyAsync(bytes_out, d_bytes.p, bases->n * 48, hipMemcpyDeviceToHost, ctx->stream));
  PM_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return PM_OK;
}
