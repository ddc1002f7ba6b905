// Raw-limb test hooks: the shared inline routines of fields.hip.h, field_inv.hip.h, ec.hip.h and ntt_kernels.hip.h, called
// as they are, on operands given as radix-2^W limbs (no fe_unpack, no reduction) and with the result limbs returned as they
// come (no fe_canon_pack).  One thread per case, one launch per call.  The tests (tests/test_gpu_field_bounds.py,
// tests/test_gpu_g1_bounds.py) feed them the worst members of the operand classes the call sites document and compare
// limb for limb with the big-integer model (oracle/fe_model.py).  What they check is the arithmetic and the bounds of
// the routines; the code the compiler generates for a production kernel that inlines them is a different instance.
// The inversion routines (fe_canon_limbs, fe_inv_int, fe_inv_dev) have a kernel of their own, raw_inv_kernel: fe_inv_int votes
// across the wave, and tests/test_gpu_field_inv.py chooses the integers the binary GCD iterates on and the company a case keeps
// in its wave.
#include <hip/hip_runtime.h>

#include "context.h"
#include "ec_mul.hip.h"
#include "field_inv.hip.h"
#include "fields.hip.h"
#include "host_field.h"
#include "jubjub_scalar.hip.h"
#include "ntt_kernels.hip.h"
#include "ntt_kernels4.hip.h"

namespace pm {

enum RawOp {
  RAW_ADD = 0, RAW_NORM, RAW_NORM_FULL, RAW_MUL, RAW_SQR, RAW_MUL_LIMB, RAW_MUL2, RAW_MUL3, RAW_MMA2, RAW_SQR2,
  RAW_REDUCE_WEAK, RAW_UNPACK, RAW_CANON_PACK, RAW_POW2, RAW_SPLIT_5_6, RAW_SPLIT_1_2, RAW_ZERO_PRODUCT, RAW_ZERO_LAZY,
  RAW_DFT8, RAW_DFT4, RAW_CANON_LIMBS, RAW_INV_INT, RAW_INV_DEV, RAW_REDUCE_CANON_PACK = 24,
  RAW_SPLIT_3_3, RAW_SPLIT_1_1, RAW_SPLIT_5_5,   // the lazy forms (D = G) the radix-4 passes use
  RAW_SUB = 32   // RAW_SUB + K: fe_sub<K, 1>
};

__host__ __device__ constexpr int raw_in(int op) {
  return op == RAW_ADD || op == RAW_MUL || op == RAW_MUL_LIMB || op == RAW_SQR2 || op >= RAW_SUB ? 2
         : op == RAW_MUL2                                                                         ? 4
         : op == RAW_MUL3 || op == RAW_MMA2                                                       ? 6
         : op == RAW_SPLIT_5_6 || op == RAW_SPLIT_5_5                                             ? 3
         : op == RAW_SPLIT_3_3                                                                    ? 4
         : op == RAW_SPLIT_1_2 || op == RAW_SPLIT_1_1                                             ? 10
         : op == RAW_DFT8                                                                         ? 11
         : op == RAW_DFT4                                                                         ? 5
                                                                                                  : 1;
}
__host__ __device__ constexpr int raw_out(int op) {
  return op == RAW_MUL2 || op == RAW_MMA2 || op == RAW_SQR2 ? 2 : op == RAW_MUL3 ? 3 : op == RAW_DFT8 ? 8 : op == RAW_DFT4 ? 4 : 1;
}

template <class P>
PM_DEV Fe<P> ld_raw(const u32* p) {
  Fe<P> r;
#pragma unroll
  for (int i = 0; i < P::N; ++i) r.l[i] = p[i];
  return r;
}
template <class P>
PM_DEV void st_raw(u32* p, const Fe<P>& v) {
#pragma unroll
  for (int i = 0; i < P::N; ++i) p[i] = v.l[i];
}

template <class P, int OP>
__global__ void raw_op_kernel(const u32* in, u32* out, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  constexpr int N = P::N, NI = raw_in(OP), NO = raw_out(OP);
  const u32* s = in + i * (size_t)(NI * N);
  u32* d = out + i * (size_t)(NO * N);
  Fe<P> x[NI], r[NO];
#pragma unroll
  for (int e = 0; e < NI; ++e) x[e] = ld_raw<P>(s + e * N);
#pragma unroll
  for (int e = 0; e < NO; ++e) r[e] = fe_zero<P>();
  if constexpr (OP == RAW_ADD) r[0] = fe_add<P>(x[0], x[1]);
  if constexpr (OP == RAW_NORM) r[0] = fe_norm<P>(x[0]);
  if constexpr (OP == RAW_NORM_FULL) r[0] = fe_norm_full<P>(x[0]);
  if constexpr (OP == RAW_MUL) r[0] = fe_mul<P>(x[0], x[1]);
  if constexpr (OP == RAW_SQR) r[0] = fe_sqr<P>(x[0]);
  if constexpr (OP == RAW_MUL_LIMB) r[0] = fe_mul_limb<P>(x[0], x[1].l[0]);
  if constexpr (OP == RAW_MUL2) fe_mul2<P>(x[0], x[1], x[2], x[3], r[0], r[1]);
  if constexpr (OP == RAW_MUL3) fe_mul3<P>(x[0], x[1], x[2], x[3], x[4], x[5], r[0], r[1], r[2]);
  if constexpr (OP == RAW_MMA2) fe_mma2<P>(x[0], x[1], x[2], x[3], x[4], x[5], r[0], r[1]);
  if constexpr (OP == RAW_SQR2) fe_sqr2<P>(x[0], x[1], r[0], r[1]);
  if constexpr (OP == RAW_REDUCE_WEAK) r[0] = fe_reduce_weak<P>(x[0]);
  if constexpr (OP == RAW_UNPACK) r[0] = fe_unpack<P>(x[0].l);          // the first NS words are the saturated limbs
  if constexpr (OP == RAW_CANON_PACK) fe_canon_pack<P>(r[0].l, x[0]);   // NS saturated words, the rest stays zero
  // the exit of the radix-4 last passes: the wave votes, cases 64 k .. 64 k + 63 share a wave (lanes past n have left)
  if constexpr (OP == RAW_REDUCE_CANON_PACK) fe_reduce_canon_pack<P>(r[0].l, x[0]);
  if constexpr (OP == RAW_POW2) {
    const u32 sel = x[0].l[0];
    r[0] = sel == 0 ? fe_pow2<P, P::W * P::N>() : sel == 1 ? fe_pow2<P, 2 * P::W * P::N - 32 * P::NS>() : fe_pow2<P, 64 * P::NS + P::W * P::N>();
  }
  if constexpr (OP == RAW_SPLIT_5_6) r[0] = fe_mul_split<P, 5, 6>(x[0], [&](int j, int b) { return x[1 + j].l[b]; });
  if constexpr (OP == RAW_SPLIT_1_2) r[0] = fe_mul_split<P, 1, 2>(x[0], [&](int j, int b) { return x[1 + j].l[b]; });
  if constexpr (OP == RAW_SPLIT_3_3) r[0] = fe_mul_split<P, 3, 3>(x[0], [&](int j, int b) { return x[1 + j].l[b]; });
  if constexpr (OP == RAW_SPLIT_1_1) r[0] = fe_mul_split<P, 1, 1>(x[0], [&](int j, int b) { return x[1 + j].l[b]; });
  if constexpr (OP == RAW_SPLIT_5_5) r[0] = fe_mul_split<P, 5, 5>(x[0], [&](int j, int b) { return x[1 + j].l[b]; });
  if constexpr (OP == RAW_ZERO_PRODUCT) r[0].l[0] = fp_is_zero_product(x[0]) ? 1u : 0u;
  if constexpr (OP == RAW_ZERO_LAZY) r[0].l[0] = fp_is_zero_lazy(x[0]) ? 1u : 0u;
  if constexpr (OP == RAW_DFT8) {
    dft8(x, x[8], x[9], x[10]);
#pragma unroll
    for (int e = 0; e < 8; ++e) r[e] = x[e];
  }
  if constexpr (OP == RAW_DFT4) {
    dft4(x[0], x[1], x[2], x[3], x[4]);
#pragma unroll
    for (int e = 0; e < 4; ++e) r[e] = x[e];
  }
  if constexpr (OP >= RAW_SUB) r[0] = fe_sub<P, OP - RAW_SUB, 1>(x[0], x[1]);
#pragma unroll
  for (int e = 0; e < NO; ++e) st_raw<P>(d + e * N, r[e]);
}

// ---- inversion (field_inv.hip.h), one operand in, one result out.  The kernel has the shape of the production call sites:
// fe_inv_int leaves its loop through a wave-wide vote, so every lane of every wave has to reach it -- a lane past n works on
// element n - 1 and stores nothing.  A block is 64 threads, ONE wave: cases 64 k .. 64 k + 63 share a wave and its vote.  The
// tests rely on that; they place a case in the company they want by ordering the inputs.
template <class P, int OP>
__global__ void __launch_bounds__(64) raw_inv_kernel(const u32* in, u32* out, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = i < n;
  const Fe<P> x = ld_raw<P>(in + (live ? i : n - 1) * (size_t)P::N);
  Fe<P> r;
  if constexpr (OP == RAW_CANON_LIMBS) r = fe_canon_limbs<P>(x);
  if constexpr (OP == RAW_INV_INT) r = fe_inv_int<P>(x);
  if constexpr (OP == RAW_INV_DEV) r = fe_inv_dev<P>(x);
  if (!live) return;
  st_raw<P>(out + i * (size_t)P::N, r);
}

// ---- group law: a point is 57 words, X | Y | ZZ | ZZZ (14 limbs each) | infinity flag
constexpr int PT_WORDS = 57;
enum G1Op { G1_DOUBLE_AFFINE = 0, G1_DOUBLE, G1_MADD, G1_ADD, G1_MUL_SMALL, G1_HALF_DOUBLE, G1_HALF_ADD };

PM_DEV Xyzz ld_raw_point(const u32* p) {
  Xyzz r;
  r.x = ld_raw<FpP>(p);
  r.y = ld_raw<FpP>(p + 14);
  r.zz = ld_raw<FpP>(p + 28);
  r.zzz = ld_raw<FpP>(p + 42);
  r.inf = p[56] != 0;
  return r;
}

template <int OP>
__global__ void g1_raw_op_kernel(const u32* a, const u32* b, u32* out, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const Xyzz p = ld_raw_point(a + PT_WORDS * i), q = ld_raw_point(b + PT_WORDS * i);
  Xyzz r;
  if constexpr (OP == G1_DOUBLE_AFFINE) r = xyzz_double_affine(p.x, p.y);
  if constexpr (OP == G1_DOUBLE) r = xyzz_double(p);
  if constexpr (OP == G1_MADD) r = xyzz_madd(p, q.x, q.y);
  if constexpr (OP == G1_ADD) r = xyzz_add(p, q);
  if constexpr (OP == G1_MUL_SMALL) r = xyzz_mul_small(p, b[PT_WORDS * i]);
  if (r.inf) r = xyzz_identity();
  u32* d = out + PT_WORDS * i;
  st_raw<FpP>(d, r.x);
  st_raw<FpP>(d + 14, r.y);
  st_raw<FpP>(d + 28, r.zz);
  st_raw<FpP>(d + 42, r.zzz);
  d[56] = r.inf ? 1u : 0u;
}

// one point per lane pair, as the reduction kernels hold it: the even lane X / ZZ, the odd lane Y / ZZZ
template <int OP>
__global__ void g1_half_op_kernel(const u32* a, const u32* b, u32* out, size_t n) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t i = t >> 1;
  const bool isB = t & 1;
  if (i >= n) return;   // both lanes of a pair leave together
  auto ld = [&](const u32* p) {
    Half h;
    h.c0 = ld_raw<FpP>(p + (isB ? 14 : 0));
    h.c1 = ld_raw<FpP>(p + (isB ? 42 : 28));
    h.inf = p[56] != 0;
    return h;
  };
  const Half p = ld(a + PT_WORDS * i), q = ld(b + PT_WORDS * i);
  Half r = OP == G1_HALF_DOUBLE ? half_double(p, isB) : half_add(p, q, isB);
  if (r.inf) r = half_identity();
  u32* d = out + PT_WORDS * i;
  st_raw<FpP>(d + (isB ? 14 : 0), r.c0);
  st_raw<FpP>(d + (isB ? 42 : 28), r.c1);
  if (!isB) d[56] = r.inf ? 1u : 0u;
}

// the GLV split as the multiplication kernels run it: load, canonical conversion, fr_glv_split
__global__ void glv_split_kernel(const u32x4* scalars, size_t n, u32 scalar_form, u32* out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  u32 w[8], k1[4], k2[4];
  fr_load_canon(scalars + 2 * i, scalar_form == PM_SCALAR_MONTGOMERY, w);
  fr_glv_split(w, k1, k2);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    out[8 * i + j] = k1[j];
    out[8 * i + 4 + j] = k2[j];
  }
}

// the integers modulo l of jubjub_scalar.hip.h: four words a value, one thread a case
__global__ void jubjub_scalar_op_kernel(int op, const u64* a, const u64* b, const u64* c, u64* out, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  u64 x[4], y[4] = {0, 0, 0, 0}, z[4] = {0, 0, 0, 0}, r[4] = {0, 0, 0, 0};
#pragma unroll
  for (int j = 0; j < 4; ++j) x[j] = a[4 * i + j];
  if (op == 1) {
#pragma unroll
    for (int j = 0; j < 4; ++j) y[j] = b[4 * i + j], z[j] = c[4 * i + j];
  }
  if (op == 0) scl_reduce(r, x);
  if (op == 1) scl_mulsub(r, x, y, z);
  if (op == 2) r[0] = scl_below_l(x) ? 1u : 0u;
#pragma unroll
  for (int j = 0; j < 4; ++j) out[4 * i + j] = r[j];
}

struct FreeAll {   // the temporaries go away on every path, error returns included
  void* p[3] = {nullptr, nullptr, nullptr};
  ~FreeAll() {
    for (void* q : p)
      if (q) (void)hipFree(q);
  }
};

template <class P>
static bool launch_raw(int op, dim3 g, dim3 blk, hipStream_t st, const u32* in, u32* out, size_t n) {
#define RAW_CASE(OP) \
  case OP: hipLaunchKernelGGL((raw_op_kernel<P, OP>), g, blk, 0, st, in, out, n); return true;
  constexpr bool FR = P::N == 9;
  switch (op) {
    RAW_CASE(RAW_ADD) RAW_CASE(RAW_NORM) RAW_CASE(RAW_NORM_FULL) RAW_CASE(RAW_MUL) RAW_CASE(RAW_SQR) RAW_CASE(RAW_MUL_LIMB)
    RAW_CASE(RAW_MUL2) RAW_CASE(RAW_MUL3) RAW_CASE(RAW_MMA2) RAW_CASE(RAW_SQR2) RAW_CASE(RAW_REDUCE_WEAK) RAW_CASE(RAW_UNPACK)
    RAW_CASE(RAW_CANON_PACK) RAW_CASE(RAW_POW2)
    RAW_CASE(RAW_SUB + 2) RAW_CASE(RAW_SUB + 3) RAW_CASE(RAW_SUB + 5)
  }
  if constexpr (FR) {
    switch (op) { RAW_CASE(RAW_SPLIT_5_6) RAW_CASE(RAW_SPLIT_1_2) RAW_CASE(RAW_DFT8) RAW_CASE(RAW_DFT4) RAW_CASE(RAW_REDUCE_CANON_PACK) RAW_CASE(RAW_SUB + 9)
                  RAW_CASE(RAW_SPLIT_3_3) RAW_CASE(RAW_SPLIT_1_1) RAW_CASE(RAW_SPLIT_5_5) RAW_CASE(RAW_SUB + 18) RAW_CASE(RAW_SUB + 34) RAW_CASE(RAW_SUB + 39) }
  } else {
    switch (op) { RAW_CASE(RAW_ZERO_PRODUCT) RAW_CASE(RAW_ZERO_LAZY) RAW_CASE(RAW_SUB + 6) RAW_CASE(RAW_SUB + 8) RAW_CASE(RAW_SUB + 11) }
  }
#undef RAW_CASE
#define RAW_INV_CASE(OP) \
  case OP: hipLaunchKernelGGL((raw_inv_kernel<P, OP>), g, blk, 0, st, in, out, n); return true;
  switch (op) { RAW_INV_CASE(RAW_CANON_LIMBS) RAW_INV_CASE(RAW_INV_INT) RAW_INV_CASE(RAW_INV_DEV) }
#undef RAW_INV_CASE
  return false;
}

}  // namespace pm

using namespace pm;

extern "C" int pm_test_field_raw_op(pm_ctx* ctx, int field, int op, const uint32_t* in, uint32_t* out, size_t n) {
  if (!ctx || !in || !out || field < 0 || field > 1 || op < 0 || op > RAW_SUB + 39) return PM_ERR_BAD_ARG;
  const bool fr = field == 0;
  {   // the (field, op) pairs that exist: every fe_sub<K, 1> the library instantiates, the split product and the butterflies for Fr, the zero tests for Fp, the inversion routines for both
    const int k = op - RAW_SUB;
    const bool sub_ok = k == 2 || k == 3 || k == 5 || (fr ? (k == 9 || k == 18 || k == 34 || k == 39) : (k == 6 || k == 8 || k == 11));
    const bool fr_only = op == RAW_SPLIT_5_6 || op == RAW_SPLIT_1_2 || op == RAW_DFT8 || op == RAW_DFT4 || op == RAW_REDUCE_CANON_PACK || (op >= RAW_SPLIT_3_3 && op <= RAW_SPLIT_5_5);
    const bool fp_only = op == RAW_ZERO_PRODUCT || op == RAW_ZERO_LAZY;
    if (op >= RAW_SUB ? !sub_ok : ((op > RAW_INV_DEV && !(op >= RAW_REDUCE_CANON_PACK && op <= RAW_SPLIT_5_5)) || (fr_only && !fr) || (fp_only && fr))) return PM_ERR_BAD_ARG;
  }
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (n == 0) return PM_OK;
  PM_HIP(ctx, hipSetDevice(ctx->device));
  const size_t limbs = fr ? FrP::N : FpP::N;
  const size_t in_bytes = n * raw_in(op) * limbs * 4, out_bytes = n * raw_out(op) * limbs * 4;
  FreeAll tmp;
  PM_HIP(ctx, hipMalloc(&tmp.p[0], in_bytes));
  PM_HIP(ctx, hipMalloc(&tmp.p[1], out_bytes));
  PM_HIP(ctx, hipMemcpyAsync(tmp.p[0], in, in_bytes, hipMemcpyHostToDevice, ctx->stream));
  dim3 g((unsigned)((n + 63) / 64)), blk(64);   // 64: raw_inv_kernel's waves are its blocks
  const u32* din = (const u32*)tmp.p[0];
  u32* dout = (u32*)tmp.p[1];
  const bool ok = fr ? launch_raw<FrP>(op, g, blk, ctx->stream, din, dout, n) : launch_raw<FpP>(op, g, blk, ctx->stream, din, dout, n);
  if (!ok) return set_err(ctx, PM_ERR_BAD_ARG, "pm_test_field_raw_op: no such (field, op)");
  PM_HIP(ctx, hipGetLastError());
  PM_HIP(ctx, hipMemcpyAsync(out, tmp.p[1], out_bytes, hipMemcpyDeviceToHost, ctx->stream));
  PM_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return PM_OK;
}

extern "C" int pm_test_g1_raw_op(pm_ctx* ctx, int op, const uint32_t* a, const uint32_t* b, uint32_t* out, size_t n) {
  if (!ctx || !a || !out || op < G1_DOUBLE_AFFINE || op > G1_HALF_ADD) return PM_ERR_BAD_ARG;
  const bool unary = op == G1_DOUBLE_AFFINE || op == G1_DOUBLE || op == G1_HALF_DOUBLE;
  if (!b) {
    if (!unary) return PM_ERR_BAD_ARG;
    b = a;   // the doublings ignore b
  }
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (n == 0) return PM_OK;
  PM_HIP(ctx, hipSetDevice(ctx->device));
  const size_t bytes = n * PT_WORDS * 4;
  FreeAll tmp;
  for (int i = 0; i < 3; ++i) PM_HIP(ctx, hipMalloc(&tmp.p[i], bytes));
  PM_HIP(ctx, hipMemcpyAsync(tmp.p[0], a, bytes, hipMemcpyHostToDevice, ctx->stream));
  PM_HIP(ctx, hipMemcpyAsync(tmp.p[1], b, bytes, hipMemcpyHostToDevice, ctx->stream));
  const u32 *da = (const u32*)tmp.p[0], *db = (const u32*)tmp.p[1];
  u32* dc = (u32*)tmp.p[2];
  const bool half = op >= G1_HALF_DOUBLE;
  const size_t threads = half ? 2 * n : n;
  dim3 g((unsigned)((threads + 63) / 64)), blk(64);
  switch (op) {
    case G1_DOUBLE_AFFINE: hipLaunchKernelGGL((g1_raw_op_kernel<G1_DOUBLE_AFFINE>), g, blk, 0, ctx->stream, da, db, dc, n); break;
    case G1_DOUBLE: hipLaunchKernelGGL((g1_raw_op_kernel<G1_DOUBLE>), g, blk, 0, ctx->stream, da, db, dc, n); break;
    case G1_MADD: hipLaunchKernelGGL((g1_raw_op_kernel<G1_MADD>), g, blk, 0, ctx->stream, da, db, dc, n); break;
    case G1_ADD: hipLaunchKernelGGL((g1_raw_op_kernel<G1_ADD>), g, blk, 0, ctx->stream, da, db, dc, n); break;
    case G1_MUL_SMALL: hipLaunchKernelGGL((g1_raw_op_kernel<G1_MUL_SMALL>), g, blk, 0, ctx->stream, da, db, dc, n); break;
    case G1_HALF_DOUBLE: hipLaunchKernelGGL((g1_half_op_kernel<G1_HALF_DOUBLE>), g, blk, 0, ctx->stream, da, db, dc, n); break;
    case G1_HALF_ADD: hipLaunchKernelGGL((g1_half_op_kernel<G1_HALF_ADD>), g, blk, 0, ctx->stream, da, db, dc, n); break;
  }
  PM_HIP(ctx, hipGetLastError());
  PM_HIP(ctx, hipMemcpyAsync(out, tmp.p[2], bytes, hipMemcpyDeviceToHost, ctx->stream));
  PM_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return PM_OK;
}

extern "C" int pm_test_glv_split(pm_ctx* ctx, const uint64_t* scalars, size_t n, uint32_t scalar_form, uint64_t* out) {
  if (!ctx || !scalars || !out || scalar_form > PM_SCALAR_CANONICAL) return PM_ERR_BAD_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (n == 0) return PM_OK;
  PM_HIP(ctx, hipSetDevice(ctx->device));
  FreeAll tmp;
  PM_HIP(ctx, hipMalloc(&tmp.p[0], n * 32));
  PM_HIP(ctx, hipMalloc(&tmp.p[1], n * 32));
  PM_HIP(ctx, hipMemcpyAsync(tmp.p[0], scalars, n * 32, hipMemcpyHostToDevice, ctx->stream));
  hipLaunchKernelGGL(glv_split_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, ctx->stream, (const u32x4*)tmp.p[0], n,
                     scalar_form, (u32*)tmp.p[1]);
  PM_HIP(ctx, hipGetLastError());
  PM_HIP(ctx, hipMemcpyAsync(out, tmp.p[1], n * 32, hipMemcpyDeviceToHost, ctx->stream));
  PM_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return PM_OK;
}

extern "C" int pm_test_host_glv_split(const uint64_t k[4], uint64_t out[4]) {
  if (!k || !out) return PM_ERR_BAD_ARG;
  GlvWords8 in{};
  for (int i = 0; i < 4; ++i) {
    in.w[2 * i] = (u32)k[i];
    in.w[2 * i + 1] = (u32)(k[i] >> 32);
  }
  const GlvHalves h = glv_split_words(in);
  out[0] = h.k1[0] | (uint64_t)h.k1[1] << 32;
  out[1] = h.k1[2] | (uint64_t)h.k1[3] << 32;
  out[2] = h.k2[0] | (uint64_t)h.k2[1] << 32;
  out[3] = h.k2[2] | (uint64_t)h.k2[3] << 32;
  return PM_OK;
}

extern "C" int pm_test_jubjub_scalar_op(pm_ctx* ctx, int op, const uint64_t* a, const uint64_t* b, const uint64_t* c, uint64_t* out,
                                        size_t n) {
  if (!ctx || !a || !out || op < 0 || op > 2 || (op == 1 && (!b || !c))) return PM_ERR_BAD_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (n == 0) return PM_OK;
  PM_HIP(ctx, hipSetDevice(ctx->device));
  FreeAll tmp;
  PM_HIP(ctx, hipMalloc(&tmp.p[0], 3 * n * 32));             // a | b | c
  PM_HIP(ctx, hipMalloc(&tmp.p[1], n * 32));
  u64* const da = (u64*)tmp.p[0];
  PM_HIP(ctx, hipMemcpyAsync(da, a, n * 32, hipMemcpyHostToDevice, ctx->stream));
  if (op == 1) {
    PM_HIP(ctx, hipMemcpyAsync(da + 4 * n, b, n * 32, hipMemcpyHostToDevice, ctx->stream));
    PM_HIP(ctx, hipMemcpyAsync(da + 8 * n, c, n * 32, hipMemcpyHostToDevice, ctx->stream));
  }
  hipLaunchKernelGGL(jubjub_scalar_op_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, ctx->stream, op, da, da + 4 * n,
                     da + 8 * n, (u64*)tmp.p[1], n);
  PM_HIP(ctx, hipGetLastError());
  PM_HIP(ctx, hipMemcpyAsync(out, tmp.p[1], n * 32, hipMemcpyDeviceToHost, ctx->stream));
  PM_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return PM_OK;
}

extern "C" int pm_test_host_jubjub_scalar_op(int op, const uint64_t* a, const uint64_t* b, const uint64_t* c, uint64_t* out, size_t n) {
  if (!a || !out || op < 0 || op > 2 || (op == 1 && (!b || !c))) return PM_ERR_BAD_ARG;
  for (size_t i = 0; i < n; ++i) {
    uint64_t r[4] = {0, 0, 0, 0};
    if (op == 0) host::mod_l(a + 4 * i, 4, r);
    if (op == 1) host::mulsub_l(a + 4 * i, b + 4 * i, c + 4 * i, r);
    if (op == 2) r[0] = host::below_l(a + 4 * i) ? 1u : 0u;
    memcpy(out + 4 * i, r, 32);
  }
  return PM_OK;
}

// the plane-major exchange of the radix-4 first and single pass kernels, from the constexpr maps the kernels themselves index with
extern "C" int pm_test_ntt_exchange_map(uint32_t S, uint32_t LT, uint32_t ufast, uint32_t step, uint32_t tid, uint32_t out[12]) {
  if (!out || S > 10 || LT > 6 || ufast > 1 || !step4_plane_major((int)S, false)) return PM_ERR_BAD_ARG;
  const int s = (int)step, last = (int)S / 2 - 1, si = (int)S, lt = (int)LT;
  if (s > last || tid >= (1u << (S - 2 + LT))) return PM_ERR_BAD_ARG;
  const bool uf = ufast != 0;
  const u32 tau = step4_pm_tau(si, lt, uf, s, tid);
  out[0] = step4_pm_butterfly(si, s, tau);
  out[1] = step4_pm_col(si, lt, uf, s, tid);
  for (int t = 0; t < 4; ++t) out[2 + t] = s < last ? step4_pm_write(si, lt, uf, s, tid, t) : 0xFFFFFFFFu;
  for (int m = 0; m < 4; ++m) out[6 + m] = s > 0 ? step4_pm_read(si, lt, uf, s, tid, m) : 0xFFFFFFFFu;
  out[10] = step4_pm_digit(si, s, tau);
  out[11] = s == 1 && step4_l1_consumer(si, lt, uf) ? 1u : 0u;
  return PM_OK;
}
