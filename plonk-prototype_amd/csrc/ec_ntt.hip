// Lagrange-form commit key: an inverse NTT over G1 points ("EC-NTT").
//
//   out[i] = [L_i(tau)] G = n^-1 sum_{j<n} w^-ij powers[j],   n = 2^log_n, w = the generator of pm_domain_info(log_n)
//
// Radix-2 decimation in time over XYZZ points: the bases are gathered in bit-reversed order into a scratch of
// 256-byte records (ec.hip.h), then log_n stages of butterflies (a + t, a - t), t = w^-k b, one butterfly per thread
// and one launch per stage, and one affine normalisation at the end (precompute_affine_kernel, msm.hip).  The
// variable-base scalar multiplication by the twiddle is the whole cost: ~254 doublings and ~127 additions per
// butterfly, against 512 bytes of scratch traffic.
//
// Thread order within a stage: consecutive threads take consecutive butterfly GROUPS of one twiddle, so a wave shares
// its twiddle (a uniform double-and-add branch, no divergence) in every stage with at least 64 groups -- all but the
// last six.  The first stage has only twiddle 1 and does no multiplication; the n^-1 scale is folded into the last
// stage (a and b both get one multiplication there: n^-1 a and n^-1 w^-k b).
//
// Exceptional cases (a == t, a == -t, identities, a twiddle product that is the identity) are the after-the-fact slow
// path of xyzz_add; the double-and-add itself never adds a point to itself (every prefix of the scalar is below r).
//
// pm_g1_bases_lagrange_ex with PM_G1_POINTS_IN_SUBGROUP instantiates the stage kernel with the GLV window ladder of
// ec_mul.hip.h instead (128 doublings and ~62 additions per butterfly; 2^20 in 307 ms against 641 ms, the same bytes;
// DESIGN.md section 7.4c).  It is valid only for points of the order-r subgroup, so the plain call keeps the ladder below.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>

#include "context.h"
#include "ec_mul.hip.h"
#include "host_field.h"

namespace pm {

// twiddle (ABI Montgomery Fr, R = 2^256) -> canonical integer, 8 saturated words (fixed_base_kernel's conversion)
PM_DEV void fr_mont_to_canon(const u32x4* p, u32 (&w)[8]) {
  Fr f = fe_zero<FrP>();
  f.l[0] = 32u;   // x 2^256 * 2^5 / 2^261 = x
  fe_canon_pack<FrP>(w, fe_mul<FrP>(fe_load<FrP>(p), f));
}

// k p, k < r < 2^255 (canonical), left-to-right double-and-add from bit 254; doubling the identity is free
PM_DEV Xyzz xyzz_mul_canon(const Xyzz& p, u32 (&k)[8]) {
  Xyzz r = xyzz_identity();
  if (p.inf) return r;
#pragma unroll 1
  for (int bit = 0; bit < 255; ++bit) {
    r = xyzz_double(r);
    if ((k[7] >> 30) & 1u) r = xyzz_add(r, p);
#pragma unroll
    for (int i = 7; i > 0; --i) k[i] = (k[i] << 1) | (k[i - 1] >> 31);
    k[0] <<= 1;
  }
  return r;
}

// scratch[i] = bases[bitrev(i)] as an XYZZ record ((0, 0) -> the identity)
__global__ void __launch_bounds__(256) ec_ntt_load_kernel(const u32x4* xy, u32 log_n, size_t n, u32x4* scratch) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const size_t j = log_n ? (size_t)(__brevll((unsigned long long)i) >> (64 - log_n)) : 0;
  Xyzz p = xyzz_identity();
  const Fp x = fe_load<FpP>(xy + 6 * j), y = fe_load<FpP>(xy + 6 * j + 3);
  u32 nz = 0;
#pragma unroll
  for (int k = 0; k < 14; ++k) nz |= x.l[k] | y.l[k];
  if (nz) {
    p.x = x;
    p.y = y;
    p.zz = fe_one<FpP>();
    p.zzz = fe_one<FpP>();
    p.inf = false;
  }
  st_xyzz(scratch, i, p);
}

// one stage of n / 2 butterflies over blocks of 2 half = 2^(log_half + 1) points.  Butterfly b: twiddle index
// k = b >> lg_groups, group g = b & (groups - 1); pair (i0, i1) = (g 2 half + k, i0 + half), both < n.
// tw[j] = w^-j (j < n / 2); in the last stage (groups = 1) tw_last[j] = n^-1 w^-j and a is scaled by tw_last[0].
// GLV = false: the bitwise ladder above, any points.  GLV = true (pm_g1_bases_lagrange_ex with PM_G1_POINTS_IN_SUBGROUP):
// xyzz_mul_glv of ec_mul.hip.h with this thread's window table tbl; the twiddle is split and recoded once per butterfly,
// before the ladder, and is the same for a whole wave in every stage with at least 64 groups.
template <bool GLV>
PM_DEV void ec_ntt_butterfly(size_t b, u32x4* pts, u32 log_half, u32 lg_groups, const u32x4* tw, const u32x4* tw_last, u32 last,
                             const MulTable& tbl) {
  const size_t k = b >> lg_groups, g = b & (((size_t)1 << lg_groups) - 1);
  const size_t i0 = (g << (log_half + 1)) + k, i1 = i0 + ((size_t)1 << log_half);
  // one multiplication at a time, nothing else live across it: a is loaded after t's, and in the last stage t waits in
  // its own record while a is scaled
  Xyzz t = ld_xyzz(pts, i1);
  u32 w[8];
  if (last || k) {
    fr_mont_to_canon(last ? tw_last + 2 * k : tw + 2 * (k << lg_groups), w);
    if constexpr (GLV)
      t = xyzz_mul_table<true>(t, w, tbl);
    else
      t = xyzz_mul_canon(t, w);
  }
  Xyzz a;
  if (last) {
    st_xyzz(pts, i1, t);
    fr_mont_to_canon(tw_last, w);
    if constexpr (GLV)
      a = xyzz_mul_table<true>(ld_xyzz(pts, i0), w, tbl);
    else
      a = xyzz_mul_canon(ld_xyzz(pts, i0), w);
    t = ld_xyzz(pts, i1);
  } else {
    a = ld_xyzz(pts, i0);
  }
  st_xyzz(pts, i0, xyzz_add(a, t));
  st_xyzz(pts, i1, xyzz_add(a, xyzz_neg(t)));
}

// GLV = false: one butterfly per thread.  GLV = true: a bounded grid with a grid-stride loop, so that the window table
// (table: 1792 bytes per thread of the grid, [entry][chunk][thread]) does not grow with n; a wave still takes 64
// consecutive butterflies per turn.
template <bool GLV>
__global__ void __launch_bounds__(128) ec_ntt_stage_kernel(u32x4* pts, size_t half_n, u32 log_half, u32 lg_groups,
                                                           const u32x4* tw, const u32x4* tw_last, u32 last, u32x4* table) {
  const size_t b = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if constexpr (GLV) {
    const size_t T = (size_t)gridDim.x * blockDim.x;
    const MulTable tbl{table + b, T};
    for (size_t i = b; i < half_n; i += T) ec_ntt_butterfly<true>(i, pts, log_half, lg_groups, tw, tw_last, last, tbl);
  } else {
    if (b >= half_n) return;
    ec_ntt_butterfly<false>(b, pts, log_half, lg_groups, tw, tw_last, last, MulTable{nullptr, 0});
  }
}

}  // namespace pm

using namespace pm;

// the body of pm_g1_bases_lagrange (glv = false) and of pm_g1_bases_lagrange_ex with the subgroup flag (glv = true)
static int bases_lagrange(pm_ctx* ctx, const pm_bases* powers, uint32_t log_n, bool glv, void* d_out_xy, void* hip_stream) {
  if (!ctx) return PM_ERR_BAD_ARG;
  if (!powers || !d_out_xy) return set_err(ctx, PM_ERR_BAD_ARG, "null pointer");
  if (log_n >= host::FR_TWO_ADICITY) return set_err(ctx, PM_ERR_DOMAIN_TOO_LARGE, "log_n >= 32");
  const size_t n = (size_t)1 << log_n, half_n = n / 2;
  if (n > powers->n) return set_err(ctx, PM_ERR_LENGTH, "2^log_n exceeds the bases");
  uint64_t w[4], wi[4], si[4];
  PM_HIP(ctx, hipSetDevice(ctx->device));
  int rc = pm_domain_info(log_n, w, wi, si);
  if (rc) return rc;
  hipStream_t st = hip_stream ? (hipStream_t)hip_stream : ctx->stream;
  // scratch: n XYZZ records + the n x 64-byte prefix of the normalisation; twiddles: w^-j and n^-1 w^-j, j < n / 2
  // with glv, the window table of the threads in flight: 128-thread workgroups, 4 per CU at the most
  void *scratch = nullptr, *tw = nullptr, *table = nullptr;
  struct Free3 {
    void** a;
    void** b;
    void** c;
    ~Free3() {
      for (void** p : {a, b, c})
        if (*p) (void)hipFree(*p);
    }
  } free3{&scratch, &tw, &table};
  const size_t glv_blocks = std::max<size_t>(std::min<size_t>((half_n + 127) / 128, (size_t)std::max(ctx->num_cus, 1) * 4), 1);
  PM_HIP(ctx, hipMalloc(&scratch, n * (256 + 64)));
  PM_HIP(ctx, hipMalloc(&tw, std::max<size_t>(half_n, 1) * 64));
  if (glv) PM_HIP(ctx, hipMalloc(&table, glv_blocks * 128 * MUL_TABLE_BYTES));
  void* tw_last = (char*)tw + half_n * 32;
  const uint64_t one[4] = {0x00000001fffffffeULL, 0x5884b7fa00034802ULL, 0x998c4fefecbc4ff5ULL, 0x1824b159acc5056fULL};
  if (half_n) {
    rc = pm_fr_powers_dev(ctx, wi, one, half_n, tw, st);
    if (!rc) rc = pm_fr_powers_dev(ctx, wi, si, half_n, tw_last, st);
    if (rc) {
      (void)hipStreamSynchronize(st);
      return rc;
    }
  }
  std::lock_guard<std::mutex> lk(ctx->mu);
  u32x4* pts = (u32x4*)scratch;
  {
    ProfScope prof(ctx, st, "g1_ec_ntt");
    hipLaunchKernelGGL(ec_ntt_load_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st,
                       (const u32x4*)powers->d_xy, log_n, n, pts);
    for (u32 s = 0; s < log_n; ++s) {
      if (glv)
        hipLaunchKernelGGL((ec_ntt_stage_kernel<true>), dim3((unsigned)glv_blocks), dim3(128), 0, st, pts, half_n, s,
                           log_n - 1 - s, (const u32x4*)tw, (const u32x4*)tw_last, (u32)(s + 1 == log_n), (u32x4*)table);
      else
        hipLaunchKernelGGL((ec_ntt_stage_kernel<false>), dim3((unsigned)((half_n + 127) / 128)), dim3(128), 0, st, pts, half_n,
                           s, log_n - 1 - s, (const u32x4*)tw, (const u32x4*)tw_last, (u32)(s + 1 == log_n), (u32x4*)nullptr);
    }
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = xyzz_records_to_affine(ctx, pts, n, pts + 16 * n, d_out_xy, true, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);   // the scratch is freed below
    if (e != hipSuccess) return set_err(ctx, PM_ERR_HIP, std::string("g1 bases lagrange: ") + hipGetErrorString(e));
  }
  return PM_OK;
}

extern "C" int pm_g1_bases_lagrange(pm_ctx* ctx, const pm_bases* powers, uint32_t log_n, void* d_out_xy, void* hip_stream) {
  return bases_lagrange(ctx, powers, log_n, false, d_out_xy, hip_stream);
}

extern "C" int pm_g1_bases_lagrange_ex(pm_ctx* ctx, const pm_bases* powers, uint32_t log_n, uint32_t flags, void* d_out_xy,
                                       void* hip_stream) {
  if (!ctx) return PM_ERR_BAD_ARG;
  if (flags & ~PM_G1_POINTS_IN_SUBGROUP) return set_err(ctx, PM_ERR_BAD_ARG, "unknown flag bits");
  return bases_lagrange(ctx, powers, log_n, (flags & PM_G1_POINTS_IN_SUBGROUP) != 0, d_out_xy, hip_stream);
}
