// Per-point scalar multiplication in G1: out[i] = scalars[i] * points[i], `G1Affine * Scalar` of dusk_bls12_381 in bulk
// (DESIGN.md section 7.4c).  One thread per point and one launch: the signed-window ladder of ec_mul.hip.h over the whole
// scalar (any curve point), or, when the caller asserts that every point lies in the order-r subgroup, over the two
// 128-bit halves of the GLV split.  Results go to XYZZ records and through the shared normalisation of msm.hip, so the
// output may alias the points.
//
// The grid is bounded (a few workgroups per CU, grid-stride loop): the thread-private window table, 1792 bytes per
// thread in flight, stays below 256 MiB whatever n is.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "context.h"
#include "ec_mul.hip.h"

namespace pm {

template <bool GLV>
__global__ void __launch_bounds__(128) g1_scalar_mul_kernel(const u32x4* points, const u32x4* scalars, size_t n, u32 scalar_form,
                                                            u32x4* records, u32x4* table) {
  const size_t T = (size_t)gridDim.x * blockDim.x;
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const MulTable tbl{table + tid, T};
  for (size_t i = tid; i < n; i += T) {
    Fp x = fe_load<FpP>(points + 6 * i), y = fe_load<FpP>(points + 6 * i + 3);
    u32 nz = 0;
#pragma unroll
    for (int k = 0; k < 14; ++k) nz |= x.l[k] | y.l[k];
    Xyzz p;
    p.x = fe_abi_to_dev<FpP>(x);
    p.y = fe_abi_to_dev<FpP>(y);
    p.zz = fe_one<FpP>();
    p.zzz = fe_one<FpP>();
    p.inf = nz == 0;
    u32 w[8];
    fr_load_canon(scalars + 2 * i, scalar_form == PM_SCALAR_MONTGOMERY, w);
    st_xyzz(records, i, xyzz_mul_table<GLV>(p, w, tbl));
  }
}

// resident bases (device form, R' = 2^392) -> ABI affine (R = 2^384); (0, 0) stays (0, 0)
__global__ void bases_export_kernel(const u32x4* in, u32x4* out, size_t n_coords) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_coords) return;
  fe_store<FpP>(out + 3 * i, fe_mul<FpP>(fe_load<FpP>(in + 3 * i), fe_pow2<FpP, 384>()));
}

// threads of a bounded grid of 128-thread workgroups for n items: 512 per CU at the most
static size_t mul_grid_threads(const pm_ctx* ctx, size_t n) {
  const size_t blocks = std::min<size_t>((n + 127) / 128, (size_t)std::max(ctx->num_cus, 1) * 4);
  return std::max<size_t>(blocks, 1) * 128;
}

}  // namespace pm

using namespace pm;

extern "C" int pm_g1_scalar_mul_dev(pm_ctx* ctx, const void* d_points_xy, const void* d_scalars, size_t n, uint32_t scalar_form,
                                    uint32_t flags, void* d_out_xy, void* hip_stream) {
  if (!ctx) return PM_ERR_BAD_ARG;
  if (scalar_form > PM_SCALAR_CANONICAL) return set_err(ctx, PM_ERR_BAD_ARG, "scalar_form");
  if (flags & ~PM_G1_POINTS_IN_SUBGROUP) return set_err(ctx, PM_ERR_BAD_ARG, "unknown flag bits");
  if (n == 0) return PM_OK;
  if (!d_points_xy || !d_scalars || !d_out_xy) return set_err(ctx, PM_ERR_BAD_ARG, "null device pointer");
  if (((uintptr_t)d_points_xy | (uintptr_t)d_scalars | (uintptr_t)d_out_xy) & 15u)
    return set_err(ctx, PM_ERR_BAD_ARG, "device pointers must be 16-byte aligned");
  if (n > 0x7fffffffu) return set_err(ctx, PM_ERR_LENGTH, "n > 2^31");
  std::lock_guard<std::mutex> lk(ctx->mu);
  PM_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t st = hip_stream ? (hipStream_t)hip_stream : ctx->stream;
  // scratch: n XYZZ records + the n x 64-byte prefix of the normalisation; the window table of the threads in flight
  void *scratch = nullptr, *table = nullptr;
  struct Free2 {
    void** a;
    void** b;
    ~Free2() {
      for (void** p : {a, b})
        if (*p) (void)hipFree(*p);
    }
  } free2{&scratch, &table};
  const size_t threads = mul_grid_threads(ctx, n);
  PM_HIP(ctx, hipMalloc(&scratch, n * (256 + 64)));
  PM_HIP(ctx, hipMalloc(&table, threads * MUL_TABLE_BYTES));
  u32x4* rec = (u32x4*)scratch;
  hipError_t e;
  {
    ProfScope prof(ctx, st, "g1_scalar_mul");
    const dim3 grid((unsigned)(threads / 128)), block(128);
    if (flags & PM_G1_POINTS_IN_SUBGROUP)
      hipLaunchKernelGGL((g1_scalar_mul_kernel<true>), grid, block, 0, st, (const u32x4*)d_points_xy, (const u32x4*)d_scalars, n,
                         scalar_form, rec, (u32x4*)table);
    else
      hipLaunchKernelGGL((g1_scalar_mul_kernel<false>), grid, block, 0, st, (const u32x4*)d_points_xy, (const u32x4*)d_scalars, n,
                         scalar_form, rec, (u32x4*)table);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = xyzz_records_to_affine(ctx, rec, n, rec + 16 * n, d_out_xy, true, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);   // the scratch is freed on return
  if (e != hipSuccess) return set_err(ctx, PM_ERR_HIP, std::string("g1 scalar mul: ") + hipGetErrorString(e));
  return PM_OK;
}

extern "C" int pm_g1_bases_to_dev(pm_ctx* ctx, const pm_bases* bases, void* d_out_xy, void* hip_stream) {
  if (!ctx) return PM_ERR_BAD_ARG;
  if (!bases) return set_err(ctx, PM_ERR_BAD_ARG, "null bases");
  if (bases->n == 0) return PM_OK;
  if (!d_out_xy || ((uintptr_t)d_out_xy & 15u)) return set_err(ctx, PM_ERR_BAD_ARG, "null or unaligned device pointer");
  std::lock_guard<std::mutex> lk(ctx->mu);
  PM_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t st = hip_stream ? (hipStream_t)hip_stream : ctx->stream;
  const size_t coords = 2 * bases->n;
  hipLaunchKernelGGL(bases_export_kernel, dim3((unsigned)((coords + 255) / 256)), dim3(256), 0, st, (const u32x4*)bases->d_xy,
                     (u32x4*)d_out_xy, coords);
  PM_HIP(ctx, hipGetLastError());
  return PM_OK;
}
