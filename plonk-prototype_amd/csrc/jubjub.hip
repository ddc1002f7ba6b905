// Native JubJub: scalar multiplications on the embedded curve outside a circuit.  gadgets.hip fills the
// ROWS of a multiplication (one wave each, every intermediate point stored); here only the product leaves the kernel, one thread
// per output, with the group law of jubjub.hip.h:
//
//   fixed base   out[i] = s_i B.  A pm_jubjub_base owns the table j 16^w B, w < 64, j = 1..8, affine (x, y, t = x y) in the
//                device form; 64 ed_madd into one extended accumulator.
//   commitment   out[i] = v_i G + b_i H: both digit strings walk into the SAME accumulator, 128 ed_madd.
//   variable     out[i] = s_i P_i: a thread's table 1 P .. 8 P in a scratch buffer, 64 windows of four doublings and an addition.
//   check        the lowest index whose point is off the curve or has a coordinate that is not below r.
// Each of the first three ends with ONE inversion (of Z) and two products.
//
// Digits.  The scalar is the INTEGER 0 <= s < r, never reduced modulo the order of a point.  Its 64 nibbles n_w become signed
// digits d_w in [-8, 8] with a carry: v = n_w + c_w; v > 8 gives d_w = v - 16 and c_(w+1) = 1, anything else d_w = v and
// c_(w+1) = 0.  Because s < r < 2^255 the top nibble is at most 7, so d_63 <= 8 and the carry out of it is 0: there is no 65th
// digit.  A digit picks entry |d| of its window (entry 1 for d = 0, so that every lane loads something) and g_sel turns what was
// loaded into the addend: negated for d < 0, the neutral addend (0, 1, 0) for d = 0.  No branch and no loop bound depends on a
// scalar or a lane; only the table index differs between the lanes of a wave.
//
// fe_inv_dev votes across the wave (field_inv.hip.h), so every lane of every wave reaches it: a lane past n works on element
// n - 1 and, not being live, stores nothing.
//
// These kernels are NOT hardened against side channels: table addresses depend on the scalar.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "context.h"
#include "field_inv.hip.h"
#include "jubjub.hip.h"

namespace pm {
namespace {

using host::HFr;

// ------------------------------------------------------------------ device side (the shared routines: jubjub.hip.h)
struct JubjubMul {
  const u32x4* tab_g;       // fixed base, commitment: the table of the (first) base
  const u32x4* tab_h;       // commitment: the table of the second base
  const u32x4* points;      // variable base: n x (x | y)
  const u32x4* scalars;     // n elements
  const u32x4* scalars_h;   // commitment: the blinders
  u32x4* out;               // n x (x | y)
  u32x4* scratch;           // variable base: [entry][chunk][thread of the grid]
  size_t n;
  u32 montgomery;           // the scalars are Montgomery elements, not plain integers
  u32 edwards_d[9];         // device form
};

// fixed base (COMMIT = false) and commitment (true): the digits from the bottom up, the order of a sum being free
template <bool COMMIT>
__global__ void __launch_bounds__(64) jubjub_fixed_kernel(const JubjubMul a) {
  const size_t g = (size_t)blockIdx.x * 64 + threadIdx.x;
  const bool live = g < a.n;
  const size_t i = live ? g : a.n - 1;
  const Fr ed = fr_limbs(a.edwards_d);
  u64 k[4], kh[4] = {0, 0, 0, 0};
  jj_load_scalar(a.scalars + 2 * i, a.montgomery != 0, k);
  if (COMMIT) jj_load_scalar(a.scalars_h + 2 * i, a.montgomery != 0, kh);
  u32 c = 0, ch = 0;
  EdPoint acc = jj_neutral();
#pragma unroll 1
  for (u32 w = 0; w < JJ_WINDOWS; ++w) {
    acc = jj_fixed_step(acc, a.tab_g, w, jj_digit((u32)k[0] & 15u, c), ed);
    jj_shr4(k);
    if (COMMIT) {
      acc = jj_fixed_step(acc, a.tab_h, w, jj_digit((u32)kh[0] & 15u, ch), ed);
      jj_shr4(kh);
    }
  }
  jj_store_affine(a.out, i, live, acc);
}

// two waves a SIMD: the register budget the allocator meets without scratch
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 2))) jubjub_var_kernel(const JubjubMul a) {
  const size_t T = (size_t)gridDim.x * 64, tid = (size_t)blockIdx.x * 64 + threadIdx.x;
  u32x4* const tbl = a.scratch + tid;
  const Fr ed = fr_limbs(a.edwards_d);
#pragma unroll 1
  for (size_t first = (size_t)blockIdx.x * 64; first < a.n; first += T) {   // wave-uniform: the lanes stay together
    const size_t g = first + threadIdx.x;
    const bool live = g < a.n;
    const size_t i = live ? g : a.n - 1;
    const Fr px = g_to_dev(ld_canon(a.points, 2 * i)), py = g_to_dev(ld_canon(a.points, 2 * i + 1));
    u64 k[4];
    jj_load_scalar(a.scalars + 2 * i, a.montgomery != 0, k);
    const u64 carries = jj_carries(k);
    jj_table_build(tbl, T, px, py, ed);
    jj_store_affine(a.out, i, live, jj_ladder(tbl, T, k, carries, JJ_WINDOWS, ed));
  }
}

__global__ void __launch_bounds__(64) jubjub_check_kernel(const u32x4* points, size_t n, const JubjubMul a /* edwards_d */,
                                                          unsigned long long* first_bad) {
  const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  Fr x, y;
  if (!jj_point_ok(points + 4 * i, fr_limbs(a.edwards_d), x, y)) atomicMin(first_bad, (unsigned long long)i);
}

// ------------------------------------------------------------------ handles and launches
// x, y, t of one table entry in the device form, 27 limbs and a zero word
void entry_limbs(u32* dst, const HPoint& p) {
  to_limbs29(dst, p.x);
  to_limbs29(dst + 9, p.y);
  to_limbs29(dst + 18, host::mul(p.x, p.y, host::FR()));
  dst[27] = 0;
}
// the point (validated) -> a handle with its table: j 16^w B built on the host with the affine law, once
int base_build(pm_ctx* ctx, const uint64_t* xy, pm_jubjub_base** out) {
  std::vector<u32> tab(JJ_BASE_TABLE_BYTES / 4);
  HPoint bw = hpoint_load(xy);                               // 16^w B
  for (u32 w = 0; w < JJ_WINDOWS; ++w) {
    HPoint e = bw;
    for (u32 j = 1; j <= 8; ++j) {
      entry_limbs(&tab[(size_t)(8 * w + j - 1) * JJ_ENTRY_CHUNKS * 4], e);
      if (j < 8) e = hpoint_add(e, bw);
    }
    bw = hpoint_add(e, e);                                   // 16 = 2 * 8
  }
  std::lock_guard<std::mutex> lk(ctx->mu);
  PM_HIP(ctx, hipSetDevice(ctx->device));
  void* d = nullptr;
  PM_HIP(ctx, hipMalloc(&d, JJ_BASE_TABLE_BYTES));
  const hipError_t e = hipMemcpy(d, tab.data(), JJ_BASE_TABLE_BYTES, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    (void)hipFree(d);
    return set_err(ctx, PM_ERR_HIP, std::string("hipMemcpy: ") + hipGetErrorString(e));
  }
  pm_jubjub_base* b = new pm_jubjub_base();
  b->device = ctx->device, b->d_tab = d;
  memcpy(b->xy, xy, 64);
  *out = b;
  return PM_OK;
}

}  // namespace

// context.h: the table gathered for a FIXED_BASE gadget (GadgetTables::tab at its offset: R points x | y, canonical) -> a handle
// for its base t[R - 1], when t[k] = 2 t[k + 1] throughout.  Waits for the context's stream.
int jubjub_base_from_table(pm_ctx* ctx, const void* d_points, uint32_t R, pm_jubjub_base** out) {
  std::vector<uint64_t> t(8 * (size_t)R);
  {
    std::lock_guard<std::mutex> lk(ctx->mu);
    PM_HIP(ctx, hipSetDevice(ctx->device));
    PM_HIP(ctx, hipStreamSynchronize(ctx->stream));
    PM_HIP(ctx, hipMemcpy(t.data(), d_points, t.size() * 8, hipMemcpyDeviceToHost));
  }
  for (size_t k = 0; k < R; ++k)
    if (point_fault(&t[8 * k]))
      return set_err(ctx, PM_ERR_BAD_ARG, "pm_jubjub_base_from_key: table point " + std::to_string(k) + " is not a canonical curve point");
  for (size_t k = 0; k + 1 < R; ++k) {
    const HPoint next = hpoint_load(&t[8 * (k + 1)]), twice = hpoint_add(next, next), here = hpoint_load(&t[8 * k]);
    if (!host::eq(twice.x, here.x) || !host::eq(twice.y, here.y))
      return set_err(ctx, PM_ERR_BAD_ARG, "pm_jubjub_base_from_key: the gadget's table is not a doubling chain at round " + std::to_string(k));
  }
  return base_build(ctx, &t[8 * ((size_t)R - 1)], out);
}

}  // namespace pm

using namespace pm;

extern "C" int pm_jubjub_base_create(pm_ctx* ctx, const uint64_t xy[8], pm_jubjub_base** out) {
  if (!ctx || !out) return PM_ERR_BAD_ARG;
  if (!xy) return set_err(ctx, PM_ERR_BAD_ARG, "null point");
  if (point_fault(xy)) return set_err(ctx, PM_ERR_BAD_ARG, "pm_jubjub_base_create: the point is not a canonical point of the curve");
  return base_build(ctx, xy, out);
}

extern "C" int pm_jubjub_base_point(const pm_jubjub_base* base, uint64_t xy[8]) {
  if (!base || !xy) return PM_ERR_BAD_ARG;
  memcpy(xy, base->xy, 64);
  return PM_OK;
}

extern "C" void pm_jubjub_base_free(pm_ctx* ctx, pm_jubjub_base* base) {
  if (!base) return;
  if (ctx) {
    std::lock_guard<std::mutex> lk(ctx->mu);
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    if (base->d_tab) (void)hipFree(base->d_tab);   // hipFree waits for the device: launches on caller streams included
  }
  delete base;
}

extern "C" int pm_jubjub_fixed_mul_dev(pm_ctx* ctx, const pm_jubjub_base* base, const void* d_scalars, size_t n, uint32_t scalar_form,
                                       void* d_out_xy, void* hip_stream) {
  if (!ctx) return PM_ERR_BAD_ARG;
  if (int rc = base_fault(ctx, base)) return rc;
  if (int rc = form_fault(ctx, scalar_form)) return rc;
  if (int rc = pointer_fault(ctx, {d_scalars, d_out_xy})) return rc;
  if (n == 0) return PM_OK;
  if (int rc = count_fault(ctx, n)) return rc;
  PM_ENTER(ctx, hip_stream, st);
  JubjubMul a{};
  a.tab_g = (const u32x4*)base->d_tab, a.scalars = (const u32x4*)d_scalars, a.out = (u32x4*)d_out_xy, a.n = n;
  a.montgomery = scalar_form == PM_SCALAR_MONTGOMERY;
  jubjub_d_limbs(a.edwards_d);
  ProfScope prof(ctx, st, "jubjub_fixed_mul");
  hipLaunchKernelGGL((jubjub_fixed_kernel<false>), dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, a);
  PM_HIP(ctx, hipGetLastError());
  return PM_OK;
}

extern "C" int pm_jubjub_commit_dev(pm_ctx* ctx, const pm_jubjub_base* g, const pm_jubjub_base* h, const void* d_values,
                                    const void* d_blinders, size_t n, uint32_t scalar_form, void* d_out_xy, void* hip_stream) {
  if (!ctx) return PM_ERR_BAD_ARG;
  if (int rc = base_fault(ctx, g)) return rc;
  if (int rc = base_fault(ctx, h)) return rc;
  if (int rc = form_fault(ctx, scalar_form)) return rc;
  if (int rc = pointer_fault(ctx, {d_values, d_blinders, d_out_xy})) return rc;
  if (n == 0) return PM_OK;
  if (int rc = count_fault(ctx, n)) return rc;
  PM_ENTER(ctx, hip_stream, st);
  JubjubMul a{};
  a.tab_g = (const u32x4*)g->d_tab, a.tab_h = (const u32x4*)h->d_tab, a.scalars = (const u32x4*)d_values;
  a.scalars_h = (const u32x4*)d_blinders, a.out = (u32x4*)d_out_xy, a.n = n, a.montgomery = scalar_form == PM_SCALAR_MONTGOMERY;
  jubjub_d_limbs(a.edwards_d);
  ProfScope prof(ctx, st, "jubjub_commit");
  hipLaunchKernelGGL((jubjub_fixed_kernel<true>), dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, a);
  PM_HIP(ctx, hipGetLastError());
  return PM_OK;
}

extern "C" int pm_jubjub_mul_dev(pm_ctx* ctx, const void* d_points_xy, const void* d_scalars, size_t n, uint32_t scalar_form,
                                 void* d_out_xy, void* hip_stream) {
  if (!ctx) return PM_ERR_BAD_ARG;
  if (int rc = form_fault(ctx, scalar_form)) return rc;
  if (int rc = pointer_fault(ctx, {d_points_xy, d_scalars, d_out_xy})) return rc;
  if (n == 0) return PM_OK;
  if (int rc = count_fault(ctx, n)) return rc;
  PM_ENTER(ctx, hip_stream, st);
  SlotScratch scratch(ctx, n);                               // the window tables of the threads in flight, 1152 bytes a thread
  PM_HIP(ctx, scratch.alloc(JJ_MUL_TABLE_BYTES, 0));
  JubjubMul a{};
  a.points = (const u32x4*)d_points_xy, a.scalars = (const u32x4*)d_scalars, a.out = (u32x4*)d_out_xy, a.scratch = scratch.slots();
  a.n = n, a.montgomery = scalar_form == PM_SCALAR_MONTGOMERY;
  jubjub_d_limbs(a.edwards_d);
  hipError_t e;
  {
    ProfScope prof(ctx, st, "jubjub_mul");
    hipLaunchKernelGGL(jubjub_var_kernel, dim3((unsigned)scratch.blocks), dim3(64), 0, st, a);
    e = hipGetLastError();
  }
  return finish_call(ctx, e, st, nullptr, nullptr, 0, scratch.base, "pm_jubjub_mul_dev");
}

extern "C" int pm_jubjub_check_dev(pm_ctx* ctx, const void* d_points_xy, size_t n, size_t* first_bad, void* hip_stream) {
  if (!ctx) return PM_ERR_BAD_ARG;
  if (!first_bad) return set_err(ctx, PM_ERR_BAD_ARG, "null first_bad");
  *first_bad = n;
  if (n == 0) return PM_OK;
  if (int rc = pointer_fault(ctx, {d_points_xy})) return rc;
  if (int rc = count_fault(ctx, n)) return rc;
  PM_ENTER(ctx, hip_stream, st);
  unsigned long long* d_bad = nullptr;
  unsigned long long bad = n;
  PM_HIP(ctx, hipMalloc((void**)&d_bad, 8));
  JubjubMul a{};
  jubjub_d_limbs(a.edwards_d);
  hipError_t e = hipMemcpyAsync(d_bad, &bad, 8, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(jubjub_check_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, (const u32x4*)d_points_xy, n, a, d_bad);
    e = hipGetLastError();
  }
  if (int rc = finish_call(ctx, e, st, &bad, d_bad, 8, d_bad, "pm_jubjub_check_dev")) return rc;
  *first_bad = (size_t)bad;
  return PM_OK;
}

extern "C" int pm_jubjub_mul_host(const uint64_t xy[8], const uint64_t scalar[4], uint32_t scalar_form, uint64_t out_xy[8]) {
  if (!xy || !scalar || !out_xy) return PM_ERR_BAD_ARG;
  if (scalar_form != PM_SCALAR_MONTGOMERY && scalar_form != PM_SCALAR_CANONICAL) return PM_ERR_BAD_ARG;
  uint64_t k[4];
  if (point_fault(xy) || !scalar_to_int(scalar, scalar_form, k)) return PM_ERR_BAD_ARG;
  hpoint_store(out_xy, hpoint_mul(hpoint_load(xy), k));
  return PM_OK;
}

extern "C" int pm_jubjub_add_host(const uint64_t p[8], const uint64_t q[8], uint64_t out_xy[8]) {
  if (!p || !q || !out_xy) return PM_ERR_BAD_ARG;
  if (point_fault(p) || point_fault(q)) return PM_ERR_BAD_ARG;
  hpoint_store(out_xy, hpoint_add(hpoint_load(p), hpoint_load(q)));
  return PM_OK;
}
