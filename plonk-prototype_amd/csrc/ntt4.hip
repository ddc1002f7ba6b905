// Instantiations of the radix-4 pass kernels (own translation unit so that it compiles in
// parallel with ntt.hip) and their lookup / table builder for ntt.hip.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "ntt_internal.h"
#include "ntt_kernels4.hip.h"

namespace pm {

struct Pass4Entry {
  int S, LT, role;  // role: 0 single, 1 first, 2 middle, 3 last
  pass_fn fn;
};
// single-pass shapes (LT = 0) and the multi-pass tiles of 2^11 elements (2^12 for S = 10)
#define PM4_SINGLE(X) X(2, 0) X(3, 0) X(4, 0) X(5, 0) X(6, 0) X(7, 0) X(8, 0) X(9, 0) X(10, 0)
#define PM4_MULTI(X) X(5, 6) X(6, 5) X(7, 4) X(8, 3) X(9, 2) X(10, 1) X(10, 2) X(5, 5) X(6, 4) X(7, 3) X(8, 2) X(10, 0) X(9, 1)
static const Pass4Entry kPass4Table[] = {
#define X(S, LT) {S, LT, 0, ntt_pass4_kernel<S, LT, false, false, false>},
    PM4_SINGLE(X)
#undef X
#define X(S, LT)                                               \
  {S, LT, 1, ntt_pass4_kernel<S, LT, true, false, true>},      \
      {S, LT, 2, ntt_pass4_kernel<S, LT, false, true, true>},  \
      {S, LT, 3, ntt_pass4_kernel<S, LT, false, true, false>},
        PM4_MULTI(X)
#undef X
};

pass_fn find_pass4(int S, int LT, int role) {
  for (const Pass4Entry& e : kPass4Table)
    if (e.S == S && e.LT == LT && e.role == role) return e.fn;
  return nullptr;
}
// does the first (role 1) or middle (role 2) pass of this shape apply the next pass's twiddles when asked (PASS_TW_OUT)
bool pass4_tw_producer(int S, int LT, int role) {
  return (role == 1 || role == 2) && find_pass4(S, LT, role) != nullptr && step4_tw_producer(S, LT, role == 1, role == 2);
}
// does this shape's kernel take wave priorities by step (PASS_STEP_PRIO)
bool pass4_step_prio(int S, int LT, int role) { return find_pass4(S, LT, role) != nullptr && step4_has_prio(S); }
// G of the lazy step table this shape's kernel reads through step_tw_lazy, 0: none
int pass4_lazy_form(int S, int LT, int role) {
  return find_pass4(S, LT, role) != nullptr ? step4_lazy_form(S, LT, role == 2 || role == 3) : 0;
}
size_t pass4_lds(int S, int LT) { return pass4_lds_bytes(S, LT); }

#ifdef PM_DEV_STAMPS
// Diagnostic build: the stamp buffer of the radix-4 pass launched next on st (see ntt_stamp in ntt_kernels4.hip.h), room for
// `waves` waves; null switches the stamps off.  pm_dev_ntt_stamps() hands ntt_run() a buffer that it deals out pass by pass.
static unsigned long long* g_host_stamps = nullptr;
static size_t g_host_stamp_waves = 0;
int ntt_stamps_arm(pm_ctx* ctx, hipStream_t st, int pass, size_t waves) {
  unsigned long long* p = nullptr;
  unsigned long long room = 0;
  if (g_host_stamps && (size_t)(pass + 1) * waves <= g_host_stamp_waves) {
    p = g_host_stamps + (size_t)pass * waves * NTT_STAMP_WORDS;
    room = waves;
  }
  PM_HIP(ctx, hipMemcpyToSymbolAsync(HIP_SYMBOL(g_ntt_stamps), &p, sizeof p, 0, hipMemcpyHostToDevice, st));
  PM_HIP(ctx, hipMemcpyToSymbolAsync(HIP_SYMBOL(g_ntt_stamp_waves), &room, sizeof room, 0, hipMemcpyHostToDevice, st));
  return PM_OK;
}
#endif
unsigned pass4_threads(int S, int LT) { return std::max(64u, (1u << (S + LT)) / 4); }

// the head (w4 and the powers of w16, nine rows each) in front, then 80 B per entry
size_t step4_table_bytes(unsigned S) {
  return ((size_t)STEP4_HEAD + (size_t)step4_tw_total((int)S) * STEP4_ENTRY) * sizeof(u32x4);
}

int build_step4_table(pm_ctx* ctx, void** out, const NttConsts& c, unsigned S, hipStream_t st) {
  const u32 total = (u32)step4_tw_total((int)S);
  // at least the threads of the head, so that it is written for every S
  PM_HIP(ctx, hipMalloc(out, step4_table_bytes(S)));
  hipLaunchKernelGGL(step4_tw_kernel, dim3((std::max(total, 9u * STEP4_HEAD_CONSTS) + 255) / 256), dim3(256), 0, st,
                     (u32x4*)*out, c, S);
  PM_HIP(ctx, hipGetLastError());
  return PM_OK;
}

// the w4 head in front, then the entries of the radix-4 steps from the third on in form G
size_t step4_lazy_table_bytes(unsigned S, unsigned G) {
  return ((size_t)STEP4_LAZY_HEAD + (size_t)step4_lazy_total((int)S) * step4_lazy_entry((int)G)) * sizeof(u32x4);
}

int build_step4_lazy_table(pm_ctx* ctx, void** out, const NttConsts& c, unsigned S, unsigned G, hipStream_t st) {
  const u32 total = (u32)step4_lazy_total((int)S);
  PM_HIP(ctx, hipMalloc(out, step4_lazy_table_bytes(S, G)));
  hipLaunchKernelGGL(step4_lazy_tw_kernel, dim3((std::max(total, 9u) + 255) / 256), dim3(256), 0, st, (u32x4*)*out, c, S, G);
  PM_HIP(ctx, hipGetLastError());
  return PM_OK;
}

}  // namespace pm

#ifdef PM_DEV_STAMPS
// d_buf: room for `waves` x 40 words of 8 bytes (all passes of the transforms that follow, 320 B per wave); null: off
extern "C" int pm_dev_ntt_stamps(void* d_buf, size_t waves) {
  pm::g_host_stamps = (unsigned long long*)d_buf;
  pm::g_host_stamp_waves = d_buf ? waves : 0;
  return 0;
}
#endif
