// The exit of the radix-4 last passes alone, for static instruction counts (profiles/ntt_exit_isa_*.txt): each kernel
// loads nine raw limbs, runs one form of the exit and stores 32 bytes.
//   exit_store_kernel   fe_reduce_weak + fe_store: the exit before fe_reduce_canon_pack existed
//   exit_raw_kernel     fe_reduce_weak + fe_pack_raw: the floor, right only where the reduction leaves r < m
//   exit_fused_kernel   fe_reduce_canon_pack: the floor plus the vote; the compare, subtract and select in a block of its own
//
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 -mllvm -pragma-unroll-threshold=1000000 --cuda-device-only -S \
//         -I plonk-prototype_amd/csrc tools/ntt_exit_harness.hip -o ntt_exit_harness.s
//   python tools/isa_kernel_stats.py ntt_exit_harness.s exit_
#include <hip/hip_runtime.h>

#include "fields.hip.h"

using namespace pm;

PM_DEV Fr ld9(const u32* in, size_t i) {
  Fr x;
#pragma unroll
  for (int k = 0; k < 9; ++k) x.l[k] = in[9 * i + k];
  return x;
}

__global__ void exit_store_kernel(const u32* in, u32x4* out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  fe_store<FrP>(out + 2 * i, fe_reduce_weak<FrP>(ld9(in, i)));
}

__global__ void exit_raw_kernel(const u32* in, u32x4* out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  u32 s[8];
  fe_pack_raw<FrP>(s, fe_reduce_weak<FrP>(ld9(in, i)));
  out[2 * i] = u32x4{s[0], s[1], s[2], s[3]};
  out[2 * i + 1] = u32x4{s[4], s[5], s[6], s[7]};
}

__global__ void exit_fused_kernel(const u32* in, u32x4* out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  u32 s[8];
  fe_reduce_canon_pack<FrP>(s, ld9(in, i));
  fe_store_words<FrP>(out + 2 * i, s);
}
