// Shared by poly.hip and plonk_rounds.hip: the canonical (ABI) <-> device-form boundary of the
// polynomial helpers.  ABI form: x * 2^256 in 4 x u64; device form: x * 2^261 in 9 x 29-bit limbs.
// fe_mul of forms 2^a and 2^b gives 2^(a + b - 261): ABI x device -> ABI, device x device -> device.
#pragma once
#include <cstring>

#include "host_field.h"
#include "fields.hip.h"

namespace pm {

using host::HFr;

// value * 2^5 for a normalised value < 2r: turns the device product a*b/2^261 into the ABI
// product a*b/2^256.  Output limbs normalised, value < 64 r.
PM_DEV Fr fr_shl5(const Fr& t) {
  constexpr u32 MASK = Consts<FrP>::MASK;
  Fr r;
  r.l[0] = (t.l[0] << 5) & MASK;
#pragma unroll
  for (int i = 1; i < 8; ++i) r.l[i] = ((t.l[i] << 5) & MASK) | (t.l[i - 1] >> 24);
  r.l[8] = (t.l[8] << 5) | (t.l[7] >> 24);
  return r;
}
// product of two ABI-form values, ABI form, value < r + r/2^16
PM_DEV Fr fr_abi_mul(const Fr& a, const Fr& b) { return fe_reduce_weak<FrP>(fr_shl5(fe_mul<FrP>(a, b))); }

PM_DEV Fr ld_canon(const u32x4* p, size_t i) { return fe_load<FrP>(p + 2 * i); }
PM_DEV void st_canon(u32x4* p, size_t i, const Fr& v) { fe_store<FrP>(p + 2 * i, v); }

// ------------------------------------------------------------------ where a kernel's constants come from
// Every kernel of poly.hip and plonk_rounds.hip that serves both one vector (or proof) per launch and a batch of them exists
// ONCE, as a template on a small "source" type: what a launch works on and where its constants sit.
//   FromArgs<T>   one vector per launch; T travels by value in the kernel arguments
//   FromTable<T>  blockIdx.y (or an index the kernel derives from it) picks one of several; T sits in a device table in the
//                 constant address space.  The index is wave-uniform, so every access is a scalar load, as from the arguments.
// Kernels whose sources differ in more than that define their own pair beside the kernel, with the same two roles.  The body
// stays IN the __global__ template: moved into a device function that two kernels call, the large ones spill (docs/HISTORY.md).
#define PM_KCONST __attribute__((address_space(4)))
template <class T>
PM_DEV const T& kconst(const PM_KCONST T* tab, u32 i) {
  return *(const T*)(tab + i);
}
template <class T>
struct FromArgs {
  T c;
  static PM_DEV u32 slot() { return 0; }
  PM_DEV const T& at(u32) const { return c; }
};
template <class T>
struct FromTable {
  const PM_KCONST T* tab;
  static PM_DEV u32 slot() { return blockIdx.y; }
  PM_DEV const T& at(u32 i) const { return kconst(tab, i); }
};

// ------------------------------------------------------------------ host helpers
static inline bool hfr_canonical(const uint64_t* v) { return !host::geq<4>(v, host::FR().m); }
static inline HFr hfr_load(const uint64_t* v) {
  HFr r;
  memcpy(r.l, v, 32);
  return r;
}
static inline void to_limbs29(u32* dst, HFr v) {  // ABI Montgomery -> device Montgomery limbs
  for (int i = 0; i < 5; ++i) v = host::add(v, v, host::FR());
  for (int i = 0; i < 9; ++i) {
    const int lo = 29 * i, j = lo / 64, sh = lo % 64;
    u64 x = v.l[j] >> sh;
    if (sh + 29 > 64 && j + 1 < 4) x |= v.l[j + 1] << (64 - sh);
    dst[i] = (u32)(x & ((1u << 29) - 1));
  }
}
static inline HFr hfr_pow_u64(HFr b, u64 e) {
  host::u64 ee[1] = {(host::u64)e};
  return host::pow(b, ee, 1, host::FR());
}
// x * 2^(256 + 5 k) as 29-bit limbs: k = 0 keeps the ABI scaling, 1 = device form, 2 = device form
// of 32 x (so that ABI x this = device form)
static inline void to_limbs29_shift(u32* dst, HFr v, int k) {
  for (int i = 0; i < 5 * (k - 1); ++i) v = host::add(v, v, host::FR());
  if (k >= 1) {
    to_limbs29(dst, v);
    return;
  }
  for (int i = 0; i < 9; ++i) {
    const int lo = 29 * i, j = lo / 64, sh = lo % 64;
    u64 x = v.l[j] >> sh;
    if (sh + 29 > 64 && j + 1 < 4) x |= v.l[j + 1] << (64 - sh);
    dst[i] = (u32)(x & ((1u << 29) - 1));
  }
}

}  // namespace pm
