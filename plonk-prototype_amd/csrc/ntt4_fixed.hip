// Fixed-shape variants of the radix-4 pass kernels (ntt_pass4_fixed_kernel, ntt_kernels4.hip.h) and the predicate that
// decides which launches take them.  A translation unit of its own: the two kernels compile beside ntt4.hip, not behind it.
#include <hip/hip_runtime.h>

#include "ntt_internal.h"
#include "ntt_kernels4.hip.h"

namespace pm {

struct Pass4FixedEntry {
  int FIX, S, LT, role;  // FIX: the log_n the variant is built for; role: 1 first, 3 last
  bool by_default;       // taken with ntt_fixed_shape = 1; the others wait for 2, which is the option's default
  pass_fn fn;
};
// The [10, 10] plan of a plain 2^20 transform, forward or inverse (the direction is in the tables).  The first pass is 4.3 - 4.8 us
// a launch faster than the generic kernel with two lazy rows and another 1.2 us with three.  The last pass was 0.25 - 0.44 us
// faster with the generic kernel's order of loads, less than the generic kernel differs by from run to run, and waited for
// ntt_fixed_shape = 2 (profiles/fixed_shape_kernel_trace.txt).  With its step twiddles kept in flight (PM_NTT_FIXED_TW_PREFETCH,
// ntt_kernels4.hip.h) it is 1.3 - 1.5 us a launch faster than the generic one, and 2 is the option's default
// (PM_NTT_FIXED_SHAPE_DEFAULT; DESIGN.md section 3, profiles/twiddle_prefetch_kernel_trace.txt).  The column by_default keeps
// what ntt_fixed_shape = 1 means: the first pass only.
static const Pass4FixedEntry kPass4FixedTable[] = {
    {20, 10, 1, 1, true, ntt_pass4_fixed_kernel<10, 1, true, false, true, 20>},
    {20, 10, 1, 3, false, ntt_pass4_fixed_kernel<10, 1, false, true, false, 20>},
};

// The fixed variant for this launch, or null: the launch must be the variant's exactly (pass4_fixed_match): its size, its
// place in the plan, the blocking of the wide vectors, all of the variant's flags and no other, in a plain transform (no
// coset) of a whole input.  Batches and their strides are free, they only move the uniform base.  mode is the option
// ntt_fixed_shape: 0 none, 1 the variants with by_default, 2 all of them.  *lazy_form (may be null) receives the G of
// the lazy step table the variant reads through step_tw_lazy.  Host arithmetic, no device call.
pass_fn find_pass4_fixed(int S, int LT, int role, unsigned log_n, unsigned log_ns, unsigned wide_glog, unsigned flags,
                         unsigned long long in_len, bool coset, long mode, int* lazy_form) {
  for (const Pass4FixedEntry& e : kPass4FixedTable)
    if (e.S == S && e.LT == LT && e.role == role && (mode == 2 || (mode == 1 && e.by_default)) &&
        pass4_fixed_match(e.FIX, S, LT, role == 3, log_n, log_ns, wide_glog, flags, in_len, coset)) {
      if (lazy_form) *lazy_form = step4_fixed_lazy_form(S, LT, role == 3, e.FIX);
      return e.fn;
    }
  return nullptr;
}

}  // namespace pm
