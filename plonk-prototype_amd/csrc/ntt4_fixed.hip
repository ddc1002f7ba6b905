// Fixed-shape variants of the radix-4 pass kernels (ntt_pass4_fixed_kernel, ntt_kernels4.hip.h) and the predicate that
// decides which launches take them.  A translation unit of its own: the two kernels compile beside ntt4.hip, not behind it.
#include <hip/hip_runtime.h>

#include "context.h"
#include "ntt_kernels4.hip.h"

namespace pm {

typedef void (*pass_fn)(const NttPassArgs, const NttConsts);
struct Pass4FixedEntry {
  int FIX, S, LT, role;  // FIX: the log_n the variant is built for; role: 1 first, 3 last
  bool by_default;       // taken with ntt_fixed_shape = 1; the others wait for 2
  pass_fn fn;
};
// The [10, 10] plan of a plain 2^20 transform, forward or inverse (the direction is in the tables).  The first pass is 4.3 - 4.8 us
// a launch faster than the generic kernel with two lazy rows and another 1.2 us with three.  The last pass is 0.25 - 0.44 us
// faster in each of three pairs of runs, which is what its 106 VALU instructions a wave fewer predict and less than the
// 0.56 us the generic kernel differs by from run to run: by the project's rule it stays off unless asked for
// (ntt_fixed_shape = 2; DESIGN.md section 3, profiles/fixed_shape_kernel_trace.txt).
static const Pass4FixedEntry kPass4FixedTable[] = {
    {20, 10, 1, 1, true, ntt_pass4_fixed_kernel<10, 1, true, false, true, 20>},
    {20, 10, 1, 3, false, ntt_pass4_fixed_kernel<10, 1, false, true, false, 20>},
};

// The fixed variant for this launch, or null: the launch must be the variant's exactly (pass4_fixed_match): its size, its
// place in the plan, the blocking of the wide vectors, all of the variant's flags and no other, in a plain transform (no
// coset) of a whole input.  Batches and their strides are free, they only move the uniform base.  mode is the option
// ntt_fixed_shape: 0 none, 1 the variants that are on by default, 2 all of them.  *lazy_form (may be null) receives the G of
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
