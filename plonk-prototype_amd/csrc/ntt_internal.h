// What the translation units of the Fr NTT share: the pass-kernel type, the roles of a pass, the lookups of the radix-4
// kernels (ntt4.hip) and of their fixed-shape variants (ntt4_fixed.hip), and the driver's functions (ntt.hip) that the
// domain helpers (domain.hip) and the distributed transform (ntt_fourstep.hip) call.
#pragma once
#include <hip/hip_runtime.h>

#include "context.h"
#include "host_field.h"

namespace pm {

struct NttPassArgs;   // ntt_kernels.hip.h
struct NttConsts;
typedef void (*pass_fn)(const NttPassArgs, const NttConsts);
enum Role { ROLE_SINGLE = 0, ROLE_FIRST = 1, ROLE_MIDDLE = 2, ROLE_LAST = 3 };

// radix-4 kernels (ntt4.hip)
pass_fn find_pass4(int S, int LT, int role);
size_t pass4_lds(int S, int LT);
unsigned pass4_threads(int S, int LT);
bool pass4_tw_producer(int S, int LT, int role);
bool pass4_step_prio(int S, int LT, int role);
int pass4_lazy_form(int S, int LT, int role);
int build_step4_table(pm_ctx* ctx, void** out, const NttConsts& c, unsigned S, hipStream_t st);
size_t step4_table_bytes(unsigned S);
int build_step4_lazy_table(pm_ctx* ctx, void** out, const NttConsts& c, unsigned S, unsigned G, hipStream_t st);
size_t step4_lazy_table_bytes(unsigned S, unsigned G);
#ifdef PM_DEV_STAMPS
int ntt_stamps_arm(pm_ctx* ctx, hipStream_t st, int pass, size_t waves);
#endif
// fixed-shape variants (ntt4_fixed.hip): the kernel for a launch that equals one exactly, else null
pass_fn find_pass4_fixed(int S, int LT, int role, unsigned log_n, unsigned log_ns, unsigned wide_glog, unsigned flags,
                         unsigned long long in_len, bool coset, long mode, int* lazy_form);

// the driver (ntt.hip): the generator of the 2^log_n domain, and the two-level power tables of a size and direction
// (dir 1: inverse), built on first use, with the coset's when asked
host::HFr domain_gen(unsigned log_n);
int get_domain_tables(pm_ctx* ctx, int dir, unsigned log_n, bool need_coset, NttDomainTables** out, hipStream_t st);

}  // namespace pm
