// Host side of the Fr NTT: the driver -- resolve a transform's passes (ntt_resolve), acquire the tables they name
// (ntt_acquire), launch (ntt_run) -- and the pm_fr_ntt*, pm_domain_prepare, pm_ntt_plan and NTT test-hook entry points.
// Mirrors dusk_plonk::fft::EvaluationDomain (dusk-plonk 0.8.2, ref:Cargo.toml:19):
//   new()      -> domain_gen()  (group_gen = ROOT_OF_UNITY^(2^(32-log_n)); pm_domain_info and the helpers: domain.hip)
//   fft/ifft/coset_fft/coset_ifft -> ntt_run() with PM_NTT_INVERSE / PM_NTT_COSET
// The transform split over ranks is ntt_fourstep.hip.
#include <hip/hip_runtime.h>

#include <condition_variable>
#include <thread>

#include <algorithm>
#include <cstring>

#include "ntt_internal.h"
#include "ntt_kernels.hip.h"

namespace pm {

using host::HFr;

// ------------------------------------------------------------------ kernel table
struct PassEntry {
  int S, LT, role;
  pass_fn fn;
};
// (S, LT): LT = 0 single-pass kernels; multi-pass tiles of 2^11 (LT = 11 - S) or 2^12 elements
#define PM_SINGLE(X) X(3, 0) X(4, 0) X(5, 0) X(6, 0) X(7, 0) X(8, 0) X(9, 0) X(10, 0)
#define PM_MULTI(X) \
  X(5, 6) X(6, 5) X(7, 4) X(8, 3) X(9, 2) X(10, 1) X(8, 4) X(9, 3) X(10, 2) X(5, 5) X(6, 4) X(7, 3) X(8, 2)
static const PassEntry kPassTable[] = {
#define X(S, LT) {S, LT, ROLE_SINGLE, ntt_pass_kernel<S, LT, false, false, false>},
    PM_SINGLE(X)
#undef X
#define X(S, LT)                                                      \
  {S, LT, ROLE_FIRST, ntt_pass_kernel<S, LT, true, false, true>},     \
      {S, LT, ROLE_MIDDLE, ntt_pass_kernel<S, LT, false, true, true>}, \
      {S, LT, ROLE_LAST, ntt_pass_kernel<S, LT, false, true, false>},
        PM_MULTI(X)
#undef X
};
static pass_fn find_pass(int S, int LT, int role) {
  for (const PassEntry& e : kPassTable)
    if (e.S == S && e.LT == LT && e.role == role) return e.fn;
  return nullptr;
}

struct Plan {
  int npass = 0;
  int S[4] = {0, 0, 0, 0};
  int LT[4] = {0, 0, 0, 0};
};
static Plan make_plan(unsigned log_n, int tile_log, int max_radix = 10, int radix = 4, unsigned min_tiles = 256,
                      unsigned batch = 1) {
  Plan p;
  if (log_n < 3) return p;  // tiny kernel
  if (log_n <= 10) {  // one workgroup per transform; beyond 2^10 two passes over many CUs are faster
    p.npass = 1;     // (measured: a single 2^12 workgroup 52 us, two passes 35 us)
    p.S[0] = (int)log_n;
    return p;
  }
  p.npass = (int)((log_n + max_radix - 1) / max_radix);
  p.npass = std::min(p.npass, (int)log_n / 5);  // multi-pass kernels exist for radix >= 2^5
  p.npass = std::min(p.npass, 4);               // ... and a plan holds four passes (ntt_max_radix 6 or 7 above 2^24 / 2^28)
  int base = (int)log_n / p.npass, extra = (int)log_n % p.npass;
  for (int i = 0; i < p.npass; ++i) {
    p.S[i] = base + (i < extra ? 1 : 0);
    // tile_log 0 = auto (measured, profiles/r01_ntt_sweep.txt): 2^10-element tiles for S <= 8 (four
    // or more independent workgroups per CU, so barrier phases of one overlap arithmetic of
    // another), never fewer than 4 adjacent columns (64-byte runs per limb group)
    // r05: a radix-2^10 pass takes TWO columns per workgroup (512 threads, 73 KB of LDS: two workgroups per CU whose load / barrier /
    // store phases overlap) -- with the r05 product (95 - 106 VGPRs) that is 204 -> 195 us per forward + inverse 2^20 transform and
    // 206 -> 191 us in a batch of four (profiles/r05_ntt_tile_ab.txt; r02 measured no difference with the 128-VGPR kernels)
    int lt = tile_log ? tile_log - p.S[i] : (p.S[i] >= 10 && radix == 4 ? 1 : std::max(10 - p.S[i], 2));
    if (p.S[i] < 8 && lt > 11 - p.S[i]) lt = 11 - p.S[i];  // 2^12-element tiles exist for S >= 8 only
    if (!tile_log && radix == 4) {
      // fill the chip: narrower tiles while there are fewer tiles than CUs (measured, profiles/r02_ntt_tile_ab.txt:
      // 2^18: 61 -> 51 us, 2^19: 89 -> 72 us; no change from 2^20 up, where 4-column tiles already give 256)
      while (lt > (p.S[i] >= 10 ? 0 : 1) && ((((size_t)batch << log_n) >> (p.S[i] + lt)) < min_tiles) &&
             find_pass4(p.S[i], lt - 1, ROLE_LAST) != nullptr)
        --lt;
    }
    if (lt < 0) lt = 0;
    if (radix != 4 && lt < 1) lt = 1;                        // single-column tiles exist in the radix-4 family only
    if (radix != 4 && tile_log == 10 && p.S[i] > 8) lt = 11 - p.S[i];
    lt = std::min(lt, (int)log_n - p.S[i]);
    p.LT[i] = lt;
  }
  return p;
}
// log2 of the block size of the wide (intermediate) layout: part of the key of the inter-pass tables
static unsigned plan_wide_glog(const Plan& plan) {
  int min_lt = 3;
  for (int i = 0; i < plan.npass; ++i) min_lt = std::min(min_lt, plan.LT[i]);
  return (unsigned)std::max(min_lt, 2);
}

// ------------------------------------------------------------------ resolution
// Everything a transform decides, before anything is allocated or launched: host arithmetic, no HIP call, no context.
// ntt_run() and pm_domain_prepare() acquire the tables the result names (ntt_acquire) and ntt_run() launches from it;
// pm_test_ntt_plan / pm_test_ntt_launches show it to the CPU tests.
struct NttOpts {   // the options "ntt_*" a plan depends on
  long tile_log, max_radix, radix, xcd, direct_tw, tw_producer, step_prio, fixed_shape;
};
static const NttOpts kDefaultOpts = {0, 10, 4, 1, 1, 1, PM_NTT_STEP_PRIO_DEFAULT, PM_NTT_FIXED_SHAPE_DEFAULT};   // a fresh context's (context.h)
// the fixed-shape variant a launch takes under ntt_fixed_shape = mode, or null: the launch of a radix-4 kernel that equals
// the variant's in every respect (find_pass4_fixed); *lazy_form (may be null) receives the G of the lazy table it reads
static pass_fn fixed_variant(int S, int LT, int role, unsigned log_n, unsigned log_ns, unsigned wide_glog, unsigned flags,
                             unsigned long long in_len, bool coset, long mode, int* lazy_form) {
  if (!mode || find_pass4(S, LT, role) == nullptr) return nullptr;
  return find_pass4_fixed(S, LT, role, log_n, log_ns, wide_glog, flags, in_len, coset, mode, lazy_form);
}
struct PassLaunch {
  int S, LT, role;
  bool r4;                  // a kernel of the radix-4 family (else radix-8)
  pass_fn fn;               // null: no kernel for this shape
  int variant;              // 1 the generic kernel, 2 its fixed-shape variant
  unsigned threads, blocks;
  size_t lds;
  u32 flags;                // the complete PASS_* word
  unsigned log_ns;          // stages done before this pass
  int lazy;                 // form G of the lazy step table the chosen kernel reads, 0: none
  int tw_in, tw_out;        // the pass whose inter-pass table this one reads (pass_tw) / applies to its outputs (pass_tw_out); -1: none
};
struct NttLaunches {
  int npass;                // 0: the tiny kernel, or nothing at all (log_n = 0)
  bool tiny;
  u32 tiny_flags;
  bool scale_folded;        // n^-1 of an inverse transform is in the last pass's inter-pass table
  unsigned wide_glog;
  PassLaunch pass[4];
};
static NttLaunches ntt_resolve(const NttOpts& o, unsigned num_cus, unsigned log_n, unsigned batch, unsigned flags,
                               unsigned long long in_len) {
  NttLaunches L;
  memset(&L, 0, sizeof L);
  const bool inverse = (flags & PM_NTT_INVERSE) != 0, coset = (flags & PM_NTT_COSET) != 0;
  const bool direct_tw = log_n <= 26 && o.direct_tw;  // tables of N x 36 B per twiddled pass and direction
  const Plan plan = make_plan(log_n, (int)o.tile_log, (int)o.max_radix, (int)o.radix, num_cus, batch);
  L.npass = plan.npass;
  // n^-1 of an inverse transform: folded into the last pass's twiddle table when there are two
  // or more passes with direct tables; otherwise multiplied explicitly (PASS_POST_SCALE)
  L.scale_folded = inverse && plan.npass > 1 && direct_tw;
  const u32 pre = (coset && !inverse) ? PASS_PRE_COSET : 0u;
  const u32 post = ((inverse && !L.scale_folded) ? PASS_POST_SCALE : 0u) | ((inverse && coset) ? PASS_POST_COSET : 0u);
  if (plan.npass == 0) {
    L.tiny = log_n > 0;   // a size-1 domain is the identity
    L.tiny_flags = pre | post;
    return L;
  }
  L.wide_glog = plan_wide_glog(plan);
  auto role_of = [&](int i) {
    return plan.npass == 1 ? ROLE_SINGLE : (i == 0 ? ROLE_FIRST : (i == plan.npass - 1 ? ROLE_LAST : ROLE_MIDDLE));
  };
  unsigned log_ns = 0;
  for (int i = 0; i < plan.npass; ++i) {
    PassLaunch& p = L.pass[i];
    const bool last = (i == plan.npass - 1);
    const int S = p.S = plan.S[i], LT = p.LT = plan.LT[i], role = p.role = role_of(i);
    pass_fn fn4 = o.radix == 4 ? find_pass4(S, LT, role) : nullptr;
    p.r4 = fn4 != nullptr;
    p.fn = p.r4 ? fn4 : find_pass(S, LT, role);
    p.variant = 1;
    p.lazy = p.r4 ? pass4_lazy_form(S, LT, role) : 0;   // this shape's step products read the lazy table
    p.threads = p.r4 ? pass4_threads(S, LT) : std::max(64u, (1u << (S + LT)) / 8);
    p.lds = p.r4 ? pass4_lds(S, LT) : pass_lds_bytes(S, LT);
    p.blocks = (unsigned)(((size_t)1 << log_n) >> (S + LT));
    p.log_ns = log_ns;
    p.tw_in = p.tw_out = -1;
    u32 tw_flag = 0;
    if (i > 0 && L.pass[i - 1].tw_out == i) {   // the pass before this one multiplied by this pass's table
      tw_flag = PASS_TW_APPLIED;
    } else if (i > 0 && direct_tw) {
      p.tw_in = i;
      tw_flag = PASS_DIRECT_TW;
    }
    // this pass applies the next one's table to its outputs where both are radix-4 kernels and its shape takes the product
    if (!last && direct_tw && o.tw_producer && p.r4 && pass4_tw_producer(S, LT, role) &&
        find_pass4(plan.S[i + 1], plan.LT[i + 1], role_of(i + 1)) != nullptr) {
      p.tw_out = i + 1;
      tw_flag |= PASS_TW_OUT;
    }
    p.flags = (i == 0 ? pre : 0u) | (last ? post : 0u) | tw_flag | (o.xcd ? PASS_XCD_REMAP : 0u);
    if (p.r4 && o.step_prio && pass4_step_prio(S, LT, role)) p.flags |= PASS_STEP_PRIO;   // wave priorities by step
    // a launch that is a fixed-shape variant's in every respect takes it: same arguments, grid and LDS, fewer instructions,
    // and the form of the lazy table that the variant reads
    if (p.r4) {
      int flazy = 0;
      if (pass_fn ffn = fixed_variant(S, LT, role, log_n, log_ns, L.wide_glog, p.flags, in_len, coset, o.fixed_shape, &flazy)) {
        p.fn = ffn;
        p.variant = 2;
        p.lazy = flazy;
      }
    }
    log_ns += (unsigned)S;
  }
  return L;
}

// ------------------------------------------------------------------ host constants
static HFr fr_pow2k(HFr x, unsigned k) {  // x^(2^k)
  for (unsigned i = 0; i < k; ++i) x = host::mul(x, x, host::FR());
  return x;
}
HFr domain_gen(unsigned log_n) { return fr_pow2k(host::fr_root_of_unity(), 32 - log_n); }
// ABI Montgomery form (x * 2^256) -> device form (x * 2^261) as 9 x 29-bit limbs
static void to_limbs(u32* dst, HFr v) {
  for (int i = 0; i < 5; ++i) v = host::add(v, v, host::FR());
  for (int i = 0; i < 9; ++i) {
    const int lo = 29 * i, j = lo / 64, sh = lo % 64;
    u64 x = v.l[j] >> sh;
    if (sh + 29 > 64 && j + 1 < 4) x |= v.l[j + 1] << (64 - sh);
    dst[i] = (u32)(x & ((1u << 29) - 1));
  }
}

static int build_pow_table(pm_ctx* ctx, void** out, const HFr& base, const HFr& mult, u32 count,
                           u32 stride, hipStream_t st) {
  PM_HIP(ctx, hipMalloc(out, (size_t)count * 48));
  NttConsts c;
  memset(&c, 0, sizeof c);
  to_limbs(c.w8[0], base);
  to_limbs(c.scale, mult);
  to_limbs(c.one, host::one(host::FR()));
  hipLaunchKernelGGL(pow_table_kernel, dim3((count + 255) / 256), dim3(256), 0, st, (u32x4*)*out, c,
                     count, stride);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    (void)hipFree(*out);
    *out = nullptr;
    return set_err(ctx, PM_ERR_HIP, std::string("pow_table_kernel: ") + hipGetErrorString(e));
  }
  return PM_OK;
}

// One cached device table: the entry of `map` under `key`, built by `build` on first use and published only when it was built.
template <class Build>
static int cached_table(std::map<unsigned, void*>& map, unsigned key, void** out, Build build) {
  auto it = map.find(key);
  if (it == map.end()) {
    void* d = nullptr;
    if (int rc = build(&d)) return rc;
    it = map.emplace(key, d).first;
  }
  *out = it->second;
  return PM_OK;
}

// The in-tile step table of radix 2^S and one direction, built once per context.  kind: STEP_R8 the radix-8 family's table,
// STEP_R4 the radix-4 family's (it starts with the split rows of this direction's w4 and of the powers of its w16), G > 0 the
// radix-4 family's lazy split table in form G (ntt_kernels4.hip.h).
enum { STEP_R8 = -1, STEP_R4 = 0 };
static int get_step_table(pm_ctx* ctx, int dir, unsigned S, int kind, void** out, hipStream_t st) {
  std::map<unsigned, void*>& map = kind == STEP_R8 ? ctx->step_tw[dir] : kind == STEP_R4 ? ctx->step4_tw[dir] : ctx->step4_lazy_tw[dir];
  return cached_table(map, kind > 0 ? (S << 8 | (unsigned)kind) : S, out, [&](void** d) -> int {
    auto root = [&](unsigned lg) { return dir ? host::inv(domain_gen(lg), host::FR()) : domain_gen(lg); };
    NttConsts c;
    memset(&c, 0, sizeof c);
    to_limbs(c.w8[0], root(S));
    if (kind != STEP_R8) to_limbs(c.w8[1], root(2));
    if (kind == STEP_R4) to_limbs(c.w8[2], root(4));
    to_limbs(c.one, host::one(host::FR()));
    if (kind > 0) return build_step4_lazy_table(ctx, d, c, S, (unsigned)kind, st);
    if (kind == STEP_R4) return build_step4_table(ctx, d, c, S, st);
    const u32 total = (u32)step_tw_total((int)S);
    PM_HIP(ctx, hipMalloc(d, (size_t)total * 48));
    hipLaunchKernelGGL(step_tw_kernel, dim3((total + 255) / 256), dim3(256), 0, st, (u32x4*)*d, c, S);
    PM_HIP(ctx, hipGetLastError());
    return PM_OK;
  });
}

int get_domain_tables(pm_ctx* ctx, int dir, unsigned log_n, bool need_coset, NttDomainTables** out, hipStream_t st) {
  NttDomainTables& t = ctx->domain[dir][log_n];
  const host::Field<4>& F = host::FR();
  t.lh = (log_n + 1) / 2;
  const u32 n_lo = 1u << t.lh, n_hi = 1u << (log_n - t.lh);
  // a pair of tables is published only when both were built: a failed second allocation must not
  // leave a half-initialised entry for the next call to launch with
  auto build_pair = [&](const HFr& base, void** lo_out, void** hi_out) -> int {
    void *lo = nullptr, *hi = nullptr;
    int rc = build_pow_table(ctx, &lo, base, host::one(F), n_lo, 1, st);
    if (!rc) rc = build_pow_table(ctx, &hi, base, host::one(F), n_hi, n_lo, st);
    if (rc) {
      if (lo) (void)hipFree(lo);
      if (hi) (void)hipFree(hi);
      return rc;
    }
    *lo_out = lo;
    *hi_out = hi;
    return PM_OK;
  };
  if (!t.tw_lo || !t.tw_hi) {
    HFr w = domain_gen(log_n);
    if (dir) w = host::inv(w, F);
    int rc = build_pair(w, &t.tw_lo, &t.tw_hi);
    if (rc) return rc;
  }
  if (need_coset && (!t.cs_lo || !t.cs_hi)) {
    HFr g = host::from_u64(host::FR_GENERATOR, F);
    if (dir) g = host::inv(g, F);
    int rc = build_pair(g, &t.cs_lo, &t.cs_hi);
    if (rc) return rc;
  }
  *out = &t;
  return PM_OK;
}

static void fill_consts(NttConsts& c, int dir, unsigned log_n) {
  const host::Field<4>& F = host::FR();
  HFr w8 = domain_gen(3);
  if (dir) w8 = host::inv(w8, F);
  HFr w = w8;
  for (int i = 0; i < 3; ++i) {
    to_limbs(c.w8[i], w);
    w = host::mul(w, w8, F);
  }
  to_limbs(c.one, host::one(F));
  if (dir)
    to_limbs(c.scale, host::inv(host::from_u64((u64)1 << log_n, F), F));
  else
    to_limbs(c.scale, host::one(F));
}

// Inter-pass twiddle table of pass i (N x 36 B, laid out like the wide data): built on first use for
// the plan in force, rebuilt when the tunables changed the plan.
static int get_pass_tw(pm_ctx* ctx, NttDomainTables* dt, int i, bool last, int dir, unsigned log_n, unsigned log_ns,
                       int S, unsigned wide_glog, const NttConsts& kc, hipStream_t st, void** out) {
  const size_t n = (size_t)1 << log_n;
  const unsigned key = (((((log_ns << 8) | (unsigned)S) << 1) | (last ? 1u : 0u)) << 2) | wide_glog;
  if (dt->pass_tw[i] && dt->pass_tw_key[i] != key) {  // the plan changed (tunables): rebuild
    PM_HIP(ctx, hipDeviceSynchronize());
    PM_HIP(ctx, hipFree(dt->pass_tw[i]));
    dt->pass_tw[i] = nullptr;
  }
  if (!dt->pass_tw[i]) {
    void* t = nullptr;
    PM_HIP(ctx, hipMalloc(&t, n * 36));
    NttConsts c2 = kc;
    if (!(last && dir)) memcpy(c2.scale, kc.one, sizeof c2.scale);  // only the inverse's last pass carries n^-1
    hipLaunchKernelGGL(pass_tw_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, t, c2, log_n, log_ns,
                       (u32)S, (const u32x4*)dt->tw_hi, (const u32x4*)dt->tw_lo, dt->lh, wide_glog);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
      (void)hipFree(t);
      return set_err(ctx, PM_ERR_HIP, std::string("pass_tw_kernel: ") + hipGetErrorString(e));
    }
    dt->pass_tw[i] = t;
    dt->pass_tw_key[i] = key;
  }
  *out = dt->pass_tw[i];
  return PM_OK;
}

// ------------------------------------------------------------------ acquisition
// Every table a resolved plan names, present in the context's caches and by pointer: the domain tables (with the coset's for
// a coset transform), per pass the step table of its family, the lazy table in the form its kernel reads, and the
// inter-pass tables it reads or applies.  Builds what is missing on st; a second call with the same plan builds nothing.
struct NttTables {
  NttDomainTables* dt;
  NttConsts kc;
  void *step[4], *lazy[4], *tw_in[4], *tw_out[4];
};
static int ntt_acquire(pm_ctx* ctx, const NttLaunches& L, unsigned log_n, unsigned flags, hipStream_t st, NttTables* T) {
  const int dir = (flags & PM_NTT_INVERSE) ? 1 : 0;
  memset(T, 0, sizeof *T);
  int rc = get_domain_tables(ctx, dir, log_n, (flags & PM_NTT_COSET) != 0, &T->dt, st);
  if (rc) return rc;
  fill_consts(T->kc, dir, log_n);
  auto pass_tw = [&](int j, void** out) {   // the inter-pass table of pass j: its consumer and its producer name the same one
    const PassLaunch& q = L.pass[j];
    return get_pass_tw(ctx, T->dt, j, q.role == ROLE_LAST, dir, log_n, q.log_ns, q.S, L.wide_glog, T->kc, st, out);
  };
  for (int i = 0; i < L.npass; ++i) {
    const PassLaunch& p = L.pass[i];
    rc = get_step_table(ctx, dir, (unsigned)p.S, p.r4 ? STEP_R4 : STEP_R8, &T->step[i], st);
    if (!rc && p.lazy) rc = get_step_table(ctx, dir, (unsigned)p.S, p.lazy, &T->lazy[i], st);
    if (!rc && p.tw_in >= 0) rc = pass_tw(p.tw_in, &T->tw_in[i]);
    if (!rc && p.tw_out >= 0) rc = pass_tw(p.tw_out, &T->tw_out[i]);
    if (rc) return rc;
  }
  return PM_OK;
}

// ------------------------------------------------------------------ execution
static NttOpts ntt_opts(const pm_ctx* ctx) {
  return NttOpts{ctx->opt_ntt_tile_log, ctx->opt_ntt_max_radix, ctx->opt_ntt_radix,     ctx->opt_ntt_xcd,
                 ctx->opt_ntt_direct_tw, ctx->opt_ntt_tw_producer, ctx->opt_ntt_step_prio, ctx->opt_ntt_fixed_shape};
}
// the argument checks of pm_fr_ntt_dev and pm_fr_ntt_batch; *empty: a batch of none, nothing to do
static int ntt_check_args(pm_ctx* ctx, size_t in_len, size_t in_stride, size_t out_stride, unsigned log_n, unsigned batch,
                          unsigned flags, bool* empty) {
  *empty = false;
  if (log_n >= host::FR_TWO_ADICITY)
    return set_err(ctx, PM_ERR_DOMAIN_TOO_LARGE, "log_n >= 32 (Fr two-adicity)");
  const size_t n = (size_t)1 << log_n;
  if (in_len > n) return set_err(ctx, PM_ERR_LENGTH, "in_len > 2^log_n");
  if (batch == 0) {
    *empty = true;
    return PM_OK;
  }
  if (batch > 1 && (in_stride < in_len || out_stride < n))
    return set_err(ctx, PM_ERR_BAD_ARG, "batch strides shorter than the vectors");
  if (flags & ~(PM_NTT_INVERSE | PM_NTT_COSET)) return set_err(ctx, PM_ERR_BAD_ARG, "unknown flags");
  return PM_OK;
}

int ntt_run(pm_ctx* ctx, const void* d_in, size_t in_len, size_t in_stride, void* d_out,
            size_t out_stride, unsigned log_n, unsigned batch, unsigned flags, hipStream_t st) {
  // validate
  bool empty = false;
  if (int rc = ntt_check_args(ctx, in_len, in_stride, out_stride, log_n, batch, flags, &empty)) return rc;
  if (empty) return PM_OK;
  const size_t n = (size_t)1 << log_n;
  PM_HIP(ctx, hipSetDevice(ctx->device));
  OrderScope order_scope(ctx, ctx->ord_ntt, st);   // scratch vectors and lazily built tables are shared by all streams
  if (order_scope.rc) return order_scope.rc;
  memset(ctx->ntt_last_variant, 0, sizeof ctx->ntt_last_variant);   // what pm_test_ntt_last_variants reports: this transform's passes

  if (log_n == 0) {  // size-1 domain: identity (w = 1, size_inv = 1, g^0 = 1); zero if in_len == 0
    for (unsigned b = 0; b < batch; ++b) {
      char* o = (char*)d_out + b * out_stride * 32;
      if (in_len == 0) {
        PM_HIP(ctx, hipMemsetAsync(o, 0, 32, st));
      } else if (o != (const char*)d_in + b * in_stride * 32) {
        PM_HIP(ctx, hipMemcpyAsync(o, (const char*)d_in + b * in_stride * 32, 32,
                                   hipMemcpyDeviceToDevice, st));
      }
    }
    return PM_OK;
  }

  // resolve, acquire, choose buffers
  const NttLaunches L = ntt_resolve(ntt_opts(ctx), (unsigned)ctx->num_cus, log_n, batch, flags, in_len);
  for (int i = 0; i < L.npass; ++i)
    if (!L.pass[i].fn) return set_err(ctx, PM_ERR_BAD_ARG, "no kernel for this pass shape");
  NttTables T;
  int rc = ntt_acquire(ctx, L, log_n, flags, st, &T);
  if (rc) return rc;
  // pass i reads what pass i - 1 wrote and writes (last ? out : tmp[i & 1]); a pass never runs in place.  Intermediate
  // vectors are 9-limb "wide" planes in ntt_tmp[]; only a single-pass in-place transform needs a canonical bounce buffer
  // (ntt_tmp[0]) plus a copy
  const bool bounce = L.npass == 1 && d_in == d_out;
  for (int i = 0; i < std::min(L.npass - 1 + (bounce ? 1 : 0), 2); ++i) {
    rc = ensure_buffer(ctx, ctx->ntt_tmp[i], (size_t)batch * n * 36);
    if (rc) return rc;
  }
  void* dst[4];
  for (int i = 0; i < L.npass; ++i) dst[i] = (i == L.npass - 1 && !bounce) ? d_out : ctx->ntt_tmp[i & 1].ptr;
  for (int i = 0; i < L.npass; ++i)
    if (L.pass[i].lds > 64 * 1024)   // once per kernel and process, not per launch
      if (int lrc = raise_lds_limit(ctx, (const void*)L.pass[i].fn, L.pass[i].lds)) return lrc;

  NttPassArgs a;
  memset(&a, 0, sizeof a);
  a.tw_hi = (const u32x4*)T.dt->tw_hi;
  a.tw_lo = (const u32x4*)T.dt->tw_lo;
  a.cs_hi = (const u32x4*)T.dt->cs_hi;
  a.cs_lo = (const u32x4*)T.dt->cs_lo;
  a.log_n = log_n;
  a.lh = T.dt->lh;
  a.batch_stride_in = in_stride;
  a.batch_stride_out = bounce ? n : out_stride;
  a.in_len = (u32)in_len;
  if (L.tiny) {
    a.in = d_in;
    a.out = d_out;
    a.flags = L.tiny_flags;
    hipLaunchKernelGGL(ntt_tiny_kernel, dim3(1, batch), dim3(64), 0, st, a, T.kc);
    PM_HIP(ctx, hipGetLastError());
    return PM_OK;
  }
  a.wide_total = (unsigned long long)batch * n;
  a.wide_glog = L.wide_glog;

  // launch
  for (int i = 0; i < L.npass; ++i) {
    const PassLaunch& p = L.pass[i];
    a.in = i ? dst[i - 1] : d_in;
    a.out = dst[i];
    a.step_tw = (const u32x4*)T.step[i];
    a.step_tw_lazy = (const u32x4*)T.lazy[i];
    a.pass_tw = T.tw_in[i];
    a.pass_tw_out = T.tw_out[i];
    a.log_ns = p.log_ns;
    a.flags = p.flags;
    ctx->ntt_last_variant[i] = (unsigned)p.variant;
#ifdef PM_DEV_STAMPS
    if (p.r4)
      if (int lrc = ntt_stamps_arm(ctx, st, i, (size_t)p.blocks * batch * ((p.threads + 63) / 64))) return lrc;
#endif
    {
      static const char* kRoleName[4] = {"ntt_pass_single", "ntt_pass_first", "ntt_pass_middle", "ntt_pass_last"};
      ProfScope prof(ctx, st, kRoleName[p.role]);
      hipLaunchKernelGGL(p.fn, dim3(p.blocks, batch), dim3(p.threads), p.lds, st, a, T.kc);
    }
    PM_HIP(ctx, hipGetLastError());
  }
  if (bounce) {
    PM_HIP(ctx, hipMemcpy2DAsync(d_out, out_stride * 32, ctx->ntt_tmp[0].ptr, n * 32, n * 32, batch,
                                 hipMemcpyDeviceToDevice, st));
  }
  return PM_OK;
}

}  // namespace pm

// ------------------------------------------------------------------ C ABI
using namespace pm;

extern "C" int pm_ntt_plan(uint32_t log_n, uint32_t radix_log2[4], uint32_t* n_passes) {
  if (log_n >= host::FR_TWO_ADICITY) return PM_ERR_DOMAIN_TOO_LARGE;
  Plan p = make_plan(log_n, 0);
  for (int i = 0; i < 4; ++i) radix_log2[i] = (uint32_t)p.S[i];
  *n_passes = (uint32_t)p.npass;
  return PM_OK;
}

// test hook (pure host): the pass plan ntt_run() follows for this size and these tunables (0 = the defaults of a fresh
// context).  out[20]: passes, then per pass (up to 4) {log2 radix S, log2 columns per tile LT, threads per workgroup,
// LDS bytes}, then a bit mask of the passes that have a kernel, then the blocked layout's log2 group size, 0.
extern "C" int pm_test_ntt_plan(uint32_t log_n, uint32_t batch, long tile_log, long max_radix, long radix, uint32_t num_cus,
                                uint32_t out[20]) {
  if (!out || !batch) return PM_ERR_BAD_ARG;
  if (log_n >= host::FR_TWO_ADICITY) return PM_ERR_DOMAIN_TOO_LARGE;
  NttOpts o = kDefaultOpts;
  o.tile_log = tile_log;
  if (max_radix) o.max_radix = max_radix;
  if (radix) o.radix = radix;
  const NttLaunches L = ntt_resolve(o, num_cus ? num_cus : 256u, log_n, batch, 0, 1ull << log_n);
  memset(out, 0, 20 * sizeof(uint32_t));
  out[0] = (uint32_t)L.npass;
  for (int i = 0; i < L.npass; ++i) {
    const PassLaunch& p = L.pass[i];
    out[1 + 4 * i] = (uint32_t)p.S;
    out[2 + 4 * i] = (uint32_t)p.LT;
    out[3 + 4 * i] = p.threads;
    out[4 + 4 * i] = (uint32_t)p.lds;
    if (p.fn != nullptr) out[17] |= 1u << i;
  }
  out[18] = L.wide_glog;
  return PM_OK;
}

// test hook (pure host, no context): everything ntt_run() resolves for a transform before it launches.  opts[8]: the options
// ntt_tile_log, ntt_max_radix, ntt_radix (0 = the default of a fresh context, as in pm_test_ntt_plan), then the switches
// ntt_xcd, ntt_direct_tw, ntt_tw_producer, ntt_step_prio and ntt_fixed_shape (a negative value = the default, since 0 is a
// value of theirs).  out[60]: {passes, log2 group size of the blocked layout, 1 if the tiny kernel runs, its PASS_* flags,
// 1 if n^-1 is folded into the last pass's table, 0, 0, 0}, then 13 words per pass (up to 4): S, LT, role, family (4 or
// 8), variant (1 generic, 2 fixed-shape), threads, LDS bytes, workgroups, PASS_* flags, log_ns, lazy-table form G (0
// none), the pass whose inter-pass table it reads through pass_tw and the pass whose table it applies through pass_tw_out
// (-1: none).  PM_ERR_BAD_ARG also when a pass has no kernel.
extern "C" int pm_test_ntt_launches(uint32_t log_n, uint32_t batch, uint32_t flags, uint64_t in_len, const long opts[8],
                                    uint32_t num_cus, int32_t out[60]) {
  if (!out || !opts || !batch || (flags & ~(PM_NTT_INVERSE | PM_NTT_COSET))) return PM_ERR_BAD_ARG;
  if (log_n >= host::FR_TWO_ADICITY) return PM_ERR_DOMAIN_TOO_LARGE;
  if (in_len > (1ull << log_n)) return PM_ERR_LENGTH;
  NttOpts o = kDefaultOpts;
  long* dst[8] = {&o.tile_log, &o.max_radix, &o.radix, &o.xcd, &o.direct_tw, &o.tw_producer, &o.step_prio, &o.fixed_shape};
  for (int k = 0; k < 8; ++k)
    if (k < 3 ? opts[k] != 0 : opts[k] >= 0) *dst[k] = opts[k];
  const NttLaunches L = ntt_resolve(o, num_cus ? num_cus : 256u, log_n, batch, flags, in_len);
  memset(out, 0, 60 * sizeof(int32_t));
  out[0] = L.npass, out[1] = (int32_t)L.wide_glog, out[2] = L.tiny, out[3] = (int32_t)L.tiny_flags, out[4] = L.scale_folded;
  for (int i = 0; i < L.npass; ++i) {
    const PassLaunch& p = L.pass[i];
    if (!p.fn) return PM_ERR_BAD_ARG;
    const int32_t rec[13] = {p.S, p.LT, p.role, p.r4 ? 4 : 8, p.variant, (int32_t)p.threads, (int32_t)p.lds, (int32_t)p.blocks,
                             (int32_t)p.flags, (int32_t)p.log_ns, p.lazy, p.tw_in, p.tw_out};
    memcpy(out + 8 + 13 * i, rec, sizeof rec);
  }
  return PM_OK;
}

// test hook (pure host): would ntt_run() give this launch its fixed-shape variant: 1, or 0 for the generic kernel.  The launch
// is a radix-4 pass of radix 2^S over 2^LT columns in `role` (1 first, 3 last) of a 2^log_n transform with log_ns done before
// it, wide vectors blocked by 2^wide_glog, the pass's PASS_* flags, in_len input elements, coset: the transform has PM_NTT_COSET;
// fixed_shape is the option's value (0, 1 or 2).
extern "C" int pm_test_ntt_fixed_match(uint32_t S, uint32_t LT, uint32_t role, uint32_t log_n, uint32_t log_ns,
                                       uint32_t wide_glog, uint32_t pass_flags, uint64_t in_len, uint32_t coset,
                                       uint32_t fixed_shape) {
  if (S > 31 || LT > 31 || role > 3 || fixed_shape > 2) return 0;
  return fixed_variant((int)S, (int)LT, (int)role, log_n, log_ns, wide_glog, pass_flags, in_len, coset != 0, (long)fixed_shape,
                       nullptr) != nullptr
             ? 1
             : 0;
}

// test hook: which kernel each pass of the context's last transform took.  out[4], a pass each: 0 no such pass (or a size
// without pass kernels), 1 the generic kernel, 2 its fixed-shape variant.
extern "C" int pm_test_ntt_last_variants(pm_ctx* ctx, uint32_t out[4]) {
  if (!ctx || !out) return PM_ERR_BAD_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  for (int i = 0; i < 4; ++i) out[i] = ctx->ntt_last_variant[i];
  return PM_OK;
}

// the two table hooks below: the step table of `kind` (get_step_table), `bytes` long, built and cached like a transform's;
// *words = its size in 32-bit words, up to max_words of them are copied to out
static int dump_step_table(pm_ctx* ctx, uint32_t inverse, uint32_t S, int kind, size_t bytes, uint32_t* out, size_t max_words,
                           size_t* words) {
  std::lock_guard<std::mutex> lk(ctx->mu);
  PM_HIP(ctx, hipSetDevice(ctx->device));
  OrderScope order_scope(ctx, ctx->ord_ntt, ctx->stream);
  if (order_scope.rc) return order_scope.rc;
  void* tab = nullptr;
  int rc = get_step_table(ctx, (int)inverse, S, kind, &tab, ctx->stream);
  if (rc) return rc;
  const size_t total = bytes / 4;
  if (words) *words = total;
  const size_t n = std::min(total, max_words);
  if (n) PM_HIP(ctx, hipMemcpyAsync(out, tab, n * 4, hipMemcpyDeviceToHost, ctx->stream));
  PM_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return PM_OK;
}
// test hook: the radix-4 step table of radix 2^S (head, then entries) as the kernels read it
extern "C" int pm_test_ntt_step4_table(pm_ctx* ctx, uint32_t inverse, uint32_t S, uint32_t* out, size_t max_words,
                                       size_t* words) {
  if (!ctx || inverse > 1 || S < 2 || S > 10 || (!out && max_words)) return PM_ERR_BAD_ARG;
  return dump_step_table(ctx, inverse, S, STEP_R4, step4_table_bytes(S), out, max_words, words);
}
// test hook: the lazy split table of radix 2^S in form G (1, 2, 3 or 5 data limbs a row) as a kernel of that form reads it:
// the w4 head, then the entries of the radix-4 steps from the third on
extern "C" int pm_test_ntt_step4_lazy_table(pm_ctx* ctx, uint32_t inverse, uint32_t S, uint32_t G, uint32_t* out,
                                            size_t max_words, size_t* words) {
  if (!ctx || inverse > 1 || S < 2 || S > 10 || !(G == 1 || G == 2 || G == 3 || G == 5) || (!out && max_words)) return PM_ERR_BAD_ARG;
  return dump_step_table(ctx, inverse, S, (int)G, step4_lazy_table_bytes(S, G), out, max_words, words);
}

// test hook: the device tables the context caches for the NTT -- domain and coset tables (two each), step tables, lazy step
// tables and inter-pass tables of both directions
extern "C" int pm_test_ntt_table_count(pm_ctx* ctx, size_t* count) {
  if (!ctx || !count) return PM_ERR_BAD_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  size_t c = 0;
  for (int d = 0; d < 2; ++d) {
    c += ctx->step_tw[d].size() + ctx->step4_tw[d].size() + ctx->step4_lazy_tw[d].size();
    for (const auto& kv : ctx->domain[d]) {
      const NttDomainTables& t = kv.second;
      for (const void* p : {t.tw_hi, t.tw_lo, t.cs_hi, t.cs_lo, t.pass_tw[0], t.pass_tw[1], t.pass_tw[2], t.pass_tw[3]}) c += p != nullptr;
    }
  }
  *count = c;
  return PM_OK;
}

extern "C" int pm_domain_prepare(pm_ctx* ctx, uint32_t log_n) {
  if (!ctx) return PM_ERR_BAD_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (log_n >= host::FR_TWO_ADICITY)
    return set_err(ctx, PM_ERR_DOMAIN_TOO_LARGE, "log_n >= 32 (Fr two-adicity)");
  PM_HIP(ctx, hipSetDevice(ctx->device));
  if (log_n == 0) return PM_OK;
  OrderScope order_scope(ctx, ctx->ord_ntt, ctx->stream);
  if (order_scope.rc) return order_scope.rc;
  // the tables of the transforms of a whole input, one vector at a time, under the options in force: fft, ifft, coset_fft and
  // coset_ifft.  A batch whose plan takes narrower tiles rebuilds the inter-pass tables it keys differently at its first call.
  for (unsigned flags : {0u, (unsigned)PM_NTT_COSET, (unsigned)PM_NTT_INVERSE, (unsigned)(PM_NTT_INVERSE | PM_NTT_COSET)}) {
    const NttLaunches L = ntt_resolve(ntt_opts(ctx), (unsigned)ctx->num_cus, log_n, 1, flags, 1ull << log_n);
    NttTables T;
    if (int rc = ntt_acquire(ctx, L, log_n, flags, ctx->stream, &T)) return rc;
  }
  PM_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return PM_OK;
}

extern "C" int pm_fr_ntt_dev(pm_ctx* ctx, const void* d_in, size_t in_len, size_t in_stride,
                             void* d_out, size_t out_stride, uint32_t log_n, uint32_t batch,
                             uint32_t flags, void* hip_stream) {
  if (!ctx) return PM_ERR_BAD_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (!d_out || (!d_in && in_len)) return set_err(ctx, PM_ERR_BAD_ARG, "null device pointer");
  hipStream_t st = hip_stream ? (hipStream_t)hip_stream : ctx->stream;
  return ntt_run(ctx, d_in, in_len, in_stride, d_out, out_stride, log_n, batch, flags, st);
}

extern "C" int pm_fr_ntt_batch(pm_ctx* ctx, const uint64_t* in, size_t in_len, size_t in_stride,
                               uint64_t* out, size_t out_stride, uint32_t log_n, uint32_t batch,
                               uint32_t flags) {
  if (!ctx) return PM_ERR_BAD_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (!out || (!in && in_len)) return set_err(ctx, PM_ERR_BAD_ARG, "null pointer");
  bool empty = false;
  if (int crc = ntt_check_args(ctx, in_len, in_stride, out_stride, log_n, batch, flags, &empty)) return crc;
  if (empty) return PM_OK;
  const size_t n = (size_t)1 << log_n;
  PM_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const size_t in_elems = std::max<size_t>(in_len, 1);
  int rc = ensure_buffer(ctx, ctx->io_in, (size_t)batch * in_elems * 32);
  if (rc) return rc;
  rc = ensure_buffer(ctx, ctx->io_out, (size_t)batch * n * 32);
  if (rc) return rc;
  if (batch == 1 || ctx->opt_ntt_pipeline == 0) {
    if (in_len)
      PM_HIP(ctx, hipMemcpy2DAsync(ctx->io_in.ptr, in_elems * 32, in, in_stride * 32, in_len * 32,
                                   batch, hipMemcpyHostToDevice, st));
    rc = ntt_run(ctx, ctx->io_in.ptr, in_len, in_elems, ctx->io_out.ptr, n, log_n, batch, flags, st);
    if (rc) return rc;
    PM_HIP(ctx, hipMemcpy2DAsync(out, out_stride * 32, ctx->io_out.ptr, n * 32, n * 32, batch,
                                 hipMemcpyDeviceToHost, st));
    PM_HIP(ctx, hipStreamSynchronize(st));
    return PM_OK;
  }
  // Several polynomials from host memory (a prover round): the transfers are 10-30x the transform, so
  // they are what gets overlapped.  PCIe is full duplex: vector b+1 goes up on `copy_in` while vector b
  // is transformed on the compute stream and vector b-1 comes down on `copy_out`.  Copies from pageable
  // memory block the calling thread, hence the downloads run on a helper thread.
  if (!ctx->copy_in) PM_HIP(ctx, hipStreamCreateWithFlags(&ctx->copy_in, hipStreamNonBlocking));
  if (!ctx->copy_out) PM_HIP(ctx, hipStreamCreateWithFlags(&ctx->copy_out, hipStreamNonBlocking));
  std::vector<hipEvent_t> ev_in(batch), ev_done(batch);
  for (uint32_t b = 0; b < batch; ++b) {
    PM_HIP(ctx, hipEventCreateWithFlags(&ev_in[b], hipEventDisableTiming));
    PM_HIP(ctx, hipEventCreateWithFlags(&ev_done[b], hipEventDisableTiming));
  }
  std::mutex mq;
  std::condition_variable cv;
  uint32_t launched = 0;          // vectors whose transform has been enqueued (guarded by mq)
  bool abort_all = false;
  hipError_t down_err = hipSuccess;
  std::thread downloader([&] {
    (void)hipSetDevice(ctx->device);
    for (uint32_t b = 0; b < batch; ++b) {
      {
        std::unique_lock<std::mutex> lk2(mq);
        cv.wait(lk2, [&] { return launched > b || abort_all; });
        if (abort_all) return;
      }
      hipError_t e = hipStreamWaitEvent(ctx->copy_out, ev_done[b], 0);
      if (e == hipSuccess)
        e = hipMemcpyAsync(out + 4 * (size_t)b * out_stride, (const char*)ctx->io_out.ptr + (size_t)b * n * 32, n * 32,
                           hipMemcpyDeviceToHost, ctx->copy_out);
      if (e == hipSuccess) e = hipStreamSynchronize(ctx->copy_out);
      if (e != hipSuccess) {
        down_err = e;
        return;
      }
    }
  });
  hipError_t up_err = hipSuccess;
  for (uint32_t b = 0; b < batch && !rc && up_err == hipSuccess; ++b) {
    char* d_in_b = (char*)ctx->io_in.ptr + (size_t)b * in_elems * 32;
    if (in_len) up_err = hipMemcpyAsync(d_in_b, in + 4 * (size_t)b * in_stride, in_len * 32, hipMemcpyHostToDevice, ctx->copy_in);
    if (up_err == hipSuccess) up_err = hipEventRecord(ev_in[b], ctx->copy_in);
    if (up_err == hipSuccess) up_err = hipStreamWaitEvent(st, ev_in[b], 0);
    if (up_err != hipSuccess) break;
    rc = ntt_run(ctx, d_in_b, in_len, in_elems, (char*)ctx->io_out.ptr + (size_t)b * n * 32, n, log_n, 1, flags, st);
    if (rc) break;
    up_err = hipEventRecord(ev_done[b], st);
    {
      std::lock_guard<std::mutex> lk2(mq);
      launched = b + 1;
    }
    cv.notify_one();
  }
  if (rc || up_err != hipSuccess) {
    std::lock_guard<std::mutex> lk2(mq);
    abort_all = true;
  }
  cv.notify_one();
  downloader.join();
  (void)hipStreamSynchronize(st);
  for (uint32_t b = 0; b < batch; ++b) {
    (void)hipEventDestroy(ev_in[b]);
    (void)hipEventDestroy(ev_done[b]);
  }
  if (rc) return rc;
  if (up_err != hipSuccess || down_err != hipSuccess)
    return set_err(ctx, PM_ERR_HIP, std::string("pipelined batch NTT: ") + hipGetErrorString(up_err != hipSuccess ? up_err : down_err));
  return PM_OK;
}

extern "C" int pm_fr_ntt(pm_ctx* ctx, const uint64_t* in, size_t in_len, uint64_t* out,
                         uint32_t log_n, uint32_t flags) {
  return pm_fr_ntt_batch(ctx, in, in_len, in_len, out, (size_t)1 << (log_n < 32 ? log_n : 0), log_n,
                         1, flags);
}
