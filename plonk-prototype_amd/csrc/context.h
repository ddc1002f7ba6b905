// Library context: one GPU, one stream, cached domain tables, reusable workspaces.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <initializer_list>
#include <map>
#include <chrono>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/plonk_mi355x.h"

// default of the option ntt_step_prio; A/B builds set the other one (make EXTRA=-DPM_NTT_STEP_PRIO_DEFAULT=0)
#ifndef PM_NTT_STEP_PRIO_DEFAULT
#define PM_NTT_STEP_PRIO_DEFAULT 1
#endif
// ... and of the option ntt_fixed_shape: 2 since the fixed last pass keeps its step twiddles in flight and measured 1.3 - 1.5 us a
// launch faster than the generic one (PM_NTT_FIXED_TW_PREFETCH, profiles/twiddle_prefetch_kernel_trace.txt)
#ifndef PM_NTT_FIXED_SHAPE_DEFAULT
#define PM_NTT_FIXED_SHAPE_DEFAULT 2
#endif
// pm_poseidon_cipher_scan_keys_dev (DESIGN.md section 7.2q has the measurement both rest on): the keys from which the call
// builds the full window table of a note, below it the single-key ladder runs per key ...
#define PM_CIPHER_SCAN_KEYS_TABLE_MIN 4
// ... and the default of the option cipher_scan_table_mb, the cap on its scratch in MiB (0 = none)
#define PM_CIPHER_SCAN_TABLE_MB_DEFAULT 0

namespace pm {

class ExchangeWatch;                                   // comm.hip
void exchange_watch_free(ExchangeWatch* w);

struct DeviceBuffer {
  void* ptr = nullptr;
  size_t bytes = 0;
};

// A group of shared resources (scratch buffers, lazily built tables) that calls on different HIP
// streams would otherwise race on.  Every call that touches the group holds an OrderScope: on entry,
// when the stream differs from the one that used the group last, the new stream first waits for the
// event the PREVIOUS call recorded on its own stream when it ended; on exit the call records that
// event for its successor.  The library never touches a stream after the call it was passed to
// returned (a caller may destroy it), and only the library's own work is ordered.  A context behaves
// like one in-order queue per group even when its *_dev entry points are driven from several
// streams; groups are independent: an NTT on one stream and an MSM on another still overlap.
// Calls on the context's OWN stream (what a caller gets by passing no stream; the library creates and destroys it)
// record lazily -- when a call on another stream next needs the event -- because an event record per call is +2 % on
// a forward + inverse 2^20 NTT (profiles/r03_order_scope_ab.txt).
struct StreamOrder {
  hipStream_t last = nullptr;
  bool used = false;      // an earlier call used the group
  bool pending = false;   // ... on the context's own stream, and its closing event is not recorded yet
  hipEvent_t ev = nullptr;
};

struct NttDomainTables {  // per (log_n, direction)
  void* tw_hi = nullptr;
  void* tw_lo = nullptr;
  void* cs_hi = nullptr;
  void* cs_lo = nullptr;
  void* pass_tw[4] = {nullptr, nullptr, nullptr, nullptr};  // direct twiddles of pass i (wide planes)
  unsigned pass_tw_key[4] = {0, 0, 0, 0};                   // (log_ns << 8 | S) << 1 | last: what it was built for
  unsigned lh = 0;
};

}  // namespace pm

struct pm_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  hipStream_t copy_in = nullptr, copy_out = nullptr;    // host-pointer batch calls: H2D / D2H beside the compute stream
  std::mutex mu;
  std::string err;
  // NTT caches
  std::map<unsigned, void*> step_tw[2];                 // [dir][S] -> device table
  std::map<unsigned, void*> step4_tw[2];                // same for the radix-4 kernels
  std::map<unsigned, void*> step4_lazy_tw[2];           // [dir][S << 8 | G] -> their lazy table in form G
  std::map<unsigned, pm::NttDomainTables> domain[2];    // [dir][log_n]
  pm::DeviceBuffer ntt_tmp[2];
  pm::DeviceBuffer io_in, io_out;                       // staging for host-pointer calls
  pm::StreamOrder ord_ntt, ord_msm, ord_poly;           // cross-stream ordering of the shared scratch + tables
  // host timeline (diagnostic, PM_HOST_MARKS=1 in the environment): (label, microseconds) pairs, printed by the prover.  Not
  // synchronised: meant for one proving thread per context (several threads in one context would interleave their marks)
  bool marks_on = false;
  std::vector<std::pair<const char*, double>> marks;
  unsigned long long stat_alltoall_calls = 0, stat_alltoall_bytes = 0, stat_allgather_calls = 0, stat_transpose_steps = 0;   // pm_comm_stats
  int calls_holding_tables = 0;                         // calls that keep table pointers across unlocked sections (four-step NTT): pm_trim refuses
  // MSM workspaces
  pm::DeviceBuffer msm_ws;
  pm::DeviceBuffer msm_ctl;                             // control block of the bucket fill (msm_sort.hip.h): zero when idle
  unsigned msm_ctl_cap = 0;                             // partitions it is laid out for
  hipStream_t msm_side = nullptr;                       // second stream of the piece pipeline of a batched MSM (msm.hip)
  std::vector<hipEvent_t> msm_events;                   // "piece i has left the accumulate"
  pm::DeviceBuffer msm_scalars;
  pm::DeviceBuffer jj_msm_ws;                           // workspace of pm_jubjub_msm_dev (jubjub_msm_plan.h), under ord_jj_msm
  pm::StreamOrder ord_jj_msm;
  pm::DeviceBuffer fr_sqrt_tab;                         // tables of the Fr square root (fr_sqrt.hip.h): built at the first call that needs them
  pm::DeviceBuffer poly_ws;                             // scratch of the polynomial helpers
  pm::DeviceBuffer poly_tab;                            // power tables of pm_fr_poly_ruffini_dev
  void* msm_host_pinned = nullptr;
  void* poly_host_pinned = nullptr;                     // 3 x PM_LINCOMB_MAX results of the evaluation batches (poly.hip)
  size_t msm_host_pinned_bytes = 0;
  // multi-GPU exchange (comm.hip): RCCL communicator of this rank, device and pinned staging buffers
  void* comm = nullptr;
  bool comm_dead = false;                               // an exchange timed out and the communicator was aborted (comm.hip)
  pm::ExchangeWatch* comm_watch = nullptr;              // the deadline thread of guarded exchanges (option comm_timeout_ms)
  int comm_rank = 0, comm_world = 1;
  void *comm_send = nullptr, *comm_recv = nullptr, *comm_host = nullptr;
  // opt-in per-kernel timing (hipEvents on the launch stream; read by bench.py)
  bool profile = false;
  std::string profile_only;      // when set, only scopes with exactly this name record events
  struct ProfPending {
    hipEvent_t start, stop;
    const char* name;
  };
  std::vector<ProfPending> prof_pending;
  std::vector<hipEvent_t> prof_pool;
  struct ProfStat {
    double total_ms = 0;
    unsigned long long count = 0;
  };
  std::map<std::string, ProfStat> prof_stats;
  // tunables
  long opt_msm_window_bits = 0;  // 0 = auto
  long opt_ntt_tile_log = 0;     // 0 = auto
  long opt_ntt_radix = 4;        // in-tile butterfly radix: 4 (4 elements per thread) or 8
  long opt_ntt_xcd = 1;          // XCD-aware blockIdx -> tile mapping
  long opt_ntt_pipeline = 1;     // host-pointer batch calls: overlap H2D / transform / D2H per vector
  long opt_ntt_max_radix = 10;   // log2 of the largest pass radix (multi-pass plans)
  long opt_ntt_direct_tw = 1;    // inter-pass twiddles from per-pass N x 36 B tables (1) or from the two-level tables + one product (0)
  long opt_ntt_tw_producer = 1;  // with direct tables: radix-4 passes multiply their outputs by the next pass's table (1) or every pass its own inputs (0)
  long opt_ntt_step_prio = PM_NTT_STEP_PRIO_DEFAULT;  // radix-4 passes of two steps or more: wave priorities by step (1), so that co-resident workgroups alternate, or age alone (0)
  long opt_ntt_fixed_shape = PM_NTT_FIXED_SHAPE_DEFAULT;  // launches whose geometry and flags equal a fixed-shape variant's take it: all of them (2, the default), the first pass's only (1), or every launch the generic kernel (0)
  unsigned ntt_last_variant[4] = {0, 0, 0, 0};  // per pass of the last transform ntt_run() launched: 0 none, 1 generic kernel, 2 fixed-shape variant (pm_test_ntt_last_variants)
  long opt_msm_chunk = 0;        // 0 = auto (entries per thread in the level-1 accumulate)
  long opt_msm_max_pairs = 0;    // 0 = 2^31 - 1; a batched MSM with more (digit, point) pairs runs in halves
  long opt_msm_lb = 0;           // 0 = auto (buckets per thread in the bucket reduce)
  long opt_comm_timeout_ms = 0;  // > 0: every exchange on the context's RCCL communicator runs under this deadline (comm.hip)
  long opt_binv_quads = 0;       // batch inversion: quads (4 elements) per thread and inversion; 0 = auto
  long opt_poly_lookback = 1;    // prefix product in one pass (decoupled look-back) instead of totals / scan / replay
  long opt_jubjub_msm_window_bits = 0;   // 0 = the rule of jubjub_msm_plan.h
  long opt_cipher_scan_table_mb = PM_CIPHER_SCAN_TABLE_MB_DEFAULT;   // pm_poseidon_cipher_scan_keys_dev: its scratch in MiB at the most; 0 = no cap
  long opt_cipher_scan_keys_table_min = 0;   // ... and the keys from which it builds the full window table; 0 = PM_CIPHER_SCAN_KEYS_TABLE_MIN
  long opt_msm_pipeline = 0;    // 1: a batched MSM runs as up to four pieces on two streams (measured: loses, see msm.hip)
  int num_cus = 256;
};

struct pm_bases {
  void* d_xy = nullptr;  // n x 96 bytes, affine Montgomery, (0,0) = identity
  void* d_table = nullptr;   // optional: ceil(256/table_c) rows of n points, row w = 2^(table_c w) * bases
  unsigned table_c = 0;      // window bits the table was built for (0 = no table)
  size_t n = 0;
  int device = 0;
};

namespace pm {

int set_err(pm_ctx* ctx, int code, const std::string& msg);
// Scoped kernel timer: records an event pair around the launches issued while it lives.
struct ProfScope {
  pm_ctx* ctx;
  hipStream_t st;
  hipEvent_t stop = nullptr;
  ProfScope(pm_ctx* c, hipStream_t s, const char* name);
  ~ProfScope();
};
int prof_collect(pm_ctx* ctx);
int ensure_buffer(pm_ctx* ctx, DeviceBuffer& b, size_t bytes);
// hipFuncAttributeMaxDynamicSharedMemorySize is a per-function attribute of the PROCESS (per device), not of a
// context: the largest value any context asked for is remembered process-wide and only ever raised (ADVICE r03:
// with a per-context record, context B could lower what context A had set and A's next launch would fail).
int raise_lds_limit(pm_ctx* ctx, const void* fn, size_t bytes);
int comm_alltoall(pm_ctx* ctx, const void* d_send, void* d_recv, size_t bytes_per_peer, hipStream_t st);   // comm.hip
// the fixed-size exchange message of the sharded / distributed prover: [count | 288 payload words]; count 0 = abort marker
static constexpr size_t COMM_MSG_WORDS = 1 + 18 * (size_t)PM_COMM_MAX_POINTS;
int comm_allgather_msg(pm_ctx* ctx, const uint64_t* msg, uint64_t* gathered);   // comm.hip; caller holds ctx->mu
int fold_gathered(const uint64_t* msgs, int world, uint32_t k_local, uint64_t* out_xyz);   // comm.hip
// quotient kernel over `rows` rows of the coset (4 rows points); halo: the arrays read at index + 4 (z, wires 0 1 3)
// carry four more points after the last row instead of wrapping around (plonk_rounds.hip)
int plonk_quotient_rows(pm_ctx* ctx, const pm_plonk_quotient_args* args, size_t rows, bool halo, void* d_out, void* hip_stream);
// planar layout of the distributed prover (plonk_rounds.hip, struct QuotLayout): four planes [s][rows] per array in the
// block-transposed order of the rank-split transform, halo rows [4][n2] for a, b, d (halo_w[0], [1], [3]) and z
struct QuotPlanar {
  uint32_t n2, rot;
  const void* halo_w[4];
  const void* halo_z;
};
int plonk_quotient_layout(pm_ctx* ctx, const pm_plonk_quotient_args* args, size_t rows, bool halo, const QuotPlanar* planar,
                          void* d_out, void* hip_stream);
inline void host_mark(pm_ctx* ctx, const char* label) {
  if (ctx && ctx->marks_on)
    ctx->marks.emplace_back(label, std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count());
}
// n XYZZ records (ec.hip.h) -> n affine points in dst (ABI form when to_abi); prefix: n x 64 bytes of scratch.  Launches
// precompute_affine_kernel on st (msm.hip)
hipError_t xyzz_records_to_affine(pm_ctx* ctx, const void* records, size_t n, void* prefix, void* dst, bool to_abi,
                                  hipStream_t st);
int fr_batch_inverse_mul(pm_ctx* ctx, void* d_inout, const void* d_mul, size_t n, void* hip_stream);   // poly.hip: mul_i / v_i in place
int poly_evaluate_groups(pm_ctx* ctx, uint32_t groups, const uint32_t* k, const void* const* const* polys,
                         const uint64_t* const* points, uint64_t* const* outs, size_t n);   // poly.hip
int coset_expand(pm_ctx* ctx, const void* const* d_src, uint32_t count, const void* d_gs_pow, size_t m, void* d_out);
int sigma_evals_from_index(pm_ctx* ctx, const int64_t* idx, size_t count, uint32_t log_n, const uint64_t omega[4],
                           const uint64_t k[3][4], void* d_out);
int sigma_evals_from_index_dev(pm_ctx* ctx, const void* d_idx /* count x int64 */, size_t count, uint32_t log_n,
                               const uint64_t omega[4], const uint64_t k[3][4], void* d_out);
// Composer-form circuits (wire_perm.hip).  sigma_index_from_wires: device wire map (4n x uint32) ->
// device sigma_index (4n x int64); synchronises st (nullptr = the context's stream) and fails on an id out of range.
// witness_from_vars: out[b][p] = vars[b][wire_vars[p]] (32-byte elements), PM_PLONK_NO_VAR -> 0; asynchronous on st.
int sigma_index_from_wires(pm_ctx* ctx, const void* d_wire_vars, size_t num_vars, size_t n, void* d_sigma_index, hipStream_t st);
int witness_from_vars(pm_ctx* ctx, const void* d_wire_vars, size_t n, const void* d_vars, size_t var_stride, uint32_t batch,
                      void* d_out, hipStream_t st);
// Gadget witnesses (gadgets.hip).  GadgetRec: one gadget as the kernels read it, in launch order
// (level, then kind, then the caller's index); GadgetGroup: the records [first, first + count) of one launch.
struct GadgetRec {
  uint32_t kind, param;
  uint32_t first_row, count;
  uint32_t in_var[2];
  uint32_t index;          // the caller's index: what a report names
  uint32_t tab;            // its first unit in the array its kind gathers into (gadget_kinds.h, GadgetTab)
};
struct GadgetGroup {
  uint32_t kind, first, count;
  uint32_t span;           // BITS: the largest count of the group (the bits run along the grid's x)
};
// What a key's gadget table holds on the device: the records, the report words of a fill (set time's verdict is the first) and
// what set time gathers for the fills.  A table point of a FIXED_BASE round is x | y; an ARITH row keeps q_m q_l q_r q_4 q_c; a
// HADES round 30 coefficients (slot 5 i + j = matrix entry (i, j), slot 25 + j = round key j) and the 30 c ids of its rows (slot
// 5 k + j = key row, x2, x4, x5 of word j for k = 0..3, slot 20 + 2 i + k = z_i, o_i; PM_PLONK_NO_VAR: a partial round has none)
constexpr size_t GADGET_POINT_BYTES = 64, GADGET_COEF_BYTES = 5 * 32, GADGET_REPORT_BYTES = 2 * 8 * (size_t)PM_PLONK_MAX_BATCH;
constexpr size_t GADGET_ROUND_COEFS = 30, GADGET_ROUND_IDS = 30, GADGET_ROUND_COEF_BYTES = GADGET_ROUND_COEFS * 32, GADGET_ROUND_ID_BYTES = GADGET_ROUND_IDS * 4;
struct GadgetTables {
  void *recs = nullptr, *tab = nullptr, *rep = nullptr, *coef = nullptr, *hcoef = nullptr, *hids = nullptr;
  size_t count = 0, points = 0, arith_rows = 0, hades_rounds = 0;   // GadgetRec; what rec.tab counts for the kinds that gather
  // every array as f(pointer, units, bytes a unit): allocated (tab: one unit at least), counted in added_bytes and freed
  template <class F>
  void each_array(F f) {
    f(recs, count, sizeof(GadgetRec)), f(tab, points ? points : 1, GADGET_POINT_BYTES), f(rep, 1, GADGET_REPORT_BYTES);
    f(coef, arith_rows, GADGET_COEF_BYTES), f(hcoef, hades_rounds, GADGET_ROUND_COEF_BYTES), f(hids, hades_rounds, GADGET_ROUND_ID_BYTES);
  }
};
// set time: the first word of t.rep = the lowest index among the records whose claimed rows miss what their kind needs (~0:
// none); the gathered arrays of t are written.  d_sel: values on H, either q_l q_r q_range q_logic q_fixed_group_add
// q_variable_group_add (all11 = false: tables of the four widget kinds) or all eleven selectors in the order of
// PM_PLONK_SELECTORS, which the other kinds need; d_wire_vars is read for those only.  Asynchronous.
int gadget_verify(pm_ctx* ctx, const GadgetTables& t, size_t n, const void* d_sel, bool all11, const void* d_wire_vars, hipStream_t st);
// one launch per group on st; t.rep: 2 x batch words (failing gadgets, then min(index * 4 + reason)), copied to rep_host after
// the launches when it is given -- the call then waits for the stream
int gadget_fill(pm_ctx* ctx, const GadgetTables& t, const std::vector<GadgetGroup>& groups, const void* d_wire_vars, size_t n,
                void* d_vars, size_t var_stride, uint32_t batch, unsigned long long* rep_host, hipStream_t st);
// Native Poseidon (hades.hip): a pm_hades_params from the rounds gathered for a HADES gadget -- R rounds
// of GADGET_ROUND_COEFS canonical coefficients at d_rounds, copied: the handle does not refer to the table.  Waits for the
// context's stream (the gather of set time has then finished).
int hades_params_from_rounds(pm_ctx* ctx, const void* d_rounds, uint32_t R, uint32_t F, pm_hades_params** out);
// Native JubJub (jubjub.hip): a pm_jubjub_base from the table points gathered for a FIXED_BASE gadget -- R
// points of GADGET_POINT_BYTES at d_points, most significant round first; the base is the last one and the points before it
// must double it round by round.  The handle does not refer to the table.  Waits for the context's stream.
int jubjub_base_from_table(pm_ctx* ctx, const void* d_points, uint32_t R, pm_jubjub_base** out);
// Native JubJub MSM (jubjub_msm.hip): the launches of pm_jubjub_msm_dev on st for arguments already
// checked.  The caller holds the context's mutex and has selected the device.  Asynchronous.
int jubjub_msm_enqueue(pm_ctx* ctx, const void* d_points_xy, const void* d_scalars, size_t n, size_t scalar_stride, uint32_t batch,
                       bool montgomery, void* d_out_xy, hipStream_t st);
// Per-proof constants of the proof-batched kernels (pm_plonk_prove_batch): a pinned host buffer and its device twin of the
// same size.  A launcher takes one region of both, fills the host side and sends it with one async copy on its stream;
// kernels read the device side as a table indexed by the proof.  reset() once per call, after the previous call has
// synchronised: regions are never reused inside a call, so no copy still in flight reads a region being rewritten.
struct ConstStage {
  char* h = nullptr;
  char* d = nullptr;
  size_t cap = 0, used = 0;
  void reset() { used = 0; }
  bool take(size_t bytes, void** hp, void** dp) {
    const size_t sz = (bytes + 255) / 256 * 256;
    if (used + sz > cap) return false;
    *hp = h + used;
    *dp = d + used;
    used += sz;
    return true;
  }
};
// proof-batched launchers (plonk_rounds.hip, poly.hip); `batch` proofs per launch, blockIdx.y = the proof.  Strides in elements.
int perm_terms_batch(pm_ctx* ctx, ConstStage& stage, const pm_plonk_perm_args* args /* [batch]: pointers of proof 0 */,
                     uint32_t batch, size_t wire_stride, size_t n, void* d_num, void* d_den, hipStream_t st);
int quotient_batch(pm_ctx* ctx, ConstStage& stage, const pm_plonk_quotient_args* args /* [batch]: pointers of proof 0 */,
                   uint32_t batch, size_t wire_stride, size_t one_stride, size_t n, void* d_out, hipStream_t st);
int lincomb_batch(pm_ctx* ctx, ConstStage& stage, uint32_t k, const void* const* d_vecs, const size_t* strides,
                  const uint64_t* coeffs /* [batch][k][4] */, uint32_t batch, size_t n, void* d_out, size_t out_stride,
                  hipStream_t st);
// prefix products of `batch` vectors of n at stride n in one look-back launch, when every tile is resident at once; returns
// PM_ERR_LENGTH (having launched nothing) when they are not: the caller then takes pm_fr_prefix_product_dev per vector
size_t prefix_product_batch_ctl_bytes(uint32_t batch, size_t n);
int prefix_product_batch(pm_ctx* ctx, const void* d_in, size_t n, uint32_t batch, void* d_out, void* d_ctl, hipStream_t st);
// polynomial evaluation: slot j of proof b is polys[j] + b strides[j] at point points[b][point_of[j]] (point_of[j] < 2);
// k <= PM_EVAL_BATCH_SLOTS.  One host synchronisation; out: [batch][k][4] host.  lens (may be null: n everywhere): the
// coefficients slot j has, at most n -- the zero-knowledge batch opens padded vectors (n = the padded stride) beside key
// polynomials that end at the circuit size
constexpr uint32_t PM_EVAL_BATCH_SLOTS = 32;
size_t evaluate_batch_ws_bytes(uint32_t k, uint32_t batch, size_t n);   // every k' <= k, batch' <= batch
int evaluate_batch(pm_ctx* ctx, ConstStage& stage, uint32_t k, const void* const* polys, const size_t* strides,
                   const uint8_t* point_of, const uint64_t* points /* [batch][2][4] */, uint32_t batch, size_t n, void* d_ws,
                   uint64_t* out, hipStream_t st, const size_t* lens = nullptr);
// Ruffini division of `count` vectors of n coefficients (d_in + v stride, d_out + v stride) by X - z_v; falls back to
// pm_fr_poly_ruffini_dev per vector when a z is zero or a vector has more than 2^20 coefficients
size_t ruffini_batch_ws_bytes(uint32_t count, size_t n);
int ruffini_batch(pm_ctx* ctx, ConstStage& stage, const void* d_in, size_t n, size_t stride, const uint64_t* zs /* [count][4] */,
                  uint32_t count, void* d_out, void* d_ws, hipStream_t st);
// zero-knowledge mode (pm_plonk_prove_zk; plonk_rounds.hip).  Coefficient vectors at a padded stride S, blinders in the
// kernel arguments as canonical Montgomery limbs.
constexpr uint32_t ZK_MAX_VECS = 5;      // a b c d z
constexpr uint32_t ZK_MAX_TERMS = 3;     // blinder terms per vector
constexpr uint32_t ZK_MAX_SHIFT = 16;    // vectors per second-coset shift launch
constexpr size_t ZK_P1_LEN = 10;         // coefficients of t' beyond X^4n: deg t' <= 4n + 9
struct ZkBlindArgs {
  void* v[ZK_MAX_VECS];                  // coefficient vectors, n coefficients + a zero-filled tail up to the stride
  uint32_t terms[ZK_MAX_VECS];           // blinder terms of each (2 or 3)
  uint64_t beta[ZK_MAX_VECS][ZK_MAX_TERMS][4];
};
struct ZkShiftArgs {
  const void* src[ZK_MAX_SHIFT];
  void* dst[ZK_MAX_SHIFT];
  uint32_t count;
};
struct ZkCombineConsts {
  uint32_t inv2[9], inv2s[9];            // 1 / 2 and 1 / (2 * 7^4n), device form
};
// w + (beta . X^i) Z_H on `count` vectors (stride S) in one launch
int zk_blind(pm_ctx* ctx, const ZkBlindArgs& a, uint32_t count, size_t n, size_t stride, hipStream_t st);
// dst_j[i] = src_j[i] w_8n^i, i < len (d_w8: w_8n^i, 4n entries)
int zk_shift(pm_ctx* ctx, const ZkShiftArgs& a, const void* d_w8, size_t len, hipStream_t st);
// the two coset quotients (d_ab: A then B(X / w_8n), 4n coefficients each) -> t_1..t_4 with their blinders, stride S
int zk_combine(pm_ctx* ctx, const void* d_ab, const void* d_w8, size_t n, size_t stride, const uint64_t inv2[4],
               const uint64_t inv2s[4], const uint64_t beta[3][4], void* d_t, hipStream_t st);
// Proof-batched forms (pm_plonk_prove_batch_zk).  The blinders of all proofs do not fit the kernel
// arguments: they sit in a device table ([batch][PM_PLONK_ZK_BLINDERS][4] canonical Montgomery limbs, staged once per call
// in the workspace's ConstStage) that the kernels read with the wave-uniform proof index.
// vectors_per_proof vectors per proof (vector v of proof b at d_vecs + (b vectors_per_proof + v) stride) get the Z_H
// blinders of wire first_wire + v (0..3 = a b c d, 4 = z); the tail [n, stride) of every vector is written
int zk_blind_batch(pm_ctx* ctx, const void* d_blinders, void* d_vecs, uint32_t vectors_per_proof, uint32_t first_wire,
                   uint32_t batch, size_t n, size_t stride, hipStream_t st);
// dst[i] = src[i] w_8n^i for up to two groups of vectors in one launch; group g holds vecs[g] vectors per proof of len[g]
// coefficients, vector v of proof b at (b vecs[g] + v) stride[g], the same layout on both sides
struct ZkShiftBatchArgs {
  const void* src[2];
  void* dst[2];
  size_t stride[2], len[2];
  uint32_t vecs[2];
  uint32_t groups;
};
int zk_shift_batch(pm_ctx* ctx, const ZkShiftBatchArgs& a, const void* d_w8, uint32_t batch, hipStream_t st);
// zk_combine for every proof: d_ab holds A of proofs 0..batch-1 and then B(X / w_8n) of proofs 0..batch-1, 4n each; the
// pieces of proof b go to d_t + 4 b stride with its blinders b_14..b_16 from the table
int zk_combine_batch(pm_ctx* ctx, const void* d_blinders, const void* d_ab, const void* d_w8, uint32_t batch, size_t n,
                     size_t stride, const uint64_t inv2[4], const uint64_t inv2s[4], void* d_t, hipStream_t st);
// Witness check (pm_plonk_check_witness; plonk_rounds.hip): every gate identity and the copy
// constraints on the rows of H.  blockIdx.y = the witness; one mask byte per row and eight counters per witness.
// Counters of witness b of `batch` (u64): [7 b .. 7 b + 5] rows with bit 0..5 set, [7 b + 6] failing rows, and [7 batch + b]
// the minimum over failing rows of row * 64 + mask -- the launcher zeroes the first 7 batch words and sets the rest to ~0.
constexpr uint32_t CHECK_COUNTERS = 8;
struct WitnessCheckArgs {
  const void* wires;               // [batch][a | b | c | d][n]
  const void* sel[PM_PLONK_SELECTORS];   // values on H; nullptr = identically zero (q_arith: or identically one)
  bool arith_is_one;
  const void* pi;                  // [batch][n] dense public inputs
  const uint32_t* sigma;           // [4 n] wire positions j' n + i'
  uint8_t* masks;                  // [batch][n]
  unsigned long long* counters;    // CHECK_COUNTERS x batch words, initialised by the launcher
};
int check_witness_rows(pm_ctx* ctx, const WitnessCheckArgs& a, size_t n, uint32_t batch, hipStream_t st);
// *d_flag |= 1 when the n elements at d_a and d_b differ anywhere (d_flag: one zeroed word)
int vec_differs(pm_ctx* ctx, const void* d_a, const void* d_b, size_t n, uint32_t* d_flag, hipStream_t st);
// poly_evaluate_groups with a length per group
int poly_evaluate_groups_n(pm_ctx* ctx, uint32_t groups, const uint32_t* k, const void* const* const* polys,
                           const uint64_t* const* points, uint64_t* const* outs, const size_t* ns);
struct OrderScope {
  pm_ctx* ctx;
  StreamOrder& o;
  hipStream_t st;
  int rc;
  OrderScope(pm_ctx* c, StreamOrder& ord, hipStream_t s);
  ~OrderScope();
  OrderScope(const OrderScope&) = delete;
  OrderScope& operator=(const OrderScope&) = delete;
};

#define PM_HIP(ctx, call)                                                                   \
  do {                                                                                      \
    hipError_t _e = (call);                                                                 \
    if (_e != hipSuccess)                                                                   \
      return pm::set_err(ctx, _e == hipErrorOutOfMemory ? PM_ERR_OOM : PM_ERR_HIP,          \
                         std::string(#call) + ": " + hipGetErrorString(_e));                \
  } while (0)

// ------------------------------------------------------------------ the mechanics of a *_dev entry point
// Used by the native calls (hades.hip, jubjub.hip, jubjub_msm.hip, schnorr.hip, cipher.hip).  They replace lines that were the
// same in every entry and nothing else: each entry keeps its own order of checks, its return codes and its messages.
// select the device and name the stream of the call; PM_ENTER takes the context's mutex first
#define PM_DEVICE_STREAM(ctx, hip_stream, st)  \
  PM_HIP(ctx, hipSetDevice(ctx->device));      \
  hipStream_t st = hip_stream ? (hipStream_t)hip_stream : ctx->stream
#define PM_ENTER(ctx, hip_stream, st)          \
  std::lock_guard<std::mutex> lk(ctx->mu);     \
  PM_DEVICE_STREAM(ctx, hip_stream, st)

inline int count_fault(pm_ctx* ctx, size_t n) {
  if (n > 0x7fffffffu) return set_err(ctx, PM_ERR_LENGTH, "n > 2^31");
  return PM_OK;
}
// a pointer of the list is not 16-byte aligned; null passes: for pointers that may be null
inline bool unaligned(std::initializer_list<const void*> ps) {
  uintptr_t acc = 0;
  for (const void* p : ps) acc |= (uintptr_t)p;
  return (acc & 15u) != 0;
}
// a pointer of the list is null or not 16-byte aligned, or `also`: what else the entry holds against its pointers
inline int pointer_fault(pm_ctx* ctx, std::initializer_list<const void*> ps, bool also = false) {
  bool null = false;
  for (const void* p : ps) null = null || !p;
  if (null || unaligned(ps) || also) return set_err(ctx, PM_ERR_BAD_ARG, "null or unaligned device pointer");
  return PM_OK;
}
// the byte ranges share a byte; an empty range overlaps nothing
inline bool overlap(const void* p, size_t pb, const void* q, size_t qb) {
  const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
  return pb && qb && a < b + qb && b < a + pb;
}
// What a call does once its launches are on the stream (e: their error so far): `bytes` of a small result back into host when
// host is set, which waits for the stream; buf, the call's own allocation (may be null), released -- the launches are ordered on
// the stream like any other and releasing the buffer waits for them (hipFree waits for the device); one message naming `who`.
inline int finish_call(pm_ctx* ctx, hipError_t e, hipStream_t st, void* host, const void* dev, size_t bytes, void* buf, const char* who) {
  if (e == hipSuccess && host) {
    e = hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
  }
  const hipError_t e2 = buf ? hipFree(buf) : hipSuccess;
  if (e == hipSuccess) e = e2;
  if (e != hipSuccess) return set_err(ctx, PM_ERR_HIP, std::string(who) + ": " + hipGetErrorString(e));
  return PM_OK;
}

}  // namespace pm
