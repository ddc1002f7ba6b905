// Native Schnorr signatures on JubJub: the check u G + c PK = R, c = H(R.x, R.y, m), that the VAR_BASE
// gadget exists to constrain, outside a circuit.  One thread per signature, over the routines of jubjub.hip.h (the group law,
// the signed base-16 digits, the window tables), hades.hip.h (one permutation on a lane's own state) and jubjub_scalar.hip.h
// (integers modulo the subgroup order l):
//
//   sign    R = k G from the base's window table (64 ed_madd), ONE inversion -- R is hashed, so it has to be affine --, one
//           permutation over (capacity, R.x, R.y, m, 1), the truncation c = h mod 2^250, u = (k - c sk) mod l, three stores.
//   verify  two kernels on the stream.  Head: the range test of u and the two point tests, the same hash, u G from the table.
//           Tail: a thread's table 1 PK .. 8 PK in the scratch buffer and c PK by the ladder of jubjub_var_kernel over 63
//           windows (c < 2^250), one addition, then X = R.x Z and Y = R.y Z.  No inversion.  u G, c and the reason of the early
//           tests pass through the thread's scratch slot, so the ladder keeps the register budget jubjub_var_kernel has and
//           the head its own (DESIGN.md has the compiler's table for this layout and for the fused kernel it was chosen over).
//   batch   one equation for n signatures: a prep kernel (the head's tests and hash, z c and z u modulo l,
//           the points PK_i, -R_i and their multipliers), a one-workgroup sum that appends (G, a), ONE MSM over 2 n + 1 points
//           (jubjub_msm.hip) and three doublings of the sum on the host.  A cofactored check: weaker than verify.
//
// Every lane runs everything: a lane past n works on element n - 1 and stores nothing (fe_inv_dev votes across the wave; its
// scratch slot is its own), and a failed early test selects the reason, it does not branch around the ladder.  Nothing is read or written at an address that
// depends on an input except the table entries, whose index is clamped to 1 .. 8.
//
// The scheme is the shape of dusk-schnorr 0.7's single-key signature as remembered: prior knowledge, pinned by nothing here.
// NOT hardened against side channels: signing reads the table at addresses that depend on the nonce k, which with the public
// (c, u) determines sk, and the arithmetic modulo l selects on its operands.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "context.h"
#include "field_inv.hip.h"
#include "hades.hip.h"
#include "jubjub.hip.h"
#include "jubjub_scalar.hip.h"

namespace pm {
namespace {

using host::HFr;

constexpr u32 SCH_WINDOWS = 63;                             // signed base-16 digits of a challenge below 2^250 (the top one <= 4)
constexpr u32 SCH_SLOT_ENTRIES = 9;                         // a thread's scratch: 1 PK .. 8 PK, then u G
constexpr size_t SCH_SLOT_BYTES = (SCH_SLOT_ENTRIES * (size_t)JJ_POINT_CHUNKS + 3) * 16;   // 1344 per thread in flight

// ------------------------------------------------------------------ the host forms (csrc/host_field.h)
// the point is not the identity and l times it is
bool point_has_order_l(const uint64_t* xy) {
  const HPoint p = hpoint_load(xy), id = hpoint_identity();
  if (host::eq(p.x, id.x) && host::eq(p.y, id.y)) return false;
  uint64_t l[4];
  memcpy(l, host::JUBJUB_L(), 32);
  const HPoint q = hpoint_mul(p, l);
  return host::eq(q.x, id.x) && host::eq(q.y, id.y);
}
// c = the canonical integer of H(R.x, R.y, m) below 2^250
void host_challenge(uint32_t R, uint32_t F, const uint64_t* ark, const uint64_t* mds, uint32_t n_mds, const uint64_t* capacity,
                    const HPoint& r, const uint64_t* msg, uint64_t (&c)[4]) {
  const host::Field<4>& Fq = host::FR();
  HFr s[5] = {hfr_load(capacity), r.x, r.y, hfr_load(msg), host::one<4>(Fq)};   // three inputs, then the padding
  host_permute(R, F, ark, mds, n_mds, s);
  HFr one_int = host::zero<4>();
  one_int.l[0] = 1;                                         // x R * 1 / R = x
  const HFr h = host::mul(s[1], one_int, Fq);
  memcpy(c, h.l, 32);
  c[3] &= (1ull << 58) - 1;
}
// the integer u -> memory in `form`
void scalar_from_int(const uint64_t (&u)[4], uint32_t form, uint64_t* out) {
  if (form == PM_SCALAR_CANONICAL) {
    memcpy(out, u, 32);
    return;
  }
  HFr t, r2;
  memcpy(t.l, u, 32);
  memcpy(r2.l, host::FR().r2, 32);
  const HFr v = host::mul(t, r2, host::FR());
  memcpy(out, v.l, 32);
}
bool host_common_fault(const uint64_t* g_xy, uint32_t R, uint32_t F, const uint64_t* ark, const uint64_t* mds, uint32_t n_mds,
                       const uint64_t* capacity, const uint64_t* msg, uint32_t form) {
  if (!g_xy || !capacity || !msg || !params_fault(R, F, ark, mds, n_mds).empty()) return true;
  if (form != PM_SCALAR_MONTGOMERY && form != PM_SCALAR_CANONICAL) return true;
  if (!hfr_canonical(capacity) || !hfr_canonical(msg)) return true;
  return point_fault(g_xy) || !point_has_order_l(g_xy);
}

// ------------------------------------------------------------------ device side
struct SchnorrIo {
  const u32x4* tab_g;       // the base's window table
  const u32x4* keys;        // sign: n secret keys
  const u32x4* nonces;      // sign: n nonces
  const u32x4* pks;         // verify: n x (x | y)
  const u32x4* msgs;        // n elements
  const u32x4* sigs_in;     // verify: n x (u | R.x | R.y)
  u32x4* sigs_out;          // sign: the same
  u32* reasons;             // verify: n, or null
  unsigned long long* first_bad;   // verify: the lowest failing index, or null
  u32x4* scratch;           // verify: [entry][chunk][thread of the grid]
  size_t n, base;           // verify: index 0 here is signature `base` of the call
  u32 montgomery;           // sk, k and u are Montgomery elements, not plain integers
  u32 edwards_d[9];         // device form
  u32 capacity[9];          // device form
};

// the sponge of hades_thread_kernel over the one chunk (x, y, m), up to its permutation: s = the state with the keys of round 0
// added; word 1 after h_rounds_thread is the hash.  x, y, m in the device form, normalised, below 2 r: with the round key a
// word stays below the 4.2 r h_absorb reduces from.
template <class Io>
PM_DEV void sch_absorb(Fr (&s)[5], const Fr& x, const Fr& y, const Fr& m, const Io& a, const HadesTab& tab) {
  const Fr zero = fe_zero<FrP>();
#pragma unroll
  for (int i = 0; i < 9; ++i) s[0].l[i] = a.capacity[i];
  s[0] = h_absorb(s[0], zero, tab.ark);
  s[1] = h_absorb(zero, x, tab.ark + 9);
  s[2] = h_absorb(zero, y, tab.ark + 18);
  s[3] = h_absorb(zero, m, tab.ark + 27);
  s[4] = h_absorb(zero, fe_one<FrP>(), tab.ark + 36);       // the padding after a chunk of three
}
// the canonical integer of h (device form) with bits 250 and above cleared
PM_DEV void sch_challenge(const Fr& h, u64 (&c)[4]) {
  u32 w[8];
  fe_canon_pack<FrP>(w, fe_mul_limb<FrP>(h, 1u));           // x 2^261 * 1 / 2^261 = x
#pragma unroll
  for (int i = 0; i < 4; ++i) c[i] = (u64)w[2 * i] | ((u64)w[2 * i + 1] << 32);
  c[3] &= (1ull << 58) - 1;
}

__global__ void __launch_bounds__(64) schnorr_sign_kernel(const HadesTab tab, const SchnorrIo a) {
  const size_t g = (size_t)blockIdx.x * 64 + threadIdx.x;
  const bool live = g < a.n;
  const size_t i = live ? g : a.n - 1;
  const Fr ed = fr_limbs(a.edwards_d);
  // ---- R = k G
  u64 k[4];
  jj_load_scalar(a.nonces + 2 * i, a.montgomery != 0, k);
  const EdPoint acc = jj_fixed_walk(a.tab_g, k, ed);
  const Fr zi = fe_inv_dev<FrP>(acc.Z);                     // every lane of the wave is here; nothing below crosses lanes
  Fr s[5];
  {
    const Fr rx = gmul(acc.X, zi), ry = gmul(acc.Y, zi);    // device x device -> device
    if (live) {                                             // R leaves before the hash: its 18 registers are free while the rounds run
      st_canon(a.sigs_out, 3 * i + 1, g_to_abi(rx));
      st_canon(a.sigs_out, 3 * i + 2, g_to_abi(ry));
    }
    sch_absorb(s, rx, ry, g_to_dev(ld_canon(a.msgs, i)), a, tab);
  }
  h_rounds_thread(s, tab);
  // ---- c, then u = (k - c sk) mod l on the integers
  u64 c[4], sk[4], u[4];
  sch_challenge(s[1], c);
  jj_load_scalar(a.nonces + 2 * i, a.montgomery != 0, k);   // the walk consumed it
  jj_load_scalar(a.keys + 2 * i, a.montgomery != 0, sk);
  scl_mulsub(u, k, sk, c);
  if (!live) return;
  u32 w[8];
#pragma unroll
  for (int j = 0; j < 4; ++j) w[2 * j] = (u32)u[j], w[2 * j + 1] = (u32)(u[j] >> 32);
  // the integer u < l times 2^261 (canonical) or 2^517 (Montgomery: u 2^256), over 2^261
  const Fr f = g_sel(a.montgomery != 0, fe_pow2<FrP, 517>(), fe_one<FrP>());
  st_canon(a.sigs_out, 3 * i, gmul(fe_unpack<FrP>(w), f));
}

// Verification is two kernels on the stream, each one thread a signature over at most one stride of them (the slots are per
// thread in flight; the host walks n in strides as jubjub_var_kernel's loop does).  What the head hands to the tail goes through
// the thread's slot: u G, the challenge (two chunks) and the reason of the early tests.
// Two to four waves a SIMD: pinned to two, as the tail is, the scheduler spends the registers and the permutation's rounds spill.
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 4))) schnorr_verify_head_kernel(const HadesTab tab,
                                                                                                             const SchnorrIo a) {
  const size_t T = (size_t)gridDim.x * 64, tid = (size_t)blockIdx.x * 64 + threadIdx.x;
  u32x4* const tbl = a.scratch + tid;
  u32x4* const pass = tbl + (size_t)SCH_SLOT_ENTRIES * JJ_POINT_CHUNKS * T;
  const size_t i = tid < a.n ? tid : a.n - 1;
  const u32x4* const sig = a.sigs_in + 6 * i;
  const Fr ed = fr_limbs(a.edwards_d);
  // ---- u < l, and u G into the slot
  u64 u[4];
  jj_load_scalar(sig, a.montgomery != 0, u);
  const bool u_ok = jj_below_r(sig[0], sig[1]) && scl_below_l(u);
  jj_table_store(tbl, T, SCH_SLOT_ENTRIES, jj_fixed_walk(a.tab_g, u, ed));
  // ---- the two points, the challenge
  Fr s[5];
  {
    Fr rx, ry, px, py;
    const bool pk_ok = jj_point_ok(a.pks + 4 * i, ed, px, py);
    const bool r_ok = jj_point_ok(sig + 2, ed, rx, ry);
    const u32 early = !u_ok ? PM_SCHNORR_U_RANGE : !r_ok ? PM_SCHNORR_R_POINT : !pk_ok ? PM_SCHNORR_PK_POINT : PM_SCHNORR_OK;
    pass[2 * T] = u32x4{early, 0, 0, 0};
    sch_absorb(s, rx, ry, g_to_dev(ld_canon(a.msgs, i)), a, tab);
  }
  h_rounds_thread(s, tab);
  u64 c[4];
  sch_challenge(s[1], c);
  pass[0] = u32x4{(u32)c[0], (u32)(c[0] >> 32), (u32)c[1], (u32)(c[1] >> 32)};
  pass[T] = u32x4{(u32)c[2], (u32)(c[2] >> 32), (u32)c[3], (u32)(c[3] >> 32)};
}

// two waves a SIMD: the ladder's register budget, as jubjub_var_kernel
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 2))) schnorr_verify_tail_kernel(const SchnorrIo a) {
  const size_t T = (size_t)gridDim.x * 64;
  const u32 tid = blockIdx.x * 64 + threadIdx.x;
  u32x4* const tbl = a.scratch + tid;
  const bool live = tid < a.n;
  const u32 i = live ? tid : (u32)a.n - 1;                  // n < 2^31; one register, not two, across the ladder
  const Fr ed = fr_limbs(a.edwards_d);
  u64 c[4];
  {
    const u32x4* const pass = tbl + (size_t)SCH_SLOT_ENTRIES * JJ_POINT_CHUNKS * T;
    const u32x4 c0 = pass[0], c1 = pass[T];
    c[0] = (u64)c0.x | ((u64)c0.y << 32), c[1] = (u64)c0.z | ((u64)c0.w << 32);
    c[2] = (u64)c1.x | ((u64)c1.y << 32), c[3] = (u64)c1.z | ((u64)c1.w << 32);
  }
  // ---- the table of PK
  jj_table_build(tbl, T, g_to_dev(ld_canon(a.pks, 2 * (size_t)i)), g_to_dev(ld_canon(a.pks, 2 * (size_t)i + 1)), ed);
  // ---- c PK from digit 62 down: digit 63 of c < 2^250 is zero and nothing carries into it
  const u64 carries = jj_carries(c) << 1;
  jj_shl4(c);
  EdPoint acc = jj_ladder(tbl, T, c, carries, SCH_WINDOWS, ed);
  // ---- u G + c PK = R: X = R.x Z and Y = R.y Z
  acc = ed_add(acc, jj_table_load(tbl, T, SCH_SLOT_ENTRIES), ed);
  const Fr rx = g_to_dev(ld_canon(a.sigs_in, 3 * (size_t)i + 1)), ry = g_to_dev(ld_canon(a.sigs_in, 3 * (size_t)i + 2));
  const bool same = jj_is_zero(gsub(acc.X, gmul(rx, acc.Z))) && jj_is_zero(gsub(acc.Y, gmul(ry, acc.Z)));
  size_t at = ((size_t)SCH_SLOT_ENTRIES * JJ_POINT_CHUNKS + 2) * T;
  asm volatile("" : "+s"(at));                               // formed here from tbl: no second address is held across the ladder
  const u32 early = tbl[at].x;
  const u32 reason = early != PM_SCHNORR_OK ? early : (same ? PM_SCHNORR_OK : PM_SCHNORR_EQUATION);
  if (!live) return;
  if (a.reasons) a.reasons[i] = reason;
  if (a.first_bad && reason != PM_SCHNORR_OK) atomicMin(a.first_bad, (unsigned long long)(a.base + i));
}


// ------------------------------------------------------------------ batch verification by one random linear combination
// W = a G + sum b_i PK_i - sum z_i R_i with b_i = z_i c_i mod l and a = sum z_i u_i mod l, then 8 W = (0, 1): the group has
// order 8 l, so reducing a multiplier modulo l changes a curve point's product by a point the factor 8 kills.  The prep kernel
// is verify's head without u G: the three structural tests, the hash, two products modulo l, and the MSM's input -- points
// PK_i and -R_i, canonical integers b_i and z_i, z_i u_i aside for the sum kernel.  An entry that fails a structural test goes
// in as the identity with zero scalars, so nothing unspecified enters the sum.
struct SchnorrBatchIo {
  const u32x4* pks;         // n x (x | y)
  const u32x4* msgs;        // n elements
  const u32x4* sigs;        // n x (u | R.x | R.y)
  const u32x4* weights;     // n x 16 bytes: z_i < 2^128, little end first
  u32x4* points;            // the MSM's 2 n + 1 points: PK_i, -R_i, ..., G
  u32x4* scalars;           // its 2 n + 1 canonical integers: b_i, z_i, ..., a
  u32x4* zu;                // n integers z_i u_i mod l
  unsigned long long* ctl;  // [0] min(index * 8 + reason) over structurally bad entries, [1] the lowest index of a zero weight
  size_t n;
  u32 montgomery;
  u32 edwards_d[9], capacity[9];
};
struct SchnorrBasePoint {
  u64 xy[8];                // canonical Montgomery
};
PM_DEV void sch_store_int(u32x4* at, const u64 (&v)[4], bool keep) {
  const u64 m = keep ? ~0ull : 0ull;                         // a mask, not a select between vectors (that one goes through scratch)
  const u64 w[4] = {v[0] & m, v[1] & m, v[2] & m, v[3] & m};
  at[0] = u32x4{(u32)w[0], (u32)(w[0] >> 32), (u32)w[1], (u32)(w[1] >> 32)};
  at[1] = u32x4{(u32)w[2], (u32)(w[2] >> 32), (u32)w[3], (u32)(w[3] >> 32)};
}
// a b mod l for a b < l 2^256
PM_DEV void scl_mulmod(u64 (&r)[4], const u64 (&a)[4], const u64 (&b)[4]) {
  const u64 r2[4] = {SCL_R2[0], SCL_R2[1], SCL_R2[2], SCL_R2[3]};
  u64 t[4];
  scl_mont(t, a, b);
  scl_mont(r, t, r2);
}
// a + b mod l for a, b < l
PM_DEV void scl_addmod(u64 (&r)[4], const u64 (&a)[4], const u64 (&b)[4]) {
  const u64 l[4] = {SCL_L[0], SCL_L[1], SCL_L[2], SCL_L[3]};
  u64 s[4], d[4], cy = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const u64 x = a[i] + b[i], y = x + cy;
    cy = (x < a[i] || y < x) ? 1u : 0u;
    s[i] = y;
  }
  const bool below = scl_sub(d, s, l) != 0;                 // 2 l < 2^253: the sum did not wrap
#pragma unroll
  for (int i = 0; i < 4; ++i) r[i] = below ? s[i] : d[i];
}

__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 4))) schnorr_batch_prep_kernel(const HadesTab tab,
                                                                                                            const SchnorrBatchIo a) {
  const size_t g = (size_t)blockIdx.x * 64 + threadIdx.x;
  const bool live = g < a.n;
  const size_t i = live ? g : a.n - 1;
  const u32x4* const sig = a.sigs + 6 * i;
  const Fr ed = fr_limbs(a.edwards_d);
  u64 u[4];
  jj_load_scalar(sig, a.montgomery != 0, u);
  const bool u_ok = jj_below_r(sig[0], sig[1]) && scl_below_l(u);
  Fr s[5];
  u32 early;
  {
    Fr rx, ry, px, py;
    const bool pk_ok = jj_point_ok(a.pks + 4 * i, ed, px, py);
    const bool r_ok = jj_point_ok(sig + 2, ed, rx, ry);
    early = !u_ok ? PM_SCHNORR_U_RANGE : !r_ok ? PM_SCHNORR_R_POINT : !pk_ok ? PM_SCHNORR_PK_POINT : PM_SCHNORR_OK;
    if (live) {                                              // PK_i and -R_i, or two identities
      const bool ok = early == PM_SCHNORR_OK;
      const Fr zero = fe_zero<FrP>(), one = g_one_abi();
      st_canon(a.points, 4 * i, g_sel(ok, g_to_abi(px), zero));
      st_canon(a.points, 4 * i + 1, g_sel(ok, g_to_abi(py), one));
      st_canon(a.points, 4 * i + 2, g_sel(ok, g_to_abi(gneg(rx)), zero));
      st_canon(a.points, 4 * i + 3, g_sel(ok, g_to_abi(ry), one));
    }
    sch_absorb(s, rx, ry, g_to_dev(ld_canon(a.msgs, i)), a, tab);
  }
  h_rounds_thread(s, tab);
  u64 c[4], b[4], v[4];
  sch_challenge(s[1], c);
  const u32x4 wz = a.weights[i];
  const u64 z[4] = {(u64)wz.x | ((u64)wz.y << 32), (u64)wz.z | ((u64)wz.w << 32), 0, 0};
  scl_mulmod(b, z, c);                                       // z c < 2^378
  scl_mulmod(v, z, u);                                       // z u < 2^383
  if (!live) return;
  const bool ok = early == PM_SCHNORR_OK;
  sch_store_int(a.scalars + 4 * i, b, ok);
  sch_store_int(a.scalars + 4 * i + 2, z, ok);
  sch_store_int(a.zu + 2 * i, v, ok);
  if (!ok) atomicMin(a.ctl, (unsigned long long)i * 8 + early);
  if ((z[0] | z[1]) == 0) atomicMin(a.ctl + 1, (unsigned long long)i);
}

// a = sum z_i u_i mod l and the last entry of the MSM's input: (G, a).  One workgroup.
__global__ void __launch_bounds__(256) schnorr_batch_sum_kernel(const SchnorrBatchIo a, const SchnorrBasePoint g) {
  __shared__ u64 lds[4][256];
  const u32 t = threadIdx.x;
  u64 acc[4] = {0, 0, 0, 0};
#pragma unroll 1
  for (size_t i = t; i < a.n; i += 256) {
    const u32x4 lo = a.zu[2 * i], hi = a.zu[2 * i + 1];
    const u64 v[4] = {(u64)lo.x | ((u64)lo.y << 32), (u64)lo.z | ((u64)lo.w << 32), (u64)hi.x | ((u64)hi.y << 32), (u64)hi.z | ((u64)hi.w << 32)};
    u64 r[4];
    scl_addmod(r, acc, v);
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = r[j];
  }
#pragma unroll 1
  for (u32 s = 128; s >= 1; s >>= 1) {
    if (t >= s && t < 2 * s) {
#pragma unroll
      for (int j = 0; j < 4; ++j) lds[j][t] = acc[j];
    }
    __syncthreads();
    if (t < s) {
      const u64 o[4] = {lds[0][t + s], lds[1][t + s], lds[2][t + s], lds[3][t + s]};
      u64 r[4];
      scl_addmod(r, acc, o);
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j] = r[j];
    }
    __syncthreads();
  }
  if (t != 0) return;
  sch_store_int(a.scalars + 4 * a.n, acc, true);
#pragma unroll
  for (int j = 0; j < 4; ++j)
    a.points[8 * a.n + j] = u32x4{(u32)g.xy[2 * j], (u32)(g.xy[2 * j] >> 32), (u32)g.xy[2 * j + 1], (u32)(g.xy[2 * j + 1] >> 32)};
}

// ------------------------------------------------------------------ launches
// the base's order, once per handle; the caller holds the context's mutex
int order_fault(pm_ctx* ctx, const pm_jubjub_base* g, const char* who) {
  if (g->order_state == 0) g->order_state = point_has_order_l(g->xy) ? 1 : -1;
  if (g->order_state < 0)
    return set_err(ctx, PM_ERR_BAD_ARG, std::string(who) + ": the base is the identity or its order is not l (l g != (0, 1))");
  return PM_OK;
}
int common_fault(pm_ctx* ctx, const pm_jubjub_base* g, const pm_hades_params* params, uint32_t scalar_form) {
  if (int rc = base_fault(ctx, g)) return rc;
  if (int rc = params_fault(ctx, params)) return rc;
  return form_fault(ctx, scalar_form);
}

}  // namespace
}  // namespace pm

using namespace pm;

extern "C" int pm_schnorr_sign_dev(pm_ctx* ctx, const pm_jubjub_base* g, const pm_hades_params* params, const uint64_t capacity[4],
                                   const void* d_secret_keys, const void* d_nonces, const void* d_msgs, size_t n,
                                   uint32_t scalar_form, void* d_sigs, void* hip_stream) {
  if (!ctx) return PM_ERR_BAD_ARG;
  if (int rc = common_fault(ctx, g, params, scalar_form)) return rc;
  SchnorrIo a{};
  if (int rc = capacity_to_dev(ctx, capacity, a.capacity)) return rc;
  if (int rc = pointer_fault(ctx, {d_secret_keys, d_nonces, d_msgs, d_sigs})) return rc;
  if (int rc = count_fault(ctx, n)) return rc;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (int rc = order_fault(ctx, g, "pm_schnorr_sign_dev")) return rc;
  if (n == 0) return PM_OK;
  PM_DEVICE_STREAM(ctx, hip_stream, st);
  a.tab_g = (const u32x4*)g->d_tab, a.keys = (const u32x4*)d_secret_keys, a.nonces = (const u32x4*)d_nonces;
  a.msgs = (const u32x4*)d_msgs, a.sigs_out = (u32x4*)d_sigs, a.n = n, a.montgomery = scalar_form == PM_SCALAR_MONTGOMERY;
  jubjub_d_limbs(a.edwards_d);
  ProfScope prof(ctx, st, "schnorr_sign");
  hipLaunchKernelGGL(schnorr_sign_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, tab_of(params), a);
  PM_HIP(ctx, hipGetLastError());
  return PM_OK;
}

extern "C" int pm_schnorr_verify_dev(pm_ctx* ctx, const pm_jubjub_base* g, const pm_hades_params* params, const uint64_t capacity[4],
                                     const void* d_pks_xy, const void* d_msgs, const void* d_sigs, size_t n, uint32_t scalar_form,
                                     void* d_reasons, size_t* first_bad, void* hip_stream) {
  if (!ctx) return PM_ERR_BAD_ARG;
  if (int rc = common_fault(ctx, g, params, scalar_form)) return rc;
  SchnorrIo a{};
  if (int rc = capacity_to_dev(ctx, capacity, a.capacity)) return rc;
  if (!d_reasons && !first_bad) return set_err(ctx, PM_ERR_BAD_ARG, "d_reasons and first_bad are both null");
  if (int rc = pointer_fault(ctx, {d_pks_xy, d_msgs, d_sigs}, ((uintptr_t)d_reasons & 3u) != 0)) return rc;
  if (int rc = count_fault(ctx, n)) return rc;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (int rc = order_fault(ctx, g, "pm_schnorr_verify_dev")) return rc;
  if (first_bad) *first_bad = n;
  if (n == 0) return PM_OK;
  PM_DEVICE_STREAM(ctx, hip_stream, st);
  // the slots of the threads in flight, and eight bytes for the lowest failing index
  SlotScratch scratch(ctx, n);
  PM_HIP(ctx, scratch.alloc(SCH_SLOT_BYTES, 16));
  unsigned long long* const d_bad = scratch.tail();
  unsigned long long bad = n;
  a.tab_g = (const u32x4*)g->d_tab, a.first_bad = first_bad ? d_bad : nullptr, a.scratch = scratch.slots();
  a.montgomery = scalar_form == PM_SCALAR_MONTGOMERY;
  jubjub_d_limbs(a.edwards_d);
  const HadesTab tab = tab_of(params);
  hipError_t e = first_bad ? hipMemcpyAsync(d_bad, &bad, 8, hipMemcpyHostToDevice, st) : hipSuccess;
  if (e == hipSuccess) {
    ProfScope prof(ctx, st, "schnorr_verify");
    for (size_t off = 0; off < n && e == hipSuccess; off += scratch.stride) {   // a stride's tail is done before the next head reuses the slots
      a.n = std::min(scratch.stride, n - off), a.base = off;
      a.pks = (const u32x4*)d_pks_xy + 4 * off, a.msgs = (const u32x4*)d_msgs + 2 * off, a.sigs_in = (const u32x4*)d_sigs + 6 * off;
      a.reasons = d_reasons ? (u32*)d_reasons + off : nullptr;
      hipLaunchKernelGGL(schnorr_verify_head_kernel, dim3((unsigned)scratch.blocks), dim3(64), 0, st, tab, a);
      hipLaunchKernelGGL(schnorr_verify_tail_kernel, dim3((unsigned)scratch.blocks), dim3(64), 0, st, a);
      e = hipGetLastError();
    }
  }
  if (int rc = finish_call(ctx, e, st, first_bad ? &bad : nullptr, d_bad, 8, scratch.base, "pm_schnorr_verify_dev")) return rc;
  if (first_bad) *first_bad = (size_t)bad;
  return PM_OK;
}

extern "C" int pm_schnorr_sign_host(const uint64_t g_xy[8], uint32_t rounds, uint32_t full_rounds, const uint64_t* ark,
                                    const uint64_t* mds, uint32_t n_mds, const uint64_t capacity[4], const uint64_t sk[4],
                                    const uint64_t nonce[4], const uint64_t msg[4], uint32_t scalar_form, uint64_t sig[12]) {
  if (!sk || !nonce || !sig || host_common_fault(g_xy, rounds, full_rounds, ark, mds, n_mds, capacity, msg, scalar_form))
    return PM_ERR_BAD_ARG;
  uint64_t ski[4], ki[4], c[4], u[4];
  if (!scalar_to_int(sk, scalar_form, ski) || !scalar_to_int(nonce, scalar_form, ki)) return PM_ERR_BAD_ARG;
  const HPoint r = hpoint_mul(hpoint_load(g_xy), ki);
  host_challenge(rounds, full_rounds, ark, mds, n_mds, capacity, r, msg, c);
  host::mulsub_l(ki, c, ski, u);
  scalar_from_int(u, scalar_form, sig);
  hpoint_store(sig + 4, r);
  return PM_OK;
}

extern "C" int pm_schnorr_verify_host(const uint64_t g_xy[8], uint32_t rounds, uint32_t full_rounds, const uint64_t* ark,
                                      const uint64_t* mds, uint32_t n_mds, const uint64_t capacity[4], const uint64_t pk_xy[8],
                                      const uint64_t msg[4], const uint64_t sig[12], uint32_t scalar_form, uint32_t* reason) {
  if (!pk_xy || !sig || !reason || host_common_fault(g_xy, rounds, full_rounds, ark, mds, n_mds, capacity, msg, scalar_form))
    return PM_ERR_BAD_ARG;
  uint64_t u[4], c[4];
  if (!scalar_to_int(sig, scalar_form, u) || !host::below_l(u)) {   // a word that is not below r is not below l either
    *reason = PM_SCHNORR_U_RANGE;
  } else if (point_fault(sig + 4)) {
    *reason = PM_SCHNORR_R_POINT;
  } else if (point_fault(pk_xy)) {
    *reason = PM_SCHNORR_PK_POINT;
  } else {
    const HPoint r = hpoint_load(sig + 4);
    host_challenge(rounds, full_rounds, ark, mds, n_mds, capacity, r, msg, c);
    const HPoint lhs = hpoint_add(hpoint_mul(hpoint_load(g_xy), u), hpoint_mul(hpoint_load(pk_xy), c));
    *reason = host::eq(lhs.x, r.x) && host::eq(lhs.y, r.y) ? PM_SCHNORR_OK : PM_SCHNORR_EQUATION;
  }
  return PM_OK;
}

extern "C" int pm_schnorr_verify_batch_dev(pm_ctx* ctx, const pm_jubjub_base* g, const pm_hades_params* params,
                                           const uint64_t capacity[4], const void* d_pks_xy, const void* d_msgs, const void* d_sigs,
                                           const void* d_weights, size_t n, uint32_t scalar_form, void* d_sum_xy, uint32_t* result,
                                           size_t* first_bad, void* hip_stream) {
  if (!ctx) return PM_ERR_BAD_ARG;
  if (int rc = common_fault(ctx, g, params, scalar_form)) return rc;
  SchnorrBatchIo a{};
  if (int rc = capacity_to_dev(ctx, capacity, a.capacity)) return rc;
  if (!result || !first_bad) return set_err(ctx, PM_ERR_BAD_ARG, "null result or first_bad");
  if (int rc = pointer_fault(ctx, {}, unaligned({d_pks_xy, d_msgs, d_sigs, d_weights, d_sum_xy}) ||
                                          (n != 0 && (!d_pks_xy || !d_msgs || !d_sigs || !d_weights))))
    return rc;
  if (n > 0x3fffffffu) return set_err(ctx, PM_ERR_LENGTH, "pm_schnorr_verify_batch_dev: n > 2^30 - 1");
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (int rc = order_fault(ctx, g, "pm_schnorr_verify_batch_dev")) return rc;
  *result = PM_SCHNORR_OK, *first_bad = n;
  PM_DEVICE_STREAM(ctx, hip_stream, st);
  if (n == 0) {                                              // the empty sum: accepted, W = (0, 1)
    if (!d_sum_xy) return PM_OK;
    if (int rc = jubjub_msm_enqueue(ctx, nullptr, nullptr, 0, 0, 1, false, d_sum_xy, st)) return rc;
    PM_HIP(ctx, hipStreamSynchronize(st));
    return PM_OK;
  }
  // the MSM's input, z_i u_i, W and the two control words
  const size_t m = 2 * n + 1, points_bytes = 64 * m, scalars_bytes = 32 * m, zu_bytes = 32 * n;
  char* buf = nullptr;
  PM_HIP(ctx, hipMalloc((void**)&buf, points_bytes + scalars_bytes + zu_bytes + 64 + 16));
  a.pks = (const u32x4*)d_pks_xy, a.msgs = (const u32x4*)d_msgs, a.sigs = (const u32x4*)d_sigs, a.weights = (const u32x4*)d_weights;
  a.points = (u32x4*)buf, a.scalars = (u32x4*)(buf + points_bytes), a.zu = (u32x4*)(buf + points_bytes + scalars_bytes);
  void* const d_w = buf + points_bytes + scalars_bytes + zu_bytes;
  a.ctl = (unsigned long long*)((char*)d_w + 64);
  a.n = n, a.montgomery = scalar_form == PM_SCALAR_MONTGOMERY;
  jubjub_d_limbs(a.edwards_d);
  SchnorrBasePoint gp;
  for (int j = 0; j < 8; ++j) gp.xy[j] = g->xy[j];
  unsigned long long ctl[2] = {~0ull, ~0ull};
  uint64_t w[8];
  int rc = PM_OK;
  hipError_t e = hipMemcpyAsync(a.ctl, ctl, 16, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) {
    ProfScope prof(ctx, st, "schnorr_verify_batch");
    hipLaunchKernelGGL(schnorr_batch_prep_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, tab_of(params), a);
    hipLaunchKernelGGL(schnorr_batch_sum_kernel, dim3(1), dim3(256), 0, st, a, gp);
    e = hipGetLastError();
    if (e == hipSuccess) rc = jubjub_msm_enqueue(ctx, a.points, a.scalars, m, m, 1, false, d_w, st);
  }
  if (e == hipSuccess && rc == PM_OK) e = hipMemcpyAsync(w, d_w, 64, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && rc == PM_OK && d_sum_xy) e = hipMemcpyAsync(d_sum_xy, d_w, 64, hipMemcpyDeviceToDevice, st);
  // the control words last: their way back is the wait for all of it
  if (int frc = finish_call(ctx, e, st, rc == PM_OK ? ctl : nullptr, a.ctl, 16, buf, "pm_schnorr_verify_batch_dev")) return frc;
  if (rc != PM_OK) return rc;
  if (ctl[1] < n)
    return set_err(ctx, PM_ERR_BAD_ARG, "pm_schnorr_verify_batch_dev: weight " + std::to_string(ctl[1]) + " is zero (it would drop its signature)");
  if (ctl[0] != ~0ull) {
    *result = (uint32_t)(ctl[0] & 7u), *first_bad = (size_t)(ctl[0] >> 3);
    return PM_OK;
  }
  // 8 W = (0, 1) on the host: three doublings of one point
  HPoint p = hpoint_load(w);
  for (int j = 0; j < 3; ++j) p = hpoint_add(p, p);
  const HPoint id = hpoint_identity();
  if (!host::eq(p.x, id.x) || !host::eq(p.y, id.y)) *result = PM_SCHNORR_EQUATION;
  return PM_OK;
}

extern "C" int pm_test_schnorr_stride(pm_ctx* ctx, size_t* stride) {
  if (!ctx || !stride) return PM_ERR_BAD_ARG;
  *stride = slot_blocks(ctx, ~(size_t)0 >> 1) * 64;
  return PM_OK;
}
