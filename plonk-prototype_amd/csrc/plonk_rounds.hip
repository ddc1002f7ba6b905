// The pointwise work of the PLONK prover rounds between the NTT and MSM calls, one fused kernel per
// round (BASELINE.json configs[3] "Full PLONK prove"):
//   pm_fr_powers_dev         domain.elements(), coset points, powers of a challenge
//   pm_fr_lincomb_dev        linearisation polynomial / aggregated opening polynomial
//   pm_plonk_perm_terms_dev  numerator and denominator of the permutation grand product
//   pm_plonk_quotient_dev    quotient numerator / Z_H on the 4n coset
// Restates dusk_plonk::proof_system::{permutation, quotient_poly, linearisation_poly} of
// dusk-plonk 0.8.2 (ref:Cargo.toml:19; not in the reference tree): the arithmetic identity (times
// q_arith), the permutation identities, and the four widgets behind the gates the reference's gadgets
// emit -- range (ref:src/zk/gadgets.rs:88-91), logic / boolean (:211), fixed-base scalar
// multiplication (:34,37; ref:src/zk/circuits.rs:64) and variable-base curve addition (:40).  The
// formulas are restated from the published dusk-plonk 0.8 design (parity unpinned).
//
// Scaling bookkeeping (poly_common.hip.h): memory holds ABI form (x 2^256); a product of forms 2^a and
// 2^b is of form 2^(a+b-261).  Wires are moved to device form (2^261) once per point, challenges are
// prepared by the host in the form that makes every sum homogeneous, the result leaves in ABI form.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "context.h"
#include "host_field.h"
#include "ntt_kernels.hip.h"
#include "poly_common.hip.h"

namespace pm {

// ABI (canonical) -> device form, (1, <1.01)
PM_DEV Fr to_dev(const Fr& x) { return fe_reduce_weak<FrP>(fr_shl5(x)); }

struct RoundConsts {
  u32 beta_k[4][9];  // beta k_j 2^266  (k_0 = 1):  x ABI  -> device form
  u32 beta[9];       // beta 2^266:                 sigma ABI -> device form
  u32 gamma[9];      // gamma 2^261
  u32 alpha[9];      // alpha 2^261
  u32 alpha2[9];     // alpha^2 2^266:              (ABI x ABI = 2^251) -> ABI
  u32 one_abi[9];    // 2^256
  u32 zh_inv[4][9];  // 1 / Z_H(x_i) by i mod 4, 2^261
};

// w + beta k x + gamma, all in device form: value < 1.01 r + 2 r + r, limbs < 3 * 2^29
PM_DEV Fr perm_factor(const Fr& w_dev, const Fr& x_abi, const u32* bk, const Fr& gamma) {
  return fe_add<FrP>(fe_add<FrP>(w_dev, fe_mul<FrP>(x_abi, fr_limbs(bk))), gamma);
}
// product of four factors (value < 4.1 r, limbs < 3 * 2^29 each) -> device form, (1, <1.1)
PM_DEV Fr prod4(const Fr& f0, const Fr& f1, const Fr& f2, const Fr& f3) {
  Fr p = fe_mul<FrP>(f0, fe_norm<FrP>(f1));   // 4.1^2 / 70 + 1 < 1.3
  p = fe_mul<FrP>(f2, p);
  return fe_mul<FrP>(f3, p);
}

// ------------------------------------------------------------------ powers
__global__ void __launch_bounds__(256) powers_kernel(u32x4* out, size_t n, const NttConsts c /* w8[0] = base,
                                                     w8[1] = base^T, scale, one = 2^256 */) {
  const size_t T = (size_t)gridDim.x * blockDim.x;
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  Fr cur = fr_pow(fr_limbs(c.w8[0]), t, fr_limbs(c.scale));
  const Fr step = fr_limbs(c.w8[1]), one_abi = fr_limbs(c.one);
  for (size_t i = t; i < n; i += T) {
    st_canon(out, i, fe_mul<FrP>(cur, one_abi));
    cur = fe_mul<FrP>(cur, step);
  }
}

// ------------------------------------------------------------------ linear combination
// out_b = sum_j c[b][j] v_j(b): term j of proof b at v[j] + b stride[j] (stride 0: a vector all proofs share, or one proof)
struct LincombArgs {
  const u32x4* v[PM_LINCOMB_MAX];
  size_t stride[PM_LINCOMB_MAX];
  u32 k;
};
// The coefficients (device form): k of them in the arguments, or row blockIdx.y of a [batch][k] table
struct CoeffArgs {
  u32 c[PM_LINCOMB_MAX][9];
  static PM_DEV u32 slot() { return 0; }
  PM_DEV Fr coeff(u32, u32, u32 j) const { return fr_limbs(c[j]); }
};
struct CoeffTable {
  const PM_KCONST u32 (*c)[9];
  static PM_DEV u32 slot() { return blockIdx.y; }
  PM_DEV Fr coeff(u32 b, u32 k, u32 j) const { return fr_limbs(kconst(c + (size_t)b * k, j)); }
};
template <class Src>
__global__ void __launch_bounds__(256) lincomb_kernel(const LincombArgs a, const Src src, u32x4* out, size_t out_stride, size_t n) {
  const u32 b = Src::slot();
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  out += 2 * (size_t)b * out_stride;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    Fr acc = fe_mul<FrP>(ld_canon(a.v[0] + 2 * (size_t)b * a.stride[0], i), src.coeff(b, a.k, 0));
    for (u32 j = 1; j < a.k; ++j)
      acc = fe_reduce_weak<FrP>(
          fe_add<FrP>(acc, fe_mul<FrP>(ld_canon(a.v[j] + 2 * (size_t)b * a.stride[j], i), src.coeff(b, a.k, j))));
    st_canon(out, i, acc);
  }
}

// ------------------------------------------------------------------ permutation terms
struct PermPtrs {
  const u32x4* w[4];
  const u32x4* s[4];
  const u32x4* roots;
  u32x4* num;
  u32x4* den;
};
// Src: FromArgs<RoundConsts> (one proof) or FromTable<RoundConsts> (blockIdx.y = proof: its wires at w[j] + b wire_stride,
// its num / den at + b n; sigmas and roots shared)
template <class Src>
__global__ void __launch_bounds__(256) perm_terms_kernel(const PermPtrs p0, const Src src, size_t n, size_t wire_stride) {
  const u32 b = Src::slot();
  const RoundConsts& kc = src.at(b);
  PermPtrs p = p0;
#pragma unroll
  for (int j = 0; j < 4; ++j) p.w[j] += 2 * (size_t)b * wire_stride;
  p.num += 2 * (size_t)b * n;
  p.den += 2 * (size_t)b * n;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  const Fr gamma = fr_limbs(kc.gamma), one_abi = fr_limbs(kc.one_abi);
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const Fr x = ld_canon(p.roots, i);
    Fr w[4], f[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) w[j] = to_dev(ld_canon(p.w[j], i));
#pragma unroll
    for (int j = 0; j < 4; ++j) f[j] = perm_factor(w[j], x, kc.beta_k[j], gamma);
    st_canon(p.num, i, fe_mul<FrP>(prod4(f[0], f[1], f[2], f[3]), one_abi));
#pragma unroll
    for (int j = 0; j < 4; ++j) f[j] = perm_factor(w[j], ld_canon(p.s[j], i), kc.beta, gamma);
    st_canon(p.den, i, fe_mul<FrP>(prod4(f[0], f[1], f[2], f[3]), one_abi));
  }
}

// ------------------------------------------------------------------ quotient
struct QuotPtrs {
  const u32x4* w[4];
  const u32x4* z;
  const u32x4 *q_m, *q_l, *q_r, *q_o, *q_4, *q_c, *pi;
  const u32x4* q_arith;                      // nullptr = the constant 1
  const u32x4 *q_range, *q_logic, *q_fixed, *q_var;   // nullptr = identically zero: the widget is skipped
  const u32x4* s[4];
  const u32x4* l1;
  const u32x4* x;
  u32x4* out;
};
// Everything the widgets multiply by, in device form (x 2^261)
struct WidgetConsts {
  u32 c1[9], c2[9], c3[9], c4[9], c9[9], c18[9], c81[9], c83[9], edwards_d[9];
  u32 range_sep[9], range_k[3][9];   // separation challenge s and kappa = s^2, kappa^2, kappa^3
  u32 logic_sep[9], logic_k[4][9];
  u32 fixed_sep[9], fixed_k[3][9];
  u32 var_sep[9], var_k[2][9];
};

// Widget arithmetic: every value in device form with normalised limbs and value < 1.05 r, closed
// under these three (fe_mul: < x y / 2^261 + r; the weak reduction after + and - brings the value
// back below r + r / 2^16).  Slower than the hand-scheduled lazy sums of the arithmetic identity, but
// the widget rows are a small part of real circuits and the kernel stays VALU-bound either way.
PM_DEV Fr wadd(const Fr& a, const Fr& b) { return fe_reduce_weak<FrP>(fe_add<FrP>(a, b)); }
PM_DEV Fr wsub(const Fr& a, const Fr& b) { return fe_reduce_weak<FrP>(fe_sub<FrP, 2, 1>(a, b)); }
PM_DEV Fr wmul(const Fr& a, const Fr& b) { return fe_mul<FrP>(a, b); }
// small multiples by additions (a product is ~225 instructions, an addition 9, a weak reduction ~40)
PM_DEV Fr wmul2(const Fr& a) { return fe_reduce_weak<FrP>(fe_add<FrP>(a, a)); }
PM_DEV Fr wmul3(const Fr& a) { return fe_reduce_weak<FrP>(fe_add<FrP>(fe_add<FrP>(a, a), a)); }
PM_DEV Fr wmul4(const Fr& a) {
  const Fr t = fe_add<FrP>(a, a);                        // limbs < 2^30 + ., value < 2.04 r
  return fe_reduce_weak<FrP>(fe_add<FrP>(t, t));         // limbs < 2^31 + ., value < 4.08 r
}
PM_DEV Fr wmul9(const Fr& a) {
  const Fr f = wmul4(a);
  return fe_reduce_weak<FrP>(fe_add<FrP>(fe_add<FrP>(f, f), a));   // 2 (4a) + a
}
PM_DEV Fr wsqr(const Fr& a) { return fe_sqr<FrP>(a); }
// f (f - 1)(f - 2)(f - 3) = u (u + 2) with u = f^2 - 3 f: zero exactly on the quads 0..3; one squaring and one
// product instead of three products
PM_DEV Fr wdelta(const Fr& f, const WidgetConsts& c) {
  const Fr u = wsub(wsqr(f), wmul3(f));
  return wmul(fe_add<FrP>(u, fr_limbs(c.c2)), u);          // first operand unreduced: limbs < 2^30 + ., value < 2.02 r
}

// Where the 4 m coset points of a launch sit.  Interleaved (one GPU, pm_plonk_quotient_dev): point 4 k + s = g w4^s w^k, the same
// polynomial at w X is index + 4 (wrapping at `wrap`).  PLANAR (the distributed prover, prover_dist.hip.h): four planes [s][m],
// plane s = the rank's rows of sub-coset g w4^s H in the block-transposed order of pm_fr_ntt_fourstep_batch_dev (position
// k1_local N2 + k2 holds k = k2 N1 + k1), so w X is index + N2 -- one row down -- and the row below the rank's last one
// is the halo row the transform delivered with it (four planes of N2 per polynomial; for the last rank it is rank 0's first
// row, where k + 1 means k2 + 1: `rot`).
struct QuotLayout {
  u32 log_m, n2, rot;
  const u32x4* halo_w[4];   // a, b, (unused), d
  const u32x4* halo_z;
};
// Whose quotient a launch computes.  OneProof: the constants travel in the kernel arguments and the pointers are the proof's
// own.  ProofTable: blockIdx.y is the proof, its constants are rows of two device tables (scalar loads, as from the
// arguments), its wires sit at w[j] + b wire_stride and its z / PI / out at + b one_stride (elements); selectors, sigmas,
// l1 and x are shared.
struct OneProof {
  RoundConsts kc;
  WidgetConsts wc;
  PM_DEV const RoundConsts& round() const { return kc; }
  PM_DEV const WidgetConsts& widget() const { return wc; }
  PM_DEV void select(QuotPtrs&) const {}
};
struct ProofTable {
  const PM_KCONST RoundConsts* kcs;
  const PM_KCONST WidgetConsts* wcs;
  size_t wire_stride, one_stride;
  PM_DEV const RoundConsts& round() const { return kconst(kcs, blockIdx.y); }
  PM_DEV const WidgetConsts& widget() const { return kconst(wcs, blockIdx.y); }
  PM_DEV void select(QuotPtrs& p) const {
    const u32 b = blockIdx.y;
    for (int j = 0; j < 4; ++j) p.w[j] += 2 * (size_t)b * wire_stride;
    p.z += 2 * (size_t)b * one_stride;
    p.pi += 2 * (size_t)b * one_stride;
    p.out += 2 * (size_t)b * one_stride;
  }
};
template <bool WIDGETS, bool PLANAR, class Src>
__global__ void __launch_bounds__(256, 2) quotient_kernel(const QuotPtrs p0, const Src src, size_t n4, size_t wrap, const QuotLayout L) {
  const RoundConsts& kc = src.round();
  const WidgetConsts& wc = src.widget();
  QuotPtrs p = p0;
  src.select(p);
  const size_t stride = (size_t)gridDim.x * blockDim.x;   // a multiple of 4: i mod 4 is fixed per thread
  const size_t t0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const u32 r4 = (u32)(t0 & 3);
  Fr zhi;
#pragma unroll
  for (int l = 0; l < 9; ++l)
    zhi.l[l] = r4 == 0 ? kc.zh_inv[0][l] : (r4 == 1 ? kc.zh_inv[1][l] : (r4 == 2 ? kc.zh_inv[2][l] : kc.zh_inv[3][l]));
  const Fr gamma = fr_limbs(kc.gamma);
  for (size_t i = t0; i < n4; i += stride) {
    size_t inext = i + 4 < wrap ? i + 4 : i + 4 - wrap;   // wrap = n4, or n4 + 4 when the rows carry a halo
    bool in_halo = false;
    if (PLANAR) {
      const u32 sp = (u32)(i >> L.log_m), pos = (u32)(i & (((size_t)1 << L.log_m) - 1)), m_ = 1u << L.log_m;
#pragma unroll
      for (int l = 0; l < 9; ++l)
        zhi.l[l] = sp == 0 ? kc.zh_inv[0][l] : (sp == 1 ? kc.zh_inv[1][l] : (sp == 2 ? kc.zh_inv[2][l] : kc.zh_inv[3][l]));
      in_halo = pos + L.n2 >= m_;
      inext = in_halo ? (size_t)sp * L.n2 + ((pos + L.n2 - m_ + L.rot) & (L.n2 - 1)) : i + L.n2;
    }
    Fr w[4], f[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) w[j] = to_dev(ld_canon(p.w[j], i));
    // arithmetic identity, ABI form: five (1, <2) products and one canonical load -> (6, <11)
    Fr g = fe_mul<FrP>(ld_canon(p.q_m, i), fe_mul<FrP>(w[0], w[1]));
    g = fe_add<FrP>(g, fe_mul<FrP>(ld_canon(p.q_l, i), w[0]));
    g = fe_add<FrP>(g, fe_mul<FrP>(ld_canon(p.q_r, i), w[1]));
    g = fe_add<FrP>(g, fe_mul<FrP>(ld_canon(p.q_o, i), w[2]));
    g = fe_add<FrP>(g, fe_mul<FrP>(ld_canon(p.q_4, i), w[3]));
    g = fe_add<FrP>(g, ld_canon(p.q_c, i));
    if (p.q_arith) g = fe_mul<FrP>(fe_norm<FrP>(g), to_dev(ld_canon(p.q_arith, i)));   // ABI x device -> ABI (1, <2)
    if (WIDGETS) {
      // the rows' other gate kinds; "next" = the same polynomial at w X = index + 4 on the 4n coset
      const Fr a = w[0], b = w[1], c = w[2], d = w[3];
      const Fr an = to_dev(ld_canon(PLANAR && in_halo ? L.halo_w[0] : p.w[0], inext)),
               bn = to_dev(ld_canon(PLANAR && in_halo ? L.halo_w[1] : p.w[1], inext)),
               dn = to_dev(ld_canon(PLANAR && in_halo ? L.halo_w[3] : p.w[3], inext));
      Fr wsum = fe_zero<FrP>();
      if (p.q_range) {
        Fr t = wdelta(wsub(c, wmul4(d)), wc);
        t = wadd(t, wmul(wdelta(wsub(b, wmul4(c)), wc), fr_limbs(wc.range_k[0])));
        t = wadd(t, wmul(wdelta(wsub(a, wmul4(b)), wc), fr_limbs(wc.range_k[1])));
        t = wadd(t, wmul(wdelta(wsub(dn, wmul4(a)), wc), fr_limbs(wc.range_k[2])));
        t = wmul(t, fr_limbs(wc.range_sep));
        wsum = wadd(wsum, wmul(to_dev(ld_canon(p.q_range, i)), t));
      }
      if (p.q_logic) {
        const Fr qa = wsub(an, wmul4(a)), qb = wsub(bn, wmul4(b)), qd = wsub(dn, wmul4(d));
        const Fr qc = to_dev(ld_canon(p.q_c, i));
        Fr t = wdelta(qa, wc);
        t = wadd(t, wmul(wdelta(qb, wc), fr_limbs(wc.logic_k[0])));
        t = wadd(t, wmul(wdelta(qd, wc), fr_limbs(wc.logic_k[1])));
        t = wadd(t, wmul(wsub(c, wmul(qa, qb)), fr_limbs(wc.logic_k[2])));
        // delta_xor_and(qa, qb, w = c, qd, q_c)
        const Fr s = wadd(qa, qb);
        Fr in = wadd(wsub(wmul4(c), wmul2(wmul9(s))), fr_limbs(wc.c81));                         // 4w - 18(a+b) + 81
        in = wadd(wmul(c, in), wmul2(wmul9(wadd(wsqr(qa), wsqr(qb)))));                          // w(..) + 18(a^2+b^2)
        in = wadd(wsub(in, wmul(s, fr_limbs(wc.c81))), fr_limbs(wc.c83));                        // - 81(a+b) + 83
        const Fr ff = wmul(c, in);
        const Fr e = wsub(wmul3(wadd(s, qd)), wadd(ff, ff));                                    // 3(a+b+c) - 2f
        const Fr bb = wmul(qc, wsub(wmul9(qd), wmul3(s)));                                      // q_c (9c - 3(a+b))
        t = wadd(t, wmul(wadd(bb, e), fr_limbs(wc.logic_k[3])));
        t = wmul(t, fr_limbs(wc.logic_sep));
        wsum = wadd(wsum, wmul(to_dev(ld_canon(p.q_logic, i)), t));
      }
      if (p.q_fixed) {
        const Fr xb = to_dev(ld_canon(p.q_l, i)), yb = to_dev(ld_canon(p.q_r, i)), xyb = to_dev(ld_canon(p.q_c, i));
        const Fr one = fr_limbs(wc.c1);
        const Fr bit = wsub(dn, wadd(d, d));
        Fr t = wmul(wmul(bit, wsub(bit, one)), wadd(bit, one));                                 // bit (bit-1)(bit+1)
        const Fr ya = wadd(wmul(wsqr(bit), wsub(yb, one)), one);
        const Fr xa = wmul(xb, bit);
        t = wadd(t, wmul(wsub(wmul(bit, xyb), c), fr_limbs(wc.fixed_k[0])));
        const Fr dxy = wmul(wmul(wmul(c, a), b), fr_limbs(wc.edwards_d));
        const Fr xacc = wsub(wadd(an, wmul(an, dxy)), wadd(wmul(a, ya), wmul(b, xa)));
        const Fr yacc = wsub(wsub(bn, wmul(bn, dxy)), wadd(wmul(b, ya), wmul(a, xa)));
        t = wadd(t, wmul(xacc, fr_limbs(wc.fixed_k[1])));
        t = wadd(t, wmul(yacc, fr_limbs(wc.fixed_k[2])));
        t = wmul(t, fr_limbs(wc.fixed_sep));
        wsum = wadd(wsum, wmul(to_dev(ld_canon(p.q_fixed, i)), t));
      }
      if (p.q_var) {
        const Fr y1x2 = wmul(b, c), y1y2 = wmul(b, d), x1x2 = wmul(a, c);
        Fr t = wsub(wmul(a, d), dn);                                                             // x1 y2 - x1y2
        const Fr dd = wmul(wmul(dn, y1x2), fr_limbs(wc.edwards_d));
        const Fr x3 = wsub(wadd(dn, y1x2), wadd(an, wmul(an, dd)));
        const Fr y3 = wsub(wadd(y1y2, x1x2), wsub(bn, wmul(bn, dd)));
        t = wadd(t, wmul(x3, fr_limbs(wc.var_k[0])));
        t = wadd(t, wmul(y3, fr_limbs(wc.var_k[1])));
        t = wmul(t, fr_limbs(wc.var_sep));
        wsum = wadd(wsum, wmul(to_dev(ld_canon(p.q_var, i)), t));
      }
      g = fe_add<FrP>(g, wmul(wsum, fr_limbs(kc.one_abi)));                                      // device x 2^256 -> ABI
    }
    g = fe_norm<FrP>(fe_add<FrP>(g, ld_canon(p.pi, i)));   // limbs back to (1)
    // permutation identity
    const Fr x = ld_canon(p.x, i);
    const Fr z = ld_canon(p.z, i);
#pragma unroll
    for (int j = 0; j < 4; ++j) f[j] = perm_factor(w[j], x, kc.beta_k[j], gamma);
    const Fr idz = fe_mul<FrP>(z, prod4(f[0], f[1], f[2], f[3]));                          // ABI (1, <2)
#pragma unroll
    for (int j = 0; j < 4; ++j) f[j] = perm_factor(w[j], ld_canon(p.s[j], i), kc.beta, gamma);
    const Fr cpz = fe_mul<FrP>(ld_canon(PLANAR && in_halo ? L.halo_z : p.z, inext), prod4(f[0], f[1], f[2], f[3]));   // ABI (1, <2)
    // idz - cpz + 3r: (4, <5); times alpha -> ABI (1, <2)
    g = fe_add<FrP>(g, fe_mul<FrP>(fe_sub<FrP, 3, 1>(idz, cpz), fr_limbs(kc.alpha)));
    // (z - 1) l1 alpha^2:  z - 1 + 2r is (4, <3); product with ABI l1 is 2^251, alpha2 restores 2^256
    const Fr zm1 = fe_sub<FrP, 2, 1>(z, fr_limbs(kc.one_abi));
    g = fe_add<FrP>(g, fe_mul<FrP>(fe_mul<FrP>(zm1, ld_canon(p.l1, i)), fr_limbs(kc.alpha2)));
    // g: value < 18 r, limbs < 3 * 2^29 + 16
    st_canon(p.out, i, fe_mul<FrP>(g, zhi));
  }
}

// sigma_j(w^i) = k_j' w^i' for a slice of the copy permutation given as wire positions q = j' n + i' (preprocessing; r01 - r04
// gathered these on the host: 4 n field products or a 4 n x 32-byte round trip through host memory)
struct SigmaConsts {
  u32 ks[4][9];   // 1, k_1, k_2, k_3 in device form
};
__global__ void __launch_bounds__(256) sigma_eval_kernel(const long long* idx, size_t count, const u32x4* tlo, const u32x4* thi, u32 h,
                                                         u32 log_n, const SigmaConsts kc, u32x4* out) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  const size_t mask_n = ((size_t)1 << log_n) - 1, mask_lo = ((size_t)1 << h) - 1;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += stride) {
    const size_t q = (size_t)idx[i], jj = (q >> log_n) & 3, ii = q & mask_n;
    Fr v = fe_mul<FrP>(ld_canon(tlo, ii & mask_lo), to_dev(ld_canon(thi, ii >> h)));   // ABI x device -> ABI, (1, <2)
    const Fr k = jj == 0 ? fr_limbs(kc.ks[0]) : (jj == 1 ? fr_limbs(kc.ks[1]) : (jj == 2 ? fr_limbs(kc.ks[2]) : fr_limbs(kc.ks[3])));
    st_canon(out, i, fe_mul<FrP>(v, k));
  }
}

// The distributed prover's way onto the 4n coset (prover_dist.hip.h): out[(4 j + s) m + i] = src_j[i] g_s^(lo + i) for the P
// polynomials of a batch and the four sub-cosets -- the inputs of 4 P size-n transforms over the ranks, one launch.
struct CosetExpandArgs {
  const u32x4* src[8];
  u32 count;
};
__global__ void __launch_bounds__(256) coset_expand_kernel(const CosetExpandArgs a, const u32x4* gs_pow /* [4][m] */, size_t m,
                                                           u32x4* out) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += stride) {
    Fr g[4];
#pragma unroll
    for (int s_ = 0; s_ < 4; ++s_) g[s_] = to_dev(ld_canon(gs_pow, (size_t)s_ * m + i));
    for (u32 j = 0; j < a.count; ++j) {
      const Fr v = ld_canon(a.src[j], i);
#pragma unroll
      for (int s_ = 0; s_ < 4; ++s_) st_canon(out, ((size_t)4 * j + s_) * m + i, fe_mul<FrP>(v, g[s_]));   // ABI x device -> ABI
    }
  }
}
static HFr load_fr(const uint64_t v[4]) {
  HFr r;
  memcpy(r.l, v, 32);
  return r;
}
static void fill_round_consts(RoundConsts& kc, const HFr& alpha, const HFr& beta, const HFr& gamma,
                              const uint64_t k[3][4], const uint64_t zh_inv[4][4]) {
  const host::Field<4>& F = host::FR();
  memset(&kc, 0, sizeof kc);
  to_limbs29_shift(kc.beta_k[0], beta, 2);
  for (int j = 0; j < 3; ++j) to_limbs29_shift(kc.beta_k[j + 1], host::mul(beta, load_fr(k[j]), F), 2);
  to_limbs29_shift(kc.beta, beta, 2);
  to_limbs29_shift(kc.gamma, gamma, 1);
  to_limbs29_shift(kc.alpha, alpha, 1);
  to_limbs29_shift(kc.alpha2, host::mul(alpha, alpha, F), 2);
  to_limbs29_shift(kc.one_abi, host::one(F), 0);
  if (zh_inv)
    for (int j = 0; j < 4; ++j) to_limbs29_shift(kc.zh_inv[j], load_fr(zh_inv[j]), 1);
}
static void fill_widget_consts(WidgetConsts& wc, const pm_plonk_quotient_args* args, bool widgets) {
  memset(&wc, 0, sizeof wc);
  if (!widgets) return;
  const host::Field<4>& F = host::FR();
  auto dev = [&](u32* dst, const HFr& v) { to_limbs29_shift(dst, v, 1); };
  const struct { u32* dst; u64 v; } small[] = {{wc.c1, 1}, {wc.c2, 2}, {wc.c3, 3}, {wc.c4, 4}, {wc.c9, 9},
                                               {wc.c18, 18}, {wc.c81, 81}, {wc.c83, 83}};
  for (const auto& c : small) dev(c.dst, host::from_u64(c.v, F));
  // JubJub d = -(10240 / 10241)
  dev(wc.edwards_d, host::sub(host::zero<4>(), host::mul(host::from_u64(10240, F), host::inv(host::from_u64(10241, F), F), F), F));
  auto sep_powers = [&](const uint64_t sep[4], u32* s_out, u32 (*k_out)[9], int nk) {
    const HFr s_ = load_fr(sep), kappa = host::mul(s_, s_, F);
    dev(s_out, s_);
    HFr kp = kappa;
    for (int i = 0; i < nk; ++i) {
      dev(k_out[i], kp);
      kp = host::mul(kp, kappa, F);
    }
  };
  sep_powers(args->range_sep, wc.range_sep, wc.range_k, 3);
  sep_powers(args->logic_sep, wc.logic_sep, wc.logic_k, 4);
  sep_powers(args->fixed_sep, wc.fixed_sep, wc.fixed_k, 3);
  sep_powers(args->var_sep, wc.var_sep, wc.var_k, 2);
}
static unsigned grid_for(const pm_ctx* ctx, size_t n) {
  return (unsigned)std::min<size_t>((n + 255) / 256, (size_t)ctx->num_cus * 16);
}

// the device pointers of the C ABI's argument structs, as the kernels take them
static PermPtrs perm_ptrs(const pm_plonk_perm_args& a, void* d_num, void* d_den) {
  PermPtrs p;
  for (int j = 0; j < 4; ++j) {
    p.w[j] = (const u32x4*)a.wires[j];
    p.s[j] = (const u32x4*)a.sigmas[j];
  }
  p.roots = (const u32x4*)a.roots;
  p.num = (u32x4*)d_num;
  p.den = (u32x4*)d_den;
  return p;
}
static QuotPtrs quot_ptrs(const pm_plonk_quotient_args& a, void* d_out) {
  QuotPtrs p;
  for (int j = 0; j < 4; ++j) {
    p.w[j] = (const u32x4*)a.wires[j];
    p.s[j] = (const u32x4*)a.sigmas[j];
  }
  p.z = (const u32x4*)a.z;
  p.q_m = (const u32x4*)a.q_m;
  p.q_l = (const u32x4*)a.q_l;
  p.q_r = (const u32x4*)a.q_r;
  p.q_o = (const u32x4*)a.q_o;
  p.q_4 = (const u32x4*)a.q_4;
  p.q_c = (const u32x4*)a.q_c;
  p.q_arith = (const u32x4*)a.q_arith;
  p.q_range = (const u32x4*)a.q_range;
  p.q_logic = (const u32x4*)a.q_logic;
  p.q_fixed = (const u32x4*)a.q_fixed_group_add;
  p.q_var = (const u32x4*)a.q_variable_group_add;
  p.pi = (const u32x4*)a.pi;
  p.l1 = (const u32x4*)a.l1;
  p.x = (const u32x4*)a.x;
  p.out = (u32x4*)d_out;
  return p;
}

int coset_expand(pm_ctx* ctx, const void* const* d_src, uint32_t count, const void* d_gs_pow, size_t m, void* d_out) {
  if (!ctx || !d_src || count == 0 || count > 8 || !d_gs_pow || !d_out) return PM_ERR_BAD_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  CosetExpandArgs a;
  memset(&a, 0, sizeof a);
  a.count = count;
  for (uint32_t j = 0; j < count; ++j) a.src[j] = (const u32x4*)d_src[j];
  PM_HIP(ctx, hipSetDevice(ctx->device));
  ProfScope prof(ctx, ctx->stream, "plonk_coset_expand");
  hipLaunchKernelGGL(coset_expand_kernel, dim3(grid_for(ctx, m)), dim3(256), 0, ctx->stream, a, (const u32x4*)d_gs_pow, m,
                     (u32x4*)d_out);
  PM_HIP(ctx, hipGetLastError());
  return PM_OK;
}

// out[p] = k_j' w^i' for p < count, q = d_idx[p] = j' n + i' (device indices, every one in [0, 4n)): two-level tables of w
// (2 sqrt(n) entries) built on the device, one gather kernel.  Synchronises the context before it returns.
int sigma_evals_from_index_dev(pm_ctx* ctx, const void* d_idx, size_t count, uint32_t log_n, const uint64_t omega[4],
                               const uint64_t k[3][4], void* d_out) {
  if (!ctx || !d_idx || !omega || !k || !d_out) return PM_ERR_BAD_ARG;
  if (count == 0) return PM_OK;
  const host::Field<4>& F = host::FR();
  const uint32_t h = (log_n + 1) / 2;
  const size_t nlo = (size_t)1 << h, nhi = (size_t)1 << (log_n - h);
  void *d_lo = nullptr, *d_hi = nullptr;
  struct Free2 {
    pm_ctx* c;
    void **a, **b;
    ~Free2() {
      for (void** p : {a, b})
        if (*p) (void)pm_dev_free(c, *p);
    }
  } free2{ctx, &d_lo, &d_hi};
  int rc = pm_dev_alloc(ctx, nlo * 32, &d_lo);
  if (!rc) rc = pm_dev_alloc(ctx, nhi * 32, &d_hi);
  if (rc) return rc;
  const HFr w = load_fr(omega), one = host::one(F);
  host::u64 e[1] = {(host::u64)nlo};
  const HFr step = host::pow<4>(w, e, 1, F);
  rc = pm_fr_powers_dev(ctx, w.l, one.l, nlo, d_lo, nullptr);
  if (!rc) rc = pm_fr_powers_dev(ctx, step.l, one.l, nhi, d_hi, nullptr);
  if (rc) return rc;
  {
    std::lock_guard<std::mutex> lk(ctx->mu);
    SigmaConsts kc;
    to_limbs29_shift(kc.ks[0], one, 1);
    for (int j = 0; j < 3; ++j) to_limbs29_shift(kc.ks[j + 1], load_fr(k[j]), 1);
    PM_HIP(ctx, hipSetDevice(ctx->device));
    ProfScope prof(ctx, ctx->stream, "plonk_sigma_evals");
    hipLaunchKernelGGL(sigma_eval_kernel, dim3(grid_for(ctx, count)), dim3(256), 0, ctx->stream, (const long long*)d_idx, count,
                       (const u32x4*)d_lo, (const u32x4*)d_hi, h, log_n, kc, (u32x4*)d_out);
    PM_HIP(ctx, hipGetLastError());
  }
  return pm_sync(ctx);   // the temporaries go away when this returns
}

// The same from host indices (already range-checked by the caller).
int sigma_evals_from_index(pm_ctx* ctx, const int64_t* idx, size_t count, uint32_t log_n, const uint64_t omega[4],
                           const uint64_t k[3][4], void* d_out) {
  if (!ctx || !idx || !omega || !k || !d_out) return PM_ERR_BAD_ARG;
  if (count == 0) return PM_OK;
  void* d_idx = nullptr;
  int rc = pm_dev_alloc(ctx, count * 8, &d_idx);
  if (!rc) rc = pm_dev_upload(ctx, d_idx, idx, count * 8);
  if (!rc) rc = sigma_evals_from_index_dev(ctx, d_idx, count, log_n, omega, k, d_out);
  if (d_idx) (void)pm_dev_free(ctx, d_idx);
  return rc;
}

// ---- launchers of the proof-batched forms (pm_plonk_prove_batch, prover_batch.hip.h).  Each stages its per-proof
// constants in `stage` (pinned host -> device table, one async copy) and launches once for all `batch` proofs on `st`.
int perm_terms_batch(pm_ctx* ctx, ConstStage& stage, const pm_plonk_perm_args* args, uint32_t batch, size_t wire_stride,
                     size_t n, void* d_num, void* d_den, hipStream_t st) {
  std::lock_guard<std::mutex> lk(ctx->mu);
  const PermPtrs p = perm_ptrs(args[0], d_num, d_den);
  RoundConsts* h;
  void* d;
  if (!stage.take(sizeof(RoundConsts) * batch, (void**)&h, &d)) return set_err(ctx, PM_ERR_OOM, "constant table full");
  for (uint32_t b = 0; b < batch; ++b)
    fill_round_consts(h[b], host::zero<4>(), load_fr(args[b].beta), load_fr(args[b].gamma), args[b].k, nullptr);
  PM_HIP(ctx, hipSetDevice(ctx->device));
  PM_HIP(ctx, hipMemcpyAsync(d, h, sizeof(RoundConsts) * batch, hipMemcpyHostToDevice, st));
  ProfScope prof(ctx, st, "plonk_perm_terms_batch");
  hipLaunchKernelGGL(perm_terms_kernel<FromTable<RoundConsts>>, dim3(grid_for(ctx, n), batch), dim3(256), 0, st, p,
                     FromTable<RoundConsts>{(const PM_KCONST RoundConsts*)d}, n, wire_stride);
  PM_HIP(ctx, hipGetLastError());
  return PM_OK;
}

int quotient_batch(pm_ctx* ctx, ConstStage& stage, const pm_plonk_quotient_args* args, uint32_t batch, size_t wire_stride,
                   size_t one_stride, size_t n, void* d_out, hipStream_t st) {
  std::lock_guard<std::mutex> lk(ctx->mu);
  const QuotPtrs p = quot_ptrs(args[0], d_out);
  const bool widgets = p.q_range || p.q_logic || p.q_fixed || p.q_var;
  RoundConsts* hk;
  WidgetConsts* hw;
  void *dk, *dw;
  if (!stage.take(sizeof(RoundConsts) * batch, (void**)&hk, &dk) || !stage.take(sizeof(WidgetConsts) * batch, (void**)&hw, &dw))
    return set_err(ctx, PM_ERR_OOM, "constant table full");
  for (uint32_t b = 0; b < batch; ++b) {
    fill_round_consts(hk[b], load_fr(args[b].alpha), load_fr(args[b].beta), load_fr(args[b].gamma), args[b].k, args[b].zh_inv);
    fill_widget_consts(hw[b], &args[b], widgets);
  }
  PM_HIP(ctx, hipSetDevice(ctx->device));
  // the two tables are adjacent regions of the stage: one copy
  PM_HIP(ctx, hipMemcpyAsync(dk, hk, (char*)hw - (char*)hk + sizeof(WidgetConsts) * batch, hipMemcpyHostToDevice, st));
  ProfScope prof(ctx, st, "plonk_quotient_batch");
  const dim3 grid(grid_for(ctx, 4 * n), batch);
  const ProofTable src{(const PM_KCONST RoundConsts*)dk, (const PM_KCONST WidgetConsts*)dw, wire_stride, one_stride};
  if (widgets)
    hipLaunchKernelGGL((quotient_kernel<true, false, ProofTable>), grid, dim3(256), 0, st, p, src, 4 * n, 4 * n, QuotLayout{});
  else
    hipLaunchKernelGGL((quotient_kernel<false, false, ProofTable>), grid, dim3(256), 0, st, p, src, 4 * n, 4 * n, QuotLayout{});
  PM_HIP(ctx, hipGetLastError());
  return PM_OK;
}

int lincomb_batch(pm_ctx* ctx, ConstStage& stage, uint32_t k, const void* const* d_vecs, const size_t* strides,
                  const uint64_t* coeffs /* [batch][k][4] */, uint32_t batch, size_t n, void* d_out, size_t out_stride,
                  hipStream_t st) {
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (k == 0 || k > PM_LINCOMB_MAX) return set_err(ctx, PM_ERR_BAD_ARG, "k must be in 1..PM_LINCOMB_MAX");
  LincombArgs a;
  memset(&a, 0, sizeof a);
  a.k = k;
  for (uint32_t j = 0; j < k; ++j) {
    a.v[j] = (const u32x4*)d_vecs[j];
    a.stride[j] = strides[j];
  }
  u32(*h)[9];
  void* d;
  if (!stage.take(36 * (size_t)k * batch, (void**)&h, &d)) return set_err(ctx, PM_ERR_OOM, "constant table full");
  for (size_t i = 0; i < (size_t)k * batch; ++i) to_limbs29_shift(h[i], load_fr(coeffs + 4 * i), 1);
  PM_HIP(ctx, hipSetDevice(ctx->device));
  PM_HIP(ctx, hipMemcpyAsync(d, h, 36 * (size_t)k * batch, hipMemcpyHostToDevice, st));
  ProfScope prof(ctx, st, "fr_lincomb_batch");
  hipLaunchKernelGGL(lincomb_kernel<CoeffTable>, dim3(grid_for(ctx, n), batch), dim3(256), 0, st, a,
                     CoeffTable{(const PM_KCONST u32(*)[9])d}, (u32x4*)d_out, out_stride, n);
  PM_HIP(ctx, hipGetLastError());
  return PM_OK;
}

// ---- zero-knowledge mode (pm_plonk_prove_zk; the batch: pm_plonk_prove_batch_zk, section 7.2c).
// Coefficient vectors live at a padded stride S = n + PM_ZK_PAD.  One proof's blinders arrive as kernel arguments (canonical
// Montgomery limbs), never through host round trips.  A batch's blinders (64 x 17 x 32 bytes) are beyond the kernel
// arguments: they are a device table in the constant address space, like the per-proof challenges, and a kernel fetches the
// few it needs with the wave-uniform proof index (scalar loads) before it picks one per lane with selects.
struct ZkBlinders {
  u32 b[PM_PLONK_ZK_BLINDERS][8];   // canonical Montgomery limbs, as the caller passed them
};
PM_DEV Fr zk_pick3(const Fr& c0, const Fr& c1, const Fr& c2, u32 i) {   // one of three uniform candidates, i per lane
  Fr r;
#pragma unroll
  for (int l = 0; l < 9; ++l) r.l[l] = i == 0 ? c0.l[l] : (i == 1 ? c1.l[l] : c2.l[l]);
  return r;
}
// three consecutive blinders of proof b from `first` on, the i-th picked per lane
PM_DEV Fr zk_blinder(const PM_KCONST ZkBlinders* bl, u32 b, u32 first, u32 i) {
  const ZkBlinders& mine = kconst(bl, b);
  return zk_pick3(fe_unpack<FrP>(mine.b[first]), fe_unpack<FrP>(mine.b[first + 1]), fe_unpack<FrP>(mine.b[first + 2]), i);
}

// Which vector blockIdx.y = v of a blinding launch is, how many blinder terms it takes and what they are.  BlindArgs: all
// three in the arguments.  BlindTable: vector v = b vpp + j of all proofs, the blinders of wire first_wire + j of proof b --
// a b c d z take 3 3 2 3 3 blinders from b_0, b_3, b_6, b_8, b_11 on (first + 2 <= 13: inside the table for c too).
struct BlindArgs {
  ZkBlindArgs a;
  PM_DEV u32x4* vec(u32 v) const { return (u32x4*)a.v[v]; }
  PM_DEV u32 terms(u32 v) const { return a.terms[v]; }
  PM_DEV Fr blinder(u32 v, u32 t) const { return fe_unpack<FrP>((const u32*)a.beta[v][t]); }
};
struct BlindTable {
  const PM_KCONST ZkBlinders* bl;
  u32x4* vecs;
  u32 vpp, first_wire;
  size_t S;
  PM_DEV u32 wire(u32 v) const { return first_wire + v % vpp; }
  PM_DEV u32x4* vec(u32 v) const { return vecs + 2 * (size_t)v * S; }
  PM_DEV u32 terms(u32 v) const { return wire(v) == 2 ? 2u : 3u; }
  PM_DEV Fr blinder(u32 v, u32 t) const {
    const u32 w = wire(v);
    return zk_blinder(bl, v / vpp, w < 3 ? 3 * w : (w == 3 ? 8u : 11u), t);
  }
};
// w(X) + (beta_0 + ... + beta_{t-1} X^{t-1}) Z_H(X) in place: coefficient i < t loses beta_i, coefficient n + i becomes
// beta_i, and the rest of the tail [n, S) is zeroed.  One block per vector (blockIdx.y), S - n <= 64 threads busy.
template <class Src>
__global__ void __launch_bounds__(64) zk_blind_kernel(const Src src, size_t n, size_t tail) {
  const u32 v = blockIdx.y, t = threadIdx.x;
  u32x4* p = src.vec(v);
  const u32 terms = src.terms(v);
  const Fr beta = t < terms ? src.blinder(v, t) : fe_zero<FrP>();
  if (t < tail) st_canon(p, n + t, beta);
  if (t < terms) st_canon(p, t, wsub(ld_canon(p, t), beta));
}
int zk_blind(pm_ctx* ctx, const ZkBlindArgs& a, uint32_t count, size_t n, size_t stride, hipStream_t st) {
  if (count == 0 || count > ZK_MAX_VECS || stride < n || stride - n > 64 || n < ZK_MAX_TERMS) return PM_ERR_BAD_ARG;
  for (uint32_t v = 0; v < count; ++v)
    if (!a.v[v] || a.terms[v] > ZK_MAX_TERMS || a.terms[v] > stride - n) return PM_ERR_BAD_ARG;
  if (!st) st = ctx->stream;   // as in every entry point: no stream = the context's own
  PM_HIP(ctx, hipSetDevice(ctx->device));
  ProfScope prof(ctx, st, "plonk_zk_blind");
  hipLaunchKernelGGL(zk_blind_kernel<BlindArgs>, dim3(1, count), dim3(64), 0, st, BlindArgs{a}, n, stride - n);
  PM_HIP(ctx, hipGetLastError());
  return PM_OK;
}
int zk_blind_batch(pm_ctx* ctx, const void* d_blinders, void* d_vecs, uint32_t vpp, uint32_t first_wire, uint32_t batch, size_t n,
                   size_t stride, hipStream_t st) {
  if (!d_blinders || !d_vecs || vpp == 0 || first_wire + vpp > 5 || batch == 0 || stride < n + ZK_MAX_TERMS || stride - n > 64 ||
      n < ZK_MAX_TERMS)
    return PM_ERR_BAD_ARG;
  if (!st) st = ctx->stream;
  PM_HIP(ctx, hipSetDevice(ctx->device));
  ProfScope prof(ctx, st, "plonk_zk_blind_batch");
  hipLaunchKernelGGL(zk_blind_kernel<BlindTable>, dim3(1, batch * vpp), dim3(64), 0, st,
                     BlindTable{(const PM_KCONST ZkBlinders*)d_blinders, (u32x4*)d_vecs, vpp, first_wire, stride}, n, stride - n);
  PM_HIP(ctx, hipGetLastError());
  return PM_OK;
}

// dst_j[i] = src_j[i] w_8n^i, i < len: p(X) -> p(w_8n X), whose 7 H_4n coset transform is p on the second coset
// 7 w_8n H_4n.  One pass for the whole batch; w8[i] = w_8n^i in ABI form.
__global__ void __launch_bounds__(256) zk_shift_kernel(const ZkShiftArgs a, const u32x4* w8, size_t len) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < len; i += stride) {
    const Fr w = to_dev(ld_canon(w8, i));
    for (u32 j = 0; j < a.count; ++j) st_canon((u32x4*)a.dst[j], i, fe_mul<FrP>(ld_canon((const u32x4*)a.src[j], i), w));   // ABI x device -> ABI
  }
}
int zk_shift(pm_ctx* ctx, const ZkShiftArgs& a, const void* d_w8, size_t len, hipStream_t st) {
  if (a.count == 0 || a.count > ZK_MAX_SHIFT || !d_w8) return PM_ERR_BAD_ARG;
  for (uint32_t j = 0; j < a.count; ++j)
    if (!a.src[j] || !a.dst[j]) return PM_ERR_BAD_ARG;
  if (len == 0) return PM_OK;
  if (!st) st = ctx->stream;
  PM_HIP(ctx, hipSetDevice(ctx->device));
  ProfScope prof(ctx, st, "plonk_zk_shift");
  hipLaunchKernelGGL(zk_shift_kernel, dim3(grid_for(ctx, len)), dim3(256), 0, st, a, (const u32x4*)d_w8, len);
  PM_HIP(ctx, hipGetLastError());
  return PM_OK;
}

// The quotient blinders b_14 .. b_16 of the proof a combine launch works on, and which of how many proofs that is.  One
// proof: the blinders sit in the arguments and are read where they are used, with the lane's index.  Proof blockIdx.y of
// gridDim.y: a table row takes a uniform index only (scalar loads), so the kernel fetches the three once, ahead of the element
// loop, into locals of its own and picks one per lane with zk_pick3 (FETCH_ONCE).  Held in a struct or behind a reference
// instead of three locals they go to scratch, 112 bytes per lane.
struct QuotBlindArgs {
  u32 beta[3][8];
  static constexpr bool FETCH_ONCE = false;
  static PM_DEV u32 slot() { return 0; }
  static PM_DEV u32 count() { return 1; }
  PM_DEV Fr blinder(u32 k) const { return fe_unpack<FrP>(beta[k]); }
};
struct QuotBlindTable {
  const PM_KCONST ZkBlinders* bl;
  static constexpr bool FETCH_ONCE = true;
  static PM_DEV u32 slot() { return blockIdx.y; }
  static PM_DEV u32 count() { return gridDim.y; }
  PM_DEV Fr blinder(u32 k) const { return fe_unpack<FrP>(kconst(bl, blockIdx.y).b[14 + k]); }
};
// The quotient t' (degree < 4n + ZK_P1_LEN) from A = t' mod (X^4n - s) and B = t' mod (X^4n + s), s = 7^4n: A is 4n
// coefficients at ab + 4n b and B(X / w_8n) (the plain coset inverse of the second-coset values) 4n at ab + 4n (batch + b), so
// B_j = B(X / w_8n)_j w_8n^-j with w_8n^-j = -w_8n^(4n - j) for j > 0.  t' = P0 + X^4n P1, P0 = (A + B) / 2, P1 = (A - B) / 2s.
// Writes the four pieces at stride S (t + 4 S b) with the X^n blinders: t_1 + b_14 X^n, t_2 - b_14 + b_15 X^n,
// t_3 - b_15 + b_16 X^n, t_4 - b_16 (t_4 = coefficients 3n .. 4n + ZK_P1_LEN); every element of the 4 x S output is written.
template <class Src>
__global__ void __launch_bounds__(256) zk_combine_kernel(const Src src, const u32x4* ab, const u32x4* w8, size_t n, size_t S,
                                                         const ZkCombineConsts kc, u32x4* t) {
  const u32 proof = Src::slot(), batch = Src::count();
  const size_t n4 = 4 * n, tail = S - n, total = n4 + 4 * tail;
  const u32x4* a_vec = ab + 2 * (size_t)proof * n4;
  const u32x4* b_vec = ab + 2 * ((size_t)batch + proof) * n4;
  t += 2 * (size_t)proof * 4 * S;
  constexpr bool ONCE = Src::FETCH_ONCE;
  const Fr zero = fe_zero<FrP>(), c0 = ONCE ? src.blinder(0) : zero, c1 = ONCE ? src.blinder(1) : zero, c2 = ONCE ? src.blinder(2) : zero;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += stride) {
    size_t k, i, j;       // output piece, index in it, and the coefficient j < 4n of A and B to combine (if any)
    bool high;            // P1_j (piece 4 beyond n) instead of P0_j
    if (e < n4) {
      j = e;
      k = j / n;
      i = j - k * n;
      high = false;
    } else {
      k = (e - n4) / tail;
      i = n + (e - n4 - k * tail);
      j = i - n;
      high = true;
      if (k < 3 || j >= ZK_P1_LEN) {   // the blinder coefficient X^n of t_1..t_3, zeros elsewhere
        const Fr b = (k < 3 && j == 0) ? (ONCE ? zk_pick3(c0, c1, c2, (u32)k) : src.blinder((u32)k)) : zero;
        st_canon(t, k * S + i, b);
        continue;
      }
    }
    const Fr a_ = ld_canon(a_vec, j);
    const Fr p = fe_mul<FrP>(ld_canon(b_vec, j), to_dev(ld_canon(w8, j ? n4 - j : 0)));   // B_j = p (j = 0), -p (j > 0)
    const bool plus = (j == 0) != high;                                                  // A + B_j or A - B_j
    const Fr s_ = plus ? wadd(a_, p) : wsub(a_, p);
    Fr v = fe_mul<FrP>(s_, fr_limbs(high ? kc.inv2s : kc.inv2));
    if (!high && i == 0 && k > 0) v = wsub(v, ONCE ? zk_pick3(c0, c1, c2, (u32)k - 1) : src.blinder((u32)k - 1));
    st_canon(t, k * S + i, v);
  }
}
static ZkCombineConsts zk_combine_consts(const uint64_t inv2[4], const uint64_t inv2s[4]) {
  ZkCombineConsts kc;
  to_limbs29(kc.inv2, load_fr(inv2));
  to_limbs29(kc.inv2s, load_fr(inv2s));
  return kc;
}
int zk_combine(pm_ctx* ctx, const void* d_ab, const void* d_w8, size_t n, size_t stride, const uint64_t inv2[4],
               const uint64_t inv2s[4], const uint64_t beta[3][4], void* d_t, hipStream_t st) {
  if (!d_ab || !d_w8 || !d_t || 4 * n < ZK_P1_LEN || stride < n + ZK_P1_LEN) return PM_ERR_BAD_ARG;
  QuotBlindArgs src;
  memcpy(src.beta, beta, sizeof src.beta);
  const size_t total = 4 * n + 4 * (stride - n);
  if (!st) st = ctx->stream;
  PM_HIP(ctx, hipSetDevice(ctx->device));
  ProfScope prof(ctx, st, "plonk_zk_combine");
  hipLaunchKernelGGL(zk_combine_kernel<QuotBlindArgs>, dim3(grid_for(ctx, total)), dim3(256), 0, st, src, (const u32x4*)d_ab,
                     (const u32x4*)d_w8, n, stride, zk_combine_consts(inv2, inv2s), (u32x4*)d_t);
  PM_HIP(ctx, hipGetLastError());
  return PM_OK;
}
int zk_combine_batch(pm_ctx* ctx, const void* d_blinders, const void* d_ab, const void* d_w8, uint32_t batch, size_t n, size_t stride,
                     const uint64_t inv2[4], const uint64_t inv2s[4], void* d_t, hipStream_t st) {
  if (!d_blinders || !d_ab || !d_w8 || !d_t || batch == 0 || 4 * n < ZK_P1_LEN || stride < n + ZK_P1_LEN) return PM_ERR_BAD_ARG;
  const size_t total = 4 * n + 4 * (stride - n);
  if (!st) st = ctx->stream;
  PM_HIP(ctx, hipSetDevice(ctx->device));
  ProfScope prof(ctx, st, "plonk_zk_combine_batch");
  hipLaunchKernelGGL(zk_combine_kernel<QuotBlindTable>, dim3(grid_for(ctx, total), batch), dim3(256), 0, st,
                     QuotBlindTable{(const PM_KCONST ZkBlinders*)d_blinders}, (const u32x4*)d_ab, (const u32x4*)d_w8, n, stride,
                     zk_combine_consts(inv2, inv2s), (u32x4*)d_t);
  PM_HIP(ctx, hipGetLastError());
  return PM_OK;
}

// zk_shift_kernel with blockIdx.y = the proof: w_8n^i is fetched and moved to device form once for all the proof's vectors
__global__ void __launch_bounds__(256) zk_shift_batch_kernel(const ZkShiftBatchArgs a, const u32x4* w8, size_t max_len) {
  const u32 b = blockIdx.y;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < max_len; i += stride) {
    const Fr w = to_dev(ld_canon(w8, i));
    for (u32 g = 0; g < a.groups; ++g) {
      if (i >= a.len[g]) continue;
      const size_t off = 2 * (size_t)b * a.vecs[g] * a.stride[g];
      const u32x4* src = (const u32x4*)a.src[g] + off;
      u32x4* dst = (u32x4*)a.dst[g] + off;
      for (u32 v = 0; v < a.vecs[g]; ++v) st_canon(dst + 2 * (size_t)v * a.stride[g], i, fe_mul<FrP>(ld_canon(src + 2 * (size_t)v * a.stride[g], i), w));
    }
  }
}
int zk_shift_batch(pm_ctx* ctx, const ZkShiftBatchArgs& a, const void* d_w8, uint32_t batch, hipStream_t st) {
  if (a.groups == 0 || a.groups > 2 || !d_w8 || batch == 0) return PM_ERR_BAD_ARG;
  size_t max_len = 0;
  for (uint32_t g = 0; g < a.groups; ++g) {
    if (!a.src[g] || !a.dst[g] || a.vecs[g] == 0 || a.len[g] > a.stride[g]) return PM_ERR_BAD_ARG;
    max_len = std::max(max_len, a.len[g]);
  }
  if (max_len == 0) return PM_OK;
  if (!st) st = ctx->stream;
  PM_HIP(ctx, hipSetDevice(ctx->device));
  ProfScope prof(ctx, st, "plonk_zk_shift_batch");
  hipLaunchKernelGGL(zk_shift_batch_kernel, dim3(grid_for(ctx, max_len), batch), dim3(256), 0, st, a, (const u32x4*)d_w8, max_len);
  PM_HIP(ctx, hipGetLastError());
  return PM_OK;
}

// ------------------------------------------------------------------ witness check
// pm_plonk_check_witness: the identities of quotient_kernel on the rows of H -- "next" is row
// i + 1 (the last row's: row 0), the selectors are their values on H -- with every summand a separation challenge joins
// tested on its own, plus the copy constraints as plain equality of the wire values a cycle links.  One mask byte per row.
struct CheckPtrs {
  const u32x4* w;            // [batch][4][n]
  const u32x4 *q_m, *q_l, *q_r, *q_o, *q_4, *q_c;     // nullptr = identically zero
  const u32x4* q_arith;      // nullptr = identically zero, or identically one (arith_is_one)
  const u32x4 *q_range, *q_logic, *q_fixed, *q_var;
  const u32x4* pi;           // [batch][n]
  const u32* sigma;          // [4 n]
  unsigned char* masks;      // [batch][n]
  unsigned long long* counters;
  u32 arith_is_one;
};
// Is the value zero?  What wadd / wsub / wmul return is below 2 r, not below r: a zero may arrive as r, so the test is made on
// the canonical limbs.
PM_DEV bool wnonzero(const Fr& v) {
  u32 s[8];
  fe_canon_pack<FrP>(s, v);
  return (s[0] | s[1] | s[2] | s[3] | s[4] | s[5] | s[6] | s[7]) != 0;
}
// canonical elements in memory, compared or tested as they are stored
PM_DEV bool raw_nonzero(const u32x4* p, size_t i) {
  const u32x4 lo = p[2 * i], hi = p[2 * i + 1];
  return (lo.x | lo.y | lo.z | lo.w | hi.x | hi.y | hi.z | hi.w) != 0;
}
PM_DEV bool raw_differ(const u32x4* p, size_t i, size_t j) {
  const u32x4 a0 = p[2 * i], a1 = p[2 * i + 1], b0 = p[2 * j], b1 = p[2 * j + 1];
  return ((a0.x ^ b0.x) | (a0.y ^ b0.y) | (a0.z ^ b0.z) | (a0.w ^ b0.w) | (a1.x ^ b1.x) | (a1.y ^ b1.y) | (a1.z ^ b1.z) |
          (a1.w ^ b1.w)) != 0;
}
PM_DEV Fr ld_dev_or_zero(const u32x4* p, size_t i) { return p ? to_dev(ld_canon(p, i)) : fe_zero<FrP>(); }

// One thread per row, grid-stride by whole waves (the loop is wave-uniform: the ballots below see all 64 lanes), blockIdx.y =
// the witness.  A widget is evaluated on the rows whose selector is not zero only.  On the way out a wave that saw a failure
// adds its per-reason popcounts and its lowest failing row to the witness's counters: one atomic per wave and counter, none
// at all for a wave of satisfied rows.
template <bool WIDGETS>
__global__ void __launch_bounds__(256) check_witness_kernel(const CheckPtrs p, const WidgetConsts wc, size_t n) {
  const u32 proof = blockIdx.y, lane = threadIdx.x & 63;
  const u32x4* const w = p.w + 2 * (size_t)proof * 4 * n;
  const u32x4* const pi = p.pi + 2 * (size_t)proof * n;
  unsigned char* const masks = p.masks + (size_t)proof * n;
  unsigned long long* const ctr = p.counters + 7 * (size_t)proof;
  unsigned long long* const first = p.counters + 7 * (size_t)gridDim.y + proof;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i0 = (size_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63u); i0 < n; i0 += stride) {
    const size_t i = i0 + lane;
    u32 m = 0;
    if (i < n) {
      const size_t inext = i + 1 < n ? i + 1 : 0;
      const Fr a = to_dev(ld_canon(w, i)), b = to_dev(ld_canon(w, n + i)), c = to_dev(ld_canon(w, 2 * n + i)),
               d = to_dev(ld_canon(w, 3 * n + i));
      {
        // arithmetic identity, device form throughout
        Fr g = ld_dev_or_zero(p.q_c, i);
        if (p.q_m) g = wadd(g, wmul(to_dev(ld_canon(p.q_m, i)), wmul(a, b)));
        if (p.q_l) g = wadd(g, wmul(to_dev(ld_canon(p.q_l, i)), a));
        if (p.q_r) g = wadd(g, wmul(to_dev(ld_canon(p.q_r, i)), b));
        if (p.q_o) g = wadd(g, wmul(to_dev(ld_canon(p.q_o, i)), c));
        if (p.q_4) g = wadd(g, wmul(to_dev(ld_canon(p.q_4, i)), d));
        if (!p.arith_is_one) g = wmul(g, ld_dev_or_zero(p.q_arith, i));
        g = wadd(g, to_dev(ld_canon(pi, i)));
        if (wnonzero(g)) m |= PM_PLONK_FAIL_ARITH;
      }
      if (WIDGETS) {
        const Fr an = to_dev(ld_canon(w, inext)), bn = to_dev(ld_canon(w, n + inext)), dn = to_dev(ld_canon(w, 3 * n + inext));
        if (p.q_range && raw_nonzero(p.q_range, i)) {
          bool f = wnonzero(wdelta(wsub(c, wmul4(d)), wc));
          f |= wnonzero(wdelta(wsub(b, wmul4(c)), wc));
          f |= wnonzero(wdelta(wsub(a, wmul4(b)), wc));
          f |= wnonzero(wdelta(wsub(dn, wmul4(a)), wc));
          if (f) m |= PM_PLONK_FAIL_RANGE;
        }
        if (p.q_logic && raw_nonzero(p.q_logic, i)) {
          const Fr qa = wsub(an, wmul4(a)), qb = wsub(bn, wmul4(b)), qd = wsub(dn, wmul4(d));
          const Fr qc = ld_dev_or_zero(p.q_c, i);
          bool f = wnonzero(wdelta(qa, wc));
          f |= wnonzero(wdelta(qb, wc));
          f |= wnonzero(wdelta(qd, wc));
          f |= wnonzero(wsub(c, wmul(qa, qb)));
          // delta_xor_and(qa, qb, w = c, qd, q_c)
          const Fr s = wadd(qa, qb);
          Fr in = wadd(wsub(wmul4(c), wmul2(wmul9(s))), fr_limbs(wc.c81));                         // 4w - 18(a+b) + 81
          in = wadd(wmul(c, in), wmul2(wmul9(wadd(wsqr(qa), wsqr(qb)))));                          // w(..) + 18(a^2+b^2)
          in = wadd(wsub(in, wmul(s, fr_limbs(wc.c81))), fr_limbs(wc.c83));                        // - 81(a+b) + 83
          const Fr ff = wmul(c, in);
          const Fr e = wsub(wmul3(wadd(s, qd)), wadd(ff, ff));                                    // 3(a+b+c) - 2f
          const Fr bb = wmul(qc, wsub(wmul9(qd), wmul3(s)));                                      // q_c (9c - 3(a+b))
          f |= wnonzero(wadd(bb, e));
          if (f) m |= PM_PLONK_FAIL_LOGIC;
        }
        if (p.q_fixed && raw_nonzero(p.q_fixed, i)) {
          const Fr xb = ld_dev_or_zero(p.q_l, i), yb = ld_dev_or_zero(p.q_r, i), xyb = ld_dev_or_zero(p.q_c, i);
          const Fr one = fr_limbs(wc.c1);
          const Fr bit = wsub(dn, wadd(d, d));
          bool f = wnonzero(wmul(wmul(bit, wsub(bit, one)), wadd(bit, one)));                     // bit (bit-1)(bit+1)
          const Fr ya = wadd(wmul(wsqr(bit), wsub(yb, one)), one);
          const Fr xa = wmul(xb, bit);
          f |= wnonzero(wsub(wmul(bit, xyb), c));
          const Fr dxy = wmul(wmul(wmul(c, a), b), fr_limbs(wc.edwards_d));
          f |= wnonzero(wsub(wadd(an, wmul(an, dxy)), wadd(wmul(a, ya), wmul(b, xa))));
          f |= wnonzero(wsub(wsub(bn, wmul(bn, dxy)), wadd(wmul(b, ya), wmul(a, xa))));
          if (f) m |= PM_PLONK_FAIL_FIXED_BASE;
        }
        if (p.q_var && raw_nonzero(p.q_var, i)) {
          const Fr y1x2 = wmul(b, c), y1y2 = wmul(b, d), x1x2 = wmul(a, c);
          bool f = wnonzero(wsub(wmul(a, d), dn));                                                // x1 y2 - x1y2
          const Fr dd = wmul(wmul(dn, y1x2), fr_limbs(wc.edwards_d));
          f |= wnonzero(wsub(wadd(dn, y1x2), wadd(an, wmul(an, dd))));
          f |= wnonzero(wsub(wadd(y1y2, x1x2), wsub(bn, wmul(bn, dd))));
          if (f) m |= PM_PLONK_FAIL_VAR_BASE;
        }
      }
      // copy constraints: the witness is canonical, so equal values are equal words
      bool cp = false;
#pragma unroll
      for (int j = 0; j < 4; ++j) cp |= raw_differ(w, (size_t)j * n + i, p.sigma[(size_t)j * n + i]);
      if (cp) m |= PM_PLONK_FAIL_COPY;
      masks[i] = (unsigned char)m;
    }
    const unsigned long long failing = __ballot(m != 0);
    if (failing) {   // wave-uniform
#pragma unroll
      for (u32 k = 0; k < 6; ++k) {
        const u32 cnt = (u32)__popcll(__ballot((m >> k) & 1));
        if (lane == 0 && cnt) atomicAdd(ctr + k, (unsigned long long)cnt);
      }
      // rows rise with the lane: the wave's lowest failing row sits in the lowest failing lane
      if (lane == (u32)__ffsll((long long)failing) - 1) {
        atomicAdd(ctr + 6, (unsigned long long)__popcll(failing));
        atomicMin(first, (unsigned long long)i * 64 + m);
      }
    }
  }
}

int check_witness_rows(pm_ctx* ctx, const WitnessCheckArgs& a, size_t n, uint32_t batch, hipStream_t st) {
  if (!ctx || !a.wires || !a.pi || !a.sigma || !a.masks || !a.counters || batch == 0 || batch > PM_PLONK_MAX_BATCH)
    return PM_ERR_BAD_ARG;
  if (n < 4 || (n & (n - 1)) || 4 * n > ((size_t)1 << 32)) return PM_ERR_LENGTH;
  std::lock_guard<std::mutex> lk(ctx->mu);
  CheckPtrs p;
  p.w = (const u32x4*)a.wires;
  const u32x4* sel[PM_PLONK_SELECTORS];
  for (int s_ = 0; s_ < PM_PLONK_SELECTORS; ++s_) sel[s_] = (const u32x4*)a.sel[s_];
  p.q_m = sel[0], p.q_l = sel[1], p.q_r = sel[2], p.q_o = sel[3], p.q_c = sel[4], p.q_4 = sel[5];   // PM_PLONK_SELECTORS order
  p.q_arith = sel[6], p.q_range = sel[7], p.q_logic = sel[8], p.q_fixed = sel[9], p.q_var = sel[10];
  p.pi = (const u32x4*)a.pi;
  p.sigma = a.sigma;
  p.masks = a.masks;
  p.counters = a.counters;
  p.arith_is_one = a.arith_is_one;
  const bool widgets = p.q_range || p.q_logic || p.q_fixed || p.q_var;
  WidgetConsts wc;
  pm_plonk_quotient_args no_challenges;
  memset(&no_challenges, 0, sizeof no_challenges);
  fill_widget_consts(wc, &no_challenges, widgets);   // the small constants and d; the check takes no separation challenge
  if (!st) st = ctx->stream;
  PM_HIP(ctx, hipSetDevice(ctx->device));
  PM_HIP(ctx, hipMemsetAsync(a.counters, 0, 7 * (size_t)batch * 8, st));
  PM_HIP(ctx, hipMemsetAsync(a.counters + 7 * (size_t)batch, 0xff, (size_t)batch * 8, st));
  ProfScope prof(ctx, st, "plonk_check_witness");
  const dim3 grid(grid_for(ctx, n), batch);
  if (widgets) hipLaunchKernelGGL(check_witness_kernel<true>, grid, dim3(256), 0, st, p, wc, n);
  else hipLaunchKernelGGL(check_witness_kernel<false>, grid, dim3(256), 0, st, p, wc, n);
  PM_HIP(ctx, hipGetLastError());
  return PM_OK;
}

__global__ void __launch_bounds__(256) vec_differs_kernel(const u32x4* a, const u32x4* b, size_t vecs, u32* flag) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  bool d = false;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < vecs; i += stride) {
    const u32x4 x = a[i], y = b[i];
    d |= ((x.x ^ y.x) | (x.y ^ y.y) | (x.z ^ y.z) | (x.w ^ y.w)) != 0;
  }
  if (__ballot(d) && (threadIdx.x & 63) == 0) atomicOr(flag, 1u);
}
int vec_differs(pm_ctx* ctx, const void* d_a, const void* d_b, size_t n, uint32_t* d_flag, hipStream_t st) {
  if (!ctx || !d_a || !d_b || !d_flag) return PM_ERR_BAD_ARG;
  if (n == 0) return PM_OK;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (!st) st = ctx->stream;
  PM_HIP(ctx, hipSetDevice(ctx->device));
  hipLaunchKernelGGL(vec_differs_kernel, dim3(grid_for(ctx, 2 * n)), dim3(256), 0, st, (const u32x4*)d_a, (const u32x4*)d_b, 2 * n,
                     d_flag);
  PM_HIP(ctx, hipGetLastError());
  return PM_OK;
}

}  // namespace pm

using namespace pm;

extern "C" int pm_fr_powers_dev(pm_ctx* ctx, const uint64_t base[4], const uint64_t scale[4], size_t n, void* d_out,
                                void* hip_stream) {
  if (!ctx || !base || !scale) return PM_ERR_BAD_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (n == 0) return PM_OK;
  if (!d_out) return set_err(ctx, PM_ERR_BAD_ARG, "null device pointer");
  PM_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t st = hip_stream ? (hipStream_t)hip_stream : ctx->stream;
  const unsigned blocks = grid_for(ctx, n);
  const u64 T = (u64)blocks * 256;
  NttConsts c;
  memset(&c, 0, sizeof c);
  const HFr b = load_fr(base);
  to_limbs29_shift(c.w8[0], b, 1);
  to_limbs29_shift(c.w8[1], hfr_pow_u64(b, T), 1);
  to_limbs29_shift(c.scale, load_fr(scale), 1);
  to_limbs29_shift(c.one, host::one(host::FR()), 0);
  ProfScope prof(ctx, st, "fr_powers");
  hipLaunchKernelGGL(powers_kernel, dim3(blocks), dim3(256), 0, st, (u32x4*)d_out, n, c);
  PM_HIP(ctx, hipGetLastError());
  return PM_OK;
}

extern "C" int pm_fr_lincomb_dev(pm_ctx* ctx, uint32_t k, const void* const* d_vecs, const uint64_t* coeffs, size_t n,
                                 void* d_out, void* hip_stream) {
  if (!ctx) return PM_ERR_BAD_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (k == 0 || k > PM_LINCOMB_MAX) return set_err(ctx, PM_ERR_BAD_ARG, "k must be in 1..PM_LINCOMB_MAX");
  if (n == 0) return PM_OK;
  if (!d_vecs || !coeffs || !d_out) return set_err(ctx, PM_ERR_BAD_ARG, "null pointer");
  LincombArgs a;
  CoeffArgs c;
  memset(&a, 0, sizeof a);
  memset(&c, 0, sizeof c);
  a.k = k;
  for (uint32_t j = 0; j < k; ++j) {
    if (!d_vecs[j]) return set_err(ctx, PM_ERR_BAD_ARG, "null device pointer");
    a.v[j] = (const u32x4*)d_vecs[j];
    to_limbs29_shift(c.c[j], load_fr(coeffs + 4 * j), 1);
  }
  PM_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t st = hip_stream ? (hipStream_t)hip_stream : ctx->stream;
  ProfScope prof(ctx, st, "fr_lincomb");
  hipLaunchKernelGGL(lincomb_kernel<CoeffArgs>, dim3(grid_for(ctx, n)), dim3(256), 0, st, a, c, (u32x4*)d_out, (size_t)0, n);
  PM_HIP(ctx, hipGetLastError());
  return PM_OK;
}

extern "C" int pm_plonk_perm_terms_dev(pm_ctx* ctx, const pm_plonk_perm_args* args, size_t n, void* d_num,
                                       void* d_den, void* hip_stream) {
  if (!ctx) return PM_ERR_BAD_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (!args) return set_err(ctx, PM_ERR_BAD_ARG, "null args");
  if (n == 0) return PM_OK;
  const PermPtrs p = perm_ptrs(*args, d_num, d_den);
  for (int j = 0; j < 4; ++j)
    if (!p.w[j] || !p.s[j]) return set_err(ctx, PM_ERR_BAD_ARG, "null device pointer");
  if (!p.roots || !p.num || !p.den) return set_err(ctx, PM_ERR_BAD_ARG, "null device pointer");
  FromArgs<RoundConsts> src;
  fill_round_consts(src.c, host::zero<4>(), load_fr(args->beta), load_fr(args->gamma), args->k, nullptr);
  PM_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t st = hip_stream ? (hipStream_t)hip_stream : ctx->stream;
  ProfScope prof(ctx, st, "plonk_perm_terms");
  hipLaunchKernelGGL(perm_terms_kernel<FromArgs<RoundConsts>>, dim3(grid_for(ctx, n)), dim3(256), 0, st, p, src, n, (size_t)0);
  PM_HIP(ctx, hipGetLastError());
  return PM_OK;
}

extern "C" int pm_plonk_quotient_dev(pm_ctx* ctx, const pm_plonk_quotient_args* args, size_t n, void* d_out,
                                     void* hip_stream) {
  return pm::plonk_quotient_rows(ctx, args, n, false, d_out, hip_stream);
}
int pm::plonk_quotient_rows(pm_ctx* ctx, const pm_plonk_quotient_args* args, size_t n, bool halo, void* d_out,
                            void* hip_stream) {
  return plonk_quotient_layout(ctx, args, n, halo, nullptr, d_out, hip_stream);
}
int pm::plonk_quotient_layout(pm_ctx* ctx, const pm_plonk_quotient_args* args, size_t n, bool halo, const QuotPlanar* planar,
                              void* d_out, void* hip_stream) {
  if (!ctx) return PM_ERR_BAD_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (!args) return set_err(ctx, PM_ERR_BAD_ARG, "null args");
  if (n == 0) return PM_OK;
  if (n & (n - 1)) return set_err(ctx, PM_ERR_LENGTH, "n must be a power of two");
  const QuotPtrs p = quot_ptrs(*args, d_out);
  const void* all[] = {p.w[0], p.w[1], p.w[2], p.w[3], p.s[0], p.s[1], p.s[2], p.s[3], p.z,  p.q_m,
                       p.q_l,  p.q_r,  p.q_o,  p.q_4,  p.q_c,  p.pi,   p.l1,   p.x,    p.out};
  for (const void* q : all)
    if (!q) return set_err(ctx, PM_ERR_BAD_ARG, "null device pointer");
  const bool widgets = p.q_range || p.q_logic || p.q_fixed || p.q_var;
  OneProof src;
  fill_round_consts(src.kc, load_fr(args->alpha), load_fr(args->beta), load_fr(args->gamma), args->k, args->zh_inv);
  fill_widget_consts(src.wc, args, widgets);
  PM_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t st = hip_stream ? (hipStream_t)hip_stream : ctx->stream;
  ProfScope prof(ctx, st, "plonk_quotient");
  QuotLayout L;
  memset(&L, 0, sizeof L);
  const size_t wrap = 4 * n + (halo ? 4 : 0);
  const dim3 grid(grid_for(ctx, 4 * n));
  if (planar) {
    while (((size_t)1 << L.log_m) < n) ++L.log_m;
    L.n2 = planar->n2;
    L.rot = planar->rot;
    for (int j = 0; j < 4; ++j) L.halo_w[j] = (const u32x4*)planar->halo_w[j];
    L.halo_z = (const u32x4*)planar->halo_z;
    if (!L.halo_z || !L.halo_w[0] || !L.halo_w[1] || !L.halo_w[3] || L.n2 == 0 || (L.n2 & (L.n2 - 1)) || L.n2 > n)
      return set_err(ctx, PM_ERR_BAD_ARG, "planar quotient layout: halo rows missing or row length not a power of two <= rows");
    if (widgets)
      hipLaunchKernelGGL((quotient_kernel<true, true, OneProof>), grid, dim3(256), 0, st, p, src, 4 * n, wrap, L);
    else
      hipLaunchKernelGGL((quotient_kernel<false, true, OneProof>), grid, dim3(256), 0, st, p, src, 4 * n, wrap, L);
  } else if (widgets) {
    hipLaunchKernelGGL((quotient_kernel<true, false, OneProof>), grid, dim3(256), 0, st, p, src, 4 * n, wrap, L);
  } else {
    hipLaunchKernelGGL((quotient_kernel<false, false, OneProof>), grid, dim3(256), 0, st, p, src, 4 * n, wrap, L);
  }
  PM_HIP(ctx, hipGetLastError());
  return PM_OK;
}
