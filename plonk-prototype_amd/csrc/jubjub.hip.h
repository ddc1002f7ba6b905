// JubJub on the device, shared by gadgets.hip (the rows of the curve gadgets) and jubjub.hip (the native calls, DESIGN.md section
// 7.2k): the twisted Edwards curve -x^2 + y^2 = 1 + d x^2 y^2 over Fr, d = -(10240 / 10241), in extended coordinates, with the
// field helpers the group law is written in.  Everything here runs in the device form (x 2^261, poly_common.hip.h).
//
// Affine addends.  ed_madd takes its second operand as (x, y, t) with t = x y; (0, 1, 0) is the neutral addend, so a digit of 0
// selects it (g_sel) and the addition still runs: no branch depends on a digit.  -(x, y, t) = (-x, y, -t).
#pragma once
#include "poly_common.hip.h"

namespace pm {

// ------------------------------------------------------------------ field helpers (operands normalised, values < 2 r)
PM_DEV Fr gadd(const Fr& a, const Fr& b) { return fe_reduce_weak<FrP>(fe_add<FrP>(a, b)); }
PM_DEV Fr gsub(const Fr& a, const Fr& b) { return fe_reduce_weak<FrP>(fe_sub<FrP, 2, 1>(a, b)); }
PM_DEV Fr gmul(const Fr& a, const Fr& b) { return fe_mul<FrP>(a, b); }
PM_DEV Fr gneg(const Fr& a) { return gsub(fe_zero<FrP>(), a); }
PM_DEV Fr g_to_dev(const Fr& abi) { return fe_reduce_weak<FrP>(fr_shl5(abi)); }
PM_DEV Fr g_to_abi(const Fr& dev) { return fe_mul<FrP>(dev, fe_pow2<FrP, 256>()); }          // x 2^261 * 2^256 / 2^261
PM_DEV Fr g_one_abi() { return fe_pow2<FrP, 256>(); }
PM_DEV Fr g_sel(bool c, const Fr& a, const Fr& b) {
  Fr r;
#pragma unroll
  for (int i = 0; i < 9; ++i) r.l[i] = c ? a.l[i] : b.l[i];
  return r;
}

// extended coordinates: x = X / Z, y = Y / Z, T = X Y / Z
struct EdPoint {
  Fr X, Y, Z, T;
};
// unified addition for a = -1 (Hisil, Wong, Carter, Dawson 2008): the projective form of the affine law above, with the same
// exceptional cases -- none on the curve.  9 products.
PM_DEV EdPoint ed_add(const EdPoint& p, const EdPoint& q, const Fr& d) {
  const Fr A = gmul(p.X, q.X), B = gmul(p.Y, q.Y), C = gmul(gmul(p.T, q.T), d), D = gmul(p.Z, q.Z);
  const Fr E = gsub(gsub(gmul(gadd(p.X, p.Y), gadd(q.X, q.Y)), A), B);
  const Fr F = gsub(D, C), G = gadd(D, C), H = gadd(B, A);
  return EdPoint{gmul(E, F), gmul(G, H), gmul(F, G), gmul(E, H)};
}
// the same with an affine second operand (x, y, t = x y): 8 products
PM_DEV EdPoint ed_madd(const EdPoint& p, const Fr& x, const Fr& y, const Fr& t, const Fr& d) {
  const Fr A = gmul(p.X, x), B = gmul(p.Y, y), C = gmul(gmul(p.T, t), d);
  const Fr E = gsub(gsub(gmul(gadd(p.X, p.Y), gadd(x, y)), A), B);
  const Fr F = gsub(p.Z, C), G = gadd(p.Z, C), H = gadd(B, A);
  return EdPoint{gmul(E, F), gmul(G, H), gmul(F, G), gmul(E, H)};
}
PM_DEV EdPoint ed_sel(bool c, const EdPoint& a, const EdPoint& b) {
  return EdPoint{g_sel(c, a.X, b.X), g_sel(c, a.Y, b.Y), g_sel(c, a.Z, b.Z), g_sel(c, a.T, b.T)};
}

// ------------------------------------------------------------------ host: the Edwards d
// JubJub d = -(10240 / 10241), canonical Montgomery: the inversion once, not per call
inline const HFr& jubjub_d_host() {
  const host::Field<4>& F = host::FR();
  static const HFr edwards_d = host::sub(host::zero<4>(), host::mul(host::from_u64(10240, F), host::inv(host::from_u64(10241, F), F), F), F);
  return edwards_d;
}
// ... as the nine 29-bit limbs of the device form, what a kernel's arguments carry
inline void jubjub_d_limbs(u32 (&dst)[9]) { to_limbs29_shift(dst, jubjub_d_host(), 1); }

}  // namespace pm
