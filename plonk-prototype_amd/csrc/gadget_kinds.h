// What a gadget kind IS, once (DESIGN.md sections 7.2f to 7.2i): one record per value of pm_plonk_gadget.kind, read by the host
// checks of pm_plonk_key_set_gadgets, the set-time kernels and the launch of a fill (gadgets.hip).  Plain C++, host and device.
#pragma once
#include <cstdint>

#include "../../include/plonk_mi355x.h"

namespace pm {

enum class GadgetTab : uint8_t { NONE, POINTS, COEF, ROUNDS };              // the gathered array rec.tab indexes, `count` units a gadget
enum class GadgetLaunch : uint8_t { NONE, PER_THREAD, PER_WAVE, BITS_X };   // a thread / a wave per (gadget, proof); bits along x
struct GadgetKind {
  GadgetLaunch launch = GadgetLaunch::NONE;   // NONE: no kind (8, 9 and everything from GADGET_KINDS on)
  // rows = rows_base + rows_per * count + rows_per_param * param (HADES: 18 a round and 12 more a full one, param of them); the
  // last `trailing` of them carry results only: no selector is looked at there
  uint32_t rows_base = 0, rows_per = 0, rows_per_param = 0, trailing = 0;
  uint32_t max_count = 0;           // 0: no limit
  const char* over_max = nullptr;   // the objection to a larger count
  uint32_t max_param = 0;           // without rows_per_param; with it param is even and at most count
  uint32_t in_vars = 0;             // in_var read: each must be below num_vars
  bool all_selectors = false;       // set time needs all eleven selectors on H, not only q_l q_r and the four widget selectors
  GadgetTab tab = GadgetTab::NONE;
  const char* refusal = nullptr;    // what the refusal of a gadget says whose rows the device objects to
};

constexpr uint32_t GADGET_KINDS = PM_PLONK_GADGET_VAR_BASE + 1;
constexpr GadgetKind gadget_kind(uint32_t kind) {
  constexpr const char* rounds = "more than PM_PLONK_GADGET_MAX_ROUNDS rounds";
  constexpr const char* sel = ": a row it claims does not have its kind's selector";
  constexpr const char* arith = ": a row it claims is not the arithmetic row its kind lays out (selectors, coefficients or wire variables)";
  using L = GadgetLaunch;
  constexpr GadgetKind table[GADGET_KINDS] = {
      {.launch = L::PER_THREAD, .rows_base = 1, .rows_per = 1, .trailing = 1, .in_vars = 1, .refusal = sel},   // 0 RANGE
      {.launch = L::PER_THREAD, .rows_base = 1, .rows_per = 1, .trailing = 1, .max_param = 1, .in_vars = 2, .refusal = sel},   // 1 LOGIC: xor
      {.launch = L::PER_WAVE, .rows_base = 1, .rows_per = 1, .trailing = 1, .max_count = PM_PLONK_GADGET_MAX_ROUNDS, .over_max = rounds,
       .in_vars = 1, .tab = GadgetTab::POINTS, .refusal = sel},   // 2 FIXED_BASE
      {.launch = L::PER_THREAD, .rows_base = 2, .trailing = 1, .refusal = sel},   // 3 CURVE_ADD
      {.launch = L::PER_THREAD, .rows_per = 1, .all_selectors = true, .tab = GadgetTab::COEF, .refusal = arith},   // 4 ARITH
      {.launch = L::BITS_X, .rows_per = 2, .max_count = PM_PLONK_COMPOSED_MAX_BITS, .over_max = "more than PM_PLONK_COMPOSED_MAX_BITS bits",
       .in_vars = 1, .all_selectors = true, .refusal = arith},   // 5 BITS
      {.launch = L::PER_THREAD, .rows_base = 3, .all_selectors = true, .refusal = arith},   // 6 MAYBE_EQUAL
      {.launch = L::PER_WAVE, .rows_per = 18, .rows_per_param = 12, .all_selectors = true, .tab = GadgetTab::ROUNDS, .refusal = arith},   // 7 HADES
      {}, {},   // 8, 9: no kinds
      {.launch = L::PER_WAVE, .rows_per = 6, .max_count = PM_PLONK_GADGET_MAX_ROUNDS, .over_max = rounds, .all_selectors = true,
       .refusal = ": a row it claims is not the row a variable-base round lays out (selectors, coefficients or wire variables)"},   // 10 VAR_BASE
  };
  static_assert(PM_PLONK_GADGET_CURVE_ADD == 3 && PM_PLONK_PERMUTATION_HADES == 7 && PM_PLONK_GADGET_VAR_BASE == 10, "indexed by kind");
  return kind < GADGET_KINDS ? table[kind] : GadgetKind{};
}
// the rows a gadget of this kind claims, the trailing ones included; 0: the kind does not take this count (one whose rows do
// not depend on count does not read it) or, with rows_per_param, this param.  max_param is not looked at
constexpr uint64_t gadget_kind_rows(const GadgetKind& k, uint64_t count, uint64_t param) {
  const bool takes = k.launch != GadgetLaunch::NONE && (count || !k.rows_per) && !(k.max_count && count > k.max_count) &&
                     !(k.rows_per_param && ((param & 1) || param > count));
  return takes ? k.rows_base + k.rows_per * count + k.rows_per_param * param : 0;
}

}  // namespace pm
