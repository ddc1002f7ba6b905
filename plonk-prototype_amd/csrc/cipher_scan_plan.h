// Plain host C++, no HIP calls: what pm_poseidon_cipher_scan_keys_dev (cipher.hip) decides before it
// launches -- the notes in flight (the stride), and the scratch they take.  pm_poseidon_cipher_scan_keys_work_bytes, the launch
// and the host hook pm_test_cipher_scan_keys_plan read the same lines.
//
// A note in flight holds
//   * its window table: with the full table, the 512 entries e 16^w R (w = 0 .. 63, e = 1 .. 8) of 144 bytes, 73 728 bytes;
//     on the per-key path (few keys) the 8 entries 1 R .. 8 R of the single-key ladder, 1152 bytes;
//   * per key a slot of 64 bytes for S = vk R (x | y, canonical) and a staging slot of 32 L bytes for the message that key opens.
// Behind the slots sits the tail: 64 bytes of signed digits per key (recode_digit_words) and 16 bytes for the count of hits.
//
// The stride is a multiple of 64 (one workgroup), at most the grid of slot_blocks (jubjub.hip.h: eight workgroups a CU) and at
// most n rounded up to whole workgroups.  A budget of table_mb MiB (0 = no cap) lowers it to the largest multiple of 64 whose
// scratch, tail included, fits; it is never below 64.  The walk's grid is n_keys times the stride, so a small stride starves the
// table build alone.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/plonk_mi355x.h"

namespace pm {

constexpr size_t CSK_FULL_TABLE_BYTES = 64 * 8 * 144;   // 73 728: JJ_WINDOWS x 8 entries of JJ_POINT_CHUNKS x 16 bytes
constexpr size_t CSK_LADDER_TABLE_BYTES = 8 * 144;      // 1152: JJ_MUL_TABLE_BYTES
constexpr size_t CSK_SECRET_BYTES = 64;                 // S, x | y
constexpr size_t CSK_DIGIT_BYTES = 64;                  // a key's 64 signed digits
constexpr size_t CSK_COUNT_BYTES = 16;                  // the count of hits, padded

struct CipherScanKeysPlan {
  size_t stride, blocks;              // notes in flight, and their workgroups
  size_t note_bytes;                  // scratch per note in flight
  size_t off_secrets, off_staging;    // [key][thread] x 64 bytes, [key][thread][L] x 32 bytes
  size_t off_digits, off_count;       // the tail
  size_t bytes;
};

inline size_t cipher_scan_keys_tail_bytes(uint32_t n_keys) { return CSK_DIGIT_BYTES * n_keys + CSK_COUNT_BYTES; }

// PM_OK or PM_ERR_BAD_ARG (n_keys outside 1 .. 64, msg_len outside 1 .. 4, a negative budget).  n = 0: a stride of 0, no bytes.
inline int cipher_scan_keys_plan(int num_cus, uint32_t n_keys, uint32_t msg_len, size_t n, long table_mb, bool full_table,
                                 CipherScanKeysPlan* p) {
  if (n_keys < 1 || n_keys > PM_CIPHER_SCAN_MAX_KEYS || msg_len < 1 || msg_len > 4 || table_mb < 0) return PM_ERR_BAD_ARG;
  CipherScanKeysPlan g{};
  if (n == 0) {
    *p = g;
    return PM_OK;
  }
  const size_t table = full_table ? CSK_FULL_TABLE_BYTES : CSK_LADDER_TABLE_BYTES;
  const size_t per_key = CSK_SECRET_BYTES + 32 * (size_t)msg_len, tail = cipher_scan_keys_tail_bytes(n_keys);
  g.note_bytes = table + n_keys * per_key;
  const size_t grid = (size_t)(num_cus > 1 ? num_cus : 1) * 8 * 64, need = (n + 63) / 64 * 64;
  size_t stride = need < grid ? need : grid;
  if (table_mb > 0) {
    const size_t budget = (size_t)table_mb << 20;
    const size_t fit = budget > tail ? (budget - tail) / g.note_bytes / 64 * 64 : 0;
    if (fit < stride) stride = fit;
  }
  g.stride = stride < 64 ? 64 : stride;
  g.blocks = g.stride / 64;
  g.off_secrets = g.stride * table;
  g.off_staging = g.off_secrets + g.stride * n_keys * CSK_SECRET_BYTES;
  g.off_digits = g.stride * g.note_bytes;
  g.off_count = g.off_digits + CSK_DIGIT_BYTES * n_keys;
  g.bytes = g.off_count + CSK_COUNT_BYTES;
  *p = g;
  return PM_OK;
}

}  // namespace pm
