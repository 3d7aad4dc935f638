// The device top-k pass's plan (include/drs_device_topk.h; the kernel is topk_pass.hip): the ORDER in which a query's samples
// rank, the arguments of the pass, the bytes its outputs occupy, and a host restatement of the tiled selection the kernel
// makes.  Plain C++ with no dependency beyond output_plan.h / input_extent.h, so that a host program can include it on its
// own (tests/test_device_topk_cpu.py does); the kernel calls the very functions the host program walks.
//
// The order is total, so the result of a selection is unique and any correct kernel gives the same bytes:
//   * a score's bits become a sortable word (topk_sortable): any NaN 0xffffffff -- NaN ranks FIRST, as torch.topk has it --
//     a negative value ~bits, everything else bits | 0x80000000.  +0.0 ranks above -0.0, +inf below NaN.
//   * the key of sample row r (topk_key) is that word in the high half and 0xffffffff - r in the low half: winners are the k
//     LARGEST keys in descending order, so equal scores rank by the LOWER row.  Keys within a query are distinct: a sample's
//     rank is the number of larger keys.
//   * the key 0 is never produced (the smallest real key is -inf's, high word 0x007fffff): it is the padding sentinel.
#pragma once
#include <stdint.h>

#include "output_plan.h"

namespace drs {

constexpr int kTopKThreads = 256;
constexpr int kTopKTile = 1024;          // rows ranked per step; a query of up to this many rows (every query of the run scripts) takes ONE step
constexpr int kTopKQueries = 16;         // == DRS_MAX_COALESCE (topk_pass.hip asserts it)
constexpr int kTopKKeys = 2 * kTopKTile; // keys in LDS at once: the carried winners and one tile (16 KB)
constexpr int kTopKPad = 16;             // the keys of a step are padded with the sentinel to a multiple of this: eight 16-byte reads in flight
#ifndef DRS_TOPK_MAX
#define DRS_TOPK_MAX 1024                /* the most rows one query hands back (include/drs_device_topk.h) */
#endif
static_assert(DRS_TOPK_MAX == kTopKTile, "the carried winners of a step fit beside one tile");
static_assert(kTopKKeys % (2 * kTopKThreads) == 0, "every thread owns the same number of key positions");
static_assert(kTopKKeys % kTopKPad == 0 && kTopKPad % 2 == 0, "the padding stays inside the keys' storage, in whole 16-byte pairs");

DRS_OUT_HD inline uint32_t topk_sortable(uint32_t bits) {
  if ((bits & 0x7fffffffu) > 0x7f800000u) return 0xffffffffu;      // NaN, either sign, any payload
  return (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u);
}
DRS_OUT_HD inline uint64_t topk_key(uint32_t bits, int64_t r) {
  return ((uint64_t)topk_sortable(bits) << 32) | (uint64_t)(0xffffffffu - (uint32_t)r);
}
// the sample row a key names
DRS_OUT_HD inline uint32_t topk_key_row(uint64_t key) { return 0xffffffffu - (uint32_t)key; }

// The selection runs in steps: step t ranks tile t -- rows [t * kTopKTile, ...) of the query -- together with the winners the
// steps before it carried, at most 2 * kTopKTile keys, and keeps the keys of rank < k as the next carry, sorted by
// construction (a key's rank is its position).  A query of up to kTopKTile rows takes one step with no carry.  The longer
// queries ("max_batch" has no upper bound) stream their tiles; that is NOT the fast path -- every step ranks up to 2 048 keys
// for 1 024 new rows.
DRS_OUT_HD inline int64_t topk_steps(int64_t bs) { return (bs + kTopKTile - 1) / kTopKTile; }
DRS_OUT_HD inline int topk_tile_rows(int64_t bs, int64_t t) {
  const int64_t left = bs - t * kTopKTile;
  return (int)(left < kTopKTile ? left : kTopKTile);
}
// the keys of a step with their padding: positions [m, topk_padded(m)) hold the sentinel 0, which exceeds nothing
DRS_OUT_HD inline int topk_padded(int m) { return (m + kTopKPad - 1) & ~(kTopKPad - 1); }
// the number of the m keys (m even; the padding counts for nothing) larger than `mine`
DRS_OUT_HD inline int topk_rank(const uint64_t* keys, int m, uint64_t mine) {
  int n = 0;
  for (int i = 0; i < m; i += 2) n += (int)(keys[i] > mine) + (int)(keys[i + 1] > mine);
  return n;
}

// a non-empty query with k > 0: its bs rows of n_out scores start at src, rows `stride` floats apart (the slot's buffer:
// n_out); its k winners' rows go to top [k, n_out] contiguous and their row numbers to idx [k]
struct TopKQuery {
  const float* src;
  int64_t stride;
  float* top;
  int32_t* idx;
  int32_t bs, k;
};
struct TopKArgs {
  const uint32_t* err;        // the slot's device error word (non-zero: -1 in every idx, kOutPassNaN in every score), or null
  int32_t n_q, n_out, col;    // workgroup i serves q[i]; the rows rank by column col
  TopKQuery q[kTopKQueries];
};

// The bytes a query's two outputs occupy: k * n_out floats and k int32 (nothing where k == 0).  false: k < 0, n_out < 1.
inline bool topk_extent_bytes(int64_t k, int64_t n_out, uint64_t* top_bytes, uint64_t* idx_bytes) {
  *top_bytes = *idx_bytes = 0;
  if (k < 0 || n_out < 1) return false;
  if (k == 0) return true;
  if (!input_extent_bytes(1, 0, k * n_out, (int64_t)sizeof(float), top_bytes)) return false;
  return input_extent_bytes(1, 0, k, (int64_t)sizeof(int32_t), idx_bytes);
}
// the bytes the pass may read of a caller's score array (drs_topk_rows): output_plan.h's rule for rows `stride` floats apart
inline bool topk_source_bytes(int64_t rows, int64_t stride, int64_t n_out, uint64_t* bytes) {
  return output_extent_bytes(rows, stride, n_out, bytes);
}
// k within 0..min(bs, DRS_TOPK_MAX)
inline bool topk_k_in_range(int64_t k, int64_t bs) { return k >= 0 && k <= bs && k <= DRS_TOPK_MAX; }

// The selection restated on the host, step by step as the kernel makes it: bits[r * stride] is the ranking column's word of
// row r; win receives the k winners' keys in descending order.  `keys` is the kernel's LDS: kTopKKeys words.
inline void topk_select_host(const uint32_t* bits, int64_t stride, int64_t bs, int k, uint64_t* win) {
  uint64_t keys[kTopKKeys], next[DRS_TOPK_MAX];
  int c = 0;                                                   // winners carried so far: keys[0 .. c)
  for (int64_t t = 0; t < topk_steps(bs); ++t) {
    const int n = topk_tile_rows(bs, t);
    for (int i = 0; i < n; ++i) {
      const int64_t r = t * kTopKTile + i;
      keys[c + i] = topk_key(bits[r * stride], r);
    }
    const int m = c + n;
    for (int i = m; i < topk_padded(m); ++i) keys[i] = 0;
    for (int p = 0; p < m; ++p) {
      const int rank = topk_rank(keys, topk_padded(m), keys[p]);
      if (rank < k) next[rank] = keys[p];
    }
    c = m < k ? m : k;                                         // (the kernel: every thread ranks its keys, a barrier, then the stores)
    for (int i = 0; i < c; ++i) keys[i] = next[i];
  }
  for (int i = 0; i < k; ++i) win[i] = keys[i];
}

}  // namespace drs
