// The plan of the per-sample weights inside the device input pass (include/drs_device_weights.h; the kernel is
// input_pass.hip's weighted instance): how many workgroups one (query, table) row of weights takes, which elements of a row
// are moved one by one because the 16-byte loads cannot reach them, and how a set's workgroups are numbered once some of
// its queries carry weights.  Plain C++ with no dependency beyond input_extent.h, so that a host program can include it on
// its own (tests/test_device_weights_cpu.py does); the kernel and the host side call the very functions the host program walks.
#pragma once
#include <stdint.h>

#include "input_extent.h"

#if defined(__HIPCC__)
#define DRS_WGT_HD __host__ __device__
#else
#define DRS_WGT_HD
#endif

namespace drs {

// weights per workgroup, picked as kInPassDense was: 256 lanes, 16-byte loads all in flight before the first store -- four
// per lane for fp32 weights, two for the half types (whose 16 bytes widen to two 16-byte stores)
constexpr int kInPassWgt = 4096;
constexpr int kInPassWgtQueries = 16;     // == DRS_MAX_COALESCE (input_pass.hip asserts it)

// workgroups per row of n weights (every table of a query has the same n)
DRS_WGT_HD inline int32_t wgt_chunks(int64_t n) { return n > 0 ? (int32_t)((n + kInPassWgt - 1) / kInPassWgt) : 0; }

// A row of n elements of `elem` bytes (4 or 2) whose first byte is at `addr` -- aligned to its element, no more: a column
// slice, an odd row stride.  `head` elements come before the first 16-byte line (0 .. 16 / elem - 1, all n where the row
// ends before that line), `nvec` whole 16-byte vectors follow, `tail` elements are left (0 .. 16 / elem - 1).
struct WgtPeel {
  int32_t head, tail;
  int64_t nvec;
};
DRS_WGT_HD inline WgtPeel wgt_peel(uint64_t addr, int32_t elem, int64_t n) {
  WgtPeel p = {0, 0, 0};
  if (n <= 0) return p;
  const int32_t per = 16 / elem;
  const int64_t to_line = (int64_t)(((16u - (uint32_t)(addr & 15u)) & 15u) / (uint32_t)elem);
  p.head = (int32_t)(to_line < n ? to_line : n);
  p.nvec = (n - p.head) / per;
  p.tail = (int32_t)(n - p.head - p.nvec * per);
  return p;
}
// the vectors chunk c of a row moves: [wgt_vec0(c, elem), wgt_vec0(c + 1, elem)) cut at nvec.  wgt_chunks(n) chunks cover
// every vector of a row of n, whatever its head (nvec <= n / per); chunk 0 also moves the head and the tail.
DRS_WGT_HD inline int64_t wgt_vec0(int32_t c, int32_t elem) { return (int64_t)c * (kInPassWgt / (16 / elem)); }

// The bytes the pass reads from one query's weights: T rows of n elements of `elem` bytes, `stride` elements apart -- (T - 1)
// * stride + n elements, nothing where n == 0.  false: a negative argument, an element size that is neither 4 nor 2, or an
// extent beyond 2^60 bytes (input_extent.h).
inline bool weight_extent_bytes(int64_t T, int64_t stride, int64_t n, int64_t elem, uint64_t* bytes) {
  *bytes = 0;
  if (elem != 4 && elem != 2) return false;
  return input_extent_bytes(T, stride, n, elem, bytes);
}

// The numbering of a weighted set's workgroups.  Query i has T lengths items, T * nb_idx[i] index items and nb_dense[i] dense
// items, numbered in that order exactly as an unweighted set numbers them, and then T * nb_wgt[i] weight items (nb_wgt[i] ==
// 0: the query is unweighted, or has no index).  Query i owns [wg0[i], wg0[i + 1]); entries past n_q hold the grid, which is
// returned (-1: it does not fit the 32-bit block numbers).
inline int64_t plan_weighted_grid(int32_t n_q, int32_t T, const int32_t* nb_idx, const int32_t* nb_dense, const int32_t* nb_wgt,
                                  int32_t* wg0) {
  int64_t grid = 0;
  for (int i = 0; i < n_q; ++i) {
    wg0[i] = (int32_t)grid;
    grid += (int64_t)T * (1 + (int64_t)nb_idx[i] + nb_wgt[i]) + nb_dense[i];
    if (grid > INT32_MAX) return -1;
  }
  for (int i = n_q; i <= kInPassWgtQueries; ++i) wg0[i] = (int32_t)grid;
  return grid;
}

}  // namespace drs
