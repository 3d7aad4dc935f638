// The device output pass's plan (include/drs_device_outputs.h; the kernel is output_pass.hip): which workgroup and lane moves
// which element of which query, the bytes a query's output occupies at its row stride, and whether two outputs overlap.
// Plain C++ with no dependency beyond input_extent.h, so that a host program can include it on its own
// (tests/test_device_outputs_cpu.py does); the kernel calls the very functions the host program walks.
#pragma once
#include <stdint.h>

#include "input_extent.h"

#if defined(__HIPCC__)
#define DRS_OUT_HD __host__ __device__
#else
#define DRS_OUT_HD
#endif

namespace drs {

constexpr int kOutPassThreads = 256;
constexpr int kOutPassPerLane = 4;                                   // one coalesced dword per lane, four rounds
constexpr int kOutPassChunk = kOutPassThreads * kOutPassPerLane;     // elements of ONE query a workgroup owns
constexpr int kOutPassQueries = 16;                                  // == DRS_MAX_COALESCE (output_pass.hip asserts it)
constexpr uint32_t kOutPassNaN = 0x7fc00000u;                        // what every element of a set with an error word holds

// a non-empty query of the set: its bs rows of n_out scores start at virtual row vstart of the slot's [Mv, n_out] buffer
// and go to dst, rows `stride` floats apart
struct OutQuery {
  float* dst;
  int64_t stride;
  int32_t vstart, bs;
};
struct OutPassArgs {
  const float* src;           // Slot::d_out
  const uint32_t* err;        // the slot's device error word: non-zero -> kOutPassNaN in place of every score
  int32_t n_q, n_out;
  int32_t blk0[kOutPassQueries + 1];   // query i owns workgroups [blk0[i], blk0[i + 1])
  OutQuery q[kOutPassQueries];
};

// fills blk0 from the rest and returns the grid (0: nothing to do).  16 queries of 2^31 - 1 rows cannot be asked for -- the
// engine's max_batch and n_out bound bs * n_out far below 2^31 * kOutPassChunk / 16 -- but the sum is kept in 64 bits and
// -1 says that it does not fit the 32-bit block numbers.
inline int64_t plan_output_pass(OutPassArgs& a) {
  int64_t grid = 0;
  for (int i = 0; i < a.n_q; ++i) {
    a.blk0[i] = (int32_t)grid;
    grid += ((int64_t)a.q[i].bs * a.n_out + kOutPassChunk - 1) / kOutPassChunk;
    if (grid > INT32_MAX) return -1;
  }
  for (int i = a.n_q; i <= kOutPassQueries; ++i) a.blk0[i] = (int32_t)grid;
  return grid;
}

// the query whose elements workgroup `block` moves (block < the grid plan_output_pass returned)
DRS_OUT_HD inline int out_owner(const OutPassArgs& a, int block) {
  int qi = 0;
  for (int i = 1; i < a.n_q; ++i) qi = block >= a.blk0[i] ? i : qi;
  return qi;
}

// the element of query qi that lane `tid` of workgroup `block` moves in round k, or -1: element e is row e / n_out,
// column e % n_out of the query
DRS_OUT_HD inline int64_t out_element(const OutPassArgs& a, int qi, int block, int k, int tid) {
  const int64_t e = (int64_t)(block - a.blk0[qi]) * kOutPassChunk + (int64_t)k * kOutPassThreads + tid;
  return e < (int64_t)a.q[qi].bs * a.n_out ? e : -1;
}
// ... where it is read (floats from OutPassArgs::src) and where it goes (floats from OutQuery::dst)
DRS_OUT_HD inline int64_t out_src_index(const OutPassArgs& a, int qi, int64_t e) { return (int64_t)a.q[qi].vstart * a.n_out + e; }
DRS_OUT_HD inline int64_t out_dst_index(const OutPassArgs& a, int qi, int64_t e) {
  const int64_t r = e / a.n_out;
  return r * a.q[qi].stride + (e - r * a.n_out);
}

// The bytes query's output occupies: (bs - 1) * stride + n_out floats, nothing for an empty query.  false: rows that would
// overlap (stride < n_out with more than one row, a negative stride among them), or an extent input_extent_bytes refuses.
inline bool output_extent_bytes(int64_t bs, int64_t stride, int64_t n_out, uint64_t* bytes) {
  *bytes = 0;
  if (bs < 0 || n_out < 1) return false;
  if (bs == 0) return true;
  if (bs > 1 && stride < n_out) return false;
  return input_extent_bytes(bs, bs > 1 ? stride : 0, n_out, (int64_t)sizeof(float), bytes);
}

// do [p, p + pb) and [q, q + qb) share a byte?  Touching ranges do not, an empty range shares nothing (by subtraction: no
// sum that could wrap)
inline bool extents_overlap(uint64_t p, uint64_t pb, uint64_t q, uint64_t qb) {
  if (pb == 0 || qb == 0) return false;
  return p <= q ? q - p < pb : p - q < qb;
}

}  // namespace drs
