// The per-call input block [dense | idx | off] -- the packed block one query's converted inputs live in, pinned on the host
// and again in HBM, laid out like a staged batch: its layout (the ONE place that says how large a region is and where it
// starts), the host pass that fills one (int64 -> int32 + Caffe2's ENFORCEs, one table of one query at a time) and the
// host-to-device copies that move what a query used of it.  Plain C++ with no HIP include, so that a host program can
// include it on its own and run the pass under a host sanitizer (tests/test_input_block_cpu.py does).
#pragma once
#include <immintrin.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/drs.h"

namespace drs {
namespace eng {

//   dense [max_batch, max(m_den, 1)] f32 | idx [T, cap] i32 | off [T, max_batch + 1] i32 (exclusive prefix sums of the lengths)
struct BlockLayout {
  int64_t max_batch = 0, T = 0, cap = 0;
  size_t dense_bytes = 0, idx_bytes = 0, off_bytes = 0;   // the three regions, in this order (m_den 0 still reserves a float per row)
  size_t bytes = 0, padded = 0;                           // all of a block | the step from one block of a launch set's to the next
  BlockLayout() {}
  BlockLayout(int64_t max_batch_, int64_t m_den, int64_t T_, int64_t cap_) : max_batch(max_batch_), T(T_), cap(cap_) {
    dense_bytes = sizeof(float) * (size_t)max_batch * (size_t)(m_den > 0 ? m_den : 1);
    idx_bytes = sizeof(int32_t) * idx_elems();
    off_bytes = sizeof(int32_t) * off_elems();
    bytes = dense_bytes + idx_bytes + off_bytes;
    padded = (bytes + 255) / 256 * 256;
  }
  size_t idx_at() const { return dense_bytes; }
  size_t off_at() const { return dense_bytes + idx_bytes; }
  size_t off_stride() const { return (size_t)max_batch + 1; }
  size_t idx_elems() const { return (size_t)T * (size_t)cap; }
  size_t off_elems() const { return (size_t)T * off_stride(); }
  // where the host copy of the prefix sums (Batch::h_off) keeps table t's indices up to sample bs
  size_t h_off_at(int64_t t, int64_t bs) const { return (size_t)t * off_stride() + (size_t)bs; }
  // the used prefix of a block: dense rows, then index rows up to the last table's last index
  size_t used_prefix(int64_t n_idx_last_table) const {
    return dense_bytes + sizeof(int32_t) * ((size_t)(T - 1) * (size_t)cap + (size_t)n_idx_last_table);
  }
};

// a block at `base` as its three regions (what a Batch's dense / idx / off are assigned from)
struct BlockView { float* dense; int32_t* idx; int32_t* off; };
inline BlockView view_block(const BlockLayout& L, void* base) {
  char* b = static_cast<char*>(base);
  return BlockView{reinterpret_cast<float*>(b), reinterpret_cast<int32_t*>(b + L.idx_at()), reinterpret_cast<int32_t*>(b + L.off_at())};
}

// int64 -> int32 with the range ENFORCE, branch-free so it vectorises (AVX2 where the host has
// it); returns the position of the first offending index or -1
template <int>
static inline int64_t narrow_checked_impl(const int64_t* __restrict__ src, int64_t n, int64_t rows,
                                          int32_t* __restrict__ dst) {
  uint64_t bad = 0;
  const uint64_t R = (uint64_t)rows;
  for (int64_t j = 0; j < n; ++j) {
    const uint64_t v = (uint64_t)src[j];       // negative -> huge: one unsigned compare
    bad |= (uint64_t)(v >= R);
    dst[j] = (int32_t)v;
  }
  if (!bad) return -1;
  for (int64_t j = 0; j < n; ++j)
    if ((uint64_t)src[j] >= R) return j;
  return -1;
}
// AVX2 form: 8 indices per step, packed into one 32-byte NON-TEMPORAL store -- the destination is a pinned
// block the DMA engine reads next, never this core: streaming stores skip the read-for-ownership of every
// destination line (a third of the pass's memory reads; 12-query sets on the GPU box's host: 43-57 k -> 59-64 k
// queries/s, the bus then carries 48 GB/s)
__attribute__((target("avx2"))) static inline int64_t narrow_checked_avx2(const int64_t* s, int64_t n, int64_t r, int32_t* d) {
  int64_t j = 0;
  uint64_t bad = 0;
  const uint64_t R = (uint64_t)r;
  for (; j < n && ((uintptr_t)(d + j) & 31); ++j) {
    const uint64_t v = (uint64_t)s[j];
    bad |= (uint64_t)(v >= R);
    d[j] = (int32_t)v;
  }
  const __m256i sign = _mm256_set1_epi64x((long long)0x8000000000000000ull);
  const __m256i lim = _mm256_set1_epi64x((long long)((R - 1) ^ 0x8000000000000000ull));   // v > R - 1, unsigned
  const __m256i pick = _mm256_setr_epi32(0, 2, 4, 6, 0, 2, 4, 6);
  __m256i acc = _mm256_setzero_si256();
  if (R > 0)
    for (; j + 8 <= n; j += 8) {
      const __m256i a = _mm256_loadu_si256(reinterpret_cast<const __m256i*>(s + j));
      const __m256i b = _mm256_loadu_si256(reinterpret_cast<const __m256i*>(s + j + 4));
      acc = _mm256_or_si256(acc, _mm256_or_si256(_mm256_cmpgt_epi64(_mm256_xor_si256(a, sign), lim),
                                                 _mm256_cmpgt_epi64(_mm256_xor_si256(b, sign), lim)));
      const __m256i lo = _mm256_permutevar8x32_epi32(a, pick), hi = _mm256_permutevar8x32_epi32(b, pick);
      const __m256i o = _mm256_blend_epi32(lo, hi, 0xf0);
      _mm256_stream_si256(reinterpret_cast<__m256i*>(d + j), o);
    }
  bad |= (uint64_t)!_mm256_testz_si256(acc, acc);
  for (; j < n; ++j) {
    const uint64_t v = (uint64_t)s[j];
    bad |= (uint64_t)(v >= R);
    d[j] = (int32_t)v;
  }
  _mm_sfence();
  if (!bad) return -1;
  for (int64_t k = 0; k < n; ++k)
    if ((uint64_t)s[k] >= R) return k;
  return -1;
}
static inline int64_t narrow_checked_base(const int64_t* s, int64_t n, int64_t r, int32_t* d) {
  return narrow_checked_impl<0>(s, n, r, d);
}
static inline int64_t narrow_checked(const int64_t* s, int64_t n, int64_t r, int32_t* d) {
  static const bool avx2 = __builtin_cpu_supports("avx2");
  return avx2 ? narrow_checked_avx2(s, n, r, d) : narrow_checked_base(s, n, r, d);
}

// Validate (the Caffe2 ENFORCEs) and narrow int64 -> int32 (the Cast op,
// models/dlrm_s_caffe2.py:308-309) into caller-provided host buffers: one table (`rows` rows) of one query of n samples
struct ConvRes { int32_t code = DRS_OK; int32_t bag = 0; int64_t pos = 0, val = 0, total = 0, n_idx = 0; bool same = true; };
inline void convert_table(const BlockLayout& L, int64_t rows, int32_t n, const int64_t* idx_t, int64_t n_idx_t,
                          const int32_t* len_t, int32_t* idx32_t /*[cap]*/, int32_t* off_t /*[off_stride]*/, ConvRes& r) {
  r = ConvRes();
  r.n_idx = n_idx_t;
  if (!idx_t && n_idx_t > 0) { r.code = DRS_ERR_BAD_ARG; r.pos = -1; return; }
  if (!len_t) { r.code = DRS_ERR_BAD_ARG; r.pos = -2; return; }
  if (n_idx_t < 0 || n_idx_t > L.cap) { r.code = DRS_ERR_BAD_ARG; r.pos = -3; return; }
  int64_t total = 0;
  off_t[0] = 0;
  const int32_t L0 = n > 0 ? len_t[0] : 0;
  bool same = true;
  for (int b = 0; b < n; ++b) {
    if (len_t[b] < 0) { r.code = DRS_ERR_LENGTHS_SUM; r.bag = b; r.pos = -1; return; }
    same = same && len_t[b] == L0;
    total += len_t[b];
    if (total > n_idx_t) break;
    off_t[b + 1] = (int32_t)total;
  }
  r.total = total;
  r.same = same;
  if (total != n_idx_t) { r.code = DRS_ERR_LENGTHS_SUM; r.pos = 0; return; }
  for (int64_t b = n; b < L.max_batch; ++b) off_t[b + 1] = (int32_t)total;
  const int64_t j = narrow_checked(idx_t, n_idx_t, rows, idx32_t);
  if (j >= 0) { r.code = DRS_ERR_INDEX_RANGE; r.pos = j; r.val = idx_t[j]; }
}

// The host-to-device copies of n converted blocks `step` bytes apart, as (offset, bytes) from the first block's start into
// out[2 n]; returns how many.  used[i]: block i's used prefix; need_off[i]: the kernels will read its prefix sums (ragged
// bags, or "sls_uniform" 0), so its offsets region travels too.  A block alone (merge false): the prefix and, where needed,
// the offsets.  The blocks of a launch set (merge): one copy of all n when they are mostly full -- up to the last block's
// end when some block needs its offsets, else up to the last block's used prefix -- and otherwise every block like a block
// alone: a set of small ragged queries must not move n full-capacity blocks.
struct BlockCopy { size_t at, bytes; };
inline int plan_block_copies(const BlockLayout& L, size_t step, int n, const size_t* used, const bool* need_off, bool merge,
                             BlockCopy* out) {
  size_t used_sum = 0;
  bool any_off = false;
  for (int i = 0; i < n; ++i) { used_sum += used[i]; any_off = any_off || need_off[i]; }
  if (merge && 2 * used_sum >= (size_t)n * step) {
    out[0] = BlockCopy{0, any_off ? (size_t)n * step : (size_t)(n - 1) * step + used[n - 1]};
    return 1;
  }
  int k = 0;
  for (int i = 0; i < n; ++i) {
    out[k++] = BlockCopy{(size_t)i * step, used[i]};
    if (need_off[i]) out[k++] = BlockCopy{(size_t)i * step + L.off_at(), L.off_bytes};
  }
  return k;
}

}  // namespace eng
}  // namespace drs
