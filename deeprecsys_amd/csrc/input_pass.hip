// libdrs_hip.so: the per-call input pass on the device (include/drs_device_inputs.h).  What engine_inputs.hip's
// convert_table does on the host for host arrays -- the Cast op int64 -> int32 (models/dlrm_s_caffe2.py:308-309), Caffe2's
// ENFORCEs, the exclusive prefix sums of the bag lengths, the dense rows into the query's block -- as ONE launch for all
// queries of a launch set whose arrays are device arrays.
//
// Safe by construction, whatever the caller's bytes are: every index stored is inside [0, rows_t) (row 0 stands in for a bad
// one), every prefix sum stored is monotone inside [0, n_idx], and nothing is read outside the extents the host checked
// before the launch ((T - 1) * stride + count elements from ids / len, bs * m_den floats from dense).  What is wrong with
// the arrays goes into the slot's error word (kErrIndex, kErrLengths) and the set that follows gathers valid rows.
#include "drs_internal.h"

namespace drs {

namespace {

// the range ENFORCE on the 64-bit value, before it is narrowed: 2^32 + 3 must not pass as 3; negative -> huge
__device__ __forceinline__ int32_t narrow_checked(uint64_t v, uint64_t R, uint32_t& bad) {
  const bool out = v >= R;
  bad |= (uint32_t)out;
  return out ? 0 : (int32_t)v;
}

// what a wave found goes into the slot's error word once (called in uniform control flow)
__device__ __forceinline__ void report(uint32_t* err, uint32_t bad, uint32_t bit) {
  if (__ballot(bad != 0) != 0 && (threadIdx.x & 63) == 0) atomicOr(err, bit);
}

// indices [2 p0, 2 p0 + kInPassIdx) of a row whose source is 16-byte aligned: four 16-byte loads per lane in flight, then
// the checks and the stores (kPacked: the destination is 8-byte aligned, one 8-byte store per pair)
template <bool kPacked>
__device__ __forceinline__ void narrow_pairs(const int64_t* __restrict__ src, int32_t* __restrict__ dst, int64_t npairs,
                                             int64_t p0, uint64_t R, uint32_t& bad) {
  constexpr int kLoads = kInPassIdx / 2 / kInPassThreads;
  static_assert(kLoads == 4, "four 16-byte loads per lane");
  const ulonglong2* s2 = reinterpret_cast<const ulonglong2*>(src);
  ulonglong2 v[kLoads];
#pragma unroll
  for (int k = 0; k < kLoads; ++k) {
    const int64_t p = p0 + k * kInPassThreads + (int)threadIdx.x;
    v[k] = p < npairs ? s2[p] : make_ulonglong2(0, 0);
  }
#pragma unroll
  for (int k = 0; k < kLoads; ++k) {
    const int64_t p = p0 + k * kInPassThreads + (int)threadIdx.x;
    if (p >= npairs) continue;
    const int32_t lo = narrow_checked(v[k].x, R, bad), hi = narrow_checked(v[k].y, R, bad);
    if (kPacked) {
      *reinterpret_cast<int2*>(dst + 2 * p) = make_int2(lo, hi);
    } else {
      dst[2 * p] = lo;
      dst[2 * p + 1] = hi;
    }
  }
}

// chunk c of one (query, table) index row.  The source is only 8-byte aligned (a column slice, an odd row stride): one
// head element is peeled where it starts on an odd 8 bytes, one tail element where an odd count is left.
__device__ __forceinline__ void narrow_item(const InPassArgs& a, const InQuery& q, int t, int c) {
  const int64_t* src = q.ids + (int64_t)t * q.ids_stride;
  int32_t* dst = q.idx + (int64_t)t * a.cap;
  const int64_t n = q.n_idx;
  const uint64_t R = (uint64_t)a.rows[t];
  const int64_t head = (n > 0 && (reinterpret_cast<uintptr_t>(src) & 8)) ? 1 : 0;
  const int64_t npairs = (n - head) >> 1;
  const bool tail = ((n - head) & 1) != 0;
  uint32_t bad = 0;
  if (c == 0) {
    if (threadIdx.x == 0 && head) dst[0] = narrow_checked((uint64_t)src[0], R, bad);
    if (threadIdx.x == 1 && tail) dst[n - 1] = narrow_checked((uint64_t)src[n - 1], R, bad);
  }
  const int64_t p0 = (int64_t)c * (kInPassIdx / 2);
  if (reinterpret_cast<uintptr_t>(dst + head) & 7) narrow_pairs<false>(src + head, dst + head, npairs, p0, R, bad);
  else narrow_pairs<true>(src + head, dst + head, npairs, p0, R, bad);
  report(a.err, bad, kErrIndex);
}

// the lengths of one (query, table): the ENFORCEs and, where the gather will read them, the exclusive prefix sums -- a
// shuffle scan inside each wave, the waves' totals through LDS, a running carry from one chunk of kInPassThreads bags to the
// next.  64-bit sums: max_batch lengths of up to 2^31 - 1 cannot wrap them.  off[0] = 0, off[b + 1] = min(sum through bag b,
// n_idx) -- a negative length counts as 0 -- and entries bs + 1 .. max_batch hold the total, as convert_table leaves them.
__device__ __forceinline__ void lengths_item(const InPassArgs& a, const InQuery& q, int t) {
  __shared__ int64_t wave_sum[kInPassThreads / 64];
  const int32_t* len = q.len + (int64_t)t * q.len_stride;
  int32_t* off = q.off + (int64_t)t * (a.max_batch + 1);
  const int tid = (int)threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int64_t n_idx = q.n_idx;
  int64_t carry = 0;
  uint32_t bad = 0;
  if (!q.store_off) {
    // a promised fixed_len whose prefix sums nobody will read: every length against the promise, nothing else (the host
    // has checked n_idx == bs * fixed_len, so lengths that all keep the promise sum to n_idx)
    for (int b = tid; b < q.bs; b += kInPassThreads) bad |= (uint32_t)(len[b] != q.fixed_len);
    report(a.err, bad, kErrLengths);
    return;
  }
  if (tid == 0) off[0] = 0;
  for (int b0 = 0; b0 < q.bs; b0 += kInPassThreads) {
    const int b = b0 + tid;
    int64_t inc = 0;
    if (b < q.bs) {
      const int32_t l = len[b];
      bad |= (uint32_t)(l < 0) | (uint32_t)(q.fixed_len >= 0 && l != q.fixed_len);
      inc = l < 0 ? 0 : l;
    }
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int64_t up = __shfl_up(inc, d, 64);
      inc += lane >= d ? up : 0;
    }
    if (lane == 63) wave_sum[w] = inc;
    __syncthreads();
    int64_t before = carry, all = 0;
#pragma unroll
    for (int k = 0; k < kInPassThreads / 64; ++k) {
      before += k < w ? wave_sum[k] : 0;
      all += wave_sum[k];
    }
    if (b < q.bs) {
      int64_t through = before + inc;
      if (through > n_idx) { bad = 1; through = n_idx; }
      off[b + 1] = (int32_t)through;
    }
    carry += all;
    __syncthreads();      // (wave_sum is written again by the next chunk)
  }
  bad |= (uint32_t)(carry != n_idx);
  const int32_t total = (int32_t)(carry < n_idx ? carry : n_idx);
  for (int b = q.bs + 1 + tid; b <= a.max_batch; b += kInPassThreads) off[b] = total;
  report(a.err, bad, kErrLengths);
}

// floats [c kInPassDense, (c + 1) kInPassDense) of a query's n dense floats (the destination, a block's first bytes, is
// 16-byte aligned; a row slice of a wider tensor need not be)
__device__ __forceinline__ void dense_item(const float* __restrict__ src, float* __restrict__ dst, int64_t n, int c) {
  const int64_t base = (int64_t)c * kInPassDense;
  const int tid = (int)threadIdx.x;
  if ((reinterpret_cast<uintptr_t>(src) & 15) == 0) {
    constexpr int kLoads = kInPassDense / 4 / kInPassThreads;
    float4 v[kLoads];
#pragma unroll
    for (int k = 0; k < kLoads; ++k) {
      const int64_t i = base + ((int64_t)k * kInPassThreads + tid) * 4;
      v[k] = i + 4 <= n ? *reinterpret_cast<const float4*>(src + i) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int k = 0; k < kLoads; ++k) {
      const int64_t i = base + ((int64_t)k * kInPassThreads + tid) * 4;
      if (i + 4 <= n) *reinterpret_cast<float4*>(dst + i) = v[k];
      else for (int64_t j = i; j < n; ++j) dst[j] = src[j];     // (the last one to three floats)
    }
  } else {
#pragma unroll 4
    for (int k = 0; k < kInPassDense / kInPassThreads; ++k) {
      const int64_t i = base + (int64_t)k * kInPassThreads + tid;
      if (i < n) dst[i] = src[i];
    }
  }
}

__global__ __launch_bounds__(kInPassThreads) void input_pass_kernel(const InPassArgs a) {
  const int wg = (int)blockIdx.x;
  int qi = 0;
  for (int i = 1; i < a.n_q; ++i) qi = wg >= a.wg0[i] ? i : qi;
  const InQuery& q = a.q[qi];
  int r = wg - a.wg0[qi];
  if (r < a.T) { lengths_item(a, q, r); return; }
  r -= a.T;
  if (r < a.T * q.nb_idx) { narrow_item(a, q, r / q.nb_idx, r % q.nb_idx); return; }
  r -= a.T * q.nb_idx;
  if (r < q.nb_dense) dense_item(q.dense, q.dst_dense, (int64_t)q.bs * a.m_den, r);
}

}  // namespace

int64_t plan_input_pass(InPassArgs& a) {
  int64_t grid = 0;
  for (int i = 0; i < a.n_q; ++i) {
    InQuery& q = a.q[i];
    q.nb_idx = (int32_t)(((int64_t)q.n_idx + kInPassIdx - 1) / kInPassIdx);
    q.nb_dense = q.dense ? (int32_t)(((int64_t)q.bs * a.m_den + kInPassDense - 1) / kInPassDense) : 0;
    a.wg0[i] = (int32_t)grid;
    grid += (int64_t)a.T * (1 + q.nb_idx) + q.nb_dense;
  }
  a.wg0[a.n_q] = (int32_t)grid;
  return grid;
}

hipError_t launch_input_pass(const InPassArgs& a, int64_t grid, hipStream_t stream) {
  if (grid <= 0) return hipSuccess;
  hipLaunchKernelGGL(input_pass_kernel, dim3((unsigned)grid), dim3(kInPassThreads), 0, stream, a);
  return hipGetLastError();
}

}  // namespace drs
