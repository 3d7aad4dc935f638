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

// ---- per-sample weights (include/drs_device_weights.h): a set in which a query carries them launches the weighted instance
// of the pass instead -- the three kinds of item above under the same numbers, and the weights' rows copied or widened to
// fp32 behind them (weight_plan.h, which drs_internal.h includes: chunks, peels, the numbering)
static_assert(kInPassWgtQueries == DRS_MAX_COALESCE, "weight_plan.h restates DRS_MAX_COALESCE");

// one stored weight -> fp32, exactly: fp16 through v_cvt_f32_f16, bf16 by its 16-bit shift
template <int kType>
__device__ __forceinline__ float widen_weight(uint32_t bits) {
  if (kType == DRS_TABLE_FP16) return (float)__builtin_bit_cast(_Float16, (unsigned short)bits);
  if (kType == DRS_TABLE_BF16) return __uint_as_float(bits << 16);
  return __uint_as_float(bits);
}

// chunk c of one (query, table) row of per-sample weights, copied (fp32) or widened (fp16, bf16) into the query's fp32
// weight row.  The source is aligned to its element only (a column slice, an odd row stride): wgt_peel (weight_plan.h)
// names the elements in front of its first 16-byte line and behind its last whole one -- at most 3 (fp32) or 7 (half) each,
// moved one per lane by chunk 0 -- and every chunk moves its share of the 16-byte vectors between them: all its loads in
// flight, then the stores (16-byte ones where the destination row, t * cap floats in and `head` further, allows them).
// Reads stay inside the row's n elements, writes inside the row's n floats; the weights are data and nothing is checked.
template <int kType>
__device__ __forceinline__ void weights_item(const InWgt& w, int64_t cap, int64_t n, int t, int c) {
  constexpr int kElem = kType == DRS_TABLE_FP32 ? 4 : 2;
  constexpr int kPer = 16 / kElem;                                   // elements per 16-byte load
  constexpr int kLoads = kInPassWgt / kPer / kInPassThreads;         // ... and loads per lane: 4 (fp32), 2 (half)
  static_assert(kLoads * kPer * kInPassThreads == kInPassWgt && kLoads >= 2, "whole 16-byte loads, several per lane");
  const char* src = static_cast<const char*>(w.src) + (int64_t)t * w.stride * kElem;
  float* dst = w.dst + (int64_t)t * cap;
  const WgtPeel p = wgt_peel(reinterpret_cast<uintptr_t>(src), kElem, n);
  const int tid = (int)threadIdx.x;
  auto one = [&](int64_t j) {
    const uint32_t bits = kElem == 4 ? reinterpret_cast<const uint32_t*>(src)[j] : (uint32_t)reinterpret_cast<const uint16_t*>(src)[j];
    dst[j] = widen_weight<kType>(bits);
  };
  if (c == 0) {
    if (tid < p.head) one(tid);
    if (tid >= 64 && tid - 64 < p.tail) one(n - p.tail + (tid - 64));
  }
  const uint4* s4 = reinterpret_cast<const uint4*>(src + (int64_t)p.head * kElem);
  float* d = dst + p.head;
  const bool packed = (reinterpret_cast<uintptr_t>(d) & 15) == 0;
  const int64_t v0 = wgt_vec0(c, kElem);
  uint4 v[kLoads];
#pragma unroll
  for (int k = 0; k < kLoads; ++k) {
    const int64_t i = v0 + k * kInPassThreads + tid;
    v[k] = i < p.nvec ? s4[i] : make_uint4(0, 0, 0, 0);
  }
#pragma unroll
  for (int k = 0; k < kLoads; ++k) {
    const int64_t i = v0 + k * kInPassThreads + tid;
    if (i >= p.nvec) continue;
    float f[kPer];
    const uint32_t u[4] = {v[k].x, v[k].y, v[k].z, v[k].w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if constexpr (kElem == 4) {
        f[j] = widen_weight<kType>(u[j]);
      } else {
        f[2 * j] = widen_weight<kType>(u[j] & 0xffffu);
        f[2 * j + 1] = widen_weight<kType>(u[j] >> 16);
      }
    }
    float* o = d + i * kPer;
    if (packed) {
#pragma unroll
      for (int j = 0; j < kPer; j += 4) *reinterpret_cast<float4*>(o + j) = make_float4(f[j], f[j + 1], f[j + 2], f[j + 3]);
    } else {
#pragma unroll
      for (int j = 0; j < kPer; ++j) o[j] = f[j];
    }
  }
}

// the weighted instance: input_pass_kernel's three kinds of item under their numbers, and behind a query's dense workgroups
// nb_wgt per table of kInPassWgt weights each
__global__ __launch_bounds__(kInPassThreads) void input_pass_weighted_kernel(const InPassWgtArgs aw) {
  const InPassArgs& a = aw.in;
  const int wg = (int)blockIdx.x;
  int qi = 0;
  for (int i = 1; i < a.n_q; ++i) qi = wg >= a.wg0[i] ? i : qi;
  const InQuery& q = a.q[qi];
  int r = wg - a.wg0[qi];
  if (r < a.T) { lengths_item(a, q, r); return; }
  r -= a.T;
  if (r < a.T * q.nb_idx) { narrow_item(a, q, r / q.nb_idx, r % q.nb_idx); return; }
  r -= a.T * q.nb_idx;
  if (r < q.nb_dense) { dense_item(q.dense, q.dst_dense, (int64_t)q.bs * a.m_den, r); return; }
  r -= q.nb_dense;
  const InWgt& w = aw.w[qi];
  if (r >= a.T * w.nb_wgt) return;
  const int t = r / w.nb_wgt, c = r % w.nb_wgt;
  if (w.dtype == DRS_TABLE_FP32) weights_item<DRS_TABLE_FP32>(w, a.cap, q.n_idx, t, c);
  else if (w.dtype == DRS_TABLE_FP16) weights_item<DRS_TABLE_FP16>(w, a.cap, q.n_idx, t, c);
  else weights_item<DRS_TABLE_BF16>(w, a.cap, q.n_idx, t, c);
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

int64_t plan_input_pass_weighted(InPassWgtArgs& aw) {
  InPassArgs& a = aw.in;
  (void)plan_input_pass(a);       // nb_idx, nb_dense
  int32_t nb_idx[DRS_MAX_COALESCE], nb_dense[DRS_MAX_COALESCE], nb_wgt[DRS_MAX_COALESCE];
  for (int i = 0; i < a.n_q; ++i) {
    aw.w[i].nb_wgt = aw.w[i].src ? wgt_chunks(a.q[i].n_idx) : 0;
    nb_idx[i] = a.q[i].nb_idx; nb_dense[i] = a.q[i].nb_dense; nb_wgt[i] = aw.w[i].nb_wgt;
  }
  return plan_weighted_grid(a.n_q, a.T, nb_idx, nb_dense, nb_wgt, a.wg0);
}

hipError_t launch_input_pass_weighted(const InPassWgtArgs& a, int64_t grid, hipStream_t stream) {
  if (grid <= 0) return hipSuccess;
  hipLaunchKernelGGL(input_pass_weighted_kernel, dim3((unsigned)grid), dim3(kInPassThreads), 0, stream, a);
  return hipGetLastError();
}

}  // namespace drs
