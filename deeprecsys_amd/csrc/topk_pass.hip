// libdrs_hip.so: the top-k pass on the device (include/drs_device_topk.h).  ONE launch per launch set, behind the set's last
// kernel: workgroup i hands back, for query i of the set, the k_i samples that rank first by one score column -- their row
// numbers and their full score rows -- from the slot's [Mv, n_out] buffer.  The arguments travel by value in the kernarg
// (TopKArgs); topk_plan.h states the order (a 64-bit key per sample: unique results) and the steps of the selection.
//
// Rank by counting in LDS: every thread builds the keys of its rows and stores them to LDS; behind one barrier it counts, for
// each key it owns, the keys in LDS that exceed it -- every lane reads the same 16 bytes, two keys per broadcast read, eight
// reads in flight (a step's keys are padded to 16 with the sentinel) -- and a key of rank < k goes to position `rank` of the winners.  At most 16 workgroups of 256 threads: the pass is bound by its
// launch and by LDS latency, not by bandwidth (bs 256: 128 reads per thread; bs 1 024: 512 reads for four keys).  A query
// beyond kTopKTile rows streams its tiles against the carried winners (topk_plan.h: not the fast path).
//
// A set whose arrays were wrong (the slot's device error word is non-zero) was computed from clamped rows: every index is
// then -1 and every score the quiet NaN kOutPassNaN -- the output pass's rule, for the same reason.
#include "drs_internal.h"
#include "topk_plan.h"

namespace drs {

static_assert(kTopKQueries == DRS_MAX_COALESCE, "TopKArgs holds one entry per query of a launch set");

namespace {

// the ranks of the NK keys a thread owns among keys[0 .. m) (m a multiple of kTopKPad): one pass over LDS serves all of them,
// kTopKPad / 2 reads in flight at a time
template <int NK>
__device__ __forceinline__ void rank_keys(const uint64_t* keys, int m, const uint64_t (&mine)[kTopKKeys / kTopKThreads],
                                          int (&rank)[kTopKKeys / kTopKThreads]) {
  constexpr int kPairs = kTopKPad / 2;
  int cnt[NK];
#pragma unroll
  for (int j = 0; j < NK; ++j) cnt[j] = 0;
  const ulonglong2* pairs = reinterpret_cast<const ulonglong2*>(keys);
  for (int i = 0; i < m / 2; i += kPairs) {
    ulonglong2 p[kPairs];
#pragma unroll
    for (int u = 0; u < kPairs; ++u) p[u] = pairs[i + u];      // (the same address in every lane: a broadcast read of 16 bytes)
#pragma unroll
    for (int u = 0; u < kPairs; ++u)
#pragma unroll
      for (int j = 0; j < NK; ++j) cnt[j] += (int)(p[u].x > mine[j]) + (int)(p[u].y > mine[j]);
  }
#pragma unroll
  for (int j = 0; j < NK; ++j) rank[j] = cnt[j];
}

__global__ __launch_bounds__(kTopKThreads) void topk_pass_kernel(const TopKArgs a) {
  constexpr int kOwn = kTopKKeys / kTopKThreads;      // key positions a thread owns: tid, tid + 256, ...
  __shared__ __attribute__((aligned(16))) uint64_t keys[kTopKKeys];
  const int tid = (int)threadIdx.x;
  const TopKQuery& q = a.q[blockIdx.x];
  const int bs = q.bs, k = q.k, n_out = a.n_out;
  const uint32_t* __restrict__ src = reinterpret_cast<const uint32_t*>(q.src);
  uint32_t* __restrict__ top = reinterpret_cast<uint32_t*>(q.top);
  const bool failed = a.err != nullptr && *a.err != 0;      // (one word, the same for every lane of every workgroup of the set)

  if (!failed) {
    int c = 0;                                        // winners carried so far: keys[0 .. c), descending
    for (int64_t t = 0; t < topk_steps(bs); ++t) {
      const int n = topk_tile_rows(bs, t);
      for (int i = tid; i < n; i += kTopKThreads) {
        const int64_t r = t * kTopKTile + i;
        keys[c + i] = topk_key(src[r * q.stride + a.col], r);
      }
      const int m = c + n, m2 = topk_padded(m);
      if (tid < m2 - m) keys[m + tid] = 0;            // the sentinel: it exceeds no key
      __syncthreads();
      uint64_t mine[kOwn];
      int rank[kOwn];
#pragma unroll
      for (int j = 0; j < kOwn; ++j) {
        const int p = tid + j * kTopKThreads;
        mine[j] = p < m ? keys[p] : ~(uint64_t)0;     // (nothing exceeds it; its rank is not read)
        rank[j] = 0;
      }
      const int own = (m + kTopKThreads - 1) / kTopKThreads;      // uniform: positions in use per thread
      if (own <= 1) rank_keys<1>(keys, m2, mine, rank);
      else if (own <= 2) rank_keys<2>(keys, m2, mine, rank);
      else if (own <= 4) rank_keys<4>(keys, m2, mine, rank);
      else rank_keys<kOwn>(keys, m2, mine, rank);
      __syncthreads();                                // every count is made: the winners may take the keys' places
#pragma unroll
      for (int j = 0; j < kOwn; ++j)
        if (tid + j * kTopKThreads < m && rank[j] < k) keys[rank[j]] = mine[j];
      c = m < k ? m : k;
      __syncthreads();
    }
  }

  // the winners' rows sit in LDS by rank: k * n_out floats, coalesced along the row, then the k row numbers
  const int64_t total = (int64_t)k * n_out;
  for (int64_t e = tid; e < total; e += kTopKThreads) {
    const int64_t w = e / n_out;
    uint32_t v = kOutPassNaN;
    if (!failed) {
      uint32_t r = topk_key_row(keys[w]);
      r = r < (uint32_t)bs ? r : 0u;                  // (never taken: a winner is a row of the query; no read leaves it)
      v = src[(int64_t)r * q.stride + (e - w * n_out)];
    }
    top[e] = v;
  }
  for (int w = tid; w < k; w += kTopKThreads) q.idx[w] = failed ? -1 : (int32_t)topk_key_row(keys[w]);
}

}  // namespace

hipError_t launch_topk_pass(const TopKArgs& a, hipStream_t stream) {
  if (a.n_q <= 0) return hipSuccess;
  hipLaunchKernelGGL(topk_pass_kernel, dim3((unsigned)a.n_q), dim3(kTopKThreads), 0, stream, a);
  return hipGetLastError();
}

}  // namespace drs
