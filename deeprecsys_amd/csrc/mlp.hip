// FC / MLP / dot-interaction kernels for gfx950 on the fp32 matrix cores.
//
// Replaces the FC + Relu|Sigmoid operator pairs of create_mlp (reference
// models/dlrm_s_caffe2.py:223-279) and the Concat/BatchMatMul/Flatten/BatchGather/
// Concat chain of create_interactions (:331-365).
//
// Arithmetic contract (see oracle/drs_oracle.c): every output element is
//     act( fma-chain over k = 0..K-1 in order, starting from 0 )  + bias
// v_mfma_f32_16x16x4_f32 is bit-for-bit a k-ordered fp32 fma chain, and the
// operands are fed so that MFMA step s carries k = 4s .. 4s+3, so GPU and oracle
// agree bitwise up to the final expf of the sigmoid.
//
// Tiling: a workgroup (8 waves) owns a 16-row slab of the batch and 128 output
// columns at a time (one 16x16 tile per wave).  W (stored [N, K], K contiguous --
// already the "B^T" layout MFMA wants) streams through LDS in 64-deep K chunks; rows
// are padded to 68 floats and rows 8..15 stored at k^2 so the per-lane ds_read_b32
// operand fetches are conflict free.  The activations of a slab never leave LDS
// between layers.  Three kernels share this contract:
//   stream_kernel  all layers of one or two chains as ONE prefetched sequence of weight
//                  tiles (the default)
//   chain_kernel   per-layer passes (fallback: widths not a multiple of 4, inputs too
//                  wide for an LDS slab)
//   fc_kernel      one layer on a 2-D grid (fallback of gemm.hip's gemm_kernel)
#include "mlp_stream.h"

namespace drs {
namespace {


// K chunk staged per step is a template parameter KC in {64, 128, 192, 256}: a dependent
// global-load round costs ~1 us on this chip (Infinity-Cache latency; per-XCD L2s start
// cold every launch), far more than the MFMAs it feeds, so layers are cut into as few
// rounds as LDS allows.  Rows of a staged chunk are padded to KC+4 floats.


struct LayerIo {
  const float* a_glb;   // A operand in global memory (first layer) or nullptr
  int64_t lda_glb;
  int64_t a_row0;       // first row of this slab inside a_glb ...
  int64_t a_rows;       // ... which has this many valid rows
  const float* a_lds;   // A operand: activation slab in LDS (later layers) or nullptr
  int lda_lds;
  float* o_glb;         // output to global (last layer) or nullptr
  int64_t ldo_glb;
  float* o_lds;         // output slab in LDS or nullptr
  int ldo_lds;
  bool o_sc1;           // outputs of the query's LAST layer: write-through (agent-scope) stores,
                        // so publishing them to the last-arriving workgroup needs no L2 write-back fence
};

// One layer for the block's 16 rows [m0, m0+16) and the columns [n_begin, n_end).
// The workgroup is 8 waves (512 threads): a pass covers 128 columns, wave w owns the
// 16-column tile at n0 + 16w (on layers narrower than 128 the upper waves only help with
// the staging).  Two waves per SIMD is the point: with one wave per SIMD the ~390
// instructions of a K-chunk round (address math, selects, LDS traffic around only 32
// MFMAs) issue back to back with nothing to hide their latencies -- the in-kernel
// timeline showed 3.6 k cycles per round against 1 k cycles of MFMA.  Eight waves split the
// same round into streams half as long that interleave on each SIMD.
// Every output element is one k-ordered fma chain.
// sA: [nbuf][16][KC+4] (used only when A comes from global), sB: [nbuf][128][KC+4];
// nbuf = 2 (double buffered) when the layer needs more than one K chunk, else 1.
constexpr int kThreads = 512;
constexpr int PN = kFcPassCols;          // columns per pass (8 waves x 16)

template <bool A_LDS, bool O_LDS, bool VEC, int KC>
__device__ __forceinline__ void layer_pass(const LayerIo io, int64_t m0, int64_t M, int K,
                                           const float* __restrict__ W, int64_t ldw,
                                           const float* __restrict__ bias, int N, int n_begin,
                                           int n_end, int act, int nbuf, float* sA, float* sB TL_PARAM) {
  constexpr int BMK = 16;
  constexpr int LD = KC + 4;
  constexpr int QPR = KC / 4;                       // float4 per staged row
  constexpr int NA = (16 * QPR + kThreads - 1) / kThreads;   // float4 of A per thread per chunk (KC=64: half the threads)
  constexpr int NB = PN * QPR / kThreads;           // float4 of W per thread per chunk
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int r = lane & 15;   // row of A / column of the tile
  const int g = lane >> 4;   // k within an MFMA step
  const int n_chunks = (K + KC - 1) / KC;

  for (int n0 = n_begin; n0 < n_end; n0 += PN) {
    const bool my_tile = n0 + wave * 16 < n_end;    // wave-uniform: is there a tile for me?
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    float4 ra[NA], rb[NB];
    auto fetch = [&](int kc) {
#pragma unroll
      for (int i = 0; i < NA; ++i) {
        const int idx = min(tid + i * kThreads, 16 * QPR - 1);
        if (!A_LDS) ra[i] = load4_raw<VEC>(io.a_glb, io.lda_glb, io.a_row0 + idx / QPR, io.a_rows, kc + (idx % QPR) * 4, K);
      }
#pragma unroll
      for (int i = 0; i < NB; ++i) {
        const int idx = tid + i * kThreads;
        rb[i] = load4_raw<VEC>(W, ldw, n0 + idx / QPR, N, kc + (idx % QPR) * 4, K);
      }
    };
    auto stash = [&](int buf, int kc) {
      const bool tail = kc + KC > K;              // uniform: only the last chunk needs the k mask
#pragma unroll
      for (int i = 0; i < NA; ++i) {
        const int idx = tid + i * kThreads;
        const int row = idx / QPR, k = (idx % QPR) * 4;
        if (!A_LDS && idx < 16 * QPR)
          *reinterpret_cast<float4*>(sA + (buf * BMK + row) * LD + k) =
              swz4(tail ? mask4(ra[i], kc + k, K) : ra[i], row);
      }
#pragma unroll
      for (int i = 0; i < NB; ++i) {
        const int idx = tid + i * kThreads;
        const int row = idx / QPR, k = (idx % QPR) * 4;
        *reinterpret_cast<float4*>(sB + (buf * PN + row) * LD + k) =
            swz4(tail ? mask4(rb[i], kc + k, K) : rb[i], row);
      }
    };
    TL(1);
    fetch(0);
    TL(2);
    stash(0, 0);
    TL(3);
    __syncthreads();
    TL(4);

    for (int c = 0; c < n_chunks; ++c) {
      const int buf = c & (nbuf - 1);
      const bool more = c + 1 < n_chunks;
      TL(10);
      if (more) fetch((c + 1) * KC);   // next chunk's global loads fly during the MFMAs
      TL(11);

      if (my_tile) {
        const int gs = swz(g, r);                         // see swz4: rows 8..15 live at k^2
        const float* pa = A_LDS ? io.a_lds + r * io.lda_lds + c * KC + gs
                                : sA + (buf * BMK + r) * LD + gs;
        const float* pb = sB + (buf * PN + wave * 16 + r) * LD + gs;
        const int ksteps = min(KC, K - c * KC + 3) / 4;   // steps that carry real k
        // Only the last chunk of an LDS activation slab can hold stale columns past K (staged
        // chunks are zero filled there): keep the select out of the steady state.
        const bool a_tail = A_LDS && (c + 1) * KC > K;
        // operands of 16 steps (64 k) are read together (one counted lgkmcnt stream), then
        // their 16 MFMAs; the SIMD's second wave covers the LDS latency in between
#pragma unroll
        for (int sg = 0; sg < KC / 64; ++sg) {
          if (16 * sg < ksteps) {                           // uniform
            float av[16], bv[16];
#pragma unroll
            for (int s = 0; s < 16; ++s) {
              av[s] = pa[4 * (16 * sg + s)];
              bv[s] = pb[4 * (16 * sg + s)];
            }
            if (a_tail) {
#pragma unroll
              for (int s = 0; s < 16; ++s) av[s] = (c * KC + 4 * (16 * sg + s) + g < K) ? av[s] : 0.f;
            }
            // fma(0, 0, acc) == acc, so a padded step is exact; skip groups of 4 uniformly
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              if (16 * sg + 4 * q < ksteps) {
#pragma unroll
                for (int s = 4 * q; s < 4 * q + 4; ++s)
                  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[s], bv[s], acc, 0, 0, 0);
              }
            }
          }
        }
      }
      TL(12);
      if (more) stash(buf ^ 1, (c + 1) * KC);
      TL(13);
      __syncthreads();
      TL(14);
    }

    // epilogue: bias + activation; lane holds rows g*4+i of its tile, column r
    const int col = n0 + wave * 16 + r;
    if (my_tile && col < N) {
      const float bcol = bias ? bias[col] : 0.f;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int row = g * 4 + i;
        const float v = act_apply(acc[i] + bcol, act);
        if (O_LDS) {
          io.o_lds[row * io.ldo_lds + swz(col, row)] = v;
        } else if (m0 + row < M) {
          float* dst = io.o_glb + (m0 + row) * io.ldo_glb + col;
          if (io.o_sc1) __hip_atomic_store(dst, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          else *dst = v;
        }
      }
    }
  }
}


// Single layer, 2-D grid: blockIdx.x = 16-row slab, blockIdx.y = 128-column group.
template <bool VEC, int KC>
__global__ __launch_bounds__(512) void fc_kernel(const float* __restrict__ x, int64_t ldx, int64_t M,
                                                 int K, const float* __restrict__ W, int64_t ldw,
                                                 const float* __restrict__ b, int N, int act,
                                                 float* __restrict__ y, int64_t ldy, int nbuf,
                                                 Done done, XSrc xs) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* sA = smem;                              // [nbuf][16][KC+4]
  float* sB = sA + nbuf * 16 * (KC + 4);         // [nbuf][128][KC+4]
#ifdef DRS_TIMELINE
  unsigned long long* g_tl_lds = reinterpret_cast<unsigned long long*>(sB + nbuf * PN * (KC + 4));
  if (threadIdx.x == 0) g_tl_lds[0] = 0;
#endif
  LayerIo io = {x, ldx, 0, 0, nullptr, 0, y, ldy, nullptr, 0, done.counter != nullptr};
  resolve_src(xs, x, M, (int64_t)blockIdx.x * 16, &io.a_glb, &io.a_row0, &io.a_rows);
  const int n0 = blockIdx.y * PN;
  layer_pass<false, false, VEC, KC>(io, (int64_t)blockIdx.x * 16, M, K, W, ldw, b, N, n0,
                                    min(n0 + PN, N), act, nbuf, sA, sB TL_ARG);
#ifdef DRS_TIMELINE
  if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) {
    const unsigned n = (unsigned)g_tl_lds[0];
    unsigned base = g_tl_n;
    for (unsigned i = 0; i < n && base + i < 16384; ++i) g_tl[base + i] = g_tl_lds[i + 1];
    g_tl_n = base + n;
  }
#endif
  signal_done(done, gridDim.x * gridDim.y, smem);
}

// One chain of layers on the block's 16 rows; activations ping-pong between two LDS slabs.
//
// The chain's input rows are streamed exactly once by exactly one workgroup, so every
// chunk of them is a compulsory miss all the way to HBM / Infinity Cache (~2 us) that a
// one-chunk-ahead prefetch cannot hide.  When they fit (slabA != nullptr) all 16 x K0
// inputs are therefore pulled into LDS with ONE round of loads up front and the first
// layer reads its A operand from LDS like every later layer; only the weights (shared by
// all workgroups, L2 resident after the warm-up) keep streaming per K chunk.
template <bool VEC, int KC>
__device__ __forceinline__ void run_chain(const ChainArgs& a, const XSrc& xs, int64_t m0, int slab_ld,
                                          int nbuf, float* sA, float* sB, float* slab0, float* slab1,
                                          float* slabA, int ldA, bool publish TL_PARAM) {
  float* cur = nullptr;
  const int K0 = a.width[0];
  const bool pre = slabA != nullptr && K0 <= 640;
  if (pre) {
    const float* base; int64_t row0, rows;
    resolve_src(xs, a.x, a.M, m0, &base, &row0, &rows);
    const int qpr = (K0 + 3) / 4;                 // float4 per row
    const int total = 16 * qpr;
    float4 v[5];
#pragma unroll
    for (int i = 0; i < 5; ++i) {
      const int idx = min((int)threadIdx.x + i * kThreads, total - 1);
      v[i] = load4_raw<VEC>(base, a.ldx, row0 + idx / qpr, rows, (idx % qpr) * 4, K0);
    }
#pragma unroll
    for (int i = 0; i < 5; ++i) {
      const int idx = threadIdx.x + i * kThreads;
      if (idx < total)
        *reinterpret_cast<float4*>(slabA + (idx / qpr) * ldA + (idx % qpr) * 4) =
            swz4(mask4(v[i], (idx % qpr) * 4, K0), idx / qpr);
    }
    __syncthreads();
  }
  for (int l = 0; l < a.n_layers; ++l) {
    const bool first = l == 0, last = l == a.n_layers - 1;
    const bool a_lds = !first || pre;
    float* nxt = (l & 1) ? slab1 : slab0;
    LayerIo io;
    io.a_glb = nullptr;
    io.a_row0 = io.a_rows = 0;
    if (first && !pre) resolve_src(xs, a.x, a.M, m0, &io.a_glb, &io.a_row0, &io.a_rows);
    io.lda_glb = a.ldx;
    io.a_lds = first ? (pre ? slabA : nullptr) : cur;
    io.lda_lds = first ? ldA : slab_ld;
    io.o_glb = last ? a.y : nullptr;
    io.ldo_glb = a.ldy;
    io.o_lds = last ? nullptr : nxt;
    io.ldo_lds = slab_ld;
    io.o_sc1 = last && publish;
    const int K = a.width[l], N = a.width[l + 1];
#define DRS_PASS(AL, OL)                                                                          \
  layer_pass<AL, OL, VEC, KC>(io, m0, a.M, K, a.W[l], K, a.b[l], N, 0, N, a.act[l], nbuf, sA, sB TL_ARG)
    if (!a_lds && last) { DRS_PASS(false, false); }
    else if (!a_lds) { DRS_PASS(false, true); }
    else if (last) { DRS_PASS(true, false); }
    else { DRS_PASS(true, true); }
#undef DRS_PASS
    __syncthreads();
    cur = nxt;
  }
}

// Up to two chains back to back in ONE launch on the same 16 rows: the bottom MLP
// (dense features -> dense_out slot of the interaction buffer) and, for the "cat"
// interaction, the top MLP that reads that buffer.  The second chain re-reads rows this
// very workgroup wrote: a workgroup-scope fence + barrier orders that.
template <bool VEC, int KC>
__global__ __launch_bounds__(512) void chain_kernel(ChainArgs a0, ChainArgs a1, int slab_ld, int nbuf,
                                                    int ldA, Done done, XSrc xs) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* sA = smem;                              // [nbuf][16][KC+4]
  float* sB = sA + nbuf * 16 * (KC + 4);         // [nbuf][128][KC+4]
  float* slab0 = sB + nbuf * PN * (KC + 4);      // [16][slab_ld]
  float* slab1 = slab0 + 16 * slab_ld;
  float* slabA = ldA > 0 ? slab1 + 16 * slab_ld : nullptr;   // [16][ldA] preloaded chain input
#ifdef DRS_TIMELINE
  unsigned long long* g_tl_lds = reinterpret_cast<unsigned long long*>(slab1 + 16 * slab_ld + (ldA > 0 ? 16 * ldA : 0));
  if (threadIdx.x == 0) g_tl_lds[0] = 0;
#endif
  const int64_t m0 = (int64_t)blockIdx.x * 16;

  // L2 warm-up.  All workgroups walk the same weights in lock step, so without help every
  // K chunk is a compulsory miss in each XCD's L2 (the gather before us has flushed it) and
  // every staging round pays a full Infinity-Cache/HBM latency (~2 us, measured: waves 53%
  // in s_waitcnt).  Here each workgroup touches ONE slice of all the weights, one load per
  // 128-B line, fire-and-forget: the XCD's 16 or so resident workgroups together pull the
  // whole set into their L2 during the first layer's prologue.  Purely a hint: a different
  // workgroup->XCD placement changes speed, not results.
  float warm[2 * DRS_MAX_CHAIN];   // consumed only at the very end: never waited for early
  {
    const unsigned part = (blockIdx.x >> 3) & 15;          // my rank among the XCD's workgroups
    auto touch = [&](const ChainArgs& c, int l) -> float {
      if (l >= c.n_layers) return 0.f;
      const int64_t lines = ((int64_t)c.width[l] * c.width[l + 1] + 31) / 32;   // 128-B lines
      // 16 parts x 512 threads x 1 line: covers 1 MB per layer (all of RM1/RM2's layers)
      const int64_t i = min(lines - 1, (int64_t)part * kThreads + threadIdx.x + (int64_t)(blockIdx.x >> 7) * 16 * kThreads);
      return c.W[l][i * 32];
    };
#pragma unroll
    for (int l = 0; l < DRS_MAX_CHAIN; ++l) {
      warm[l] = touch(a0, l);
      warm[DRS_MAX_CHAIN + l] = touch(a1, l);
    }
  }

  // zero both slabs once: padded K tails of later layers must read finite values
  for (int i = threadIdx.x; i < 2 * 16 * slab_ld; i += blockDim.x) slab0[i] = 0.f;
  __syncthreads();

  run_chain<VEC, KC>(a0, xs, m0, slab_ld, nbuf, sA, sB, slab0, slab1, slabA, ldA,
                     done.counter != nullptr && a1.n_layers == 0 TL_ARG);
  if (a1.n_layers > 0) {
    __threadfence_block();
    __syncthreads();
    XSrc none;
    none.q.n_q = 0;
    run_chain<VEC, KC>(a1, none, m0, slab_ld, nbuf, sA, sB, slab0, slab1, slabA, ldA,
                       done.counter != nullptr TL_ARG);
  }
#pragma unroll
  for (int l = 0; l < 2 * DRS_MAX_CHAIN; ++l) asm volatile("" ::"v"(warm[l]));
#ifdef DRS_TIMELINE
  if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) {
    const unsigned n = (unsigned)g_tl_lds[0];
    unsigned base = g_tl_n;
    for (unsigned i = 0; i < n && base + i < 16384; ++i) g_tl[base + i] = g_tl_lds[i + 1];
    g_tl_n = base + n;
  }
#endif
  signal_done(done, gridDim.x, smem);
}

// The packed twin of a layer's weights (stream_kernel<true>): tile (pass p, chunk c) = 8192 floats,
// wave w's block = 1024, float4 q of lane (r, g) = { W[128 p + 16 w + r][64 c + 16 q + 4 j + g] : j = 0..3 },
// i.e. element j of float4 q is the B operand of MFMA step s = 4 q + j (k = 64 c + 4 s + g: natural
// k order); rows beyond N and k beyond K are zeros.
__global__ __launch_bounds__(512) void pack_stream_kernel(const float* __restrict__ W, int K, int N,
                                                          float* __restrict__ Wp) {
  const int nch = (K + 63) >> 6;
  const int tile = blockIdx.x, p = tile / nch, c = tile - p * nch;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int row = 128 * p + 16 * wave + r;
  float* o = Wp + (size_t)tile * 8192 + wave * 1024 + lane * 4;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    float4 v;
    float* vv = reinterpret_cast<float*>(&v);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int k = 64 * c + 16 * q + 4 * j + g;
      vv[j] = (row < N && k < K) ? W[(size_t)row * K + k] : 0.f;
    }
    *reinterpret_cast<float4*>(o + q * 256) = v;
  }
}

// ---------------------------------------------------------------------------
// dot interaction: one wave per sample.  T[b] is [F, D]; Z = T T^T is computed
// in 16x16 MFMA tiles (A and B operands are the same register: B[k][j] = T[j][k]),
// the strictly-lower (or lower, with `itself`) triangle is scattered in the
// row-major BatchGather order i*(i-1)/2 + j (resp. i*(i+1)/2 + j) behind a copy
// of the dense row T[b][0][:].
__global__ __launch_bounds__(256) void interact_dot_kernel(const float* __restrict__ T, int64_t ldt,
                                                           int64_t B, int F, int D, int itself,
                                                           float* __restrict__ R, int64_t ldr) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int64_t b = (int64_t)blockIdx.x * 4 + wave;
  const int Fp = (F + 15) & ~15;
  const int ldl = D + 1;                       // odd stride: conflict-free column reads
  float* t = smem + (size_t)wave * Fp * ldl;
  if (b >= B) return;                          // whole wave exits together
  const float* src = T + b * ldt;
  for (int i = lane; i < Fp * D; i += 64) {
    const int f = i / D, d = i - f * D;
    t[f * ldl + d] = f < F ? src[(int64_t)f * D + d] : 0.f;
  }
  __builtin_amdgcn_wave_barrier();
  float* out = R + b * ldr;
  for (int d = lane; d < D; d += 64) out[d] = t[d];
  const int r = lane & 15, g = lane >> 4;
  const int ksteps = (D + 3) / 4;
  for (int ti = 0; ti < Fp; ti += 16)
    for (int tj = 0; tj <= ti; tj += 16) {
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      for (int s = 0; s < ksteps; ++s) {
        const int k = 4 * s + g;
        const float av = k < D ? t[(ti + r) * ldl + k] : 0.f;
        const float bv = k < D ? t[(tj + r) * ldl + k] : 0.f;
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc, 0, 0, 0);
      }
      const int j = tj + r;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int i = ti + g * 4 + q;
        if (i < F && (itself ? j <= i : j < i)) {
          const int p = itself ? i * (i + 1) / 2 + j : i * (i - 1) / 2 + j;
          out[D + p] = acc[q];
        }
      }
    }
}

__global__ void add_rows_kernel(const float* __restrict__ a, int64_t lda, const float* __restrict__ b,
                                int64_t ldb, float* __restrict__ o, int64_t ldo, int64_t M, int D) {
  const int64_t n = M * D;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t m = i / D;
    const int d = (int)(i - m * D);
    const float v = b ? a[m * lda + d] + b[m * ldb + d] : a[m * lda + d];
    o[m * ldo + d] = v;
  }
}

// Dense rows of up to DRS_MAX_COALESCE coalesced queries (one staged array per query) -> their virtual rows
// of the concat buffer, in ONE launch (W&D has no bottom MLP: models/wide_and_deep.py:271-281).
// V = 4: 16 bytes per thread (m_den, ldo multiples of 4, every pointer 16-byte aligned) -- the owner lookup below
// is per THREAD, and at a dword per thread it made W&D's 4 096 x 512 copy a 23-us launch (0.7 TB/s).
template <int V>
__global__ void copy_rows_multi_kernel(XSrc xs, int m_den, float* __restrict__ o, int64_t ldo) {
  const int64_t Mv = xs.q.vstart[xs.q.n_q];
  const int mv = m_den / V;
  const int64_t n = Mv * mv;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t v = i / mv;
    const int d = (int)(i - v * mv) * V;
    const float* p = xs.x[0];
    int lo = xs.q.vstart[0], nb = xs.q.bs[0];
#pragma unroll
    for (int k = 1; k < 8; ++k) {
      const bool in = k < xs.q.n_q && v >= xs.q.vstart[k];
      p = in ? xs.x[k] : p;
      lo = in ? xs.q.vstart[k] : lo;
      nb = in ? xs.q.bs[k] : nb;
    }
    if (xs.q.n_q > 8) {   // (launch sets of 9 .. 16 queries only: smaller ones never touch the upper half of the argument arrays)
#pragma unroll
      for (int k = 8; k < DRS_MAX_COALESCE; ++k) {
        const bool in = k < xs.q.n_q && v >= xs.q.vstart[k];
        p = in ? xs.x[k] : p;
        lo = in ? xs.q.vstart[k] : lo;
        nb = in ? xs.q.bs[k] : nb;
      }
    }
    const int64_t r = v - lo;
    if (r < nb) {
      if (V == 4) *reinterpret_cast<float4*>(o + v * ldo + d) = *reinterpret_cast<const float4*>(p + r * m_den + d);
      else o[v * ldo + d] = p[r * m_den + d];
    }
  }
}

}  // namespace

int64_t stream_packed_floats(int K, int N) {
  if (K <= 0 || N <= 0) return 0;
  return (int64_t)((N + 127) / 128) * ((K + 63) / 64) * 8192;
}

hipError_t launch_pack_stream_weights(const float* W, int32_t K, int32_t N, float* Wp, hipStream_t s) {
  const unsigned tiles = (unsigned)(((N + 127) / 128) * ((K + 63) / 64));
  if (!tiles) return hipSuccess;
  hipLaunchKernelGGL(pack_stream_kernel, dim3(tiles), dim3(512), 0, s, W, K, N, Wp);
  return hipGetLastError();
}

#define DRS_FOR_EACH_KC(X) X(64) X(128) X(192) X(256)

// HIP function attributes are per device: device_init() (engine.hip) calls this once for
// every device an engine is created on.
hipError_t mlp_set_attrs() {
  hipError_t e = hipSuccess;
#define SET_ATTR(KC_)                                                               \
  if (e == hipSuccess) e = set_max_lds(fc_kernel<true, KC_>);                       \
  if (e == hipSuccess) e = set_max_lds(fc_kernel<false, KC_>);                      \
  if (e == hipSuccess) e = set_max_lds(chain_kernel<true, KC_>);                    \
  if (e == hipSuccess) e = set_max_lds(chain_kernel<false, KC_>);
  DRS_FOR_EACH_KC(SET_ATTR)
#undef SET_ATTR
  if (e == hipSuccess) e = stream8_set_attrs();
  if (e == hipSuccess) e = stream4_set_attrs();
  if (e == hipSuccess) e = set_max_lds(interact_dot_kernel);
  return e;
}

// DRS_TIMELINE builds: the mlp.hip / stream kernels stamp into 8 KB behind the LDS they use
static size_t launch_lds(const MlpPlan& p) {
#ifdef DRS_TIMELINE
  if (p.form < MlpForm::gemm) return p.lds + 8192;
#endif
  return p.lds;
}

hipError_t launch_plan(const MlpPlan& p, const Tune& tune, hipStream_t s) {
  static const char* const names[] = {
      "stream4_kernel", "stream4_kernel<sum>", "stream4_kernel<2cu>", "stream4_kernel<rows32>", "stream4_kernel<nsplit2>",
      "stream4_kernel<nsplit4>", "stream4_kernel<rows32,nsplit2>", "stream4_kernel<rows32,nsplit4>", "stream_kernel<packed>",
      "stream_kernel<packed,2cu>", "stream_kernel<lds>", "chain_kernel", "fc_kernel", "gemm_kernel", "gemm_kernel",
      "gemm32_kernel", "gemm32_kernel", "gemm32_kernel", "gemm_bf16_kernel", "fused_bf16_kernel", "fused_bf16_kernel<sum>"};
  const char* name = names[(int)p.form];
  const size_t lds = launch_lds(p);
  const int K = p.a.width[0], N = p.a.width[1];
  // which form serves this launch (drs_last_dispatch; DESIGN.md dispatch table)
  if (p.form < MlpForm::chain)
    log_launch(tune.log, "%s[%u wg, %d layers%s, %zu B lds]", name, p.grid_x, p.sa.n_layers, p.sa.inter_on ? ", dot" : "", lds);
  else if (p.form == MlpForm::chain)
    log_launch(tune.log, "%s<%s,%d>[%u wg, %d layers]", name, p.vec ? "vec" : "scalar", p.kc, p.grid_x, p.a.n_layers + p.b.n_layers);
  else if (p.form == MlpForm::fc)
    log_launch(tune.log, "%s<%s,%d>[%u x %u wg, %dx%d]", name, p.vec ? "vec" : "scalar", p.kc, p.grid_x, p.grid_y, K, N);
  else if (p.form == MlpForm::fused_bf16 || p.form == MlpForm::fused_bf16_sum)
    log_launch(tune.log, "%s[%u wg, %d layers, %d bf16%s, %zu B lds]", name, p.grid_x, p.fa.n_layers, p.fa.n_bf16, p.fa.dot ? ", dot" : "", lds);
  else if (p.form == MlpForm::gemm_bf16)
    log_launch(tune.log, "%s<%dx%d%s>[%u x %u wg, %dx%d]", name, 32 * p.tm, 32 * p.tn, p.vec ? "" : ",scalar", p.grid_x, p.grid_y, K, N);
  else if (p.form == MlpForm::gemm32_split)
    log_launch(tune.log, "%s<%d,%d,sbase,split%d>[%u x %u wg, %dx%d]", name, p.tm, p.tn, p.xs.ksplit, p.grid_x, p.grid_y, K, N);
  else
    log_launch(tune.log, "%s<%d,%d%s>[%u x %u wg, %dx%d]", name, p.tm, p.tn,
               p.form == MlpForm::gemm_2cu ? ",2cu" : p.form == MlpForm::gemm32_sbase ? ",sbase" : "", p.grid_x, p.grid_y, K, N);
  const dim3 grid(p.grid_x, p.grid_y);
  switch (p.form) {
    case MlpForm::chain:
#define LAUNCH(KC_)                                                                                                        \
  if (p.kc == KC_) {                                                                                                       \
    if (p.vec)                                                                                                             \
      hipLaunchKernelGGL((chain_kernel<true, KC_>), grid, dim3(kThreads), lds, s, p.a, p.b, p.sld, p.nbuf, p.lda, p.done, p.xs);  \
    else                                                                                                                   \
      hipLaunchKernelGGL((chain_kernel<false, KC_>), grid, dim3(kThreads), lds, s, p.a, p.b, p.sld, p.nbuf, p.lda, p.done, p.xs); \
  }
      DRS_FOR_EACH_KC(LAUNCH)
#undef LAUNCH
      return hipGetLastError();
    case MlpForm::fc: {
      const ChainArgs& L = p.a;
#define LAUNCH(KC_)                                                                                                        \
  if (p.kc == KC_) {                                                                                                       \
    if (p.vec)                                                                                                             \
      hipLaunchKernelGGL((fc_kernel<true, KC_>), grid, dim3(kThreads), lds, s, L.x, L.ldx, L.M, K, L.W[0], (int64_t)K,      \
                         L.b[0], N, L.act[0], L.y, L.ldy, p.nbuf, p.done, p.xs);                                            \
    else                                                                                                                   \
      hipLaunchKernelGGL((fc_kernel<false, KC_>), grid, dim3(kThreads), lds, s, L.x, L.ldx, L.M, K, L.W[0], (int64_t)K,     \
                         L.b[0], N, L.act[0], L.y, L.ldy, p.nbuf, p.done, p.xs);                                            \
  }
      DRS_FOR_EACH_KC(LAUNCH)
#undef LAUNCH
      return hipGetLastError();
    }
    case MlpForm::gemm: case MlpForm::gemm_2cu: case MlpForm::gemm32: case MlpForm::gemm32_sbase: case MlpForm::gemm32_split:
      return launch_gemm(p, tune.zero, s);
    case MlpForm::gemm_bf16:
      return launch_gemm_bf16(p, s);
    case MlpForm::fused_bf16: case MlpForm::fused_bf16_sum:
      return launch_fused_bf16(p, s);
    case MlpForm::stream_packed: case MlpForm::stream_packed_2cu: case MlpForm::stream_lds:
      return launch_stream8(p, lds, s);
    default:
      return launch_stream4(p, lds, s);
  }
}

#ifdef DRS_TIMELINE
// (every MLP translation unit keeps its own stamp buffer: whichever kernel ran last has stamps to hand over)
extern "C" int drs_debug_timeline(unsigned long long* out, int cap, int reset) {
  int n = tl_fetch_stream4(out, cap, reset);
  if (n == 0) n = tl_fetch_stream8(out, cap, reset);
  if (n == 0) n = tl_fetch_here(out, cap, reset);
  return n;
}
#endif

hipError_t launch_interact_dot(const float* T, int64_t ldt, int64_t B, int32_t F, int32_t D,
                               int32_t itself, float* R, int64_t ldr, hipStream_t s) {
  if (B <= 0) return hipSuccess;
  const int Fp = (F + 15) & ~15;
  const size_t lds = sizeof(float) * 4 * (size_t)Fp * (D + 1);
  if (lds > 160 * 1024) return hipErrorInvalidValue;   // (attribute: mlp_set_attrs, per device)
  hipLaunchKernelGGL(interact_dot_kernel, dim3((unsigned)((B + 3) / 4)), dim3(256), lds, s, T, ldt,
                     B, F, D, itself, R, ldr);
  return hipGetLastError();
}

static unsigned ew_grid(int64_t n) {
  int64_t g = (n + 255) / 256;
  return (unsigned)(g < 1 ? 1 : (g > 2048 ? 2048 : g));
}

hipError_t launch_add_rows(const float* a, int64_t lda, const float* b, int64_t ldb, float* out,
                           int64_t ldo, int64_t M, int32_t D, hipStream_t s) {
  if (M <= 0) return hipSuccess;
  hipLaunchKernelGGL(add_rows_kernel, dim3(ew_grid(M * D)), dim3(256), 0, s, a, lda, b, ldb, out,
                     ldo, M, D);
  return hipGetLastError();
}

hipError_t launch_copy_rows(const float* a, int64_t lda, float* out, int64_t ldo, int64_t M,
                            int32_t D, hipStream_t s) {
  return launch_add_rows(a, lda, nullptr, 0, out, ldo, M, D, s);
}

hipError_t launch_copy_rows_multi(const XSrc& xs, int32_t m_den, float* out, int64_t ldo, hipStream_t s) {
  const int64_t Mv = xs.q.n_q > 0 ? xs.q.vstart[xs.q.n_q] : 0;
  if (Mv <= 0 || m_den <= 0) return hipSuccess;
  bool vec = !(m_den & 3) && !(ldo & 3) && aligned16(out);
  for (int i = 0; i < xs.q.n_q; ++i) vec = vec && aligned16(xs.x[i]);
  if (vec) hipLaunchKernelGGL(copy_rows_multi_kernel<4>, dim3(ew_grid(Mv * (m_den / 4))), dim3(256), 0, s, xs, m_den, out, ldo);
  else hipLaunchKernelGGL(copy_rows_multi_kernel<1>, dim3(ew_grid(Mv * m_den)), dim3(256), 0, s, xs, m_den, out, ldo);
  return hipGetLastError();
}

}  // namespace drs
