// DLRM's bottom MLP + interaction + top MLP of a 16-row slab in ONE launch, with the bf16 layers of "mlp_dtype" 2 on the
// bf16 matrix cores (engine option "mlp_bf16_fuse" 1).
//
// The one-launch structure of chain_kernel / stream4_kernel (mlp.hip, mlp_stream4.hip): a workgroup owns 16 virtual rows,
// the activations of the slab stay in LDS in fp32 from the dense rows to the last layer, the launch reads the queries' own
// dense arrays (XSrc) and signs the set off in its epilogue (Done, signal_done).  Per layer, by the rule bf16_shape(K, N):
//   bf16 layer    the contract of gemm_bf16.hip to the bit: the slab row is rounded to bf16 when it is read (the plain cast,
//                 v_cvt_pk_bf16_f32: nearest even, NaN stays NaN), the weights come from the layer's twin Wb [N, Kpad],
//                 v_mfma_f32_16x16x32_bf16 accumulates from zero with k ascending over the zero-padded K (64-deep chunks),
//                 weight rows the A operand and slab rows the B operand; fp32 bias and activation afterwards.
//   other layers  the k-ordered v_mfma_f32_16x16x4_f32 chain from zero of every fp32 form (mlp.hip), bias afterwards.
//   dot           interact_pairs_mfma (mlp_stream.h), the pairs' chains of every other form.
// An output's bits depend on its row of x and its row of W only: the launch returns what the layer-by-layer
// path returns.
//
// Weights are not staged in LDS: with ONE 16-row tile of x per workgroup every weight element is used by exactly one
// wave, once -- a lane loads its MFMA operand (16 bytes of Wb, or one float of W) straight from L2 into registers, PD
// K chunks ahead of the MFMAs that consume it.  All workgroups walk the same few hundred KB: the fire-and-forget warm-up
// of chain_kernel pulls them into each XCD's L2 during the prologue.
//
// LDS: slabs of 16 rows, 64 m + 4 floats apart (the ds_read_b128 operand reads of 16 lanes then cover 56 of the 64 banks
// once and 8 twice; MI355X LDS, 64 x 4 B banks): X0 (dense rows) | RS (dense_out | pooled rows: the cat top input or the
// dot interaction's T slab) | RI (dot: the top input) | P | Q (ping-pong layer outputs).  A layer zero-fills its output
// columns up to the next multiple of 64, so a bf16 layer's padded k reads zeros.
//
// NCF's one-launch form (Sum + MLP branch + predictor; stream_kernel<packed>'s SumArgs form in fp32) is a kernel of its
// own, fused_bf16_sum_kernel, from the same passes: no dense rows and no XSrc -- X0 is Concat(emb2, emb3) out of T, RS is
// the predictor's input [ mf = emb0 + emb1 | the branch's output ], i.e. the chain's output goes BEHIND the staged block
// (column D), not in front of it; both halves are also left in the engine's buffer (drs_fetch_interaction).
#include "mlp_stream.h"

namespace drs {
namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr int FW = 8;                 // waves per workgroup: two per SIMD, each covers the other's L2 and LDS latencies
constexpr int kFThreads = 64 * FW;
constexpr int PD = 4;                 // 64-k chunks of weights in flight per tile ahead of the MFMAs

__device__ __forceinline__ bf16x8 to_bf16x8(const float4 lo, const float4 hi) {
  bf16x8 r;
  r[0] = (__bf16)lo.x; r[1] = (__bf16)lo.y; r[2] = (__bf16)lo.z; r[3] = (__bf16)lo.w;
  r[4] = (__bf16)hi.x; r[5] = (__bf16)hi.y; r[6] = (__bf16)hi.z; r[7] = (__bf16)hi.w;
  return r;
}

__device__ __forceinline__ void store_out(float* dst, float v, bool sc1) {
  if (sc1) __hip_atomic_store(dst, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // write-through: signal_done reads it back
  else *dst = v;
}

// ... four consecutive outputs, dst 16-byte aligned.  (s_nop 1: two wait states between a store of more than 64 bits and
// a VALU write of its data registers, which the compiler does not see inside the statement: signal_done, mlp_dev.h)
__device__ __forceinline__ void store_out4(float* dst, const float (&v)[4], bool sc1) {
  const f32x4 x = {v[0], v[1], v[2], v[3]};
  if (sc1) asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" ::"v"(dst), "v"(x) : "memory");
  else *reinterpret_cast<f32x4*>(dst) = x;
}

// 16 rows x cols of a global matrix -> an LDS slab, zeros in columns [cols, cols_pad).  Row i comes from row
// min(row0 + i, rows - 1): rows past the end only feed outputs that are never stored.  All loads of a round are issued
// before its first store (one latency per round of 4 x 512 pieces, not one per piece).
template <bool VEC>
__device__ __forceinline__ void stage_rows(const float* __restrict__ base, int64_t ld, int row0, int rows, int gcol0,
                                           int cols, int cols_pad, float* dst, int dst_ld, int dst_col0) {
  constexpr int V = VEC ? 4 : 1;
  const int ppr = cols_pad / V, total = 16 * ppr;          // pieces per row (cols_pad: a multiple of 4 when VEC)
  if (total <= 0) return;
  for (int i0 = 0; i0 < total; i0 += 4 * kFThreads) {
    float4 v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int idx = min(i0 + (int)threadIdx.x + j * kFThreads, total - 1);
      const int row = idx / ppr, c = (idx - row * ppr) * V;
      const int gr = row0 + row < rows ? row0 + row : rows - 1;
      const float* q = base + (int64_t)gr * ld + gcol0 + (c < cols ? c : 0);
      if (VEC) v[j] = *reinterpret_cast<const float4*>(q);
      else v[j].x = *q;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int idx = i0 + (int)threadIdx.x + j * kFThreads;
      const int row = idx / ppr, c = (idx - row * ppr) * V;
      if (idx < total) {
        float* d = dst + row * dst_ld + dst_col0 + c;
        if (VEC) *reinterpret_cast<float4*>(d) = c < cols ? v[j] : make_float4(0.f, 0.f, 0.f, 0.f);
        else *d = c < cols ? v[j].x : 0.f;
      }
    }
  }
}

// A bf16 layer.  Wave w owns the 16-column tiles w, w + FW, ...; two of them at a time share the converted slab operand.
// Lane (r, g): A operand = bf16 k = 32 s + 8 g .. + 7 of weight row 16 t + r, B operand = the same k of slab row r;
// accumulator register q = output row r, column 16 t + 4 g + q (gemm_bf16_kernel's roles).
// SUM (fused_bf16_sum_kernel's build): the output slab may start at any column (NCF's branch output behind D columns of
// mf): 16-byte LDS stores only where they are aligned; and a lane's four outputs of a row go out as ONE 16-byte store
// where the rows allow it (NCF's predictor hands 64 floats per row over, not one: as 4-byte write-through stores, four
// lanes of a row apart, they were a quarter of a 64-byte line per instruction).
template <bool SUM>
__device__ __forceinline__ void bf16_pass(const FLayer& L, float* lds, int m0, int M, int wave, int lane) {
  const int r = lane & 15, g = lane >> 4;
  const int K = L.K, N = L.N;
  const int Kpad = (K + 63) & ~63, nch = Kpad >> 6;
  const int ntl = ((L.out_off >= 0 && L.out_pad > N ? L.out_pad : N) + 15) >> 4;
  const float* const xa = lds + L.in_off + r * L.in_ld + 8 * g;
  const float* const bias = L.b;
  float* const o_lds = L.out_off >= 0 ? lds + L.out_off + r * L.out_ld : nullptr;
  float* const o_glb = L.g_out && m0 + r < M ? L.g_out + (int64_t)(m0 + r) * L.g_ld : nullptr;
  const bool sc1 = L.g_sc1 != 0;
  const bool st4 = !SUM || !(L.out_off & 3);
  const bool g4 = SUM && !(reinterpret_cast<uintptr_t>(L.g_out) & 15) && !(L.g_ld & 3);

  auto epilogue = [&](int t, const f32x4 acc) {
    const int col = 16 * t + 4 * g;
    float v[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int cq = col + q;
      const float bq = (bias && cq < N) ? bias[cq < N ? cq : 0] : 0.f;
      v[q] = cq < N ? act_apply(acc[q] + bq, L.act) : 0.f;
    }
    if (o_lds) {
      if (st4 && col + 3 < L.out_pad) {
        *reinterpret_cast<float4*>(o_lds + col) = make_float4(v[0], v[1], v[2], v[3]);
      } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) if (col + q < L.out_pad) o_lds[col + q] = v[q];
      }
    }
    if (o_glb) {
      if (g4 && col + 3 < N) {
        store_out4(o_glb + col, v, sc1);
      } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) if (col + q < N) store_out(o_glb + col + q, v[q], sc1);
      }
    }
  };

  for (int t0 = wave; t0 < ntl; t0 += 2 * FW) {
    const int t1 = t0 + FW;
    const bool two = t1 < ntl;                                     // wave-uniform
    // weight rows past N are clamped: they feed columns that are stored as zeros or not at all
    const uint16_t* const w0 = L.Wb + (int64_t)min(16 * t0 + r, N - 1) * Kpad + 8 * g;
    const uint16_t* const w1 = L.Wb + (int64_t)min(16 * (two ? t1 : t0) + r, N - 1) * Kpad + 8 * g;
    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
    u32x4 ring[PD][2][2];                                          // [chunk in flight][tile][MFMA of the chunk]
    auto fetch = [&](int j, int c) {                               // (c clamped by the caller: always a valid chunk)
      ring[j][0][0] = *reinterpret_cast<const u32x4*>(w0 + c * 64);
      ring[j][0][1] = *reinterpret_cast<const u32x4*>(w0 + c * 64 + 32);
      ring[j][1][0] = *reinterpret_cast<const u32x4*>(w1 + c * 64);
      ring[j][1][1] = *reinterpret_cast<const u32x4*>(w1 + c * 64 + 32);
    };
#pragma unroll
    for (int j = 0; j < PD; ++j) fetch(j, min(j, nch - 1));
    for (int c0 = 0; c0 < nch; c0 += PD) {
#pragma unroll
      for (int j = 0; j < PD; ++j) {
        const int c = c0 + j;
        if (c < nch) {                                             // uniform
          const float* const px = xa + c * 64;
          const bf16x8 fx0 = to_bf16x8(*reinterpret_cast<const float4*>(px), *reinterpret_cast<const float4*>(px + 4));
          const bf16x8 fx1 = to_bf16x8(*reinterpret_cast<const float4*>(px + 32), *reinterpret_cast<const float4*>(px + 36));
          acc0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, ring[j][0][0]), fx0, acc0, 0, 0, 0);
          acc0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, ring[j][0][1]), fx1, acc0, 0, 0, 0);
          if (two) {
            acc1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, ring[j][1][0]), fx0, acc1, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, ring[j][1][1]), fx1, acc1, 0, 0, 0);
          }
          fetch(j, min(c + PD, nch - 1));                          // (past the end: a repeat of the last chunk, never used)
        }
      }
    }
    epilogue(t0, acc0);
    if (two) epilogue(t1, acc1);
  }
}

// An fp32 layer: the k-ordered fma chain of layer_pass (mlp.hip).  Lane (r, g) feeds slab row r (A) and weight row
// 16 t + r (B) at k = 4 s + g of MFMA step s, 16 steps' operands at a time; k >= K feeds selected zeros (fma(0, 0, acc) is
// exact), whole groups of four padded steps are skipped.  Lane holds rows 4 g + i of column 16 t + r.
__device__ __forceinline__ void fp32_pass(const FLayer& L, float* lds, int m0, int M, int wave, int lane) {
  const int r = lane & 15, g = lane >> 4;
  const int K = L.K, N = L.N;
  const int nst = (K + 3) >> 2;
  const int ntl = ((L.out_off >= 0 && L.out_pad > N ? L.out_pad : N) + 15) >> 4;
  const float* const xa = lds + L.in_off + r * L.in_ld;
  const bool sc1 = L.g_sc1 != 0;
  for (int t = wave; t < ntl; t += FW) {
    const float* const wrow = L.W + (int64_t)min(16 * t + r, N - 1) * K;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int s0 = 0; s0 < nst; s0 += 16) {
      float av[16], bv[16];
#pragma unroll
      for (int s = 0; s < 16; ++s) {
        const int k = 4 * (s0 + s) + g, kk = min(k, K - 1);
        bv[s] = wrow[kk];
        av[s] = xa[kk];
      }
#pragma unroll
      for (int s = 0; s < 16; ++s) {
        const bool in = 4 * (s0 + s) + g < K;
        av[s] = in ? av[s] : 0.f;
        bv[s] = in ? bv[s] : 0.f;
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if (s0 + 4 * q < nst) {                                    // uniform
#pragma unroll
          for (int s = 4 * q; s < 4 * q + 4; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[s], bv[s], acc, 0, 0, 0);
        }
      }
    }
    const int col = 16 * t + r;
    const float bcol = (L.b && col < N) ? L.b[col < N ? col : 0] : 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = 4 * g + i;
      const float v = col < N ? act_apply(acc[i] + bcol, L.act) : 0.f;
      if (L.out_off >= 0 && col < L.out_pad) lds[L.out_off + row * L.out_ld + col] = v;
      if (L.g_out && col < N && m0 + row < M) store_out(L.g_out + (int64_t)(m0 + row) * L.g_ld + col, v, sc1);
    }
  }
}

__global__ __launch_bounds__(kFThreads) void fused_bf16_kernel(FArgs a, Done done, XSrc xs) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int m0 = (int)blockIdx.x * 16, M = (int)a.M;      // (virtual rows of a slot: 32 bits)

  // L2 warm-up (chain_kernel's idea): every wave touches a slice of the weights of layers `wave` and `wave + FW`, one
  // load per 128-byte line, four lines per lane, never waited for before the very end -- the XCD's 16 or so resident
  // workgroups together pull 512 KB per layer into their L2 during the prologue.  A hint: another workgroup -> XCD
  // placement changes speed, not results.
  float warm[2][4];
  {
    const int64_t part = ((blockIdx.x >> 3) & 15) + 16 * (int64_t)(blockIdx.x >> 7);   // my rank among the XCD's workgroups
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int l = wave + FW * h;
#pragma unroll
      for (int j = 0; j < 4; ++j) warm[h][j] = 0.f;
      if (l < a.n_layers) {                                        // wave-uniform
        const FLayer& L = a.L[l];
        const int64_t bytes = L.Wb ? (int64_t)L.N * ((L.K + 63) & ~63) * 2 : (int64_t)L.N * L.K * 4;
        const int64_t lines = (bytes + 127) >> 7;
        const char* p = L.Wb ? reinterpret_cast<const char*>(L.Wb) : reinterpret_cast<const char*>(L.W);
#pragma unroll
        for (int j = 0; j < 4; ++j)
          warm[h][j] = *reinterpret_cast<const float*>(p + min(lines - 1, (part * 64 + lane) * 4 + j) * 128);
      }
    }
  }

  // inputs: the slab's dense rows from their query's own array, the pooled rows the gather left in T
  {
    const float* base; int64_t row0, rows;
    resolve_src(xs, nullptr, M, m0, &base, &row0, &rows);
    const int k0_pad = (a.k0 + 63) & ~63;
    if (a.vec_x) stage_rows<true>(base, a.ldx, (int)row0, (int)rows, 0, a.k0, k0_pad, smem + a.x0_off, a.x0_ld, 0);
    else stage_rows<false>(base, a.ldx, (int)row0, (int)rows, 0, a.k0, k0_pad, smem + a.x0_off, a.x0_ld, 0);
    if (a.vec_t) stage_rows<true>(a.T, a.ldt, m0, M, a.p_col0, a.p_cols, a.p_cols_pad, smem + a.rs_off, a.rs_ld, a.p_col0);
    else stage_rows<false>(a.T, a.ldt, m0, M, a.p_col0, a.p_cols, a.p_cols_pad, smem + a.rs_off, a.rs_ld, a.p_col0);
    // dot: the top input's columns from D + P up to the next multiple of 64 read as zeros
    if (a.dot) for (int i = tid; i < 16 * a.ri_ld; i += kFThreads) smem[a.ri_off + i] = 0.f;
  }
  __syncthreads();

  for (int l = 0; l < a.n_layers; ++l) {
    const FLayer& L = a.L[l];
    if (L.Wb) bf16_pass<false>(L, smem, m0, M, wave, lane);
    else fp32_pass(L, smem, m0, M, wave, lane);
    __syncthreads();
    // (the loop counter through an opaque move: what the interaction needs is then worked out where it runs, once, and
    // not hoisted in front of the layer loop, where two dozen loop-invariant scalars and lane masks overflowed the SGPR file)
    int l_now = l;
    asm volatile("" : "+s"(l_now));
    if (a.dot && l_now == a.n_bot - 1) {
      // RS = the sample's F x D feature block -> RI = [ dense_out | pairs ], also kept in R (drs_fetch_interaction)
      int D = a.D;
      asm volatile("" : "+s"(D));
      const float* const Ts = smem + a.rs_off;
      float* const Rs = smem + a.ri_off;
      for (int i = tid; i < 16 * D; i += kFThreads) {
        const int row = i / D, d = i - row * D;
        const float v = Ts[row * a.rs_ld + d];
        Rs[row * a.ri_ld + d] = v;
        if (m0 + row < M) a.R[(int64_t)(m0 + row) * a.ldr + d] = v;
      }
      interact_pairs_mfma(Ts, a.rs_ld, Rs, a.ri_ld, 16, a.F, D, a.itself, a.R, a.ldr, m0, M, FW, wave, lane,
                          [](int c, int) { return c; });
      __syncthreads();
    }
  }
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int j = 0; j < 4; ++j) asm volatile("" ::"v"(warm[h][j]));
  signal_done(done, gridDim.x, smem);
}

// NCF's Sum: columns [0, D) of 16 rows of T + columns [col_b, col_b + D) -> slab columns [0, D) and R's.  One fp32 add
// per element, operands in this order (add_rows_kernel, the stream kernels' SumArgs).  VEC: D % 4 == 0, T rows 16-byte
// aligned; VEC_R: R's rows too.
template <bool VEC>
__device__ __forceinline__ void sum_rows(const float* __restrict__ T, int64_t ldt, int m0, int M, int col_b, int D,
                                         float* dst, int dst_ld, float* __restrict__ R, int64_t ldr, bool vec_r) {
  constexpr int V = VEC ? 4 : 1;
  const int ppr = D / V, total = 16 * ppr;
  for (int i = threadIdx.x; i < total; i += kFThreads) {
    const int row = i / ppr, c = (i - row * ppr) * V;
    const float* q = T + (int64_t)(m0 + row < M ? m0 + row : M - 1) * ldt + c;
    float* d = dst + row * dst_ld + c;
    float* g = m0 + row < M ? R + (int64_t)(m0 + row) * ldr + c : nullptr;
    if (VEC) {
      const float4 x = *reinterpret_cast<const float4*>(q), y = *reinterpret_cast<const float4*>(q + col_b);
      const float4 v = make_float4(x.x + y.x, x.y + y.y, x.z + y.z, x.w + y.w);
      *reinterpret_cast<float4*>(d) = v;
      if (g) {
        if (vec_r) *reinterpret_cast<float4*>(g) = v;
        else { g[0] = v.x; g[1] = v.y; g[2] = v.z; g[3] = v.w; }
      }
    } else {
      const float v = q[0] + q[col_b];
      *d = v;
      if (g) *g = v;
    }
  }
}

__global__ __launch_bounds__(kFThreads) void fused_bf16_sum_kernel(FArgs a, Done done) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int m0 = (int)blockIdx.x * 16, M = (int)a.M;

  // L2 warm-up: fused_bf16_kernel's
  float warm[2][4];
  {
    const int64_t part = ((blockIdx.x >> 3) & 15) + 16 * (int64_t)(blockIdx.x >> 7);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int l = wave + FW * h;
#pragma unroll
      for (int j = 0; j < 4; ++j) warm[h][j] = 0.f;
      if (l < a.n_layers) {                                        // wave-uniform
        const FLayer& L = a.L[l];
        const int64_t bytes = L.Wb ? (int64_t)L.N * ((L.K + 63) & ~63) * 2 : (int64_t)L.N * L.K * 4;
        const int64_t lines = (bytes + 127) >> 7;
        const char* p = L.Wb ? reinterpret_cast<const char*>(L.Wb) : reinterpret_cast<const char*>(L.W);
#pragma unroll
        for (int j = 0; j < 4; ++j)
          warm[h][j] = *reinterpret_cast<const float*>(p + min(lines - 1, (part * 64 + lane) * 4 + j) * 128);
      }
    }
  }

  // inputs, all from the pooled rows the gather left in T: the branch's Concat and the Sum
  {
    const int k0_pad = (a.k0 + 63) & ~63;
    if (a.vec_t) {
      stage_rows<true>(a.T, a.ldt, m0, M, a.p_col0, a.k0, k0_pad, smem + a.x0_off, a.x0_ld, 0);
      sum_rows<true>(a.T, a.ldt, m0, M, a.p_cols, a.D, smem + a.rs_off, a.rs_ld, a.R, a.ldr, a.vec_x != 0);
    } else {
      stage_rows<false>(a.T, a.ldt, m0, M, a.p_col0, a.k0, k0_pad, smem + a.x0_off, a.x0_ld, 0);
      sum_rows<false>(a.T, a.ldt, m0, M, a.p_cols, a.D, smem + a.rs_off, a.rs_ld, a.R, a.ldr, false);
    }
  }
  __syncthreads();

  for (int l = 0; l < a.n_layers; ++l) {
    const FLayer& L = a.L[l];
    if (L.Wb) bf16_pass<true>(L, smem, m0, M, wave, lane);
    else fp32_pass(L, smem, m0, M, wave, lane);
    __syncthreads();
  }
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int j = 0; j < 4; ++j) asm volatile("" ::"v"(warm[h][j]));
  signal_done(done, gridDim.x, smem);
}

}  // namespace

// per device (device_init)
hipError_t fused_bf16_set_attrs() {
  const hipError_t e = set_max_lds(fused_bf16_kernel);
  return e != hipSuccess ? e : set_max_lds(fused_bf16_sum_kernel);
}

hipError_t launch_fused_bf16(const MlpPlan& p, hipStream_t s) {
  if (p.form == MlpForm::fused_bf16_sum)
    hipLaunchKernelGGL(fused_bf16_sum_kernel, dim3(p.grid_x), dim3(kFThreads), p.lds, s, p.fa, p.done);
  else
    hipLaunchKernelGGL(fused_bf16_kernel, dim3(p.grid_x), dim3(kFThreads), p.lds, s, p.fa, p.done, p.xs);
  return hipGetLastError();
}

}  // namespace drs
