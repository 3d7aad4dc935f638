// FC layers on the bf16 matrix cores ("mlp_dtype" 2): y[M, N] = act(bf16(x)[M, K] . bf16(W)[N, K]^T + b), fp32 accumulation.
//
// The half-precision counterpart of gemm.hip for the same FC + Relu|Sigmoid operator pair (reference
// models/dlrm_s_caffe2.py:258-272).  The arithmetic contract, the same for every instance:
//   x (fp32, as the previous step left it) and W are rounded to bf16, nearest even, NaN stays NaN (a plain cast:
//   v_cvt_pk_bf16_f32); products are exact in fp32; ONE instruction shape, v_mfma_f32_16x16x32_bf16, accumulates them in
//   fp32, 32 k per instruction, k ascending from a zero accumulator, no split-K; k from K up to the next multiple of 64
//   contributes 0 * 0; bias, activation and the stored y are fp32.
// So an output's bits depend on its row of x and its row of W alone: not on the tile shape, the grid or the row count.
//
// Operands: x stays fp32 in memory and is converted while it is staged into LDS (no bf16 copy of an activation is ever
// written); W comes from the layer's bf16 twin Wb [N, Kpad] (Kpad = K rounded up to 64, zero padded), built once from
// the fp32 weights by launch_bf16_twin.
//
// A workgroup of 4 waves (2 x 2) owns 32 TM rows x 32 TN columns; a wave owns TM x TN MFMA tiles.  As in gemm.hip the
// WEIGHT rows are the A operand and the input rows the B operand, so a lane ends up with four consecutive output columns
// of one row: one 16-byte store.  Per 64-deep K chunk: the global loads of chunk c + 1 are issued into registers, the
// 2 TM TN MFMAs of chunk c run from LDS buffer c & 1, the registers are converted and stored into buffer (c + 1) & 1, one
// barrier.  LDS rows are 64 bf16 + 16 bytes of padding (144 bytes: the 16 lanes of a ds_read_b128 phase hit 16
// different 16-byte bank groups).
#include <string.h>

#include "drs_internal.h"
#include "mlp_stream.h"

namespace drs {
namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr int kBThreads = 256;
constexpr int BKC = 64;          // k per chunk (two MFMAs deep)
constexpr int BLD = 72;          // bf16 per LDS row: 64 + 8 of padding (144 bytes)

struct BArgs {
  const float* x;
  int64_t ldx;
  int64_t M;
  const uint16_t* Wb;  // [N, Kpad] bf16, zero padded
  const float* b;
  float* y;
  int64_t ldy;
  int32_t K, Kpad, N, act, sc1;
};

// output stores through inline asm, as gemm.hip's: nothing waits on them before signal_done's own drain;
// SC1 = write-through (outputs the hand-off reads back)
template <bool SC1>
__device__ __forceinline__ void bst4(float* p, const f32x4 v) {
  // (s_nop 1: the wait states gfx940+ wants before a VALU may overwrite the data registers of a store of more than 64 bits)
  if (SC1) asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" : : "v"(p), "v"(v) : "memory");
  else asm volatile("global_store_dwordx4 %0, %1, off\n\ts_nop 1" : : "v"(p), "v"(v) : "memory");
}
template <bool SC1>
__device__ __forceinline__ void bst1(float* p, const float v) {
  if (SC1) asm volatile("global_store_dword %0, %1, off sc1" : : "v"(p), "v"(v) : "memory");
  else asm volatile("global_store_dword %0, %1, off" : : "v"(p), "v"(v) : "memory");
}

// fp32 -> bf16, nearest even, NaN stays NaN: the plain cast (v_cvt_pk_bf16_f32)
__device__ __forceinline__ bf16x4 to_bf16x4(const float4 v) {
  bf16x4 r;
  r[0] = (__bf16)v.x; r[1] = (__bf16)v.y; r[2] = (__bf16)v.z; r[3] = (__bf16)v.w;
  return r;
}

// VEC: x (every source array), ldx and K allow 16-byte loads that never straddle the end of a row
template <int TM, int TN, bool VEC>
__global__ __launch_bounds__(kBThreads) void gemm_bf16_kernel(BArgs a, Done done, XSrc xs) {
  constexpr int BM = 32 * TM, BN = 32 * TN;
  constexpr int NA = BM / 16;      // float4 of x per thread per chunk
  constexpr int NB = BN / 32;      // 16-byte pieces of Wb per thread per chunk: row wrow + 32 j, bf16 wk .. wk + 7
  constexpr int NH = BM > 64 ? BM / 64 : 1;   // 64-row runs of the tile (a run never straddles two queries)
  extern __shared__ __attribute__((aligned(16))) float smem[];
  __bf16* const sX = reinterpret_cast<__bf16*>(smem);   // [2][BM][BLD]
  __bf16* const sW = sX + 2 * BM * BLD;                 // [2][BN][BLD]
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int wm = wave & 1, wn = wave >> 1;
  const int64_t m0 = (int64_t)blockIdx.x * BM;
  const int n0 = blockIdx.y * BN;
  const int K = a.K, N = a.N;
  const int nch = a.Kpad / BKC;

  // staging roles.  x: row xr0 + XS j of the tile, floats fk .. fk + 3 of the chunk; a 128-row tile is two 64-row runs,
  // waves 0-1 stage the first and waves 2-3 the second (one look-up of the run's query per wave)
  constexpr int XS = 16 / NH;
  const int half = NH > 1 ? __builtin_amdgcn_readfirstlane(tid >> 7) : 0;
  const int xr0 = 64 * half + ((tid & (kBThreads / NH - 1)) >> 4), fk = (tid & 15) * 4;
  const int wrow = tid >> 3, wk = (tid & 7) * 8;
  const float* xrow[NA];
  {
    const float* xb; int64_t row0, rows;
    resolve_src(xs, a.x, a.M, m0 + 64 * half, &xb, &row0, &rows);
#pragma unroll
    for (int j = 0; j < NA; ++j) {
      // rows past the end are clamped: they only feed outputs that are never stored
      const int64_t rr = row0 + (xr0 - 64 * half) + XS * j;
      xrow[j] = xb + (rr < rows ? rr : (rows > 0 ? rows - 1 : 0)) * a.ldx;
    }
  }
  const uint16_t* wrowp[NB];
#pragma unroll
  for (int j = 0; j < NB; ++j) wrowp[j] = a.Wb + (int64_t)min(n0 + wrow + 32 * j, N - 1) * a.Kpad + wk;

  float4 ra[NA];
  u32x4 rb[NB];
  auto fetch = [&](int c) {
    const int k = c * BKC + fk;
#pragma unroll
    for (int j = 0; j < NA; ++j) {
      if (VEC) {
        ra[j] = *reinterpret_cast<const float4*>(xrow[j] + (k < K ? k : 0));
      } else {
        const float* q = xrow[j];
        ra[j] = make_float4(q[min(k + 0, K - 1)], q[min(k + 1, K - 1)], q[min(k + 2, K - 1)], q[min(k + 3, K - 1)]);
      }
    }
#pragma unroll
    for (int j = 0; j < NB; ++j) rb[j] = *reinterpret_cast<const u32x4*>(wrowp[j] + c * BKC);
  };
  auto stash = [&](int c) {
    const int k = c * BKC + fk;
    __bf16* const dx = sX + (c & 1) * BM * BLD + xr0 * BLD + fk;
    __bf16* const dw = sW + (c & 1) * BN * BLD + wrow * BLD + wk;
#pragma unroll
    for (int j = 0; j < NA; ++j)   // k >= K: zeros (selected, so that a NaN or an infinity clamped into the tail never counts)
      *reinterpret_cast<bf16x4*>(dx + XS * j * BLD) = to_bf16x4(mask4(ra[j], k, K));
#pragma unroll
    for (int j = 0; j < NB; ++j) *reinterpret_cast<u32x4*>(dw + 32 * j * BLD) = rb[j];
  };

  f32x4 acc[TN][TM];
#pragma unroll
  for (int i = 0; i < TN; ++i)
#pragma unroll
    for (int j = 0; j < TM; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  fetch(0);
  stash(0);
  __syncthreads();
  for (int c = 0; c < nch; ++c) {
    if (c + 1 < nch) fetch(c + 1);
    // my operands of chunk c: lane (r, g) holds k = 32 s + 8 g .. + 7 of row r of each of its tiles
    const __bf16* const px = sX + (c & 1) * BM * BLD + (16 * TM * wm + r) * BLD + 8 * g;
    const __bf16* const pw = sW + (c & 1) * BN * BLD + (16 * TN * wn + r) * BLD + 8 * g;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      bf16x8 fw[TN], fx[TM];
#pragma unroll
      for (int i = 0; i < TN; ++i) fw[i] = *reinterpret_cast<const bf16x8*>(pw + 16 * i * BLD + 32 * s);
#pragma unroll
      for (int j = 0; j < TM; ++j) fx[j] = *reinterpret_cast<const bf16x8*>(px + 16 * j * BLD + 32 * s);
#pragma unroll
      for (int i = 0; i < TN; ++i)
#pragma unroll
        for (int j = 0; j < TM; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fw[i], fx[j], acc[i][j], 0, 0, 0);
    }
    if (c + 1 < nch) stash(c + 1);   // (buffer (c + 1) & 1 was last read in iteration c - 1, before its barrier)
    __syncthreads();
  }

  // epilogue: accumulator register q of tile (i, j) is output row 16 j + r, column 16 i + 4 g + q of the wave's block
  const bool vec = !(N & 3) && !(a.ldy & 3) && !((reinterpret_cast<uintptr_t>(a.y) | reinterpret_cast<uintptr_t>(a.b)) & 15);
#pragma unroll
  for (int i = 0; i < TN; ++i) {
    const int col = n0 + 16 * TN * wn + 16 * i + 4 * g;
    f32x4 b4 = {0.f, 0.f, 0.f, 0.f};
    if (a.b) {
#pragma unroll
      for (int q = 0; q < 4; ++q) if (col + q < N) b4[q] = a.b[col + q];
    }
#pragma unroll
    for (int j = 0; j < TM; ++j) {
      const int64_t row = m0 + 16 * TM * wm + 16 * j + r;
      if (row >= a.M) continue;
      float* const yrow = a.y + row * a.ldy;
      f32x4 v = acc[i][j];
#pragma unroll
      for (int q = 0; q < 4; ++q) v[q] = act_apply(v[q] + b4[q], a.act);
      if (vec) {
        if (col < N) { if (a.sc1) bst4<true>(yrow + col, v); else bst4<false>(yrow + col, v); }
      } else {
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (col + q < N) { if (a.sc1) bst1<true>(yrow + col + q, v[q]); else bst1<false>(yrow + col + q, v[q]); }
      }
    }
  }
  signal_done(done, gridDim.x * gridDim.y, smem);
}

// W [N, K] fp32 -> Wb [N, Kpad] bf16 (nearest even, NaN stays NaN), zeros from K on
__global__ __launch_bounds__(256) void bf16_twin_kernel(const float* __restrict__ W, int32_t K, int32_t N, int32_t Kpad,
                                                         __bf16* __restrict__ Wb) {
  const int64_t n = (int64_t)N * Kpad;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t row = i / Kpad;
    const int k = (int)(i - row * Kpad);
    Wb[i] = k < K ? (__bf16)W[row * K + k] : (__bf16)0.0f;
  }
}

template <int TM, int TN>
size_t bf16_lds() { return sizeof(uint16_t) * 2 * (32 * TM + 32 * TN) * BLD; }

}  // namespace

// per device (device_init)
hipError_t gemm_bf16_set_attrs() {
  for (const void* k : {reinterpret_cast<const void*>(gemm_bf16_kernel<4, 4, true>), reinterpret_cast<const void*>(gemm_bf16_kernel<4, 4, false>),
                        reinterpret_cast<const void*>(gemm_bf16_kernel<2, 2, true>), reinterpret_cast<const void*>(gemm_bf16_kernel<2, 2, false>),
                        reinterpret_cast<const void*>(gemm_bf16_kernel<1, 2, true>), reinterpret_cast<const void*>(gemm_bf16_kernel<1, 2, false>)}) {
    hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

hipError_t launch_bf16_twin(const float* W, int32_t K, int32_t N, uint16_t* Wb, hipStream_t s) {
  const int Kpad = bf16_kpad(K);
  const int64_t n = (int64_t)N * Kpad;
  if (n <= 0) return hipSuccess;
  const int64_t g = (n + 255) / 256;
  hipLaunchKernelGGL(bf16_twin_kernel, dim3((unsigned)(g > 4096 ? 4096 : g)), dim3(256), 0, s, W, K, N, Kpad,
                     reinterpret_cast<__bf16*>(Wb));
  return hipGetLastError();
}

// The bf16 GEMM form of the layer p->a (p->wb: its twin).  Tile shapes, as TM * 10 + TN: 44 (128 x 128: full launch sets
// of thousands of rows), 22 (64 x 64) and 12 (32 x 64: sets of 64 - 512 rows), the largest that still gives every CU
// (256) a workgroup; tune.bf16_tile ("mlp_bf16_tile") forces one.  false: no such form (a split input row).
bool gemm_bf16_plan(const Tune& tune, MlpPlan* p) {
  const ChainArgs& L = p->a;
  const int64_t M = L.M;
  const int N = L.width[1];
  if (!p->wb || p->xs.ksplit > 0 || L.width[0] < 64 || N < 64) return false;
  auto blocks = [&](int tm, int tn) { return ((M + 32 * tm - 1) / (32 * tm)) * (int64_t)((N + 32 * tn - 1) / (32 * tn)); };
  int t = tune.bf16_tile;
  if (!t) t = blocks(4, 4) >= 256 ? 44 : blocks(2, 2) >= 256 ? 22 : 12;
  p->form = MlpForm::gemm_bf16;
  p->tm = t / 10; p->tn = t % 10;
  p->grid_x = (unsigned)((M + 32 * p->tm - 1) / (32 * p->tm));
  p->grid_y = (unsigned)((N + 32 * p->tn - 1) / (32 * p->tn));
  p->lds = t == 44 ? bf16_lds<4, 4>() : t == 22 ? bf16_lds<2, 2>() : bf16_lds<1, 2>();
  auto al = [](const void* q) { return (((uintptr_t)q) & 15) == 0; };
  bool vec = !(L.width[0] & 3) && !(L.ldx & 3) && al(L.x);
  for (int i = 0; i < p->xs.q.n_q; ++i) vec = vec && al(p->xs.x[i]);
  p->vec = vec;
  return true;
}

hipError_t launch_gemm_bf16(const MlpPlan& p, hipStream_t s) {
  const ChainArgs& L = p.a;
  BArgs a;
  memset(&a, 0, sizeof a);
  a.x = L.x; a.ldx = L.ldx; a.M = L.M; a.Wb = p.wb; a.b = L.b[0]; a.y = L.y; a.ldy = L.ldy;
  a.K = L.width[0]; a.Kpad = bf16_kpad(a.K); a.N = L.width[1]; a.act = L.act[0]; a.sc1 = p.done.counter != nullptr;
  const dim3 grid(p.grid_x, p.grid_y);
#define DRS_BLAUNCH(TM_, TN_)                                                                                        \
  if (p.tm == TM_ && p.tn == TN_) {                                                                                  \
    if (p.vec) hipLaunchKernelGGL((gemm_bf16_kernel<TM_, TN_, true>), grid, dim3(kBThreads), p.lds, s, a, p.done, p.xs);  \
    else hipLaunchKernelGGL((gemm_bf16_kernel<TM_, TN_, false>), grid, dim3(kBThreads), p.lds, s, a, p.done, p.xs);       \
    return hipGetLastError();                                                                                        \
  }
  DRS_BLAUNCH(4, 4) DRS_BLAUNCH(2, 2) DRS_BLAUNCH(1, 2)
#undef DRS_BLAUNCH
  return hipErrorInvalidValue;
}

}  // namespace drs
