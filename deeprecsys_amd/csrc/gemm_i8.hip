// FC layers on the int8 matrix cores ("mlp_int8" 1): y[M, N] = act(dequant(q(x)[M, K] . q(W)[N, K]^T) + b), int32 accumulation.
//
// The eight-bit counterpart of gemm_bf16.hip for the same FC + Relu|Sigmoid operator pair (reference
// models/dlrm_s_caffe2.py:258-272), with dynamic per-row activation scales and per-output-channel weight scales (the
// dynamic quantized linear of the Caffe2 lineage).  The arithmetic contract, the same for every instance, every step
// fp32 unless it says otherwise:
//   1. absmax   a(v) of a vector v (a row of x over k < K, a row n of W): the largest |v_k|, taken as the largest bit
//               pattern bits & 0x7fffffff, so that a NaN or an infinity is seen (fmaxf would drop a NaN).
//   2. scale    a not finite: scale = the quiet NaN 0x7fc00000, every code 0.  a < 2^-119: scale = +0.0, every code 0 (127 / a
//               stays finite).  Else inv = 127.0f / a and scale = a / 127.0f, both correctly rounded, and
//               code_k = clamp((int)rintf(v_k * inv), -127, 127): one rounded multiply, round-half-even.  -128 never
//               occurs.  k from K up to the padded length has code 0, chosen by value (never 0 times a clamped load).
//   3. sum      acc = sum_k qx_rk qw_nk, exact in int32 (K <= 131 072 keeps K 127^2 below 2^31), by ONE instruction shape,
//               v_mfma_i32_16x16x64_i8; the sum is exact, so the k order is free; no split-K.
//   4. dequant  y = act((float)acc * (sx_r * sw_n) + b_n): int -> float nearest even, then three separately rounded
//               operations -- two multiplies and an add, NOT an fma (dequant below switches contraction off); b_n = 0
//               where the layer has no bias; act is act_apply, as in every other form.
// So an output's bits depend on its row of x and its row of W alone: not on the tile shape, the grid, the row count or
// what the query was coalesced with.  A row of x holding a NaN or an infinity gives NaN in every column (then act); a
// weight row n holding one gives NaN in column n of every row; an all-zero row gives act(b).
//
// Operands: x stays fp32 in memory and is quantized while it is staged into LDS (no int8 copy of an activation is ever
// written); W comes from the layer's int8 twin Wq [N, Kpad] (Kpad = K rounded up to 64, zero codes in the padding) and
// sw [N], built once from the fp32 weights by launch_i8_twin.
//
// A workgroup of 4 waves (2 x 2) owns 32 TM rows x 32 TN columns; a wave owns TM x TN MFMA tiles.  As in gemm_bf16.hip the
// WEIGHT rows are the A operand, so a lane ends up with four consecutive output columns of one row: one 16-byte store.
//   prologue   the workgroup owns whole rows of x, so it finds their scales itself: 16 lanes per row fold the |bits|
//              maximum over the row (float4 pieces, dwords where the rows are only 4-byte aligned), finish it across the
//              16 lanes and leave inv_r and sx_r in LDS (2 BM floats).  The row is read a second time by the main loop,
//              mostly from L2.
//   main loop  per 128-deep K chunk (two MFMAs deep; the last chunk may be 64): the global loads of chunk c + 1 are
//              issued into registers, the MFMAs of chunk c run from LDS buffer c & 1, the registers are quantized with
//              the row's inv, packed four codes to a dword and stored into buffer (c + 1) & 1, one barrier.  Wq pieces
//              are copied as they are, 16 bytes a load.  A lane's MFMA operand is 16 consecutive k of one row: one
//              ds_read_b128.  LDS rows are 128 codes + 16 bytes of padding (144 bytes: the 16 lanes of a ds_read_b128
//              phase hit 16 different 16-byte bank groups).
//   epilogue   sx_r from LDS, sw and b as one 16-byte load each per lane where aligned, the contract's three operations,
//              act, and the stores of gemm_bf16.hip (write-through and signal_done when the launch is its set's last).
#include <string.h>

#include "drs_internal.h"
#include "mlp_stream.h"

namespace drs {
namespace {

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr int kIThreads = 256;
constexpr int IKC = 128;         // k per chunk (two MFMAs deep)
constexpr int ILD = 144;         // bytes per LDS row: 128 codes + 16 of padding
constexpr uint32_t kAbsMask = 0x7fffffffu, kInfBits = 0x7f800000u;
constexpr float kTinyAbsmax = 0x1p-119f;

struct IArgs {
  const float* x;
  int64_t ldx;
  int64_t M;
  const int8_t* Wq;    // [N, Kpad] codes, zero padded
  const float* sw;     // [N] weight scales
  const float* b;
  float* y;
  int64_t ldy;
  int32_t K, Kpad, N, act, sc1;
};

// output stores through inline asm, as gemm_bf16.hip's: nothing waits on them before signal_done's own drain;
// SC1 = write-through (outputs the hand-off reads back)
template <bool SC1>
__device__ __forceinline__ void ist4(float* p, const f32x4 v) {
  // (s_nop 1: the wait states gfx940+ wants before a VALU may overwrite the data registers of a store of more than 64 bits)
  if (SC1) asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" : : "v"(p), "v"(v) : "memory");
  else asm volatile("global_store_dwordx4 %0, %1, off\n\ts_nop 1" : : "v"(p), "v"(v) : "memory");
}
template <bool SC1>
__device__ __forceinline__ void ist1(float* p, const float v) {
  if (SC1) asm volatile("global_store_dword %0, %1, off sc1" : : "v"(p), "v"(v) : "memory");
  else asm volatile("global_store_dword %0, %1, off" : : "v"(p), "v"(v) : "memory");
}

__device__ __forceinline__ uint32_t abs_bits(float v) { return __float_as_uint(v) & kAbsMask; }

// contract step 2: absmax bits -> (inv, scale).  inv == 0 says "every code is 0" (127 / a is never 0 for a finite a)
__device__ __forceinline__ void scale_of(uint32_t amax_bits, float* inv, float* scale) {
  const float a = __uint_as_float(amax_bits);
  if (amax_bits >= kInfBits) { *inv = 0.f; *scale = __uint_as_float(0x7fc00000u); }
  else if (a < kTinyAbsmax) { *inv = 0.f; *scale = 0.f; }
  else { *inv = __fdiv_rn(127.0f, a); *scale = __fdiv_rn(a, 127.0f); }
}
// ... and one code, as the low byte of a word.  in: k < K and inv != 0, else the code is 0 by value
__device__ __forceinline__ uint32_t code_of(float v, float inv, bool in) {
  int c = (int)__builtin_rintf(__fmul_rn(v, inv));     // (one multiply and nothing to fuse it with; v_rndne_f32)
  c = c < -127 ? -127 : c > 127 ? 127 : c;
  return in ? (uint32_t)c & 0xffu : 0u;
}
__device__ __forceinline__ uint32_t pack4(const float4 v, float inv, int k, int K) {
  const bool on = inv != 0.f;
  return code_of(v.x, inv, on && k + 0 < K) | code_of(v.y, inv, on && k + 1 < K) << 8 |
         code_of(v.z, inv, on && k + 2 < K) << 16 | code_of(v.w, inv, on && k + 3 < K) << 24;
}
// contract step 4 before the activation: three roundings, never an fma
__device__ __forceinline__ float dequant(int acc, float sx, float sw, float b) {
#pragma clang fp contract(off)
  const float s = sx * sw;
  const float t = (float)acc * s;
  return t + b;
}

// VEC: x (every source array), ldx and K allow 16-byte loads that never straddle the end of a row
template <bool VEC>
__device__ __forceinline__ float4 xload4(const float* q, int k, int K) {
  if (VEC) return *reinterpret_cast<const float4*>(q + (k < K ? k : 0));
  return make_float4(q[min(k + 0, K - 1)], q[min(k + 1, K - 1)], q[min(k + 2, K - 1)], q[min(k + 3, K - 1)]);
}

template <int TM, int TN, bool VEC>
__global__ __launch_bounds__(kIThreads) void gemm_i8_kernel(IArgs a, Done done, XSrc xs) {
  constexpr int BM = 32 * TM, BN = 32 * TN;
  constexpr int NA = BM / 8;       // float4 of x per thread per chunk
  constexpr int NB = BN / 32;      // 16-byte pieces of Wq per thread per chunk: row wrow + 32 j, codes wk .. wk + 15
  constexpr int NH = BM > 64 ? BM / 64 : 1;   // 64-row runs of the tile (a run never straddles two queries)
  constexpr int HT = kIThreads / NH;          // threads that serve one run
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* const sInv = smem;                    // [BM] 127 / absmax of the tile's rows (0: every code is 0) ...
  float* const sSx = smem + BM;                // [BM] ... and their scales
  int8_t* const sX = reinterpret_cast<int8_t*>(smem + 2 * BM);   // [2][BM][ILD]
  int8_t* const sW = sX + 2 * BM * ILD;                          // [2][BN][ILD]
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int wm = wave & 1, wn = wave >> 1;
  const int64_t m0 = (int64_t)blockIdx.x * BM;
  const int n0 = blockIdx.y * BN;
  const int K = a.K, N = a.N, Kpad = a.Kpad;
  const int nch = (Kpad + IKC - 1) / IKC;

  // staging roles.  x: row xr0 + XS j of the tile, floats fk .. fk + 3 of the chunk; a 128-row tile is two 64-row runs,
  // waves 0-1 stage the first and waves 2-3 the second (one look-up of the run's query per wave)
  constexpr int XS = 8 / NH;
  const int half = NH > 1 ? __builtin_amdgcn_readfirstlane(tid >> 7) : 0;
  const int ht = tid & (HT - 1);
  const int xr0 = 64 * half + (ht >> 5), fk = (tid & 31) * 4;
  const int wrow = tid >> 3, wk = (tid & 7) * 16;
  const float* xb; int64_t row0, rows;
  resolve_src(xs, a.x, a.M, m0 + 64 * half, &xb, &row0, &rows);
  // rows past the end are clamped: they only feed outputs that are never stored
  auto row_ptr = [&](int tile_row) {
    const int64_t rr = row0 + (tile_row - 64 * half);
    return xb + (rr < rows ? rr : (rows > 0 ? rows - 1 : 0)) * a.ldx;
  };
  const float* xrow[NA];
#pragma unroll
  for (int j = 0; j < NA; ++j) xrow[j] = row_ptr(xr0 + XS * j);
  const int8_t* wrowp[NB];
#pragma unroll
  for (int j = 0; j < NB; ++j) wrowp[j] = a.Wq + (int64_t)min(n0 + wrow + 32 * j, N - 1) * Kpad;

  float4 ra[NA];
  u32x4 rb[NB];
  auto fetch = [&](int c) {
    const int k = c * IKC + fk;
#pragma unroll
    for (int j = 0; j < NA; ++j) ra[j] = xload4<VEC>(xrow[j], k, K);
    // (the second half of a 64-deep last chunk lies behind the row: fetched from the row's start, never multiplied)
    const int kw = c * IKC + wk;
#pragma unroll
    for (int j = 0; j < NB; ++j) rb[j] = *reinterpret_cast<const u32x4*>(wrowp[j] + (kw < Kpad ? kw : 0));
  };

  fetch(0);

  // prologue: the scales of my run's rows, 16 lanes a row, HT / 16 rows a pass
  {
    constexpr int RP = HT / 16;
    const int l16 = tid & 15;
    for (int p = 0; p < BM / NH / RP; ++p) {
      const int trow = 64 * half + p * RP + (ht >> 4);
      const float* q = row_ptr(trow);
      uint32_t m = 0;
      for (int k = 4 * l16; k < K; k += 64) {
        const float4 v = xload4<VEC>(q, k, K);      // (k + i >= K re-reads element K - 1: the same maximum)
        m = max(max(m, abs_bits(v.x)), max(abs_bits(v.y), max(abs_bits(v.z), abs_bits(v.w))));
      }
#pragma unroll
      for (int s = 1; s < 16; s <<= 1) m = max(m, (uint32_t)__shfl_xor((int)m, s));
      if (l16 == 0) scale_of(m, &sInv[trow], &sSx[trow]);
    }
  }
  __syncthreads();
  float rinv[NA];
#pragma unroll
  for (int j = 0; j < NA; ++j) rinv[j] = sInv[xr0 + XS * j];

  auto stash = [&](int c) {
    const int k = c * IKC + fk;
    int8_t* const dx = sX + (c & 1) * BM * ILD + xr0 * ILD + fk;
    int8_t* const dw = sW + (c & 1) * BN * ILD + wrow * ILD + wk;
#pragma unroll
    for (int j = 0; j < NA; ++j) *reinterpret_cast<uint32_t*>(dx + XS * j * ILD) = pack4(ra[j], rinv[j], k, K);
#pragma unroll
    for (int j = 0; j < NB; ++j) *reinterpret_cast<u32x4*>(dw + 32 * j * ILD) = rb[j];
  };

  i32x4 acc[TN][TM];
#pragma unroll
  for (int i = 0; i < TN; ++i)
#pragma unroll
    for (int j = 0; j < TM; ++j) acc[i][j] = i32x4{0, 0, 0, 0};

  stash(0);
  __syncthreads();
  for (int c = 0; c < nch; ++c) {
    if (c + 1 < nch) fetch(c + 1);
    // my operands of chunk c: lane (r, g) holds k = 64 s + 16 g .. + 15 of row r of each of its tiles
    const int8_t* const px = sX + (c & 1) * BM * ILD + (16 * TM * wm + r) * ILD + 16 * g;
    const int8_t* const pw = sW + (c & 1) * BN * ILD + (16 * TN * wn + r) * ILD + 16 * g;
    const int deep = Kpad - c * IKC >= IKC ? 2 : 1;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      if (s < deep) {
        i32x4 fw[TN], fx[TM];
#pragma unroll
        for (int i = 0; i < TN; ++i) fw[i] = *reinterpret_cast<const i32x4*>(pw + 16 * i * ILD + 64 * s);
#pragma unroll
        for (int j = 0; j < TM; ++j) fx[j] = *reinterpret_cast<const i32x4*>(px + 16 * j * ILD + 64 * s);
#pragma unroll
        for (int i = 0; i < TN; ++i)
#pragma unroll
          for (int j = 0; j < TM; ++j) acc[i][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(fw[i], fx[j], acc[i][j], 0, 0, 0);
      }
    }
    if (c + 1 < nch) stash(c + 1);   // (buffer (c + 1) & 1 was last read in iteration c - 1, before its barrier)
    __syncthreads();
  }

  // epilogue: accumulator register q of tile (i, j) is output row 16 j + r, column 16 i + 4 g + q of the wave's block
  float sx[TM];
#pragma unroll
  for (int j = 0; j < TM; ++j) sx[j] = sSx[16 * TM * wm + 16 * j + r];
  const bool vec = !(N & 3) && !(a.ldy & 3) && !((reinterpret_cast<uintptr_t>(a.y) | reinterpret_cast<uintptr_t>(a.b)) & 15);
  const bool vsw = !(reinterpret_cast<uintptr_t>(a.sw) & 15);
#pragma unroll
  for (int i = 0; i < TN; ++i) {
    const int col = n0 + 16 * TN * wn + 16 * i + 4 * g;
    f32x4 b4 = {0.f, 0.f, 0.f, 0.f}, w4 = {0.f, 0.f, 0.f, 0.f};
    if (vsw && col + 3 < N) {
      w4 = *reinterpret_cast<const f32x4*>(a.sw + col);
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q) if (col + q < N) w4[q] = a.sw[col + q];
    }
    if (a.b) {
      if (vec && col < N) {
        b4 = *reinterpret_cast<const f32x4*>(a.b + col);
      } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) if (col + q < N) b4[q] = a.b[col + q];
      }
    }
#pragma unroll
    for (int j = 0; j < TM; ++j) {
      const int64_t row = m0 + 16 * TM * wm + 16 * j + r;
      if (row >= a.M) continue;
      float* const yrow = a.y + row * a.ldy;
      f32x4 v;
#pragma unroll
      for (int q = 0; q < 4; ++q) v[q] = act_apply(dequant(acc[i][j][q], sx[j], w4[q], b4[q]), a.act);
      if (vec) {
        if (col < N) { if (a.sc1) ist4<true>(yrow + col, v); else ist4<false>(yrow + col, v); }
      } else {
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (col + q < N) { if (a.sc1) ist1<true>(yrow + col + q, v[q]); else ist1<false>(yrow + col + q, v[q]); }
      }
    }
  }
  signal_done(done, gridDim.x * gridDim.y, smem);
}

// W [N, K] fp32 -> Wq [N, Kpad] codes (zeros from K on) and sw [N]: one wave per weight row, the absmax reduction over the
// row, then the quantizing pass, four codes to a dword
__global__ __launch_bounds__(256) void i8_twin_kernel(const float* __restrict__ W, int32_t K, int32_t N, int32_t Kpad,
                                                       int8_t* __restrict__ Wq, float* __restrict__ sw) {
  const int lane = threadIdx.x & 63;
  const int64_t n = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (n >= N) return;
  const float* const w = W + n * K;
  uint32_t m = 0;
  for (int k = lane; k < K; k += 64) m = max(m, abs_bits(w[k]));
#pragma unroll
  for (int s = 1; s < 64; s <<= 1) m = max(m, (uint32_t)__shfl_xor((int)m, s));
  float inv, scale;
  scale_of(m, &inv, &scale);
  if (lane == 0) sw[n] = scale;
  uint32_t* const out = reinterpret_cast<uint32_t*>(Wq + n * Kpad);
  for (int k = 4 * lane; k < Kpad; k += 256)
    out[k >> 2] = pack4(make_float4(w[min(k + 0, K - 1)], w[min(k + 1, K - 1)], w[min(k + 2, K - 1)], w[min(k + 3, K - 1)]), inv, k, K);
}

template <int TM, int TN>
size_t i8_lds() { return sizeof(float) * 2 * 32 * TM + (size_t)2 * (32 * TM + 32 * TN) * ILD; }

}  // namespace

// per device (device_init)
hipError_t gemm_i8_set_attrs() {
  for (const void* k : {reinterpret_cast<const void*>(gemm_i8_kernel<4, 4, true>), reinterpret_cast<const void*>(gemm_i8_kernel<4, 4, false>),
                        reinterpret_cast<const void*>(gemm_i8_kernel<2, 2, true>), reinterpret_cast<const void*>(gemm_i8_kernel<2, 2, false>),
                        reinterpret_cast<const void*>(gemm_i8_kernel<1, 2, true>), reinterpret_cast<const void*>(gemm_i8_kernel<1, 2, false>)}) {
    hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

hipError_t launch_i8_twin(const float* W, int32_t K, int32_t N, int8_t* Wq, float* sw, hipStream_t s) {
  if (N <= 0 || K <= 0) return hipSuccess;
  hipLaunchKernelGGL(i8_twin_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, s, W, K, N, i8_kpad(K), Wq, sw);
  return hipGetLastError();
}

// The int8 GEMM form of the layer p->a (p->wq, p->wsc: its twin).  Tile shapes, as TM * 10 + TN: 44 (128 x 128), 22
// (64 x 64) and 12 (32 x 64), the ones gemm_bf16_plan picks among and by its rule -- the largest that still gives every CU
// (256) a workgroup; tune.i8_tile ("mlp_i8_tile") forces one.  false: no such form (a split input row).
bool gemm_i8_plan(const Tune& tune, MlpPlan* p) {
  const ChainArgs& L = p->a;
  const int64_t M = L.M;
  const int N = L.width[1];
  if (!p->wq || !p->wsc || p->xs.ksplit > 0 || L.width[0] < 64 || N < 64 || L.width[0] > kI8MaxK) return false;
  auto blocks = [&](int tm, int tn) { return ((M + 32 * tm - 1) / (32 * tm)) * (int64_t)((N + 32 * tn - 1) / (32 * tn)); };
  int t = tune.i8_tile;
  if (!t) t = blocks(4, 4) >= 256 ? 44 : blocks(2, 2) >= 256 ? 22 : 12;
  p->form = MlpForm::gemm_i8;
  p->tm = t / 10; p->tn = t % 10;
  p->grid_x = (unsigned)((M + 32 * p->tm - 1) / (32 * p->tm));
  p->grid_y = (unsigned)((N + 32 * p->tn - 1) / (32 * p->tn));
  p->lds = t == 44 ? i8_lds<4, 4>() : t == 22 ? i8_lds<2, 2>() : i8_lds<1, 2>();
  bool vec = !(L.width[0] & 3) && !(L.ldx & 3) && aligned16(L.x);
  for (int i = 0; i < p->xs.q.n_q; ++i) vec = vec && aligned16(p->xs.x[i]);
  p->vec = vec;
  return true;
}

hipError_t launch_gemm_i8(const MlpPlan& p, hipStream_t s) {
  const ChainArgs& L = p.a;
  IArgs a;
  memset(&a, 0, sizeof a);
  a.x = L.x; a.ldx = L.ldx; a.M = L.M; a.Wq = p.wq; a.sw = p.wsc; a.b = L.b[0]; a.y = L.y; a.ldy = L.ldy;
  a.K = L.width[0]; a.Kpad = i8_kpad(a.K); a.N = L.width[1]; a.act = L.act[0]; a.sc1 = p.done.counter != nullptr;
  const dim3 grid(p.grid_x, p.grid_y);
#define DRS_ILAUNCH(TM_, TN_)                                                                                       \
  if (p.tm == TM_ && p.tn == TN_) {                                                                                 \
    if (p.vec) hipLaunchKernelGGL((gemm_i8_kernel<TM_, TN_, true>), grid, dim3(kIThreads), p.lds, s, a, p.done, p.xs);   \
    else hipLaunchKernelGGL((gemm_i8_kernel<TM_, TN_, false>), grid, dim3(kIThreads), p.lds, s, a, p.done, p.xs);        \
    return hipGetLastError();                                                                                       \
  }
  DRS_ILAUNCH(4, 4) DRS_ILAUNCH(2, 2) DRS_ILAUNCH(1, 2)
#undef DRS_ILAUNCH
  return hipErrorInvalidValue;
}

}  // namespace drs
