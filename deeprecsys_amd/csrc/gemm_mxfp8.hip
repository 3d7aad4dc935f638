// FC layers in MXFP8 on the block-scaled matrix cores ("mlp_mxfp8" 1): y[M, N] = act(mx(x)[M, K] . mx(W)[N, K]^T + b), fp32 accumulation.
//
// The OCP MX counterpart of gemm_bf16.hip and gemm_i8.hip for the same FC + Relu|Sigmoid operator pair (reference
// models/dlrm_s_caffe2.py:258-272): fp8 e4m3 elements under one power-of-two scale per 32 consecutive k, the scales
// applied inside the matrix instruction.  The arithmetic contract, the same for every instance:
//   1. blocks   block j of a row covers k in [32 j, 32 j + 32); a row is a row of x over k, or row n of W.  K is padded to
//               Kpad = round_up(K, 128); every padded k has code 0, set by value (a select), never by a multiply.
//   2. scale    a = the largest bits & 0x7fffffff of the block; the E8M0 byte is s = max(expfield(a) - 8, 0) (expfield:
//               a's fp32 exponent field), i.e. the scale 2^(s - 127).  A zero block gets byte 0; the byte never reaches
//               0xFF for finite input; emax of e4m3 is 8, so a 2^(127 - s) < 512.
//   3. codes    c_k = e4m3_rne(clamp(v_k 2^(127 - s), -448, 448)): the multiply by a power of two is exact, the clamp is
//               by value ahead of the conversion (OCP MX's saturating conversion -- values in (448, 512) do occur), the
//               conversion is round-to-nearest-even to OCP e4m3 (v_cvt_pk_fp8_f32: the bytes of table_convert.hip's
//               e4m3_rne for a finite value).
//   4. non-finite  a row of x holding a NaN or an infinity gives NaN in every column of that row, weight row n holding
//               one gives NaN in column n of every row, and no other output changes a bit: a per-row flag, applied by a
//               select in the epilogue.  A tainted block's codes are 0; nothing rests on scale byte 0xFF.
//   5. sum      acc[r, n] = sum_j 2^(sx_rj + sw_nj - 254) sum_{k in block j} cx_rk cw_nk by ONE instruction shape,
//               v_mfma_scale_f32_16x16x128_f8f6f4 with both operands fp8 e4m3; k ascending in steps of 128 on a single
//               accumulator, no split-K.  The instruction's internal order and rounding are the hardware's.
//   6. epilogue y = act(acc + b_n): one fp32 add, b_n = 0 where the layer has no bias, act is act_apply.
// So an output depends on its row of x and its row of W alone: not on the tile shape, the grid, the row count or what
// the query was coalesced with.
//
// Operands: x stays fp32 in memory and is quantized in the one pass that stages it into LDS (a block's scale depends on
// its 32 values only: no prologue, no second read, no fp8 copy of an activation in memory); W comes from the layer's MX
// twin, built once from the fp32 weights by launch_mx_twin: codes Wq [N, Kpad], scale bytes We [N, Kpad / 32] and the
// non-finite flags wbad [round_up(N, 4)].
//
// A workgroup of 4 waves (2 x 2) owns 32 TM rows x 32 TN columns; a wave owns TM x TN MFMA tiles.  As in gemm_bf16.hip the
// WEIGHT rows are the A operand, so a lane ends up with four consecutive output columns of one row: one 16-byte store.
//   main loop  per 128-deep K chunk: the global loads of chunk c + 1 go into registers while the TM TN MFMAs of chunk c
//              (ONE per tile pair) run from LDS buffer c & 1.  32 lanes hold a row's 128 floats, eight adjacent lanes one
//              block (8 x float4): three v_max_u32_dpp steps (two quad permutes and row_half_mirror) give every lane the
//              block's a; each lane makes its four codes with two v_cvt_pk_fp8_f32, and stores the dword into buffer
//              (c + 1) & 1; one lane of the eight stores the scale byte into a [rows][4] array per buffer.  Wq pieces
//              (16 bytes a load) and We bytes (one dword per row and chunk) are copied as they are.  One barrier.
//   operands   as measured on an MI355X (profiles/r36_mlp_mxfp8.md), the instruction lays k out like two 16x16x64 steps:
//              lane (r = lane % 16, g = lane / 16) feeds, for row r, k = 16 g .. 16 g + 15 of the chunk in its first four
//              operand registers and k = 64 + 16 g .. 64 + 16 g + 15 in its last four -- two ds_read_b128, 64 bytes apart
//              -- while its SCALE register carries block g (k = 32 g .. 32 g + 31) of row r in the low byte (op_sel 0): the
//              hardware scales the codes of k by the byte of lane 16 (k / 32) + r.  (32 consecutive codes per lane, the
//              layout one would guess, pairs half of every block with another block's scale; the exact-input test of
//              tests/test_mxfp8_mlp.py tells the two apart.)  LDS rows are 128 codes + 16 bytes of padding (144 bytes:
//              the 16 lanes of a ds_read_b128 phase hit different bank groups).
//   epilogue   b as one 16-byte load per lane where aligned, the add, the two flags' selects, act, and the stores of
//              gemm_bf16.hip (write-through and signal_done when the launch is its set's last).
#include <string.h>

#include "drs_internal.h"
#include "mlp_stream.h"

namespace drs {
namespace {

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr int kXThreads = 256;
constexpr int XKC = 128;         // k per chunk: one MFMA deep, four blocks
constexpr int XLD = 144;         // bytes per LDS row: 128 codes + 16 of padding
constexpr uint32_t kAbsMask = 0x7fffffffu, kInfBits = 0x7f800000u;

struct XArgs {
  const float* x;
  int64_t ldx;
  int64_t M;
  const uint8_t* Wq;   // [N, Kpad] e4m3 codes, zero padded
  const uint8_t* We;   // [N, Kpad / 32] E8M0 scale bytes
  const uint8_t* wbad; // [round_up(N, 4)] 1: the weight row holds a NaN or an infinity
  const float* b;
  float* y;
  int64_t ldy;
  int32_t K, Kpad, N, act, sc1;
};

// output stores through inline asm, as gemm_bf16.hip's: nothing waits on them before signal_done's own drain;
// SC1 = write-through (outputs the hand-off reads back)
template <bool SC1>
__device__ __forceinline__ void xst4(float* p, const f32x4 v) {
  // (s_nop 1: the wait states gfx940+ wants before a VALU may overwrite the data registers of a store of more than 64 bits)
  if (SC1) asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" : : "v"(p), "v"(v) : "memory");
  else asm volatile("global_store_dwordx4 %0, %1, off\n\ts_nop 1" : : "v"(p), "v"(v) : "memory");
}
template <bool SC1>
__device__ __forceinline__ void xst1(float* p, const float v) {
  if (SC1) asm volatile("global_store_dword %0, %1, off sc1" : : "v"(p), "v"(v) : "memory");
  else asm volatile("global_store_dword %0, %1, off" : : "v"(p), "v"(v) : "memory");
}

__device__ __forceinline__ uint32_t abs_bits(float v) { return __float_as_uint(v) & kAbsMask; }

// contract step 2, first half: the block's a in every one of the eight adjacent lanes that hold it (4 values each).
// Every lane of the wave must be active: lane l takes from l ^ 1, l ^ 2 and 7 - l % 8 of its own eight.
__device__ __forceinline__ uint32_t block_amax(const float4 v) {
  uint32_t m = max(max(abs_bits(v.x), abs_bits(v.y)), max(abs_bits(v.z), abs_bits(v.w)));
  m = max(m, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)m, 0xB1, 0xf, 0xf, true));    // quad_perm:[1,0,3,2]
  m = max(m, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)m, 0x4E, 0xf, 0xf, true));    // quad_perm:[2,3,0,1]
  m = max(m, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)m, 0x141, 0xf, 0xf, true));   // row_half_mirror
  return m;
}
// ... second half: a's E8M0 byte (finite a: at most 246)
__device__ __forceinline__ uint32_t mx_byte(uint32_t amax_bits) {
  const uint32_t e = amax_bits >> 23;
  return e > 8u ? e - 8u : 0u;
}
// contract step 3: four codes as a dword, lowest k in the lowest byte.  v holds 0.0f for every k >= K (by value); a tainted
// block (a not finite) has the codes 0, by value as well
__device__ __forceinline__ uint32_t mx_codes(const float4 v, uint32_t byte, bool tainted) {
  const float inv = __uint_as_float((254u - byte) << 23);     // 2^(127 - s): a normal number for every s <= 246
  auto sat = [&](float t) { return fminf(fmaxf(__fmul_rn(t, inv), -448.0f), 448.0f); };
  int w = __builtin_amdgcn_cvt_pk_fp8_f32(sat(v.x), sat(v.y), 0, false);
  w = __builtin_amdgcn_cvt_pk_fp8_f32(sat(v.z), sat(v.w), w, true);
  return tainted ? 0u : (uint32_t)w;
}

// VEC: x (every source array), ldx and K allow 16-byte loads that never straddle the end of a row.  Elements from K on
// are 0.0f by value (the loads behind them re-read an element of the row)
template <bool VEC>
__device__ __forceinline__ float4 xload4(const float* q, int k, int K) {
  float4 v;
  if (VEC) v = *reinterpret_cast<const float4*>(q + (k < K ? k : 0));
  else v = make_float4(q[min(k + 0, K - 1)], q[min(k + 1, K - 1)], q[min(k + 2, K - 1)], q[min(k + 3, K - 1)]);
  v.x = k + 0 < K ? v.x : 0.f; v.y = k + 1 < K ? v.y : 0.f; v.z = k + 2 < K ? v.z : 0.f; v.w = k + 3 < K ? v.w : 0.f;
  return v;
}

template <int TM, int TN, bool VEC>
__global__ __launch_bounds__(kXThreads) void gemm_mxfp8_kernel(XArgs a, Done done, XSrc xs) {
  constexpr int BM = 32 * TM, BN = 32 * TN;
  constexpr int NA = BM / 8;       // float4 of x per thread per chunk
  constexpr int NB = BN / 32;      // 16-byte pieces of Wq per thread per chunk: row wrow + 32 j, codes wk .. wk + 15
  constexpr int NH = BM > 64 ? BM / 64 : 1;   // 64-row runs of the tile (a run never straddles two queries)
  constexpr int HT = kXThreads / NH;          // threads that serve one run
  extern __shared__ __attribute__((aligned(16))) float smem[];
  uint32_t* const sBad = reinterpret_cast<uint32_t*>(smem);          // [BM] the row of x holds a NaN or an infinity
  uint8_t* const sXe = reinterpret_cast<uint8_t*>(smem + BM);        // [2][BM][4] scale bytes of the staged blocks of x ...
  uint8_t* const sWe = sXe + 2 * BM * 4;                             // [2][BN][4] ... and of W
  uint8_t* const sX = sWe + 2 * BN * 4;                              // [2][BM][XLD] codes
  uint8_t* const sW = sX + 2 * BM * XLD;                             // [2][BN][XLD]
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int wm = wave & 1, wn = wave >> 1;
  const int64_t m0 = (int64_t)blockIdx.x * BM;
  const int n0 = blockIdx.y * BN;
  const int K = a.K, N = a.N, Kpad = a.Kpad;
  const int nch = Kpad / XKC;
  const int eld = Kpad / 32;       // scale bytes per row of We

  // staging roles.  x: row xr0 + XS j of the tile, floats fk .. fk + 3 of the chunk (block fk / 32: lanes 8 b .. 8 b + 7
  // of a 32-lane row group); a 128-row tile is two 64-row runs, waves 0-1 stage the first and waves 2-3 the second (one
  // look-up of the run's query per wave)
  constexpr int XS = 8 / NH;
  const int half = NH > 1 ? __builtin_amdgcn_readfirstlane(tid >> 7) : 0;
  const int ht = tid & (HT - 1);
  const int xr0 = 64 * half + (ht >> 5), fk = (tid & 31) * 4;
  const int wrow = tid >> 3, wk = (tid & 7) * 16;
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
  const uint8_t* wrowp[NB];
#pragma unroll
  for (int j = 0; j < NB; ++j) wrowp[j] = a.Wq + (int64_t)min(n0 + wrow + 32 * j, N - 1) * Kpad + wk;
  // We: thread t < BN copies the four bytes of weight row n0 + t per chunk
  const uint8_t* const werow = a.We + (int64_t)min(n0 + (tid < BN ? tid : 0), N - 1) * eld;

  for (int i = tid; i < BM; i += kXThreads) sBad[i] = 0u;   // (ordered before every stash by the barrier below)

  float4 ra[NA];
  u32x4 rb[NB];
  uint32_t re = 0;
  auto fetch = [&](int c) {
    const int k = c * XKC + fk;
#pragma unroll
    for (int j = 0; j < NA; ++j) ra[j] = xload4<VEC>(xrow[j], k, K);
#pragma unroll
    for (int j = 0; j < NB; ++j) rb[j] = *reinterpret_cast<const u32x4*>(wrowp[j] + c * XKC);
    if (tid < BN) re = *reinterpret_cast<const uint32_t*>(werow + 4 * c);
  };
  auto stash = [&](int c) {
    uint8_t* const dx = sX + (c & 1) * BM * XLD + xr0 * XLD + fk;
    uint8_t* const de = sXe + (c & 1) * BM * 4 + xr0 * 4 + (fk >> 5);
    uint8_t* const dw = sW + (c & 1) * BN * XLD + wrow * XLD + wk;
#pragma unroll
    for (int j = 0; j < NA; ++j) {
      const uint32_t amax = block_amax(ra[j]);
      const bool tainted = amax >= kInfBits;
      const uint32_t byte = tainted ? 0u : mx_byte(amax);
      *reinterpret_cast<uint32_t*>(dx + XS * j * XLD) = mx_codes(ra[j], byte, tainted);
      if (!(tid & 7)) {
        de[XS * j * 4] = (uint8_t)byte;
        if (tainted) sBad[xr0 + XS * j] = 1u;
      }
    }
#pragma unroll
    for (int j = 0; j < NB; ++j) *reinterpret_cast<u32x4*>(dw + 32 * j * XLD) = rb[j];
    if (tid < BN) *reinterpret_cast<uint32_t*>(sWe + (c & 1) * BN * 4 + tid * 4) = re;
  };

  f32x4 acc[TN][TM];
#pragma unroll
  for (int i = 0; i < TN; ++i)
#pragma unroll
    for (int j = 0; j < TM; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  fetch(0);
  __syncthreads();
  stash(0);
  __syncthreads();
  for (int c = 0; c < nch; ++c) {
    if (c + 1 < nch) fetch(c + 1);
    // my operands of chunk c: lane (r, g) holds k = 16 g .. + 15 and 64 + 16 g .. + 15 of row r of each of its tiles, and the
    // scale byte of the row's block g
    const uint8_t* const px = sX + (c & 1) * BM * XLD + (16 * TM * wm + r) * XLD + 16 * g;
    const uint8_t* const pw = sW + (c & 1) * BN * XLD + (16 * TN * wn + r) * XLD + 16 * g;
    const uint8_t* const ex = sXe + (c & 1) * BM * 4 + (16 * TM * wm + r) * 4 + g;
    const uint8_t* const ew = sWe + (c & 1) * BN * 4 + (16 * TN * wn + r) * 4 + g;
    i32x8 fw[TN], fx[TM];
    int sw[TN], sx[TM];
#pragma unroll
    for (int i = 0; i < TN; ++i) {
      const i32x4 lo = *reinterpret_cast<const i32x4*>(pw + 16 * i * XLD), hi = *reinterpret_cast<const i32x4*>(pw + 16 * i * XLD + 64);
      fw[i] = i32x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
      sw[i] = ew[16 * i * 4];
    }
#pragma unroll
    for (int j = 0; j < TM; ++j) {
      const i32x4 lo = *reinterpret_cast<const i32x4*>(px + 16 * j * XLD), hi = *reinterpret_cast<const i32x4*>(px + 16 * j * XLD + 64);
      fx[j] = i32x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
      sx[j] = ex[16 * j * 4];
    }
#pragma unroll
    for (int i = 0; i < TN; ++i)
#pragma unroll
      for (int j = 0; j < TM; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(fw[i], fx[j], acc[i][j], 0, 0, 0, sw[i], 0, sx[j]);
    if (c + 1 < nch) stash(c + 1);   // (buffer (c + 1) & 1 was last read in iteration c - 1, before its barrier)
    __syncthreads();
  }

  // epilogue: accumulator register q of tile (i, j) is output row 16 j + r, column 16 i + 4 g + q of the wave's block
  bool xbad[TM];
#pragma unroll
  for (int j = 0; j < TM; ++j) xbad[j] = sBad[16 * TM * wm + 16 * j + r] != 0u;
  const float qnan = __uint_as_float(0x7fc00000u);
  const bool vec = !(N & 3) && !(a.ldy & 3) && !((reinterpret_cast<uintptr_t>(a.y) | reinterpret_cast<uintptr_t>(a.b)) & 15);
#pragma unroll
  for (int i = 0; i < TN; ++i) {
    const int col = n0 + 16 * TN * wn + 16 * i + 4 * g;
    f32x4 b4 = {0.f, 0.f, 0.f, 0.f};
    uint32_t wb4 = 0;              // the four columns' flags, one byte each (wbad is padded to a multiple of 4)
    if (col < N) wb4 = *reinterpret_cast<const uint32_t*>(a.wbad + col);
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
      for (int q = 0; q < 4; ++q) {
        const float t = acc[i][j][q] + b4[q];
        v[q] = act_apply(xbad[j] || ((wb4 >> (8 * q)) & 0xffu) ? qnan : t, a.act);
      }
      if (vec) {
        if (col < N) { if (a.sc1) xst4<true>(yrow + col, v); else xst4<false>(yrow + col, v); }
      } else {
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (col + q < N) { if (a.sc1) xst1<true>(yrow + col + q, v[q]); else xst1<false>(yrow + col + q, v[q]); }
      }
    }
  }
  signal_done(done, gridDim.x * gridDim.y, smem);
}

// W [N, K] fp32 -> the MX twin: one wave per weight row, 256 k a pass -- eight adjacent lanes hold a block exactly as in
// gemm_mxfp8_kernel's staging (the same three device functions), so both operands share one quantizer
__global__ __launch_bounds__(256) void mx_twin_kernel(const float* __restrict__ W, int32_t K, int32_t N, int32_t Kpad,
                                                       uint8_t* __restrict__ Wq, uint8_t* __restrict__ We, uint8_t* __restrict__ wbad) {
  const int lane = threadIdx.x & 63;
  const int64_t n = min((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), (int64_t)N - 1);   // (a last block's spare waves redo row N - 1: every lane stays active for the DPP steps)
  const float* const w = W + n * K;
  bool bad = false;
  for (int k0 = 0; k0 < Kpad; k0 += 256) {
    const int k = k0 + 4 * lane;
    const float4 v = xload4<false>(w, k, K);
    const uint32_t amax = block_amax(v);
    const bool tainted = amax >= kInfBits;
    const uint32_t byte = tainted ? 0u : mx_byte(amax);
    const uint32_t codes = mx_codes(v, byte, tainted);
    bad = bad || tainted;
    if (k < Kpad) {
      *reinterpret_cast<uint32_t*>(Wq + n * Kpad + k) = codes;
      if (!(lane & 7)) We[n * (Kpad / 32) + (k >> 5)] = (uint8_t)byte;
    }
  }
  const bool any = __any(bad);
  if (lane == 0) wbad[n] = any ? 1 : 0;
}

template <int TM, int TN>
size_t mx_lds() { return (size_t)4 * 32 * TM + (size_t)2 * (32 * TM + 32 * TN) * (XLD + 4); }

}  // namespace

// per device (device_init)
hipError_t gemm_mxfp8_set_attrs() {
  for (const void* k : {reinterpret_cast<const void*>(gemm_mxfp8_kernel<4, 4, true>), reinterpret_cast<const void*>(gemm_mxfp8_kernel<4, 4, false>),
                        reinterpret_cast<const void*>(gemm_mxfp8_kernel<2, 2, true>), reinterpret_cast<const void*>(gemm_mxfp8_kernel<2, 2, false>),
                        reinterpret_cast<const void*>(gemm_mxfp8_kernel<1, 2, true>), reinterpret_cast<const void*>(gemm_mxfp8_kernel<1, 2, false>)}) {
    hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

hipError_t launch_mx_twin(const float* W, int32_t K, int32_t N, uint8_t* Wq, uint8_t* We, uint8_t* wbad, hipStream_t s) {
  if (N <= 0 || K <= 0) return hipSuccess;
  hipLaunchKernelGGL(mx_twin_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, s, W, K, N, mx_kpad(K), Wq, We, wbad);
  return hipGetLastError();
}

// The MXFP8 GEMM form of the layer p->a (p->mq, me, mbad: its twin).  Tile shapes, as TM * 10 + TN: 44 (128 x 128), 22
// (64 x 64) and 12 (32 x 64), the ones gemm_bf16_plan picks among and by its rule -- the largest that still gives every CU
// (256) a workgroup; tune.mx_tile ("mlp_mx_tile") forces one.  false: no such form (a split input row).
bool gemm_mxfp8_plan(const Tune& tune, MlpPlan* p) {
  const ChainArgs& L = p->a;
  const int64_t M = L.M;
  const int N = L.width[1];
  if (!p->mq || !p->me || !p->mbad || p->xs.ksplit > 0 || L.width[0] < 64 || N < 64) return false;
  auto blocks = [&](int tm, int tn) { return ((M + 32 * tm - 1) / (32 * tm)) * (int64_t)((N + 32 * tn - 1) / (32 * tn)); };
  int t = tune.mx_tile;
  if (!t) t = blocks(4, 4) >= 256 ? 44 : blocks(2, 2) >= 256 ? 22 : 12;
  p->form = MlpForm::gemm_mxfp8;
  p->tm = t / 10; p->tn = t % 10;
  p->grid_x = (unsigned)((M + 32 * p->tm - 1) / (32 * p->tm));
  p->grid_y = (unsigned)((N + 32 * p->tn - 1) / (32 * p->tn));
  p->lds = t == 44 ? mx_lds<4, 4>() : t == 22 ? mx_lds<2, 2>() : mx_lds<1, 2>();
  bool vec = !(L.width[0] & 3) && !(L.ldx & 3) && aligned16(L.x);
  for (int i = 0; i < p->xs.q.n_q; ++i) vec = vec && aligned16(p->xs.x[i]);
  p->vec = vec;
  return true;
}

hipError_t launch_gemm_mxfp8(const MlpPlan& p, hipStream_t s) {
  const ChainArgs& L = p.a;
  XArgs a;
  memset(&a, 0, sizeof a);
  a.x = L.x; a.ldx = L.ldx; a.M = L.M; a.Wq = p.mq; a.We = p.me; a.wbad = p.mbad; a.b = L.b[0]; a.y = L.y; a.ldy = L.ldy;
  a.K = L.width[0]; a.Kpad = mx_kpad(a.K); a.N = L.width[1]; a.act = L.act[0]; a.sc1 = p.done.counter != nullptr;
  const dim3 grid(p.grid_x, p.grid_y);
#define DRS_XLAUNCH(TM_, TN_)                                                                                          \
  if (p.tm == TM_ && p.tn == TN_) {                                                                                    \
    if (p.vec) hipLaunchKernelGGL((gemm_mxfp8_kernel<TM_, TN_, true>), grid, dim3(kXThreads), p.lds, s, a, p.done, p.xs);   \
    else hipLaunchKernelGGL((gemm_mxfp8_kernel<TM_, TN_, false>), grid, dim3(kXThreads), p.lds, s, a, p.done, p.xs);        \
    return hipGetLastError();                                                                                          \
  }
  DRS_XLAUNCH(4, 4) DRS_XLAUNCH(2, 2) DRS_XLAUNCH(1, 2)
#undef DRS_XLAUNCH
  return hipErrorInvalidValue;
}

}  // namespace drs
