// Device code shared by the gather translation units (sls.hip, sls_wflat.hip): the row-element policies ("table_dtype")
// and the kernel templates of the one-lookup, the phased flat and the coalesced flat forms.  sls.hip instantiates their
// unweighted instances, sls_wflat.hip the weighted ones (element type Wgt<policy>), so that the two compile side by side.
#pragma once
#include <type_traits>

#include "drs_internal.h"
#include "owner_dev.h"

namespace drs {
namespace {

__device__ __forceinline__ float4 vzero4() { return make_float4(0.f, 0.f, 0.f, 0.f); }
__device__ __forceinline__ void vadd(float4& a, const float4& b) {
  a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
}
__device__ __forceinline__ float4 vshfl_xor(const float4& a, int m) {
  return make_float4(__shfl_xor(a.x, m), __shfl_xor(a.y, m), __shfl_xor(a.z, m),
                     __shfl_xor(a.w, m));
}
__device__ __forceinline__ float4 vsel(bool keep, const float4& v) {
  return make_float4(keep ? v.x : 0.f, keep ? v.y : 0.f, keep ? v.z : 0.f, keep ? v.w : 0.f);
}

// "sls_pool" 1 (SlsArgs::pool, mean pooling): a bag's FINISHED fp32 sum -- after every cross-lane combine, never a partial
// one -- is divided by its length just before the store: one IEEE fp32 division per element (v_div_scale / v_div_fmas /
// v_div_fixup, correctly rounded, subnormal quotients included), never a multiplication by a reciprocal, which differs
// from torch's EmbeddingBag(mode="mean") on the CPU in about a quarter of the elements.  An empty bag divides its +0.0
// by 1: it stays +0.0.  pool is a kernel argument, i.e. wave-uniform: a scalar branch around the epilogue, and with 0
// the sum is stored as it is.
__device__ __forceinline__ float pool_finish(float sum, int pool, int len) {
  return pool ? __fdiv_rn(sum, len > 0 ? (float)len : 1.0f) : sum;
}
__device__ __forceinline__ void pool_finish(float4& acc, int pool, int len) {
  if (pool) {
    const float d = len > 0 ? (float)len : 1.0f;
    acc = make_float4(__fdiv_rn(acc.x, d), __fdiv_rn(acc.y, d), __fdiv_rn(acc.z, d), __fdiv_rn(acc.w, d));
  }
}

// table rows are read once per launch (~1 % reuse inside a batch): "sls_nt" reads them with the
// non-temporal hint (same-session A/B on RMC1, two boxes: +1.5 % queries/s)
typedef float f4v_nt __attribute__((ext_vector_type(4)));
typedef float f2v_nt __attribute__((ext_vector_type(2)));
__device__ __forceinline__ float4 ld_nt(const float4* p) {
  const f4v_nt t = __builtin_nontemporal_load(reinterpret_cast<const f4v_nt*>(p));
  return make_float4(t.x, t.y, t.z, t.w);
}
__device__ __forceinline__ float2 ld_nt(const float2* p) {
  const f2v_nt t = __builtin_nontemporal_load(reinterpret_cast<const f2v_nt*>(p));
  return make_float2(t.x, t.y);
}
typedef unsigned int u2v_nt __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint2 ld_nt(const uint2* p) {
  const u2v_nt t = __builtin_nontemporal_load(reinterpret_cast<const u2v_nt*>(p));
  return make_uint2(t.x, t.y);
}

__device__ __forceinline__ uint32_t ld_nt(const uint32_t* p) { return __builtin_nontemporal_load(p); }
__device__ __forceinline__ uint16_t ld_nt(const uint16_t* p) { return __builtin_nontemporal_load(p); }

// Row-element policies ("table_dtype"): what a table element is, the PIECE a lane loads -- 4 elements, 16 B of fp32,
// 8 B of fp16 / bf16, 4 B of fp8 or int8 codes or 2 B of int4 codes, one load instruction -- and how a piece of a row is added
// into the fp32 accumulator.  Every fp16 / bf16 value is an fp32 value, so a half form sums exactly what its fp32 twin sums on the
// upcast table, in the same order: the same bits.  tag: the dispatch log's dtype token (none for fp32).
//   sb: what a lane loads per row besides its piece (int8 rowwise: the row's fp32 scale and bias; int4 rowwise: one dword,
//   its fp16 scale and bias; nothing otherwise)
//   pieces_per_row(D): the row stride in pieces; a.tab_off counts `elem`s
//   row_piece(r, pr, ln): where row r starts in its table, in pieces (pr: the row stride) -- r * pr, but for I8L and I4L,
//   whose launch constants `ln` a kernel reads with DRS_ROW_LINES (nothing for every other policy)
//   add(acc, keep, piece, sb): acc += the row's values (keep == false: the row contributes +0)
//   scaled: true for F8 alone -- a bag's FINISHED sum is multiplied by its table's SlsArgs::tab_scale entry just before
//   pool_finish (scale_finish below); with it false nothing that names a scale exists
//   weighted: false for every policy itself; Wgt<E> (below) is E with weighted == true, the element type of a WEIGHTED
//   instance of the one-lookup, flat and flatc kernels -- their unweighted instances keep their symbols that way
struct NoSb {};
template <class Self>
struct PlainRow {
  static constexpr bool rowwise = false, lines = false, weighted = false, scaled = false;
  using sb = NoSb;
  using ln_t = NoSb;
  __host__ __device__ static constexpr uint32_t pieces_per_row(int D) { return (uint32_t)D >> 2; }
  __device__ static __forceinline__ uint32_t row_piece(uint32_t r, uint32_t pr, NoSb) { return r * pr; }
  template <bool NT, class P>
  __device__ static __forceinline__ NoSb load_sb(const P*, int) { return NoSb{}; }
  template <class P>
  __device__ static __forceinline__ void add(float4& acc, bool keep, const P& p, NoSb) { vadd(acc, vsel(keep, Self::up(p))); }
  // the weighted step, acc = fma(w, x, acc) per column: torch's CPU embedding_bag(per_sample_weights=), one rounding per
  // column and row.  w == 1.0f is add's acc + x.  A row that must not count comes with keep == false and is zeroed before
  // the fma, as add zeroes it: fma(w, +0, acc) == acc for every finite w (acc is never -0: it starts at +0 and a sum that
  // cancels is +0).  Its weight alone must not mask it -- fma(0, x, acc) is acc for a finite x only, NaN for +-inf and NaN.
  template <class P>
  __device__ static __forceinline__ void addw(float4& acc, bool keep, float w, const P& p, NoSb) {
    const float4 x = vsel(keep, Self::up(p));
    acc.x = __fmaf_rn(w, x.x, acc.x); acc.y = __fmaf_rn(w, x.y, acc.y); acc.z = __fmaf_rn(w, x.z, acc.z); acc.w = __fmaf_rn(w, x.w, acc.w);
  }
  __device__ static __forceinline__ float addw1(float acc, float w, float x) { return __fmaf_rn(w, x, acc); }
};
struct F32 : PlainRow<F32> {
  using elem = float;
  using piece = float4;
  static constexpr const char* tag = "";
  __device__ static __forceinline__ float4 up(const float4& p) { return p; }
  __device__ static __forceinline__ float up1(float x) { return x; }
};
struct F16 : PlainRow<F16> {
  using elem = uint16_t;
  using piece = uint2;
  static constexpr const char* tag = "f16";
  __device__ static __forceinline__ float up1(uint16_t x) { return (float)__builtin_bit_cast(_Float16, x); }
  __device__ static __forceinline__ float4 up(const uint2& p) {
    return make_float4(up1((uint16_t)p.x), up1((uint16_t)(p.x >> 16)), up1((uint16_t)p.y), up1((uint16_t)(p.y >> 16)));
  }
};
struct BF16 : PlainRow<BF16> {
  using elem = uint16_t;
  using piece = uint2;
  static constexpr const char* tag = "bf16";
  __device__ static __forceinline__ float up1(uint16_t x) { return __uint_as_float((uint32_t)x << 16); }
  __device__ static __forceinline__ float4 up(const uint2& p) {
    return make_float4(__uint_as_float(p.x << 16), __uint_as_float(p.x & 0xffff0000u), __uint_as_float(p.y << 16),
                       __uint_as_float(p.y & 0xffff0000u));
  }
};
// fp8 e4m3 ("table_dtype" 4): OCP e4m3 codes (torch's float8_e4m3fn; gfx950's conversions are the OCP ones), a row is D
// bytes and a piece one aligned dword, widened by two v_cvt_pk_f32_fp8.  Table t stores e4m3_rne(x * 2^k_t): the kernels
// sum the decoded codes as F16 sums upcast halves and multiply a bag's finished accumulator by 2^-k_t (scale_finish).
// A power of two commutes with every fp32 add, fma and division short of a subnormal or overflowing intermediate --
// none with |k| <= 64 and codes that are multiples of 2^-9 up to 448 -- so every form serves the bits its fp32 twin
// serves on the decoded table decode(code) * 2^-k_t, in the same order.  a.tab_off counts bytes.
typedef float f2v_cvt __attribute__((ext_vector_type(2)));
struct F8 : PlainRow<F8> {
  static constexpr bool scaled = true;
  using elem = uint8_t;
  using piece = uint32_t;
  static constexpr const char* tag = "f8";
  __device__ static __forceinline__ float up1(uint8_t x) { return __builtin_amdgcn_cvt_f32_fp8((uint32_t)x, 0); }
  __device__ static __forceinline__ float4 up(uint32_t p) {
    const f2v_cvt lo = __builtin_amdgcn_cvt_pk_f32_fp8(p, false), hi = __builtin_amdgcn_cvt_pk_f32_fp8(p, true);
    return make_float4(lo.x, lo.y, hi.x, hi.y);
  }
};
// 8-bit rowwise ("table_dtype" 8, Caffe2's Fused8BitRowwise): a row is D uint8 codes, zero padding to round_up(D, 8)
// bytes, then the fp32 scale and the fp32 bias (S = round_up(D, 8) + 8 bytes, every row 8-byte aligned).  a.tab_off
// counts bytes.  A piece is one dword of codes (v_cvt_f32_ubyte0..3); the lanes of a row group load the same 8 bytes of
// scale and bias beside it.  A row adds acc = fmaf(scale, q, acc + bias) per column: FBGEMM's and Caffe2's order, so the
// sequential form is bit-identical to embedding_bag_byte_rowwise_offsets.  A masked row adds with scale = bias = 0:
// acc + 0 + 0 * q == acc (acc is never -0: every step is an fma onto a sum with +0) -- the zeros are SELECTED, never the
// product of a zero weight and the row's header.  A finite fp32 row whose range overflows its header (max - min above
// fp32's largest value here, (max - bias) / 15 above fp16's for int4) is stored with the scale +inf and the codes 0, as
// torch's prepack operators store it, and decodes to inf * 0 = NaN in every column: that NaN reaches the bags that name
// the row, as in torch's rowwise bags, and no other.
struct I8 {
  static constexpr bool rowwise = true, lines = false, weighted = false, scaled = false;
  using elem = uint8_t;
  using piece = uint32_t;
  using sb = float2;
  using ln_t = NoSb;
  static constexpr const char* tag = "i8";
  __host__ __device__ static constexpr int padded(int D) { return (D + 7) & ~7; }
  __host__ __device__ static constexpr uint32_t pieces_per_row(int D) { return ((uint32_t)padded(D) >> 2) + 2u; }
  __device__ static __forceinline__ uint32_t row_piece(uint32_t r, uint32_t pr, NoSb) { return r * pr; }
  // code: the lane's piece of the row; delta: bytes from it to the row's scale (round_up(D, 8) - the lane's column)
  template <bool NT>
  __device__ static __forceinline__ float2 load_sb(const uint32_t* code, int delta) {
    const float2* p = reinterpret_cast<const float2*>(reinterpret_cast<const uint8_t*>(code) + delta);
    if constexpr (NT) return ld_nt(p); else return *p;
  }
  __device__ static __forceinline__ float row1(float s, float b, float q, float acc) { return __fmaf_rn(s, q, __fadd_rn(acc, b)); }
  // a whole row at `row` (sls_any_kernel, the table kernels): its scale and bias, and the code of column c
  __device__ static __forceinline__ float2 row_sb(const uint8_t* row, int D) { return *reinterpret_cast<const float2*>(row + padded(D)); }
  __device__ static __forceinline__ float code(const uint8_t* row, int c) { return (float)row[c]; }
  __device__ static __forceinline__ void add(float4& acc, bool keep, uint32_t p, float2 sb) {
    const float s = keep ? sb.x : 0.f, b = keep ? sb.y : 0.f;
    acc.x = row1(s, b, (float)(p & 0xffu), acc.x);
    acc.y = row1(s, b, (float)((p >> 8) & 0xffu), acc.y);
    acc.z = row1(s, b, (float)((p >> 16) & 0xffu), acc.z);
    acc.w = row1(s, b, (float)(p >> 24), acc.w);
  }
  // the weighted step (FBGEMM's and torch's embedding_bag_byte_rowwise_offsets with per_sample_weights): the row's scale
  // and bias are multiplied by its weight first -- two fp32 products -- and go through row1 as they are.  w == 1.0f
  // is add.  A row that must not count (keep == false) is dropped AFTER the products, as add drops it: s = b = +0 and
  // acc + 0 + 0 * q == acc.  Masking its weight instead (w = 0) leaves s = 0 * scale, which is NaN for the scale +inf
  // of a row whose header overflowed -- row 0, which every empty bag reads, above all.
  // (The two products are written under contract(off): __fmul_rn is a plain, contractable `x * y` to this compiler, which
  // folds w * bias into row1's acc + b as one fma in some instances -- the weighted flat forms at 20 loads per lane --
  // and then rounds once where the operator rounds twice.  The pragma does not reach into an inlined callee.)
  __device__ static __forceinline__ void addw(float4& acc, bool keep, float w, uint32_t p, float2 sb) {
#pragma clang fp contract(off)
    const float ws = w * sb.x, wb = w * sb.y;
    const float s = keep ? ws : 0.f, b = keep ? wb : 0.f;
    acc.x = row1(s, b, (float)(p & 0xffu), acc.x);
    acc.y = row1(s, b, (float)((p >> 8) & 0xffu), acc.y);
    acc.z = row1(s, b, (float)((p >> 16) & 0xffu), acc.z);
    acc.w = row1(s, b, (float)(p >> 24), acc.w);
  }
};
// The same rows in the line-packed layout ("table_int8_lines" 1, drs_internal.h I8Lines): n = 128 / S rows to a 128-byte
// line, so that no row crosses one.  Only where a row starts differs -- r * PR + (r / n) * pad pieces into its table, the
// quotient one v_mul_hi_u32 and a shift by the launch's constants -- so every form sums the same values in the same order
// as I8.  The range check stays r < rows: the unused slots of a table's last line are out of range like any other index.
struct LineMap { uint32_t mul, shift, pad; };   // SlsArgs::ln_mul, ln_shift, ln_pad
struct I8L : I8 {
  static constexpr bool lines = true;
  using ln_t = LineMap;
  static constexpr const char* tag = "i8l";
  __device__ static __forceinline__ uint32_t row_piece(uint32_t r, uint32_t pr, LineMap ln) {
    const uint32_t q = ln.mul ? __umulhi(r, ln.mul) >> ln.shift : r;
    return r * pr + q * ln.pad;
  }
};
// 4-bit rowwise ("table_dtype" 9, FBGEMM's Fused4BitRowwise, torch's embedding_bag_4bit_prepack byte for byte): a row is
// D / 2 code bytes -- column 2j the low nibble of byte j, column 2j + 1 the high one -- zero padding to round_up(D / 2, 4)
// bytes, then the fp16 scale and the fp16 bias (S = round_up(D / 2, 4) + 4 bytes, every row and every scale / bias pair
// 4-byte aligned; D even).  a.tab_off counts bytes.  A piece is the 2 bytes that hold a lane's 4 codes; the lanes of a row
// group load the same dword of scale and bias beside it and widen the two halves in registers.  A row adds with I8's step,
// acc = fmaf(scale, q, acc + bias): the sequential form is bit-identical to embedding_bag_4bit_rowwise_offsets, and every
// form sums the same values in the order its int8 twin does.
struct I4 {
  static constexpr bool rowwise = true, lines = false, weighted = false, scaled = false;
  using elem = uint8_t;
  using piece = uint16_t;
  using sb = uint32_t;
  using ln_t = NoSb;
  static constexpr const char* tag = "i4";
  __host__ __device__ static constexpr int padded(int D) { return ((D >> 1) + 3) & ~3; }   // code bytes of a row
  __host__ __device__ static constexpr uint32_t pieces_per_row(int D) { return ((uint32_t)padded(D) >> 1) + 2u; }
  __device__ static __forceinline__ uint32_t row_piece(uint32_t r, uint32_t pr, NoSb) { return r * pr; }
  // code: the lane's piece of the row; delta: bytes from it to the row's scale (padded(D) - the lane's column / 2)
  template <bool NT>
  __device__ static __forceinline__ uint32_t load_sb(const uint16_t* code, int delta) {
    const uint32_t* p = reinterpret_cast<const uint32_t*>(reinterpret_cast<const uint8_t*>(code) + delta);
    if constexpr (NT) return ld_nt(p); else return *p;
  }
  __device__ static __forceinline__ float2 up_sb(uint32_t w) { return make_float2(F16::up1((uint16_t)w), F16::up1((uint16_t)(w >> 16))); }
  __device__ static __forceinline__ float row1(float s, float b, float q, float acc) { return I8::row1(s, b, q, acc); }
  __device__ static __forceinline__ float2 row_sb(const uint8_t* row, int D) { return up_sb(*reinterpret_cast<const uint32_t*>(row + padded(D))); }
  __device__ static __forceinline__ float code(const uint8_t* row, int c) { return (float)((row[c >> 1] >> ((c & 1) * 4)) & 15u); }
  __device__ static __forceinline__ void add(float4& acc, bool keep, uint16_t p16, uint32_t w) {
    const float2 f = up_sb(w);
    const float s = keep ? f.x : 0.f, b = keep ? f.y : 0.f;
    const uint32_t p = p16;
    acc.x = row1(s, b, (float)(p & 15u), acc.x);
    acc.y = row1(s, b, (float)((p >> 4) & 15u), acc.y);
    acc.z = row1(s, b, (float)((p >> 8) & 15u), acc.z);
    acc.w = row1(s, b, (float)(p >> 12), acc.w);
  }
  // the weighted step: I8's, on the widened fp16 scale and bias (embedding_bag_4bit_rowwise_offsets with per_sample_weights)
  __device__ static __forceinline__ void addw(float4& acc, bool keep, float w, uint16_t p16, uint32_t w32) {
#pragma clang fp contract(off)   // (as I8::addw: the two products stay products, and the row is dropped after them)
    const float2 f = up_sb(w32);
    const float ws = w * f.x, wb = w * f.y;
    const float s = keep ? ws : 0.f, b = keep ? wb : 0.f;
    const uint32_t p = p16;
    acc.x = row1(s, b, (float)(p & 15u), acc.x);
    acc.y = row1(s, b, (float)((p >> 4) & 15u), acc.y);
    acc.z = row1(s, b, (float)((p >> 8) & 15u), acc.z);
    acc.w = row1(s, b, (float)(p >> 12), acc.w);
  }
};
// The same rows in the line-packed layout ("table_int4_lines" 1): I8L's rule with int4's S and 2-byte pieces -- n = 128 / S
// rows to a line, row r at r * PR + (r / n) * pad pieces with PR = S / 2 and pad = 64 - n * PR.  Every form sums the same
// values in the same order as I4; the range check stays r < rows.
struct I4L : I4 {
  static constexpr bool lines = true;
  using ln_t = LineMap;
  static constexpr const char* tag = "i4l";
  __device__ static __forceinline__ uint32_t row_piece(uint32_t r, uint32_t pr, LineMap ln) { return I8L::row_piece(r, pr, ln); }
};
// E in a weighted instance of sls_one_kernel, sls_flat_kernel and sls_flatc_kernel (sls_wflat.hip): the same rows, the
// same tag, and E::addw where the unweighted instance calls E::add
template <class E>
struct Wgt : E {
  static constexpr bool weighted = true;
};
// E::scaled (fp8): the finished sum of table t's bag, out of the code domain -- times the table's 2^-k, before pool_finish
template <class E>
__device__ __forceinline__ void scale_finish(float4& acc, const SlsArgs& a, int t) {
  if constexpr (E::scaled) {
    const float s = a.tab_scale[t];
    acc = make_float4(__fmul_rn(acc.x, s), __fmul_rn(acc.y, s), __fmul_rn(acc.z, s), __fmul_rn(acc.w, s));
  }
}
#define DRS_ROW_LINES(E, a, ln) \
  typename E::ln_t ln{};        \
  if constexpr (E::lines) ln = LineMap{(a).ln_mul, (a).ln_shift, (a).ln_pad};
template <class E>
__device__ __forceinline__ const typename E::elem* table_base(const float* tables) {
  return reinterpret_cast<const typename E::elem*>(tables);
}
// a piece in `elem`s (4, but int4 rowwise: 2 bytes), and where column `col` (a multiple of 4) of a row is, in `elem`s
template <class E>
constexpr int kPieceElems = (int)(sizeof(typename E::piece) / sizeof(typename E::elem));
template <class E>
__device__ __forceinline__ int col_elems(int col) {
  if constexpr (kPieceElems<E> == 4) return col; else return (col >> 2) * kPieceElems<E>;
}
// bytes from a lane's piece (at column `col`) to its row's scale: the rowwise types only (their `elem` is a byte)
template <class E>
__device__ __forceinline__ int sb_delta(int D, int col) {
  if constexpr (E::rowwise) return E::padded(D) - col_elems<E>(col); else return 0;
}

// ---------------------------------------------------------------------------
// ONE lookup per bag (W&D, MT-WnD, NCF, DIEN: num_indices_per_lookup 1, fixed): the pooled "sum" is an indexed row
// copy, and the lane-group-per-bag walk above spends it waiting -- three dependent round trips (index, row, store)
// for the 1 KB a wave has in flight.  Here a wave takes 64 samples of ONE table: lane i reads sample i's index (one
// coalesced request per query the tile touches) and finds its output row; lane group g then copies bags g G ..
// g G + G - 1, M = min(G, 8) rows in flight per lane (8 KB per wave at D 32), the row numbers and output rows
// coming over the cross-lane network.  The value stored is 0.0f + row, the sequential form's single addition:
// the same bits.  D == 4 G exactly.  BW = samples per wave: 64, or 16 for launches that would otherwise be a few dozen
// waves (one query of NCF: 4 tables x 256 samples) -- lanes 0 .. 15 fetch the indices then.
// WGT: the weighted instance ("sls_weighted_flat" 1; a.wgt, a null entry weighs every row 1.0f).  Lane i reads sample i's
// weight beside its index -- the owning query differs per lane, so its a.wgt entry comes down the same select chain -- the
// copying lanes take it over the cross-lane network beside the row number, and the value stored is addw(+0, w, row), the
// sequential form's single weighted step: the same bits.  WGT is E::weighted (E = Wgt<policy>); with it false nothing
// that names a weight exists.
template <int G, int BW, class E = F32>
__global__ __launch_bounds__(64) void sls_one_kernel(SlsArgs a, int tiles) {
  constexpr bool WGT = E::weighted;
  using piece = typename E::piece;
  using wt = std::conditional_t<WGT, float, NoSb>;
  constexpr int NG = 64 / G, PER = BW / NG;          // bags a lane group copies
  constexpr uint32_t PR = E::pieces_per_row(4 * G);  // row stride in pieces (G: 4 elements per lane)
  constexpr int M = PER < 8 ? PER : 8;               // ... M at a time
  static_assert(PER >= 1 && PER % M == 0, "whole rounds");
  if (a.ts && threadIdx.x == 0) a.ts[2 * blockIdx.x] = wall_clock64();
  const int lane = threadIdx.x;
  const int g = lane / G, gl = lane - g * G;
  const int n_smp = a.q.cum[a.q.n_q];
  const int t = (int)blockIdx.x / tiles;                   // (uniform: table bases and row counts are scalar loads)
  const int smp = ((int)blockIdx.x - t * tiles) * BW + lane;
  const bool ok = lane < BW && smp < n_smp;
  DRS_OWNER_OF(a, smp, b, vrow, ulen, qidx, qoff)
  const uint32_t rows = (uint32_t)a.tab_rows[t];
  uint32_t r = ok ? (uint32_t)qidx[(int64_t)t * a.idx_stride + b] : 0u;
  const bool bad = r >= rows;                               // Caffe2's ENFORCE: flag it, contribute zero
  if (bad) atomicOr(a.err, 1);
  r = bad ? 0u : r;
  [[maybe_unused]] wt wl{};
  if constexpr (WGT) {   // (an out-of-range row takes the weight 0)
    const float* qwgt = a.wgt[0];
    DRS_OWNER_CHAIN(a.q, smp, qwgt = in ? a.wgt[i] : qwgt;)
    wl = ok && qwgt ? qwgt[(int64_t)t * a.idx_stride + b] : 1.0f;
    wl = bad ? 0.0f : wl;
  }
  // what the copying lanes need of sample i: its row number, and its output row (-1: nothing to store)
  const int dst = ok ? vrow : -1;
  const int keep = bad ? 0 : 1;
  const piece* __restrict__ W = reinterpret_cast<const piece*>(table_base<E>(a.tables) + a.tab_off[t]) + gl;
  float* __restrict__ out = a.out + a.col0 + (int64_t)t * (4 * G) + gl * 4;
  const int sbd = sb_delta<E>(4 * G, gl * 4);
  DRS_ROW_LINES(E, a, ln)
#pragma unroll
  for (int j0 = 0; j0 < PER; j0 += M) {
    piece v[M];
    typename E::sb sb[M];
    int vr[M], kp[M];
    [[maybe_unused]] wt wj[M];
#pragma unroll
    for (int j = 0; j < M; ++j) {
      const int src = g * PER + j0 + j;
      const uint32_t rj = (uint32_t)__shfl((int)r, src);
      vr[j] = __shfl(dst, src);
      kp[j] = __shfl(keep, src);
      if constexpr (WGT) wj[j] = __shfl(wl, src);
      const uint32_t ro = E::row_piece(rj, PR, ln);            // rows * D / 4 < 2^32 (enforced at table creation)
      v[j] = W[(uint64_t)ro];
      sb[j] = E::template load_sb<false>(W + (uint64_t)ro, sbd);
    }
#pragma unroll
    for (int j = 0; j < M; ++j)
      if (vr[j] >= 0) {
        float4 o = vzero4();                                  // 0.0f + row: the one-row bag's value
        if constexpr (WGT) E::addw(o, kp[j] != 0, wj[j], v[j], sb[j]);
        else E::add(o, kp[j] != 0, v[j], sb[j]);
        scale_finish<E>(o, a, t);
        pool_finish(o, a.pool, 1);                            // a one-row bag's mean: x / 1.0f == x, the same bits
        *reinterpret_cast<float4*>(out + (int64_t)vr[j] * a.ld_out) = o;
      }
  }
  if (a.ts) {
    __builtin_amdgcn_s_waitcnt(0);
    if (threadIdx.x == 0) a.ts[2 * blockIdx.x + 1] = wall_clock64();
  }
}

// ---------------------------------------------------------------------------
// FLAT variant: fixed-length bags, G lanes per row (16 B per lane), NL loads per lane, BPW
// bags (same sample, consecutive tables) per wave.  Requires L * BPW <= NL * (64 / G) and
// T % BPW == 0 (checked by plan_sls).
// WGT: the weighted instance ("sls_weighted_flat" 1).  A row's weight lies where its index lies in the owning query's
// a.wgt entry (the sample is wave-uniform: a scalar pointer; null: every weight 1.0f): phase 1 loads it through the
// address pattern of the index, and bag k adds E::addw with it in the order of the unweighted sums -- a row of another bag
// or past the wave's rows is dropped (keep == false: its value never reaches the sum, whatever it holds), an out-of-range
// row takes the weight 0.0f.  WGT is E::weighted (E = Wgt<policy>); with it false nothing
// that names a weight exists.
template <int G, int NL, int BPW, bool NT = false, class E = F32>
__global__ __launch_bounds__(64) void sls_flat_kernel(SlsArgs a, int L, int xcd_order) {
  constexpr bool WGT = E::weighted;
  using elem = typename E::elem;
  using piece = typename E::piece;
  using wt = std::conditional_t<WGT, float, NoSb>;
  constexpr int NG = 64 / G;                       // lane groups = rows per load instruction
  // Work item w = (table group, sample), numbered TABLE-MAJOR; everything that depends only on
  // the wave (sample, query, tables) is scalar.  XCD-aware order (xcd_order != 0): workgroup id
  // lands on XCD id % 8 (observed dispatch order; speed only, never correctness), and XCD x walks
  // the contiguous slice [x*per, (x+1)*per) of the work list -- so one XCD's L2 and TLBs see one or
  // two tables (and contiguous pieces of their index arrays) instead of all T of them.
  const unsigned wg = blockIdx.x;
  if (a.ts && threadIdx.x == 0) a.ts[2 * wg] = wall_clock64();
  const unsigned n_smp = (unsigned)a.q.cum[a.q.n_q];
  const unsigned n_work = n_smp * (unsigned)(a.T / BPW);
  unsigned w = wg;
  if (xcd_order) {
    const unsigned per = (n_work + 7u) >> 3;
    w = (wg & 7u) * per + (wg >> 3);
    if ((wg >> 3) >= per || w >= n_work) {
      if (a.ts && threadIdx.x == 0) a.ts[2 * wg + 1] = a.ts[2 * wg];   // keep (min, max) well defined
      return;
    }
  }
  const unsigned tg = (unsigned)__builtin_amdgcn_readfirstlane((int)(w / n_smp));

  const int lane = threadIdx.x;
  const int g = lane / G;
  const int gl = lane - g * G;
  const int col = min(gl * 4, a.D - 4);            // clamp idle lanes onto valid columns
  const bool col_ok = gl * 4 < a.D;

  const int smp = (int)(w - tg * n_smp);
  const int t0 = (int)tg * BPW;
  DRS_OWNER_OF(a, smp, b, vrow, ulen, qidx, qoff)
  [[maybe_unused]] const float* qwgt = nullptr;
  if constexpr (WGT) {
    qwgt = a.wgt[0];
    DRS_OWNER_CHAIN(a.q, smp, qwgt = in ? a.wgt[i] : qwgt;)
  }
  const int R = BPW * L;
  const uint32_t D4 = E::pieces_per_row(a.D);      // row stride in pieces: rows * D / 4 < 2^32 (enforced at table creation)
  const int sbd = sb_delta<E>(a.D, col);
  DRS_ROW_LINES(E, a, ln)
  // table bases and row counts of the wave's BPW tables: scalar loads, issued now and waited
  // for only when the row addresses are formed, i.e. in the shadow of the index loads.  (Left
  // to the compiler they become vector loads -- it cannot prove the arrays are not written by
  // this kernel -- and cost a dependent round trip BEFORE the index loads.)
  uint64_t tab_off_k[BPW], tab_rows_k[BPW];
  {
    const uint32_t boff = (uint32_t)__builtin_amdgcn_readfirstlane(t0) * 8u;
#pragma unroll
    for (int k = 0; k < BPW; ++k) {
      asm volatile("s_load_dwordx2 %0, %1, %2" : "=s"(tab_off_k[k]) : "s"(a.tab_off), "s"(boff + 8u * k));
      asm volatile("s_load_dwordx2 %0, %1, %2" : "=s"(tab_rows_k[k]) : "s"(a.tab_rows), "s"(boff + 8u * k));
    }
  }
  // which of the wave's bags does flattened row j belong to (j < R)
  auto bag_of = [&](int j) {
    int k = 0;
#pragma unroll
    for (int q = 1; q < BPW; ++q) k += j >= q * L ? 1 : 0;
    return k;
  };

  // ---- phase 1: the index of every row this lane will load.  The G lanes of a group read the
  // same word and the 64/G groups adjacent words: one 32..128-B segment per instruction, all NL
  // of them in flight together -------------------------------------------------------------
  const int32_t* ip[NL];
  int kj[NL];
#pragma unroll
  for (int u = 0; u < NL; ++u) {
    const int jj = min(g + NG * u, R - 1);
    kj[u] = bag_of(jj);
    ip[u] = qidx + (int64_t)(t0 + kj[u]) * a.idx_stride + (int64_t)b * L + (jj - kj[u] * L);
  }
  __builtin_amdgcn_sched_barrier(0);
  uint32_t ridx[NL];
#pragma unroll
  for (int u = 0; u < NL; ++u) ridx[u] = (uint32_t)*ip[u];
  [[maybe_unused]] wt wr[NL];
  if constexpr (WGT) {   // the rows' weights: the same words of the weight array, in flight with the indices
    if (qwgt) {
#pragma unroll
      for (int u = 0; u < NL; ++u) wr[u] = qwgt[ip[u] - qidx];
    } else {
#pragma unroll
      for (int u = 0; u < NL; ++u) wr[u] = 1.0f;
    }
  }
  __builtin_amdgcn_sched_barrier(0);
  // (the s_loads above: not tracked by the compiler's counters)
  if (BPW == 1) asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(tab_off_k[0]), "+s"(tab_rows_k[0]));
  else if (BPW == 2) asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(tab_off_k[0]), "+s"(tab_rows_k[0]), "+s"(tab_off_k[BPW > 1 ? 1 : 0]), "+s"(tab_rows_k[BPW > 1 ? 1 : 0]));
  else asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(tab_off_k[0]), "+s"(tab_rows_k[0]), "+s"(tab_off_k[BPW > 1 ? 1 : 0]), "+s"(tab_rows_k[BPW > 1 ? 1 : 0]),
                    "+s"(tab_off_k[BPW > 2 ? 2 : 0]), "+s"(tab_rows_k[BPW > 2 ? 2 : 0]), "+s"(tab_off_k[BPW > 3 ? 3 : 0]), "+s"(tab_rows_k[BPW > 3 ? 3 : 0]));

  // ---- phase 2: range check (Caffe2 ENFORCE) and every row address of the wave ----------------
  const elem* rp[NL];
  bool bad = false;
#pragma unroll
  for (int u = 0; u < NL; ++u) {
    const elem* W = table_base<E>(a.tables) + tab_off_k[0];
    uint32_t rk = (uint32_t)tab_rows_k[0];
#pragma unroll
    for (int z = 1; z < BPW; ++z) {
      W = kj[u] == z ? table_base<E>(a.tables) + tab_off_k[z] : W;
      rk = kj[u] == z ? (uint32_t)tab_rows_k[z] : rk;
    }
    bad |= g + NG * u < R && ridx[u] >= rk;
    if constexpr (WGT) wr[u] = ridx[u] < rk ? wr[u] : 0.0f;
    const uint32_t ro = E::row_piece(ridx[u] < rk ? ridx[u] : 0u, D4, ln) + ((uint32_t)col >> 2);
    rp[u] = W + (uint64_t)ro * kPieceElems<E>;
  }
  // ---- phase 3: all row loads, back to back, nothing else in between --------------------------
  __builtin_amdgcn_sched_barrier(0);
  piece v[NL];
  typename E::sb sb[NL];
#pragma unroll
  for (int u = 0; u < NL; ++u) {
    if constexpr (NT) v[u] = ld_nt(reinterpret_cast<const piece*>(rp[u]));
    else v[u] = *reinterpret_cast<const piece*>(rp[u]);
    sb[u] = E::template load_sb<NT>(reinterpret_cast<const piece*>(rp[u]), sbd);
  }
  __builtin_amdgcn_sched_barrier(0);

  // ---- phase 4: per-bag sums in arrival order, then the butterfly over the lane groups --------
  float4 acc[BPW];
#pragma unroll
  for (int k = 0; k < BPW; ++k) acc[k] = vzero4();
#pragma unroll
  for (int u = 0; u < NL; ++u) {
    const int j = g + NG * u;
    if constexpr (WGT) {
#pragma unroll
      for (int k = 0; k < BPW; ++k) E::addw(acc[k], j < R && kj[u] == k, wr[u], v[u], sb[u]);
    } else if (BPW == 1) {
      E::add(acc[0], j < R, v[u], sb[u]);
    } else {
#pragma unroll
      for (int k = 0; k < BPW; ++k) E::add(acc[k], j < R && kj[u] == k, v[u], sb[u]);
    }
  }
#pragma unroll
  for (int k = 0; k < BPW; ++k)
#pragma unroll
    for (int m = G; m < 64; m <<= 1) vadd(acc[k], vshfl_xor(acc[k], m));

  if (bad) atomicOr(a.err, 1);
#pragma unroll
  for (int k = 0; k < BPW; ++k) {
    scale_finish<E>(acc[k], a, t0 + k);
    pool_finish(acc[k], a.pool, L);
  }
  // every group holds every sum after the butterfly; group 0 stores them, one 128..512-B row per
  // bag.  (Letting group k store bag k needs acc[g]: the optimiser turns that select chain into a
  // dynamically indexed array, i.e. SCRATCH memory -- which capped the BPW > 1 variants at half
  // the speed of BPW == 1 until it was spotted in the ISA.)
  if (col_ok && g == 0) {
    float* o = a.out + (int64_t)vrow * a.ld_out + a.col0 + (int64_t)t0 * a.D + col;
#pragma unroll
    for (int k = 0; k < BPW; ++k) *reinterpret_cast<float4*>(o + (int64_t)k * a.D) = acc[k];
  }
  if (a.ts) {
    __builtin_amdgcn_s_waitcnt(0);   // include the output store in the span
    if (threadIdx.x == 0) a.ts[2 * wg + 1] = wall_clock64();
  }
}

// The first form of the flat variant, one bag per wave: ONE coalesced index read (lane i owns
// row i), indices handed to the loading lanes over the cross-lane network, and the row loads /
// sums left to the compiler's schedule -- which turns them into groups of four or five loads in
// flight with the sums of one group under the next.  Measured against the phased form above
// (everything in flight at once) on RMC1's 80 x 256-B bags beside the MLP launch: 0.74 vs 0.72 of
// peak for 8-query launches, 0.57-0.59 vs 0.51 for a single query; so one-bag-per-wave launches
// take this one ("sls_flat" 1) and the phased form serves the several-bags-per-wave shapes.
// WGT: the weighted instance ("sls_weighted_flat" 1).  The lane that owns flattened row i reads its weight beside its index
// -- the same coalesced pattern on the owning query's a.wgt entry (the sample is wave-uniform: a scalar pointer; null:
// every weight 1.0f), 0.0f for an out-of-range row -- and at sum time the loading lanes fetch it as they fetched the row
// offset; the sum is E::addw in the same u order with the unweighted j < R as its keep (the re-read row R - 1 is dropped,
// whatever it holds), then the same butterfly.  WGT is E::weighted
// (E = Wgt<policy>); with it false nothing that names a weight exists.
template <int G, int NL, bool NT, class E = F32>
__global__ __launch_bounds__(64) void sls_flatc_kernel(SlsArgs a, int L) {
  constexpr bool WGT = E::weighted;
  using elem = typename E::elem;
  using piece = typename E::piece;
  using wt = std::conditional_t<WGT, float, NoSb>;
  constexpr int BPW = 1;
  constexpr int NG = 64 / G;                       // lane groups = rows per load instruction
  constexpr int NI = (NL * NG + 63) / 64;          // index registers per lane
  if (a.ts && threadIdx.x == 0) a.ts[2 * blockIdx.x] = wall_clock64();

  const int lane = threadIdx.x;
  const int g = lane / G;
  const int gl = lane - g * G;
  const int col = min(gl * 4, a.D - 4);            // clamp idle lanes onto valid columns
  const bool col_ok = gl * 4 < a.D;

  // the wave's bags: all of one sample (T % BPW == 0), tables t0 .. t0+BPW-1 -- uniform
  const int64_t bag0 = (int64_t)blockIdx.x * BPW;
  const int smp = (int)(bag0 / a.T);
  const int t0 = (int)(bag0 - (int64_t)smp * a.T);
  DRS_OWNER_OF(a, smp, b, vrow, ulen, qidx, qoff)
  [[maybe_unused]] const float* qwgt = nullptr;
  if constexpr (WGT) {
    qwgt = a.wgt[0];
    DRS_OWNER_CHAIN(a.q, smp, qwgt = in ? a.wgt[i] : qwgt;)
  }
  const int R = BPW * L;
  const uint32_t D4 = E::pieces_per_row(a.D);      // row stride in pieces: rows * D / 4 < 2^32 (enforced at table creation)
  const int sbd = sb_delta<E>(a.D, col);
  DRS_ROW_LINES(E, a, ln)
  const elem* Wk[BPW];
  uint32_t rows_k[BPW];
#pragma unroll
  for (int k = 0; k < BPW; ++k) {
    Wk[k] = table_base<E>(a.tables) + a.tab_off[t0 + k] + col_elems<E>(col);
    rows_k[k] = (uint32_t)a.tab_rows[t0 + k];
  }
  // which of the wave's bags does flattened row j belong to (j < R)
  auto bag_of = [&](int j) {
    int k = 0;
#pragma unroll
    for (int q = 1; q < BPW; ++q) k += j >= q * L ? 1 : 0;
    return k;
  };

  // ONE coalesced index read: lane i owns flattened rows i, i+64, ...; range check (Caffe2
  // ENFORCE) and the row's element offset inside its table are computed by the owner
  uint32_t roff[NI];
  [[maybe_unused]] wt rwgt[NI];
  bool bad = false;
#pragma unroll
  for (int q = 0; q < NI; ++q) {
    const int i = lane + 64 * q;
    const int ii = min(i, R - 1);
    const int k = bag_of(ii);
    const int32_t* ip = qidx + (int64_t)(t0 + k) * a.idx_stride + (int64_t)b * L + (ii - k * L);
    uint32_t r = (uint32_t)*ip;
    uint32_t rk = rows_k[0];
#pragma unroll
    for (int z = 1; z < BPW; ++z) rk = k == z ? rows_k[z] : rk;
    bad |= i < R && r >= rk;
    if constexpr (WGT) {
      const float w = qwgt ? qwgt[ip - qidx] : 1.0f;
      rwgt[q] = i < R && r < rk ? w : 0.0f;
    }
    r = r < rk ? r : 0u;
    roff[q] = E::row_piece(r, D4, ln);
  }

  // every row load of the wave, back to back
  piece v[NL];
  typename E::sb sb[NL];
#pragma unroll
  for (int u = 0; u < NL; ++u) {
    const int j = g + NG * u;                      // (j >> 6) == (NG * u) >> 6: compile time
    const uint32_t ro = (uint32_t)__shfl((int)roff[(NG * u) >> 6], j & 63);
    const elem* W = Wk[0];
    if (BPW > 1) {
      const int k = bag_of(min(j, R - 1));
#pragma unroll
      for (int z = 1; z < BPW; ++z) W = k == z ? Wk[z] : W;
    }
    // NT ("sls_nt" 1): the rows are read once (~1 % reuse inside a batch): non-temporal loads
    if constexpr (NT) {
      v[u] = ld_nt(reinterpret_cast<const piece*>(W) + (uint64_t)ro);
    } else {
      v[u] = reinterpret_cast<const piece*>(W)[(uint64_t)ro];
    }
    sb[u] = E::template load_sb<NT>(reinterpret_cast<const piece*>(W) + (uint64_t)ro, sbd);
  }
  // int8 rowwise: every code and scale / bias load of the wave is issued before the first sum (left to the scheduler,
  // the sums went in between and a vmcnt(0) drain put the last loads a second round trip behind the first)
  if constexpr (E::rowwise) __builtin_amdgcn_sched_barrier(0);

  float4 acc[BPW];
#pragma unroll
  for (int k = 0; k < BPW; ++k) acc[k] = vzero4();
#pragma unroll
  for (int u = 0; u < NL; ++u) {
    const int j = g + NG * u;
    if constexpr (WGT) {   // (one bag per wave; row j >= R is the re-read row R - 1: dropped like the unweighted one)
      static_assert(BPW == 1, "one bag per wave");
      E::addw(acc[0], j < R, __shfl(rwgt[(NG * u) >> 6], j & 63), v[u], sb[u]);
    } else if (BPW == 1) {
      E::add(acc[0], j < R, v[u], sb[u]);
    } else {
      const int kj = bag_of(min(j, R - 1));
#pragma unroll
      for (int k = 0; k < BPW; ++k) E::add(acc[k], j < R && kj == k, v[u], sb[u]);
    }
  }
#pragma unroll
  for (int k = 0; k < BPW; ++k)
#pragma unroll
    for (int m = G; m < 64; m <<= 1) vadd(acc[k], vshfl_xor(acc[k], m));

  if (bad) atomicOr(a.err, 1);
#pragma unroll
  for (int k = 0; k < BPW; ++k) {
    scale_finish<E>(acc[k], a, t0 + k);
    pool_finish(acc[k], a.pool, L);
  }
  // lane group k stores bag k (every group holds every sum after the butterfly)
  if (col_ok && g < BPW) {
    float4 o4 = acc[0];
#pragma unroll
    for (int k = 1; k < BPW; ++k) o4 = g == k ? acc[k] : o4;
    float* o = a.out + (int64_t)vrow * a.ld_out + a.col0 + (int64_t)(t0 + g) * a.D + col;
    *reinterpret_cast<float4*>(o) = o4;
  }
  if (a.ts) {
    __builtin_amdgcn_s_waitcnt(0);   // include the output store in the span
    if (threadIdx.x == 0) a.ts[2 * blockIdx.x + 1] = wall_clock64();
  }
}

}  // namespace
}  // namespace drs
