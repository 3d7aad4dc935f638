// Writing embedding tables: the device fill and every "table_dtype" / "table_int8_lines" / "table_int4_lines" conversion.
//
// Nothing here serves a query.  A pass has a SOURCE, a reader functor `float operator()(int64_t r, int D, int c)` giving
// column c of the pass's row r as fp32 (SrcElems: fp32 / fp16 / bf16 elements, SrcFill: the uniform fill's values, SrcI8 /
// SrcI4: each rowwise row's value, SrcF8: each fp8 code's value), and a DESTINATION, one kernel template per stored form,
// generic over the reader: write_elems_kernel (fp32 / fp16 / bf16 elements), quantize_rows_kernel (int8 rowwise),
// pack4_rows_kernel (int4 rowwise), to_fp8_rows_kernel (fp8 e4m3 codes), absmax_rows_kernel (the reduction that picks an
// fp8 table's scale).  relayout_rows_kernel moves rowwise rows between the plain and the line-packed layout, bytes as
// they are.  The fill of an fp32 / fp16 / bf16 table and the whole-arena pass between those types have no row structure
// and stay flat-indexed (fill_uniform_kernel, convert_table_kernel: measured, the fill is a fifth slower row by row).  The
// launches at the end pick reader and destination from the two sides' types (TableSide, drs_internal.h); a new table type
// adds one reader and, where it is a new stored form, one destination kernel.
#include "drs_internal.h"
#include "sls_dev.h"

namespace drs {

// ---------------------------------------------------------------------------
// device-side table fill, bit-identical to oracle/drs_oracle.c fill_value()
__device__ __forceinline__ float fill_value(int64_t i, int32_t t, float lo, float span, uint64_t seed) {
  uint64_t z = seed + 0x9E3779B97F4A7C15ull * ((uint64_t)i + ((uint64_t)(uint32_t)t << 40) + 1ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  const float u = (float)(uint32_t)(z >> 40) * (1.0f / 16777216.0f);
  return __fmaf_rn(u, span, lo);
}

// "table_dtype": an fp32 value as it is stored in a table of element type dt (fp16 / bf16: the hardware's
// round-to-nearest-even conversions, v_cvt_f16_f32 / v_cvt_pk_bf16_f32 -- NaN stays NaN, overflow gives +-inf, fp16
// subnormals are kept), and back (exact)
__device__ __forceinline__ void store_elem(void* W, int dt, int64_t i, float x) {
  if (dt == DRS_TABLE_FP16) static_cast<_Float16*>(W)[i] = (_Float16)x;
  else if (dt == DRS_TABLE_BF16) static_cast<__bf16*>(W)[i] = (__bf16)x;
  else static_cast<float*>(W)[i] = x;
}
__device__ __forceinline__ float load_elem(const void* W, int dt, int64_t i) {
  if (dt == DRS_TABLE_FP16) return F16::up1(static_cast<const uint16_t*>(W)[i]);
  if (dt == DRS_TABLE_BF16) return BF16::up1(static_cast<const uint16_t*>(W)[i]);
  return static_cast<const float*>(W)[i];
}

// The two passes without a row structure, flat-indexed: a reader would add a 64-bit r * D + c (or a division) per element
// to passes over gigabytes.  The fill's values of table t, rounded to the table's element type dt (fp32 / fp16 / bf16) ...
__global__ void fill_uniform_kernel(void* W, int dt, int64_t n, int32_t t, float lo, float hi, uint64_t seed) {
  const float span = hi - lo;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    store_elem(W, dt, i, fill_value(i, t, lo, span, seed));
}
// ... and n elements of type sdt -> type ddt (the arena conversion of "table_dtype" between fp32 / fp16 / bf16: one pass over the
// whole arena, the gaps between its tables included)
__global__ void convert_table_kernel(const void* src, int sdt, void* dst, int ddt, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    store_elem(dst, ddt, i, load_elem(src, sdt, i));
}

// ---------------------------------------------------------------------------
// the readers
struct SrcElems {      // row r of a table of element type dt at src (D elements per row)
  const void* src;
  int dt;
  __device__ __forceinline__ float operator()(int64_t r, int D, int c) const { return load_elem(src, dt, r * D + c); }
};
struct SrcFill {       // fill_uniform_kernel's values of table t
  int32_t t;
  float lo, span;
  uint64_t seed;
  __device__ __forceinline__ float operator()(int64_t r, int D, int c) const { return fill_value(r * D + c, t, lo, span, seed); }
};
// Where the rowwise rows of a launch go, or come from: `base` is the TABLE's first byte, the launch's row r is the table's row
// first + r (drs_set_table stages a table in chunks) of `total`, n = I8Lines::n of the layout (0: plain); S: the row stride.
struct I8Rows {
  uint8_t* base;
  int64_t first, total;
  int32_t n;
  __device__ __forceinline__ uint8_t* row(int64_t r, int64_t S) const { return base + i8_row_offset(first + r, S, n); }
  // line-packed layout: the bytes of its line behind row r that belong to no row -- the line's last 128 - n S bytes after
  // its last slot, and the unused slots too after the table's last row
  __device__ __forceinline__ int tail(int64_t r, int64_t S) const {
    if (!n) return 0;
    const int slot = (int)((first + r) % n);
    return slot == n - 1 || first + r == total - 1 ? 128 - (slot + 1) * (int)S : 0;
  }
};
struct SrcI8 {         // each int8 rowwise row's value, fmaf(scale, q, 0.0f + bias)
  I8Rows rows;
  __device__ __forceinline__ float operator()(int64_t r, int D, int c) const {
    const uint8_t* row = rows.row(r, I8::padded(D) + 8);
    const float2 sb = I8::row_sb(row, D);
    return I8::row1(sb.x, sb.y, I8::code(row, c), 0.0f);
  }
};
// int4 rowwise rows (layout: struct I4), as I8Rows with the stride of a row of D columns ("table_int4_lines")
struct I4Rows {
  uint8_t* base;
  int64_t first, total;
  int32_t n;
  __device__ __forceinline__ uint8_t* row(int64_t r, int D) const { return base + i8_row_offset(first + r, I4::padded(D) + 4, n); }
  // the bytes of its line behind row r that belong to no row (I8Rows::tail; a multiple of 4 here)
  __device__ __forceinline__ int tail(int64_t r, int D) const { return I8Rows{base, first, total, n}.tail(r, I4::padded(D) + 4); }
};
struct SrcI4 {         // each int4 rowwise row's value
  I4Rows rows;
  __device__ __forceinline__ float operator()(int64_t r, int D, int c) const {
    const uint8_t* row = rows.row(r, D);
    const float2 sb = I4::row_sb(row, D);
    return I4::row1(sb.x, sb.y, I4::code(row, c), 0.0f);
  }
};
struct SrcF8 {         // each fp8 code's value, decode(code) * 2^-k of its table
  const uint8_t* codes;
  float scale;
  __device__ __forceinline__ float operator()(int64_t r, int D, int c) const { return __fmul_rn(F8::up1(codes[r * D + c]), scale); }
};
// the readers whose values are the fp32 the caller gave: what an fp8 table is encoded from (the engine refuses 8 -> 4 and
// 9 -> 4: quantizing quantized rows a second time is not offered in one step)
template <class Src> constexpr bool kFp8Source = std::is_same_v<Src, SrcElems> || std::is_same_v<Src, SrcFill>;

// ---------------------------------------------------------------------------
// the destinations.  The row kernels run one wave per row, four rows per workgroup (row_grid), any D.
//
// Elements of type dt: dst[r * D + c] = the source's value, rounded to dt (out of a rowwise type: the one-row bag's
// value fmaf(scale, q, 0.0f + bias))
template <class Src>
__global__ __launch_bounds__(256) void write_elems_kernel(Src src, void* dst, int dt, int64_t rows, int D) {
  const int lane = threadIdx.x & 63;
  for (int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < rows; r += (int64_t)gridDim.x * 4)
    for (int c = lane; c < D; c += 64) store_elem(dst, dt, r * D + c, src(r, D, c));
}

// "table_dtype" 8, 8-bit rowwise tables (layout: struct I8).  Quantizing a row, FBGEMM's embedding_bag_byte_prepack in
// IEEE fp32 without contraction: mn = min, mx = max, range = mx - mn, scale = range / 255, bias = mn,
// inv = 255 / (range + 1e-8), q = rint((x - mn) * inv).  The row is read twice (the second time from the cache).  Rows
// holding inf or NaN are outside the contract: the clamp keeps every code a byte.  A finite row with mx - mn = inf
// (+3e38 beside -3e38) is inside it: scale = inf, inv = 0 and every code 0 (fminf(fmaxf(NaN, 0), 255) is 0 for the element
// whose x - mn is inf) -- embedding_bag_byte_prepack's bytes; the row decodes to inf * 0 = NaN and the gather keeps that
// NaN to the bags that name it (I8::addw).
template <class Src>
__global__ __launch_bounds__(256) void quantize_rows_kernel(Src src, I8Rows dst, int64_t rows, int D) {
  const int lane = threadIdx.x & 63;
  const int D8 = I8::padded(D);
  const int64_t S = D8 + 8;
  for (int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < rows; r += (int64_t)gridDim.x * 4) {
    float mn = INFINITY, mx = -INFINITY;
    for (int c = lane; c < D; c += 64) {
      const float x = src(r, D, c);
      mn = fminf(mn, x);
      mx = fmaxf(mx, x);
    }
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
      mn = fminf(mn, __shfl_xor(mn, m));
      mx = fmaxf(mx, __shfl_xor(mx, m));
    }
    const float range = __fsub_rn(mx, mn);
    const float inv = __fdiv_rn(255.0f, __fadd_rn(range, 1e-8f));
    uint8_t* row = dst.row(r, S);
    for (int c = lane; c < D8; c += 64) {
      const float q = c < D ? rintf(__fmul_rn(__fsub_rn(src(r, D, c), mn), inv)) : 0.f;
      row[c] = (uint8_t)fminf(fmaxf(q, 0.f), 255.f);
    }
    if (lane == 0) *reinterpret_cast<float2*>(row + D8) = make_float2(__fdiv_rn(range, 255.0f), mn);
    for (int c = lane * 8, z = dst.tail(r, S); c < z; c += 64 * 8) *reinterpret_cast<uint2*>(row + S + c) = make_uint2(0u, 0u);
  }
}

// "table_dtype" 9, 4-bit rowwise tables (layout: struct I4).  Quantizing a row, torch's embedding_bag_4bit_prepack in IEEE
// fp32 without contraction: bias = fp16(min), scale = fp16((max - (float)bias) / 15), a zero scale becomes 1,
// inv = 1 / (float)scale (infinite: scale = inv = 1), q = clamp(rint((x - (float)bias) * inv), 0, 15).  Any even D; the
// row is read twice (the second time from the cache).  Rows holding inf or NaN, or values beyond fp16's range, are
// outside the contract: the clamp keeps every code a nibble.  A finite row with (max - bias) / 15 >= 65520 -- one element
// of 1e6 -- takes the scale +inf, inv = 0 and every code 0, embedding_bag_4bit_prepack's bytes: it decodes to
// inf * 0 = NaN in every column, and the gather keeps that NaN to the bags that name it (I4::addw).
template <class Src>
__global__ __launch_bounds__(256) void pack4_rows_kernel(Src src, I4Rows dst, int64_t rows, int D) {
  const int lane = threadIdx.x & 63;
  const int P = I4::padded(D);
  for (int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < rows; r += (int64_t)gridDim.x * 4) {
    float mn = INFINITY, mx = -INFINITY;
    for (int c = lane; c < D; c += 64) {
      const float x = src(r, D, c);
      mn = fminf(mn, x);
      mx = fmaxf(mx, x);
    }
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
      mn = fminf(mn, __shfl_xor(mn, m));
      mx = fmaxf(mx, __shfl_xor(mx, m));
    }
    const _Float16 bias_h = (_Float16)mn;
    const float bias = (float)bias_h;
    _Float16 scale_h = (_Float16)__fdiv_rn(__fsub_rn(mx, bias), 15.0f);
    if (scale_h == (_Float16)0.0f) scale_h = (_Float16)1.0f;
    float inv = __fdiv_rn(1.0f, (float)scale_h);
    if (isinf(inv)) { scale_h = (_Float16)1.0f; inv = 1.0f; }
    uint8_t* row = dst.row(r, D);
    for (int j = lane; j < P; j += 64) {          // byte j: columns 2 j (low nibble) and 2 j + 1
      uint32_t b = 0;
      if (2 * j < D) {
        const float q0 = rintf(__fmul_rn(__fsub_rn(src(r, D, 2 * j), bias), inv));
        const float q1 = rintf(__fmul_rn(__fsub_rn(src(r, D, 2 * j + 1), bias), inv));
        b = (uint32_t)fminf(fmaxf(q0, 0.f), 15.f) | ((uint32_t)fminf(fmaxf(q1, 0.f), 15.f) << 4);
      }
      row[j] = (uint8_t)b;
    }
    if (lane == 0)
      *reinterpret_cast<uint32_t*>(row + P) = (uint32_t)__builtin_bit_cast(uint16_t, scale_h) | ((uint32_t)__builtin_bit_cast(uint16_t, bias_h) << 16);
    for (int c = lane * 4, z = dst.tail(r, D); c < z; c += 64 * 4) *reinterpret_cast<uint32_t*>(row + P + 4 + c) = 0u;
  }
}

// Rowwise rows of stride S (a multiple of 4) from one layout to the other ("table_int8_lines" / "table_int4_lines" set on
// an arena of that type): the rows' bytes as they are, the rest of a line cleared
__global__ __launch_bounds__(256) void relayout_rows_kernel(I8Rows src, I8Rows dst, int64_t rows, int S) {
  const int lane = threadIdx.x & 63;
  for (int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < rows; r += (int64_t)gridDim.x * 4) {
    const uint8_t* from = src.row(r, S);
    uint8_t* to = dst.row(r, S);
    for (int c = lane * 4; c < S; c += 64 * 4) *reinterpret_cast<uint32_t*>(to + c) = *reinterpret_cast<const uint32_t*>(from + c);
    for (int c = lane * 4, z = dst.tail(r, S); c < z; c += 64 * 4) *reinterpret_cast<uint32_t*>(to + S + c) = 0u;
  }
}

// "table_dtype" 4, fp8 e4m3 tables (layout: struct F8).  e4m3_rne: an fp32 value as its OCP e4m3 code, torch's
// float8_e4m3fn conversion in integer arithmetic, bit for bit: round to nearest even, the subnormal codes (multiples of
// 2^-9 below 2^-6) through the add of 2^14 whose ulp they are, 0x7F (NaN) with the sign bit for NaN, +-inf and everything
// that rounds beyond 448 -- which no finite element does after the table's scale.
__device__ __forceinline__ uint8_t e4m3_rne(float x) {
  uint32_t b = __float_as_uint(x);
  const uint32_t sign = b & 0x80000000u;
  b ^= sign;
  uint32_t q;
  if (b >= 0x43F00000u) {                           // >= 480, +-inf, NaN
    q = 0x7Fu;
  } else if (b < (121u << 23)) {                    // below 2^-6
    q = __float_as_uint(__fadd_rn(__uint_as_float(b), __uint_as_float(141u << 23))) - (141u << 23);
  } else {
    const uint32_t odd = (b >> 20) & 1u;
    b += ((uint32_t)(7 - 127) << 23) + 0x7FFFFu + odd;
    q = b >> 20;
  }
  return (uint8_t)(q | (sign >> 24));
}
// the largest |x| over the source's finite values, as its bits: one atomicMax per wave into *out (zeroed by the caller)
template <class Src>
__global__ __launch_bounds__(256) void absmax_rows_kernel(Src src, int64_t rows, int D, uint32_t* out) {
  const int64_t n = rows * D;
  uint32_t m = 0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / D;
    const uint32_t b = __float_as_uint(src(r, D, (int)(i - r * D))) & 0x7fffffffu;
    m = b < 0x7f800000u && b > m ? b : m;
  }
#pragma unroll
  for (int k = 1; k < 64; k <<= 1) {
    const uint32_t o = (uint32_t)__shfl_xor((int)m, k);
    m = o > m ? o : m;
  }
  if ((threadIdx.x & 63) == 0 && m) atomicMax(out, m);
}
// rows x D source values -> codes: dst[r * D + c] = e4m3_rne(x * mul), mul = 2^k
template <class Src>
__global__ __launch_bounds__(256) void to_fp8_rows_kernel(Src src, uint8_t* dst, int64_t rows, int D, float mul) {
  const int64_t n = rows * D;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / D;
    dst[i] = e4m3_rne(__fmul_rn(src(r, D, (int)(i - r * D)), mul));
  }
}

// ---------------------------------------------------------------------------
// the launches: workgroups of 256 threads, at most 16384 of them (every kernel above strides over the rest)
static unsigned grid_of(int64_t want) { return (unsigned)(want < 16384 ? want : 16384); }
static unsigned row_grid(int64_t rows) { return grid_of((rows + 3) / 4); }
static unsigned elem_grid(int64_t n) { return grid_of((n + 255) / 256); }
static bool plain_dtype(int dtype) { return dtype == DRS_TABLE_FP32 || dtype == DRS_TABLE_FP16 || dtype == DRS_TABLE_BF16; }

// the window's rows out of reader `src`, stored as dst asks
template <class Src>
static hipError_t write_rows(Src src, const TableSide& dst, const RowWindow& w, int D, hipStream_t s) {
  const dim3 grid(row_grid(w.rows)), block(256);
  uint8_t* to = static_cast<uint8_t*>(dst.base);
  if (dst.dtype == DRS_TABLE_INT8_ROWWISE) {
    if constexpr (std::is_same_v<Src, SrcI8>) return hipErrorInvalidValue;   // (the same type: launch_convert_rows moves the bytes)
    else hipLaunchKernelGGL(quantize_rows_kernel<Src>, grid, block, 0, s, src, I8Rows{to, w.first, w.total, dst.lines_n}, w.rows, D);
  } else if (dst.dtype == DRS_TABLE_INT4_ROWWISE) {
    // (odd D -- internal guard: the engine refuses table_dtype 9 on odd D before any launch)
    if constexpr (std::is_same_v<Src, SrcI4>) return hipErrorInvalidValue;
    else if (D & 1) return hipErrorInvalidValue;
    else hipLaunchKernelGGL(pack4_rows_kernel<Src>, grid, block, 0, s, src, I4Rows{to, w.first, w.total, dst.lines_n}, w.rows, D);
  } else if (dst.dtype == DRS_TABLE_FP8_E4M3) {
    if constexpr (!kFp8Source<Src>) return hipErrorInvalidValue;
    else hipLaunchKernelGGL(to_fp8_rows_kernel<Src>, dim3(elem_grid(w.rows * D)), block, 0, s, src, to, w.rows, D, dst.scale);
  } else if (plain_dtype(dst.dtype)) {
    if constexpr (std::is_same_v<Src, SrcFill>) return hipErrorInvalidValue;   // (launch_fill_rows: the flat kernel)
    else hipLaunchKernelGGL(write_elems_kernel<Src>, grid, block, 0, s, src, dst.base, dst.dtype, w.rows, D);
  } else {
    return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t launch_convert_rows(const TableSide& src, const TableSide& dst, const RowWindow& w, int D, hipStream_t s) {
  if (w.rows <= 0) return hipSuccess;
  uint8_t* from = static_cast<uint8_t*>(src.base);
  const I8Rows rows{from, w.first, w.total, src.lines_n};
  if (table_rowwise(src.dtype) && src.dtype == dst.dtype) {   // the rows' bytes, into the other layout
    if (src.dtype == DRS_TABLE_INT4_ROWWISE && (D & 1)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(relayout_rows_kernel, dim3(row_grid(w.rows)), dim3(256), 0, s, rows,
                       I8Rows{static_cast<uint8_t*>(dst.base), w.first, w.total, dst.lines_n}, w.rows, (int)table_row_stride(src.dtype, D));
    return hipGetLastError();
  }
  switch (src.dtype) {
    case DRS_TABLE_INT8_ROWWISE: return write_rows(SrcI8{rows}, dst, w, D, s);
    case DRS_TABLE_INT4_ROWWISE:   // (odd D: unreachable through the engine, convert_tables refuses it)
      return D & 1 ? hipErrorInvalidValue : write_rows(SrcI4{I4Rows{from, w.first, w.total, src.lines_n}}, dst, w, D, s);
    case DRS_TABLE_FP8_E4M3:       // (whole tables only: the reader counts from the codes' first row)
      return w.first != 0 ? hipErrorInvalidValue : write_rows(SrcF8{from, src.scale}, dst, w, D, s);
    default:
      return plain_dtype(src.dtype) ? write_rows(SrcElems{src.base, src.dtype}, dst, w, D, s) : hipErrorInvalidValue;
  }
}

hipError_t launch_fill_rows(const TableSide& dst, int64_t rows, int D, int32_t t, float lo, float hi, uint64_t seed, hipStream_t s) {
  const int64_t n = rows * D;
  if (n <= 0) return hipSuccess;
  if (!plain_dtype(dst.dtype)) return write_rows(SrcFill{t, lo, hi - lo, seed}, dst, RowWindow{0, rows, rows}, D, s);
  hipLaunchKernelGGL(fill_uniform_kernel, dim3(elem_grid(n)), dim3(256), 0, s, dst.base, dst.dtype, n, t, lo, hi, seed);
  return hipGetLastError();
}

hipError_t launch_absmax_rows(const TableSide& src, int64_t rows, int D, uint32_t* d_bits, hipStream_t s) {
  if (rows <= 0) return hipSuccess;
  if (!plain_dtype(src.dtype)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(absmax_rows_kernel<SrcElems>, dim3(elem_grid(rows * D)), dim3(256), 0, s, SrcElems{src.base, src.dtype}, rows, D, d_bits);
  return hipGetLastError();
}

hipError_t launch_convert_table(const void* src, int src_dtype, void* dst, int dst_dtype, int64_t n, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(convert_table_kernel, dim3(elem_grid(n)), dim3(256), 0, s, src, src_dtype, dst, dst_dtype, n);
  return hipGetLastError();
}

}  // namespace drs
