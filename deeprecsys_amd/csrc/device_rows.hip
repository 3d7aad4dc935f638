// Single table rows updated and read back from DEVICE arrays (include/drs_device_rows.h): drs_update_rows_device and
// drs_get_rows_device, the twins of engine_rows.hip's two calls for ids and values that live in HBM.  What that file does on
// the host -- the range check of every id, last-wins de-duplication, the fp8 fit check -- is a few passes here, all on one
// engine stream (the one the device input pass uses), one launch wherever a pass must see another's writes:
//   1. check_insert_kernel   one thread per id: the range check on the 64-bit value, then (id, position) into an
//                            open-addressing table that keeps each id's LARGEST position (row_dedup.h);
//      fit_scan_kernel       fp8 tables: every value against the table's scale, the host's predicate on the widened value.
//                            Failures land in a device status word (RowStatus): a code and the lowest offending position.
//   2. winner_mask_kernel    position r is written iff the table's entry for ids[r] holds r.
//   3. launch_convert_rows   per chunk (whole rows, at most 16 M elements), the caller's rows -- copied side by side first
//                            where they are strided -- into a packed buffer of the table's type: the kernels drs_set_table
//                            runs (table_convert.hip), so an updated row holds its bytes by construction.  fp32 rows of an
//                            fp32 table ARE the stored bytes and are placed from where they lie.
//   4. place_rows_kernel     move_rows_kernel's shape (table_rows.hip): one wave per row, 64-bit offsets through
//                            i8_row_offset.  It reads the status word first and writes nothing where it is non-zero, and
//                            skips the rows that lost.  Passes 1 and 2 cover the whole call and precede the first place
//                            launch in stream order: a refused call changes nothing.
// The read-back runs pass 1 without the table, waits for the status word on the host (nothing is written to d_V by a call
// that failed), then place_rows_kernel out of the table and write_elems_kernel into the caller's rows.
#include "engine.h"
#include "input_extent.h"
#include "row_dedup.h"
#include "sls_dev.h"

namespace drs {
namespace {

constexpr uint32_t kRowsBadId = 1u, kRowsBadValue = 2u, kRowsInternal = 4u;
// the status word of one call: what failed, the lowest position whose id is out of range, the lowest element (r * D + c)
// whose value does not fit the fp8 table's scale
struct RowStatus {
  uint32_t code, pad_;
  unsigned long long bad_id, bad_value;
};

// row_dedup.h's atomics policy on global memory
struct DedupDeviceAtomics {
  __device__ uint64_t load(const uint64_t* p) const { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
  __device__ uint64_t cas(uint64_t* p, uint64_t expect, uint64_t v) const {
    return (uint64_t)atomicCAS(reinterpret_cast<unsigned long long*>(p), (unsigned long long)expect, (unsigned long long)v);
  }
  __device__ void max(uint64_t* p, uint64_t v) const { (void)atomicMax(reinterpret_cast<unsigned long long*>(p), (unsigned long long)v); }
};

__device__ __forceinline__ float widen(const void* V, int dt, int64_t i) {
  if (dt == DRS_TABLE_FP16) return F16::up1(static_cast<const uint16_t*>(V)[i]);
  if (dt == DRS_TABLE_BF16) return BF16::up1(static_cast<const uint16_t*>(V)[i]);
  return static_cast<const float*>(V)[i];
}

__global__ void status_init_kernel(RowStatus* st) {
  st->code = 0u;
  st->pad_ = 0u;
  st->bad_id = ~0ull;
  st->bad_value = ~0ull;
}

// Pass 1.  No id is dereferenced as a row before this has seen it.  slots == nullptr: the check alone (the read-back).
__global__ __launch_bounds__(256) void check_insert_kernel(const int64_t* ids, int64_t n, int64_t table_rows, uint64_t* slots, uint64_t cap,
                                                           RowStatus* st) {
  for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < n; r += (int64_t)gridDim.x * 256) {
    const int64_t id = ids[r];
    if (id < 0 || id >= table_rows) {
      atomicOr(&st->code, kRowsBadId);
      atomicMin(&st->bad_id, (unsigned long long)r);
    } else if (slots && !dedup_insert(slots, cap, id, r, DedupDeviceAtomics())) {
      atomicOr(&st->code, kRowsInternal);        // (a full table: the capacity rule excludes it; reported, never spun on)
    }
  }
}

// ... and, under fp8, every value: a finite |x| with |x| * 2^k > 448 does not fit (drs_update_rows' predicate)
__global__ __launch_bounds__(256) void fit_scan_kernel(const void* V, int dt, int64_t stride, int64_t n, int D, float mul, RowStatus* st) {
  const int64_t total = n * D;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t r = i / D;
    const float x = fabsf(widen(V, dt, r * stride + (i - r * D)));
    if (__fmul_rn(x, mul) > 448.0f && x < INFINITY) {
      atomicOr(&st->code, kRowsBadValue);
      atomicMin(&st->bad_value, (unsigned long long)i);
    }
  }
}

// Pass 2, behind every insert: mask[r] = position r is its id's last occurrence
__global__ __launch_bounds__(256) void winner_mask_kernel(const int64_t* ids, int64_t n, const uint64_t* slots, uint64_t cap, uint8_t* mask,
                                                          RowStatus* st) {
  if (st->code) return;                            // (an id out of range was never inserted)
  for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < n; r += (int64_t)gridDim.x * 256) {
    const int64_t pos = dedup_lookup(slots, cap, ids[r], DedupDeviceAtomics());
    if (pos < 0) atomicOr(&st->code, kRowsInternal);
    mask[r] = pos == r;
  }
}

// `rows` rows of `units` elements W between two row strides (elements): strided rows side by side, or back
template <class W>
__global__ __launch_bounds__(256) void copy_rows_kernel(const W* src, int64_t src_stride, W* dst, int64_t dst_stride, int64_t rows, int units) {
  const int64_t total = rows * units;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t r = i / units, c = i - r * units;
    dst[r * dst_stride + c] = src[r * src_stride + c];
  }
}

// Pass 4.  One wave per row, four rows per workgroup: row r of `buf` (r * buf_stride bytes in) <-> row ids[r] of the table at
// `table`, whose rows lie where i8_row_offset puts them -- all in 64 bits.  A wave touches the S bytes of its own row and
// nothing else.  mask (into the table only): the rows that are written; the ids of the rows that are are distinct.
template <class W>
__global__ __launch_bounds__(256) void place_rows_kernel(uint8_t* buf, int64_t buf_stride, uint8_t* table, const int64_t* ids, const uint8_t* mask,
                                                         const RowStatus* st, int64_t rows, int S, int32_t n, int to_table) {
  if (st->code) return;
  const int lane = threadIdx.x & 63;
  for (int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < rows; r += (int64_t)gridDim.x * 4) {
    if (mask && !mask[r]) continue;
    uint8_t* packed = buf + r * buf_stride;
    uint8_t* stored = table + i8_row_offset(ids[r], S, n);
    const uint8_t* from = to_table ? packed : stored;
    uint8_t* to = to_table ? stored : packed;
    for (int c = lane * (int)sizeof(W); c < S; c += 64 * (int)sizeof(W)) *reinterpret_cast<W*>(to + c) = *reinterpret_cast<const W*>(from + c);
  }
}

unsigned grid_of(int64_t want) { return (unsigned)(want < 16384 ? (want > 0 ? want : 1) : 16384); }

hipError_t launch_place_rows(void* buf, int64_t buf_stride, void* table, const int64_t* d_ids, const uint8_t* mask, const RowStatus* st, int64_t rows,
                             int64_t S, int32_t lines_n, bool to_table, hipStream_t s) {
  if (rows <= 0) return hipSuccess;
  if (S <= 0 || S > (1 << 20)) return hipErrorInvalidValue;
  const dim3 grid(grid_of((rows + 3) / 4)), block(256);
  uint8_t* b = static_cast<uint8_t*>(buf);
  uint8_t* t = static_cast<uint8_t*>(table);
  const bool words = S % 4 == 0 && buf_stride % 4 == 0 && (reinterpret_cast<uintptr_t>(buf) & 3) == 0;
  if (words) hipLaunchKernelGGL(place_rows_kernel<uint32_t>, grid, block, 0, s, b, buf_stride, t, d_ids, mask, st, rows, (int)S, lines_n, (int)to_table);
  else hipLaunchKernelGGL(place_rows_kernel<uint8_t>, grid, block, 0, s, b, buf_stride, t, d_ids, mask, st, rows, (int)S, lines_n, (int)to_table);
  return hipGetLastError();
}

// strides in ELEMENTS of `elem` bytes (2 or 4)
hipError_t launch_copy_rows_strided(const void* src, int64_t src_stride, void* dst, int64_t dst_stride, int64_t rows, int D, int64_t elem, hipStream_t s) {
  if (rows <= 0) return hipSuccess;
  const dim3 grid(grid_of((rows * D + 255) / 256)), block(256);
  if (elem == 4)
    hipLaunchKernelGGL(copy_rows_kernel<uint32_t>, grid, block, 0, s, static_cast<const uint32_t*>(src), src_stride, static_cast<uint32_t*>(dst), dst_stride, rows, D);
  else
    hipLaunchKernelGGL(copy_rows_kernel<uint16_t>, grid, block, 0, s, static_cast<const uint16_t*>(src), src_stride, static_cast<uint16_t*>(dst), dst_stride, rows, D);
  return hipGetLastError();
}

// the device buffers of one call, allocated inside it and freed when it returns, however it returns (as engine_rows.hip's RowStage): the status word, the
// de-duplication table and the winner mask, the chunk's rows side by side and packed in the table's type
struct DeviceRowStage {
  DeviceBuf<RowStatus> status;
  DeviceBuf<uint64_t> slots;
  DeviceBuf<uint8_t> mask;
  DeviceBuf<void> side, packed;
  Event ev;
};

int64_t chunk_rows(int64_t n, int64_t D) { return std::min<int64_t>(n, std::max<int64_t>(((int64_t)16 << 20) / D, 1)); }
int64_t elem_bytes(int32_t dt) { return dt == DRS_TABLE_FP32 ? 4 : 2; }

// everything the host can refuse, each before anything is enqueued; *done: nothing to do (n == 0)
int32_t check_device_rows(drs_engine* e, const char* what, int32_t t, int64_t n, const int64_t* d_ids, const void* d_V, int64_t stride, int32_t val_dtype,
                          int32_t ordered, bool* done) {
  *done = false;
  if (t < 0 || t >= e->T) return fail(e, DRS_ERR_BAD_ARG, "%s: bad table id %d", what, t);
  if (n < 0) return fail(e, DRS_ERR_BAD_ARG, "%s: n = %lld", what, (long long)n);
  if (!e->table_set[(size_t)t]) return fail(e, DRS_ERR_BAD_ARG, "%s: table %d was never set or filled", what, t);
  if (ordered != 0 && ordered != 1) return fail(e, DRS_ERR_BAD_ARG, "%s: ordered=%d: 0 or 1", what, ordered);
  if (val_dtype != DRS_TABLE_FP32 && val_dtype != DRS_TABLE_FP16 && val_dtype != DRS_TABLE_BF16)
    return fail(e, DRS_ERR_BAD_ARG, "%s: val_dtype=%d: 0 (fp32), 1 (fp16) or 2 (bf16)", what, val_dtype);
  if (n == 0) { *done = true; return DRS_OK; }
  if (!d_ids || !d_V) return fail(e, DRS_ERR_BAD_ARG, "%s: null ids / values", what);
  if (n > DRS_DEVICE_ROWS_MAX) return fail(e, DRS_ERR_BAD_ARG, "%s: n = %lld exceeds %lld rows per call", what, (long long)n, (long long)DRS_DEVICE_ROWS_MAX);
  const int64_t elem = elem_bytes(val_dtype);
  if ((reinterpret_cast<uintptr_t>(d_ids) & 7) || (reinterpret_cast<uintptr_t>(d_V) & (uintptr_t)(elem - 1)))
    return fail(e, DRS_ERR_BAD_ARG, "%s: a pointer is not aligned to its element type", what);
  if (n > 1 && stride < e->D) return fail(e, DRS_ERR_BAD_ARG, "%s: val_row_stride %lld < D = %d: the rows would overlap", what, (long long)stride, e->D);
  uint64_t ids_bytes, val_bytes;
  if (!input_extent_bytes(1, 0, n, sizeof(int64_t), &ids_bytes) || !input_extent_bytes(n, n > 1 ? stride : 0, e->D, elem, &val_bytes))
    return fail(e, DRS_ERR_BAD_ARG, "%s: a row stride beyond any allocation", what);
  const char* why;
  if ((why = device_range_fault(e, d_ids, ids_bytes))) return fail(e, DRS_ERR_BAD_ARG, "%s: d_ids %s", what, why);
  if ((why = device_range_fault(e, d_V, val_bytes))) return fail(e, DRS_ERR_BAD_ARG, "%s: d_V %s", what, why);
  return DRS_OK;
}

// the stream every pass of a call runs on, behind the caller's stream where the call is ordered
int32_t pass_stream(drs_engine* e, DeviceRowStage& st, void* stream, int32_t ordered, hipStream_t* out) {
  int32_t rc;
  if ((rc = copy_stream(e))) return rc;
  if (ordered) {
    // the engine's streams are non-blocking: the edge from the caller's stream (the null stream too) is an event
    HIP_TRY(e, st.ev.create(hipEventDisableTiming));
    HIP_TRY(e, hipEventRecord(st.ev, static_cast<hipStream_t>(stream)));
    HIP_TRY(e, hipStreamWaitEvent(e->stream_h2d, st.ev, 0));
  }
  *out = e->stream_h2d;
  return DRS_OK;
}

// what the passes found, once the stream is idle (DRS_OK: nothing)
int32_t report_status(drs_engine* e, const char* what, const RowStatus& h, int32_t t, const int64_t* d_ids, const void* d_V, int64_t stride,
                      int32_t val_dtype) {
  if (h.code & kRowsBadId) {
    int64_t id = 0;
    (void)hipMemcpy(&id, d_ids + h.bad_id, sizeof id, hipMemcpyDeviceToHost);
    return fail(e, DRS_ERR_INDEX_RANGE, "%s: ids[%lld] = %lld, table %d has %lld rows", what, (long long)h.bad_id, (long long)id, t,
                (long long)e->rows[(size_t)t]);
  }
  if (h.code & kRowsBadValue) {
    const int64_t r = (int64_t)(h.bad_value / (uint64_t)e->D), c = (int64_t)(h.bad_value % (uint64_t)e->D);
    const int64_t elem = elem_bytes(val_dtype);
    uint32_t raw = 0;
    (void)hipMemcpy(&raw, static_cast<const char*>(d_V) + (r * stride + c) * elem, (size_t)elem, hipMemcpyDeviceToHost);
    float v;
    if (val_dtype == DRS_TABLE_FP16) v = (float)__builtin_bit_cast(_Float16, (uint16_t)raw);
    else if (val_dtype == DRS_TABLE_BF16) v = __builtin_bit_cast(float, raw << 16);
    else v = __builtin_bit_cast(float, raw);
    return fail(e, DRS_ERR_BAD_ARG, "%s: |%g| (row %lld, column %lld) exceeds 448 * 2^%d, the range of fp8 table %d under its scale; "
                "drs_set_table on the whole table picks a new scale", what, (double)v, (long long)r, (long long)c, -e->fp8_k[(size_t)t], t);
  }
  if (h.code) return fail(e, DRS_ERR_HIP, "%s: the de-duplication table overflowed (internal error, status %u)", what, h.code);
  return DRS_OK;
}

}  // namespace
}  // namespace drs

extern "C" {

int32_t drs_update_rows_device(drs_handle e, int32_t t, int64_t n, const int64_t* d_ids, const void* d_V, int64_t val_row_stride, int32_t val_dtype,
                               void* stream, int32_t ordered) {
  const char* what = "drs_update_rows_device";
  int32_t rc = check_handle(e);
  if (rc) return rc;
  bool done = false;
  if ((rc = check_device_rows(e, what, t, n, d_ids, d_V, val_row_stride, val_dtype, ordered, &done)) || done) return rc;
  if ((rc = drs_sync(e))) return rc;
  drop_other_placements(e);
  const int dt = e->table_dtype;
  const int64_t D = e->D, S = table_row_stride(dt, D), elem = elem_bytes(val_dtype);
  const int64_t stride = n > 1 ? val_row_stride : D;             // (the stride of a single row is not read)
  const bool tight = stride == D;
  const bool direct = dt == DRS_TABLE_FP32 && val_dtype == DRS_TABLE_FP32;   // the caller's rows are the stored bytes
  const int64_t chunk = chunk_rows(n, D);
  const uint64_t cap = dedup_capacity(n);
  const float mul = dt == DRS_TABLE_FP8_E4M3 ? fp8_pow2(e->fp8_k[(size_t)t]) : 1.0f;   // the table keeps its scale

  DeviceRowStage st;
  hipStream_t s = nullptr;
  HIP_TRY(e, st.status.alloc(1));
  HIP_TRY(e, st.slots.alloc((size_t)cap));
  HIP_TRY(e, st.mask.alloc((size_t)n));
  if (!direct) HIP_TRY(e, st.packed.alloc((size_t)(chunk * S)));
  if (!direct && !tight) HIP_TRY(e, st.side.alloc((size_t)(chunk * D * elem)));
  if ((rc = pass_stream(e, st, stream, ordered, &s))) return rc;

  // passes 1 and 2 over the whole call
  hipLaunchKernelGGL(status_init_kernel, dim3(1), dim3(1), 0, s, st.status);
  HIP_TRY(e, hipGetLastError());
  HIP_TRY(e, hipMemsetAsync(st.slots, 0xff, sizeof(uint64_t) * (size_t)cap, s));      // kDedupEmpty in every slot
  const dim3 per_id(grid_of((n + 255) / 256)), block(256);
  hipLaunchKernelGGL(check_insert_kernel, per_id, block, 0, s, d_ids, n, e->rows[(size_t)t], st.slots, cap, st.status);
  HIP_TRY(e, hipGetLastError());
  if (dt == DRS_TABLE_FP8_E4M3) {
    hipLaunchKernelGGL(fit_scan_kernel, dim3(grid_of((n * D + 255) / 256)), block, 0, s, d_V, (int)val_dtype, stride, n, (int)D, mul, st.status);
    HIP_TRY(e, hipGetLastError());
  }
  hipLaunchKernelGGL(winner_mask_kernel, per_id, block, 0, s, d_ids, n, st.slots, cap, st.mask, st.status);
  HIP_TRY(e, hipGetLastError());

  // passes 3 and 4, chunk by chunk: the stream orders a chunk's convert behind the place launch that read the buffers before
  char* table = table_ptr(e->tables, e->tab_off, t, dt);
  for (int64_t i = 0; i < n; i += chunk) {
    const int64_t c = std::min(chunk, n - i);
    char* src = static_cast<char*>(const_cast<void*>(d_V)) + i * stride * elem;
    if (direct) {
      HIP_TRY(e, launch_place_rows(src, stride * elem, table, d_ids + i, st.mask + i, st.status, c, S, e->i8l.n, true, s));
      continue;
    }
    if (!tight) {
      HIP_TRY(e, launch_copy_rows_strided(src, stride, st.side, D, c, (int)D, elem, s));
      src = static_cast<char*>(st.side.get());
    }
    // the chunk as c rows of a plain-layout table of the arena's type (a row that loses is converted too, and never placed)
    HIP_TRY(e, launch_convert_rows(TableSide{src, val_dtype}, TableSide{st.packed, dt, 0, mul}, RowWindow{0, c, c}, (int)D, s));
    HIP_TRY(e, launch_place_rows(st.packed, S, table, d_ids + i, st.mask + i, st.status, c, S, e->i8l.n, true, s));
  }
  HIP_TRY(e, hipStreamSynchronize(s));
  RowStatus h;
  HIP_TRY(e, hipMemcpy(&h, st.status, sizeof h, hipMemcpyDeviceToHost));
  return report_status(e, what, h, t, d_ids, d_V, stride, val_dtype);
}

int32_t drs_get_rows_device(drs_handle e, int32_t t, int64_t n, const int64_t* d_ids, float* d_V, int64_t val_row_stride, void* stream, int32_t ordered) {
  const char* what = "drs_get_rows_device";
  int32_t rc = check_handle(e);
  if (rc) return rc;
  bool done = false;
  if ((rc = check_device_rows(e, what, t, n, d_ids, d_V, val_row_stride, DRS_TABLE_FP32, ordered, &done)) || done) return rc;
  if ((rc = drs_sync(e))) return rc;
  const int dt = e->table_dtype;
  const int64_t D = e->D, S = table_row_stride(dt, D);
  const int64_t stride = n > 1 ? val_row_stride : D;
  const bool tight = stride == D;
  const bool direct = dt == DRS_TABLE_FP32;
  const int64_t chunk = chunk_rows(n, D);
  const float scale = dt == DRS_TABLE_FP8_E4M3 ? fp8_pow2(-e->fp8_k[(size_t)t]) : 1.0f;

  DeviceRowStage st;
  hipStream_t s = nullptr;
  HIP_TRY(e, st.status.alloc(1));
  if (!direct) HIP_TRY(e, st.packed.alloc((size_t)(chunk * S)));
  if (!direct && !tight) HIP_TRY(e, st.side.alloc(sizeof(float) * (size_t)(chunk * D)));
  if ((rc = pass_stream(e, st, stream, ordered, &s))) return rc;

  // pass 1, the check alone; its verdict on the host before anything touches d_V
  hipLaunchKernelGGL(status_init_kernel, dim3(1), dim3(1), 0, s, st.status);
  HIP_TRY(e, hipGetLastError());
  hipLaunchKernelGGL(check_insert_kernel, dim3(grid_of((n + 255) / 256)), dim3(256), 0, s, d_ids, n, e->rows[(size_t)t], (uint64_t*)nullptr, (uint64_t)0,
                     st.status);
  HIP_TRY(e, hipGetLastError());
  HIP_TRY(e, hipStreamSynchronize(s));
  RowStatus h;
  HIP_TRY(e, hipMemcpy(&h, st.status, sizeof h, hipMemcpyDeviceToHost));
  if ((rc = report_status(e, what, h, t, d_ids, d_V, stride, DRS_TABLE_FP32))) return rc;

  char* table = table_ptr(e->tables, e->tab_off, t, dt);
  for (int64_t i = 0; i < n; i += chunk) {
    const int64_t c = std::min(chunk, n - i);
    float* dst = d_V + i * stride;
    if (direct) {
      HIP_TRY(e, launch_place_rows(dst, stride * (int64_t)sizeof(float), table, d_ids + i, nullptr, st.status, c, S, e->i8l.n, false, s));
      continue;
    }
    // the named rows' stored bytes side by side, then every row's served value (write_elems_kernel)
    HIP_TRY(e, launch_place_rows(st.packed, S, table, d_ids + i, nullptr, st.status, c, S, e->i8l.n, false, s));
    HIP_TRY(e, launch_convert_rows(TableSide{st.packed, dt, 0, scale}, TableSide{tight ? (void*)dst : st.side, DRS_TABLE_FP32}, RowWindow{0, c, c}, (int)D, s));
    if (!tight) HIP_TRY(e, launch_copy_rows_strided(st.side, D, dst, stride, c, (int)D, sizeof(float), s));
  }
  HIP_TRY(e, hipStreamSynchronize(s));
  return DRS_OK;
}

}  // extern "C"
