// libdrs_hip.so, host side: single rows of a loaded table, written and read back in the arena's stored type
// (include/drs_rows.h).  Rows and ids cross the bus in chunks through staging buffers, as drs_set_table's do: whole rows,
// at most 16 M elements per chunk.  The bytes of an updated row are made by the kernels drs_set_table runs
// (launch_convert_rows into a packed buffer of the table's type); launch_move_rows places them (table_rows.hip).
#include "engine.h"

namespace {

// the refusals both calls share, each before anything is touched; *done: nothing to do (n == 0)
int32_t check_rows(drs_engine* e, const char* what, int32_t t, int64_t n, const int64_t* h_ids, const void* h_V, bool* done) {
  *done = false;
  if (t < 0 || t >= e->T) return fail(e, DRS_ERR_BAD_ARG, "%s: bad table id %d", what, t);
  if (n < 0) return fail(e, DRS_ERR_BAD_ARG, "%s: n = %lld", what, (long long)n);
  if (!e->table_set[(size_t)t]) return fail(e, DRS_ERR_BAD_ARG, "%s: table %d was never set or filled", what, t);
  if (n == 0) { *done = true; return DRS_OK; }
  if (!h_ids || !h_V) return fail(e, DRS_ERR_BAD_ARG, "%s: null ids / values", what);
  for (int64_t i = 0; i < n; ++i)
    if (h_ids[i] < 0 || h_ids[i] >= e->rows[(size_t)t])
      return fail(e, DRS_ERR_INDEX_RANGE, "%s: ids[%lld] = %lld, table %d has %lld rows", what, (long long)i, (long long)h_ids[i], t,
                  (long long)e->rows[(size_t)t]);
  return DRS_OK;
}

// the device buffers of one call: fp32 rows, their ids, and the same rows packed in the table's type (null under fp32:
// the fp32 rows are the stored bytes)
struct RowStage {
  DeviceBuf<float> f32;
  DeviceBuf<int64_t> ids;
  DeviceBuf<void> packed;
  hipError_t alloc(int64_t chunk, int64_t D, int dt) {
    hipError_t r = f32.alloc((size_t)(chunk * D));
    if (r == hipSuccess) r = ids.alloc((size_t)chunk);
    if (r == hipSuccess && dt != DRS_TABLE_FP32) r = packed.alloc((size_t)(chunk * table_row_stride(dt, D)));
    return r;
  }
};

int64_t chunk_rows(int64_t n, int64_t D) { return std::min<int64_t>(n, std::max<int64_t>(((int64_t)16 << 20) / D, 1)); }

}  // namespace

extern "C" {

int32_t drs_update_rows(drs_handle e, int32_t t, int64_t n, const int64_t* h_ids, const float* h_V) {
  int32_t rc = check_handle(e);
  if (rc) return rc;
  bool done = false;
  if ((rc = check_rows(e, "drs_update_rows", t, n, h_ids, h_V, &done)) || done) return rc;
  const int dt = e->table_dtype;
  const int64_t D = e->D, S = table_row_stride(dt, D);
  float mul = 1.0f;
  if (dt == DRS_TABLE_FP8_E4M3) {
    // the table keeps its scale: every finite element must fit e4m3 under it (|x| 2^k <= 448; the product is exact)
    mul = fp8_pow2(e->fp8_k[(size_t)t]);
    for (int64_t i = 0; i < n * D; ++i) {
      const float v = fabsf(h_V[i]) * mul;
      if (v > 448.0f && fabsf(h_V[i]) < INFINITY)
        return fail(e, DRS_ERR_BAD_ARG, "drs_update_rows: |%g| (row %lld) exceeds 448 * 2^%d, the range of fp8 table %d under its scale; "
                    "drs_set_table on the whole table picks a new scale", (double)h_V[i], (long long)(i / D), -e->fp8_k[(size_t)t], t);
    }
  }
  // duplicate ids: the last occurrence wins, settled here so that no two waves write one row -- `keep` names the
  // occurrences that are written, in the caller's order (empty: every id is distinct and all are written; strictly rising
  // ids are known to be without a sort)
  std::vector<int64_t> keep;
  bool rising = true;
  for (int64_t i = 1; i < n && rising; ++i) rising = h_ids[i - 1] < h_ids[i];
  if (!rising) {
    std::vector<std::pair<int64_t, int64_t>> by_id((size_t)n);
    for (int64_t i = 0; i < n; ++i) by_id[(size_t)i] = {h_ids[i], i};
    std::sort(by_id.begin(), by_id.end());
    for (size_t i = 0; i < by_id.size(); ++i)
      if (i + 1 == by_id.size() || by_id[i + 1].first != by_id[i].first) keep.push_back(by_id[i].second);
    if ((int64_t)keep.size() == n) keep.clear();
    else std::sort(keep.begin(), keep.end());
  }
  const bool dups = !keep.empty();

  if ((rc = drs_sync(e))) return rc;
  drop_other_placements(e);
  const int64_t rows = dups ? (int64_t)keep.size() : n, chunk = chunk_rows(rows, D);
  RowStage st;
  HIP_TRY(e, st.alloc(chunk, D, dt));
  std::vector<float> h_rows;       // with duplicates: the kept rows of a chunk, side by side
  std::vector<int64_t> h_kept;
  if (dups) { h_rows.resize((size_t)(chunk * D)); h_kept.resize((size_t)chunk); }
  char* table = table_ptr(e->tables, e->tab_off, t, dt);
  hipError_t r = hipSuccess;
  for (int64_t i = 0; i < rows && r == hipSuccess; i += chunk) {
    const int64_t c = std::min(chunk, rows - i);
    const float* src = h_V + i * D;
    const int64_t* ids = h_ids + i;
    if (dups) {
      for (int64_t j = 0; j < c; ++j) {
        const int64_t from = keep[(size_t)(i + j)];
        memcpy(h_rows.data() + j * D, h_V + from * D, sizeof(float) * (size_t)D);
        h_kept[(size_t)j] = h_ids[from];
      }
      src = h_rows.data();
      ids = h_kept.data();
    }
    r = hipMemcpy(st.f32, src, sizeof(float) * (size_t)(c * D), hipMemcpyHostToDevice);
    if (r == hipSuccess) r = hipMemcpy(st.ids, ids, sizeof(int64_t) * (size_t)c, hipMemcpyHostToDevice);
    // the chunk as c rows of a plain-layout table of the arena's type, then each row to its place
    if (r == hipSuccess && st.packed)
      r = launch_convert_rows(TableSide{st.f32, DRS_TABLE_FP32}, TableSide{st.packed, dt, 0, mul}, RowWindow{0, c, c}, (int)D, nullptr);
    if (r == hipSuccess) r = launch_move_rows(st.packed ? st.packed : st.f32, table, st.ids, c, S, e->i8l.n, true, nullptr);
    if (r == hipSuccess) r = hipStreamSynchronize(nullptr);    // (before the next chunk overwrites the staging buffers)
  }
  if (r != hipSuccess) return fail(e, DRS_ERR_HIP, "drs_update_rows: %s", hipGetErrorString(r));
  return DRS_OK;
}

int32_t drs_get_rows(drs_handle e, int32_t t, int64_t n, const int64_t* h_ids, float* h_V) {
  int32_t rc = check_handle(e);
  if (rc) return rc;
  bool done = false;
  if ((rc = check_rows(e, "drs_get_rows", t, n, h_ids, h_V, &done)) || done) return rc;
  if ((rc = drs_sync(e))) return rc;
  const int dt = e->table_dtype;
  const int64_t D = e->D, S = table_row_stride(dt, D), chunk = chunk_rows(n, D);
  RowStage st;
  HIP_TRY(e, st.alloc(chunk, D, dt));
  char* table = table_ptr(e->tables, e->tab_off, t, dt);
  const float scale = dt == DRS_TABLE_FP8_E4M3 ? fp8_pow2(-e->fp8_k[(size_t)t]) : 1.0f;
  hipError_t r = hipSuccess;
  for (int64_t i = 0; i < n && r == hipSuccess; i += chunk) {
    const int64_t c = std::min(chunk, n - i);
    r = hipMemcpy(st.ids, h_ids + i, sizeof(int64_t) * (size_t)c, hipMemcpyHostToDevice);
    // the named rows' stored bytes side by side, then every row's served value (write_elems_kernel)
    if (r == hipSuccess) r = launch_move_rows(st.packed ? st.packed : st.f32, table, st.ids, c, S, e->i8l.n, false, nullptr);
    if (r == hipSuccess && st.packed)
      r = launch_convert_rows(TableSide{st.packed, dt, 0, scale}, TableSide{st.f32, DRS_TABLE_FP32}, RowWindow{0, c, c}, (int)D, nullptr);
    if (r == hipSuccess) r = hipMemcpy(h_V + i * D, st.f32, sizeof(float) * (size_t)(c * D), hipMemcpyDeviceToHost);
  }
  if (r != hipSuccess) return fail(e, DRS_ERR_HIP, "drs_get_rows: %s", hipGetErrorString(r));
  return DRS_OK;
}

}  // extern "C"
