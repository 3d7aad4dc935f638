// libdrs_hip.so, host side: launch sets that hand back each query's top-k rows (include/drs_device_topk.h).  A device-input
// set (engine_device_inputs.hip: the same checks, the same input pass, the same launches, per-sample weights if it carries
// any) with what the device-output form adds (engine_device_outputs.hip) in another shape: one launch of the top-k pass
// (topk_pass.hip) behind the set's last kernel ranks every query by one score column of Slot::d_out and writes its winners'
// row numbers and score rows to the caller's device arrays, and -- ordered == 1 -- two event edges tie the set to the
// caller's stream.  drs_wait stays the slot's completion; wait_slot waits for the pass's event.  drs_topk_rows is the same
// pass at operator level, on an array of the caller's.
#include "engine.h"
#include "topk_plan.h"

namespace drs {
namespace eng {

// one output array of the set: where it is, how long, whose it is
struct TopKExtent {
  uintptr_t p;
  uint64_t bytes;
  int query;
  const char* name;
};

static int32_t check_topk_output(drs_engine* e, int i, const char* name, const void* p, uint64_t bytes) {
  if (!p) return fail(e, DRS_ERR_BAD_ARG, "query %d: null %s", i, name);
  if (reinterpret_cast<uintptr_t>(p) & 3) return fail(e, DRS_ERR_BAD_ARG, "query %d: %s is not aligned to its element type", i, name);
  const char* why = device_range_fault(e, p, bytes);
  if (why) return fail(e, DRS_ERR_BAD_ARG, "query %d: %s %s", i, name, why);
  return DRS_OK;
}

static int32_t device_topk_set(drs_engine* e, int32_t slot, const DeviceSet& d, int64_t Mv, const int32_t* k, int32_t col,
                               int32_t* const* d_top_idx, float* const* d_top_scores, void* stream, int32_t ordered) {
  const int32_t n = d.n;
  const int32_t* bs = d.bs;
  int32_t rc;
  // what the host can see of the outputs, before anything is enqueued (a slot in flight is not even waited for)
  if (ordered != 0 && ordered != 1) return fail(e, DRS_ERR_BAD_ARG, "ordered=%d: 0 (complete inputs, drs_wait) or 1 (both ends on the stream)", ordered);
  if (col < 0 || col >= e->n_out) return fail(e, DRS_ERR_BAD_ARG, "col=%d: the rows have %d score columns", col, e->n_out);
  if (!k) return fail(e, DRS_ERR_BAD_ARG, "a null k table");
  TopKExtent x[2 * DRS_MAX_COALESCE];
  int n_x = 0;
  for (int i = 0; i < n; ++i) {
    if (!topk_k_in_range(k[i], bs[i]))
      return fail(e, DRS_ERR_BAD_ARG, "query %d: k=%d outside 0..min(bs=%d, %d)", i, k[i], bs[i], DRS_TOPK_MAX);
    if (k[i] == 0) continue;
    if (!d_top_idx || !d_top_scores) return fail(e, DRS_ERR_BAD_ARG, "bad per-query top-k output tables");
    uint64_t top_bytes, idx_bytes;
    if (!topk_extent_bytes(k[i], e->n_out, &top_bytes, &idx_bytes)) return fail(e, DRS_ERR_BAD_ARG, "query %d: the top-k extents", i);
    if ((rc = check_topk_output(e, i, "d_top_idx", d_top_idx[i], idx_bytes))) return rc;
    if ((rc = check_topk_output(e, i, "d_top_scores", d_top_scores[i], top_bytes))) return rc;
    x[n_x++] = {reinterpret_cast<uintptr_t>(d_top_idx[i]), idx_bytes, i, "d_top_idx"};
    x[n_x++] = {reinterpret_cast<uintptr_t>(d_top_scores[i]), top_bytes, i, "d_top_scores"};
  }
  for (int i = 0; i < n_x; ++i)
    for (int j = i + 1; j < n_x; ++j)
      if (extents_overlap(x[i].p, x[i].bytes, x[j].p, x[j].bytes))
        return fail(e, DRS_ERR_BAD_ARG, "%s of query %d and %s of query %d overlap", x[i].name, x[i].query, x[j].name, x[j].query);

  hipStream_t caller = static_cast<hipStream_t>(stream);      // (NULL is HIP's null stream: `ordered` says whether it counts)
  if ((rc = enqueue_device_set(e, slot, d, Mv, ordered ? &caller : nullptr))) return rc;
  Slot& s = e->slots[slot];
  if (s.last_bs == 0) return DRS_OK;                           // nothing was launched: no pass, no edge
  TopKArgs a;
  memset(&a, 0, sizeof a);
  a.err = s.d_err; a.n_out = e->n_out; a.col = col;
  for (int i = 0; i < n; ++i) {
    if (bs[i] == 0 || k[i] == 0) continue;
    TopKQuery& q = a.q[a.n_q++];
    q.src = s.d_out + (size_t)s.q_vstart[i] * e->n_out; q.stride = e->n_out;
    q.top = d_top_scores[i]; q.idx = d_top_idx[i];
    q.bs = bs[i]; q.k = k[i];
  }
  // on s.stream: hand_off has brought the set back there, behind its last kernel.  A set whose every k is 0 launches no
  // pass; its event still closes the set, so that both ends keep their order
  HIP_TRY(e, launch_topk_pass(a, s.stream));
  HIP_TRY(e, hipEventRecord(s.ev_out, s.stream));
  s.out_pass = true;
  if (ordered) HIP_TRY(e, hipStreamWaitEvent(caller, s.ev_out, 0));
  if (e->dispatch_log && a.n_q > 0) log_launch(&s.dlog, "topk_pass[%d x %d]", a.n_q, kTopKThreads);
  return DRS_OK;
}

}  // namespace eng
}  // namespace drs

extern "C" {

int32_t drs_run_queues_device_topk_multi_async(drs_handle e, int32_t slot, int32_t n, const int32_t* bs,
                                               const float* const* d_dense, const int64_t* const* d_ids,
                                               const int64_t* ids_row_stride, const int64_t* n_idx_per_table,
                                               const int32_t* const* d_lengths, const int64_t* len_row_stride,
                                               const int32_t* fixed_len, const void* const* d_weights,
                                               const int64_t* wgt_row_stride, const int32_t* wgt_dtype, const int32_t* k,
                                               int32_t col, int32_t* const* d_top_idx, float* const* d_top_scores, void* stream,
                                               int32_t ordered) {
  // a NULL d_weights table: the set carries no weights, and is the device-input call's set
  const DeviceSet d = {n, bs, d_dense, d_ids, ids_row_stride, n_idx_per_table, d_lengths, len_row_stride, fixed_len,
                       d_weights, wgt_row_stride, wgt_dtype, d_weights != nullptr};
  int64_t Mv = 0;
  const int32_t rc = check_device_set(e, slot, d, &Mv);
  return rc ? rc : device_topk_set(e, slot, d, Mv, k, col, d_top_idx, d_top_scores, stream, ordered);
}

int32_t drs_topk_rows(drs_handle e, const float* d_scores, int64_t rows, int32_t n_out, int64_t row_stride, int32_t col, int32_t k,
                      int32_t* d_idx, float* d_top, void* stream) {
  int32_t rc = check_handle(e);
  if (rc) return rc;
  if (rows < 1 || rows > INT32_MAX || n_out < 1) return fail(e, DRS_ERR_BAD_ARG, "drs_topk_rows: %lld rows of %d scores", (long long)rows, n_out);
  if (k < 1 || !topk_k_in_range(k, rows)) return fail(e, DRS_ERR_BAD_ARG, "drs_topk_rows: k=%d outside 1..min(rows=%lld, %d)", k, (long long)rows, DRS_TOPK_MAX);
  if (col < 0 || col >= n_out) return fail(e, DRS_ERR_BAD_ARG, "drs_topk_rows: col=%d: the rows have %d score columns", col, n_out);
  uint64_t src_bytes, top_bytes, idx_bytes;
  if (!topk_source_bytes(rows, row_stride, n_out, &src_bytes))
    return fail(e, DRS_ERR_BAD_ARG, "drs_topk_rows: a row stride of %lld floats for rows of %d (below the row, or beyond any allocation)", (long long)row_stride, n_out);
  if (!topk_extent_bytes(k, n_out, &top_bytes, &idx_bytes)) return fail(e, DRS_ERR_BAD_ARG, "drs_topk_rows: the top-k extents");
  if ((rc = check_topk_output(e, 0, "d_scores", d_scores, src_bytes))) return rc;
  if ((rc = check_topk_output(e, 0, "d_idx", d_idx, idx_bytes))) return rc;
  if ((rc = check_topk_output(e, 0, "d_top", d_top, top_bytes))) return rc;
  if (extents_overlap(reinterpret_cast<uintptr_t>(d_idx), idx_bytes, reinterpret_cast<uintptr_t>(d_top), top_bytes))
    return fail(e, DRS_ERR_BAD_ARG, "drs_topk_rows: d_idx and d_top overlap");
  TopKArgs a;
  memset(&a, 0, sizeof a);
  a.n_q = 1; a.n_out = n_out; a.col = col;
  a.q[0].src = d_scores; a.q[0].stride = rows > 1 ? row_stride : 0;
  a.q[0].top = d_top; a.q[0].idx = d_idx; a.q[0].bs = (int32_t)rows; a.q[0].k = k;
  HIP_TRY(e, launch_topk_pass(a, static_cast<hipStream_t>(stream)));
  return DRS_OK;
}

}  // extern "C"
