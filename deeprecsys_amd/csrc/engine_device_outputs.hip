// libdrs_hip.so, host side: launch sets whose results STAY on the device (include/drs_device_outputs.h).  A device-input set
// (engine_device_inputs.hip: the same checks, the same input pass, the same launches) with two things more: one launch of
// the output pass (output_pass.hip) behind the set's last kernel moves every query's scores from Slot::d_out to the
// caller's own device arrays, and -- ordered == 1 -- two event edges tie the set to the caller's stream, in front of the
// input pass and behind the output pass.  drs_wait stays the slot's completion; wait_slot waits for the pass's event.
#include "engine.h"
#include "output_plan.h"

namespace drs {
namespace eng {

// the device set `d` (checked: Mv is check_device_set's) with its results left in d_out -- shared by
// drs_run_queues_device_io_multi_async and the form of it that carries per-sample weights
static int32_t device_io_set(drs_engine* e, int32_t slot, const DeviceSet& d, int64_t Mv, float* const* d_out,
                             const int64_t* out_row_stride, void* stream, int32_t ordered) {
  const int32_t n = d.n;
  const int32_t* bs = d.bs;
  int32_t rc;
  // what the host can see of the outputs, before anything is enqueued (a slot in flight is not even waited for)
  if (ordered != 0 && ordered != 1) return fail(e, DRS_ERR_BAD_ARG, "ordered=%d: 0 (complete inputs, drs_wait) or 1 (both ends on the stream)", ordered);
  if (!d_out || !out_row_stride) return fail(e, DRS_ERR_BAD_ARG, "bad per-query output tables");
  uint64_t bytes[DRS_MAX_COALESCE];
  for (int i = 0; i < n; ++i) {
    if (bs[i] > 0 && !d_out[i]) return fail(e, DRS_ERR_BAD_ARG, "query %d: null d_out", i);
    if (reinterpret_cast<uintptr_t>(d_out[i]) & 3) return fail(e, DRS_ERR_BAD_ARG, "query %d: d_out is not aligned to its element type", i);
    if (!output_extent_bytes(bs[i], out_row_stride[i], e->n_out, &bytes[i]))
      return fail(e, DRS_ERR_BAD_ARG, "query %d: an output row stride of %lld floats for rows of %d (below the row, or beyond any allocation)",
                  i, (long long)out_row_stride[i], e->n_out);
    const char* why;
    if (d_out[i] && (why = device_range_fault(e, d_out[i], bytes[i]))) return fail(e, DRS_ERR_BAD_ARG, "query %d: d_out %s", i, why);
  }
  for (int i = 0; i < n; ++i)
    for (int j = i + 1; j < n; ++j)
      if (extents_overlap(reinterpret_cast<uintptr_t>(d_out[i]), bytes[i], reinterpret_cast<uintptr_t>(d_out[j]), bytes[j]))
        return fail(e, DRS_ERR_BAD_ARG, "queries %d and %d: their outputs overlap", i, j);

  hipStream_t caller = static_cast<hipStream_t>(stream);      // (NULL is HIP's null stream: `ordered` says whether it counts)
  if ((rc = enqueue_device_set(e, slot, d, Mv, ordered ? &caller : nullptr))) return rc;
  Slot& s = e->slots[slot];
  if (s.last_bs == 0) return DRS_OK;                           // nothing was launched: no pass, no edge
  OutPassArgs a;
  memset(&a, 0, sizeof a);
  a.src = s.d_out; a.err = s.d_err; a.n_out = e->n_out;
  for (int i = 0; i < n; ++i) {
    if (bs[i] == 0) continue;
    OutQuery& q = a.q[a.n_q++];
    q.dst = d_out[i]; q.stride = bs[i] > 1 ? out_row_stride[i] : 0;
    q.vstart = s.q_vstart[i]; q.bs = bs[i];
  }
  const int64_t grid = plan_output_pass(a);
  if (grid <= 0) return fail(e, DRS_ERR_BAD_ARG, "the set's %lld output floats do not fit one output pass", (long long)s.last_bs * e->n_out);
  // on s.stream: hand_off has brought the set back there, behind its last kernel
  HIP_TRY(e, launch_output_pass(a, grid, s.stream));
  HIP_TRY(e, hipEventRecord(s.ev_out, s.stream));
  s.out_pass = true;
  if (ordered) HIP_TRY(e, hipStreamWaitEvent(caller, s.ev_out, 0));
  if (e->dispatch_log) log_launch(&s.dlog, "output_pass[%lld x %d]", (long long)grid, kOutPassThreads);
  return DRS_OK;
}

}  // namespace eng
}  // namespace drs

extern "C" {

int32_t drs_run_queues_device_io_multi_async(drs_handle e, int32_t slot, int32_t n, const int32_t* bs,
                                             const float* const* d_dense, const int64_t* const* d_ids,
                                             const int64_t* ids_row_stride, const int64_t* n_idx_per_table,
                                             const int32_t* const* d_lengths, const int64_t* len_row_stride,
                                             const int32_t* fixed_len, float* const* d_out, const int64_t* out_row_stride,
                                             void* stream, int32_t ordered) {
  const DeviceSet d = {n, bs, d_dense, d_ids, ids_row_stride, n_idx_per_table, d_lengths, len_row_stride, fixed_len};
  int64_t Mv = 0;
  const int32_t rc = check_device_set(e, slot, d, &Mv);
  return rc ? rc : device_io_set(e, slot, d, Mv, d_out, out_row_stride, stream, ordered);
}

// both forms with per-sample weights (include/drs_device_weights.h): d_out == NULL is the host-output form
int32_t drs_run_queues_device_weighted_multi_async(drs_handle e, int32_t slot, int32_t n, const int32_t* bs,
                                                   const float* const* d_dense, const int64_t* const* d_ids,
                                                   const int64_t* ids_row_stride, const int64_t* n_idx_per_table,
                                                   const int32_t* const* d_lengths, const int64_t* len_row_stride,
                                                   const int32_t* fixed_len, const void* const* d_weights,
                                                   const int64_t* wgt_row_stride, const int32_t* wgt_dtype, float* const* d_out,
                                                   const int64_t* out_row_stride, void* stream, int32_t ordered) {
  const DeviceSet d = {n, bs, d_dense, d_ids, ids_row_stride, n_idx_per_table, d_lengths, len_row_stride, fixed_len,
                       d_weights, wgt_row_stride, wgt_dtype, true};
  int64_t Mv = 0;
  const int32_t rc = check_device_set(e, slot, d, &Mv);
  if (rc) return rc;
  if (d_out) return device_io_set(e, slot, d, Mv, d_out, out_row_stride, stream, ordered);
  if (ordered != 0) return fail(e, DRS_ERR_BAD_ARG, "ordered=%d without d_out: the host-output form takes complete inputs (ordered 0)", ordered);
  return enqueue_device_set(e, slot, d, Mv, nullptr);
}

int32_t drs_run_queues_device_io_async(drs_handle e, int32_t slot, int32_t bs, const float* d_dense, const int64_t* d_ids,
                                       int64_t ids_row_stride, int64_t n_idx_per_table, const int32_t* d_lengths,
                                       int64_t len_row_stride, int32_t fixed_len, float* d_out, int64_t out_row_stride,
                                       void* stream, int32_t ordered) {
  return drs_run_queues_device_io_multi_async(e, slot, 1, &bs, &d_dense, &d_ids, &ids_row_stride, &n_idx_per_table, &d_lengths,
                                              &len_row_stride, &fixed_len, &d_out, &out_row_stride, stream, ordered);
}

}  // extern "C"
