// libdrs_hip.so, host side: launch sets whose per-query arrays are DEVICE arrays (include/drs_device_inputs.h).  The host
// refuses what it can see (shapes, NULLs, pointers that are not device memory or run past their allocation), one launch of
// the input pass (input_pass.hip) converts and checks the arrays into the slot's per-query HBM blocks on the stream the
// host form puts its DMA copy on, and the set is then enqueued exactly like a host set (enqueue_forward on Slot::mq).
// The two steps are functions of their own (check_device_set, enqueue_device_set): the form that also leaves its results
// on the device (engine_device_outputs.hip) puts its own refusals between them and its output pass behind them.
#include "engine.h"
#include "input_extent.h"
#include "weight_plan.h"

namespace drs {
namespace eng {

const char* device_range_fault(const drs_engine* e, const void* p, size_t bytes) {
  hipPointerAttribute_t at;
  memset(&at, 0, sizeof at);
  if (hipPointerGetAttributes(&at, p) != hipSuccess) {
    (void)hipGetLastError();
    return "is not memory the HIP runtime knows";
  }
  if (at.type != hipMemoryTypeDevice || at.isManaged) return "is not plain device memory (host, pinned and managed memory are refused)";
  if (at.device != e->device) return "lives on another device";
  hipDeviceptr_t base = nullptr;
  size_t size = 0;
  if (hipMemGetAddressRange(&base, &size, const_cast<void*>(p)) != hipSuccess) {
    (void)hipGetLastError();
    return "has no allocation the HIP runtime knows";
  }
  if (!extent_inside(reinterpret_cast<uintptr_t>(p), bytes, reinterpret_cast<uintptr_t>(base), size)) return "runs past the end of its allocation";
  return nullptr;
}

int32_t check_device_set(drs_engine* e, int32_t slot, const DeviceSet& d, int64_t* Mv_out) {
  const int32_t n = d.n;
  const int32_t* bs = d.bs;
  const float* const* d_dense = d.d_dense;
  const int64_t* const* d_ids = d.d_ids;
  const int32_t* const* d_lengths = d.d_lengths;
  const int64_t *ids_row_stride = d.ids_row_stride, *n_idx_per_table = d.n_idx_per_table, *len_row_stride = d.len_row_stride;
  const int32_t* fixed_len = d.fixed_len;
  int32_t rc = check_handle(e);
  if (rc) return rc;
  if (slot < 0 || slot >= e->n_slots) return fail(e, DRS_ERR_BAD_ARG, "slot %d of %d", slot, e->n_slots);
  if (n < 1 || n > DRS_MAX_COALESCE) return fail(e, DRS_ERR_BAD_ARG, "1..%d queries per launch", DRS_MAX_COALESCE);
  if (!bs || !d_dense || !d_ids || !ids_row_stride || !n_idx_per_table || !d_lengths || !len_row_stride)
    return fail(e, DRS_ERR_BAD_ARG, "bad per-query array tables");
  const int T = e->T;
  // everything the host can see, before anything is enqueued (a slot in flight is not even waited for)
  int64_t Mv = 0;
  for (int i = 0; i < n; ++i) {
    const int32_t fl = fixed_len ? fixed_len[i] : -1;
    const int64_t ni = n_idx_per_table[i];
    if ((rc = check_bs(e, i, bs[i]))) return rc;
    if (ni < 0 || ni > e->cap) return fail(e, DRS_ERR_BAD_ARG, "query %d: %lld indices per table exceed staging capacity %lld", i, (long long)ni, (long long)e->cap);
    if (fl < -1) return fail(e, DRS_ERR_BAD_ARG, "query %d: fixed_len=%d", i, fl);
    if (ids_row_stride[i] < 0 || len_row_stride[i] < 0) return fail(e, DRS_ERR_BAD_ARG, "query %d: negative row stride", i);
    if (bs[i] > 0 && (!d_ids[i] || !d_lengths[i])) return fail(e, DRS_ERR_BAD_ARG, "query %d: null ids / lengths", i);
    if ((rc = check_dense(e, i, d_dense[i], bs[i]))) return rc;
    Mv += padded_rows(bs[i]);
  }
  if ((rc = check_set_rows(e, Mv))) return rc;
  for (int i = 0; i < n; ++i) {
    const int32_t fl = fixed_len ? fixed_len[i] : -1;
    const int64_t ni = n_idx_per_table[i];
    if (fl >= 0 && ni != (int64_t)bs[i] * fl)
      return fail(e, DRS_ERR_LENGTHS_SUM, "query %d: %lld indices per table, but %d bags of the promised length %d", i, (long long)ni, bs[i], fl);
    if (bs[i] == 0 && ni != 0)
      return fail(e, DRS_ERR_LENGTHS_SUM, "query %d: sum(lengths)=0 != len(indices)=%lld", i, (long long)ni);
  }
  // the pointer check: three pointers per query, each with the extent the pass will read
  // (an empty query's pointers are checked too where it has any: what they are is refused even when nothing is read)
  for (int i = 0; i < n; ++i) {
    const int64_t ni = n_idx_per_table[i];
    uint64_t ids_bytes, len_bytes, dense_bytes;
    if (!input_extent_bytes(T, ids_row_stride[i], ni, sizeof(int64_t), &ids_bytes) ||
        !input_extent_bytes(T, len_row_stride[i], bs[i], sizeof(int32_t), &len_bytes) ||
        !input_extent_bytes(1, 0, (int64_t)bs[i] * (e->m_den > 0 ? e->m_den : 0), sizeof(float), &dense_bytes))
      return fail(e, DRS_ERR_BAD_ARG, "query %d: a row stride beyond any allocation", i);
    const char* why;
    if ((reinterpret_cast<uintptr_t>(d_ids[i]) & 7) || (reinterpret_cast<uintptr_t>(d_lengths[i]) & 3) ||
        (reinterpret_cast<uintptr_t>(d_dense[i]) & 3))
      return fail(e, DRS_ERR_BAD_ARG, "query %d: a pointer is not aligned to its element type", i);
    if (d_ids[i] && (why = device_range_fault(e, d_ids[i], ids_bytes))) return fail(e, DRS_ERR_BAD_ARG, "query %d: d_ids %s", i, why);
    if (d_lengths[i] && (why = device_range_fault(e, d_lengths[i], len_bytes))) return fail(e, DRS_ERR_BAD_ARG, "query %d: d_lengths %s", i, why);
    if (e->m_den > 0 && d_dense[i] && (why = device_range_fault(e, d_dense[i], dense_bytes)))
      return fail(e, DRS_ERR_BAD_ARG, "query %d: d_dense %s", i, why);
  }
  // per-sample weights (include/drs_device_weights.h): one more array per weighted query, checked like the others
  if (d.weights_call) {
    if (!d.d_weights || !d.wgt_row_stride) return fail(e, DRS_ERR_BAD_ARG, "bad per-query weight tables");
    for (int i = 0; i < n; ++i) {
      const void* w = d.d_weights[i];
      if (!w) continue;
      if (e->kind == DRS_MODEL_DIN || e->kind == DRS_MODEL_DIEN)
        return fail(e, DRS_ERR_UNSUPPORTED, "drs_run_queues_device_weighted_multi_async: DIN and DIEN pool their bags by the plain sum only");
      if (e->sls_pool)
        return fail(e, DRS_ERR_UNSUPPORTED, "drs_run_queues_device_weighted_multi_async: \"sls_pool\" 1 has no weighted form (there is no weighted mean)");
      const int32_t ty = d.weight_type(i);
      if (ty != DRS_TABLE_FP32 && ty != DRS_TABLE_FP16 && ty != DRS_TABLE_BF16)
        return fail(e, DRS_ERR_BAD_ARG, "query %d: wgt_dtype=%d: 0 (fp32), 1 (fp16) or 2 (bf16)", i, ty);
      const int64_t elem = ty == DRS_TABLE_FP32 ? 4 : 2;
      if (d.wgt_row_stride[i] < 0) return fail(e, DRS_ERR_BAD_ARG, "query %d: negative weight row stride", i);
      uint64_t wgt_bytes;
      if (!weight_extent_bytes(T, d.wgt_row_stride[i], n_idx_per_table[i], elem, &wgt_bytes))
        return fail(e, DRS_ERR_BAD_ARG, "query %d: a weight row stride beyond any allocation", i);
      if (reinterpret_cast<uintptr_t>(w) & (uintptr_t)(elem - 1))
        return fail(e, DRS_ERR_BAD_ARG, "query %d: d_weights is not aligned to its element type", i);
      const char* why = device_range_fault(e, w, wgt_bytes);
      if (why) return fail(e, DRS_ERR_BAD_ARG, "query %d: d_weights %s", i, why);
    }
  }
  *Mv_out = Mv;
  return DRS_OK;
}

// the slot's weight blocks, allocated when it first sees a weighted set (an engine that never sees weights allocates nothing)
static int32_t weight_blocks(drs_engine* e, Slot& s) {
  if (s.d_wgt) return DRS_OK;
  const hipError_t r = s.d_wgt.alloc(e->blk.idx_elems() * DRS_MAX_COALESCE);
  if (r != hipSuccess) {
    (void)hipGetLastError();
    return fail(e, r == hipErrorOutOfMemory ? DRS_ERR_OOM : DRS_ERR_HIP, "per-sample weight blocks of a launch set: %s", hipGetErrorString(r));
  }
  return DRS_OK;
}

int32_t enqueue_device_set(drs_engine* e, int32_t slot, const DeviceSet& d, int64_t Mv, const hipStream_t* behind) {
  const int32_t n = d.n;
  const int32_t *bs = d.bs, *fixed_len = d.fixed_len;
  const int T = e->T;
  int32_t rc;
  Slot& s = e->slots[slot];
  if (s.busy && (rc = wait_slot(e, s, nullptr))) return rc;
  if ((rc = multi_blocks(e, s, false))) return rc;
  bool any_w = false, pass_w = false;   // a query carries weights: the slot's weight blocks; a non-empty one: the weighted instance of the pass
  for (int i = 0; i < n; ++i) {
    any_w |= d.weights_of(i) != nullptr;
    pass_w |= bs[i] > 0 && d.weights_of(i) != nullptr;
  }
  if (any_w && (rc = weight_blocks(e, s))) return rc;
  if ((rc = copy_stream(e))) return rc;

  InPassWgtArgs aw;
  memset(&aw, 0, sizeof aw);
  InPassArgs& a = aw.in;
  a.T = T; a.m_den = e->m_den; a.max_batch = e->max_batch; a.cap = e->cap;
  a.rows = e->d_tab_rows; a.err = s.d_err;
  const Batch* bts[DRS_MAX_COALESCE];
  for (int i = 0; i < n; ++i) {
    Batch& b = s.mq[i];
    const int32_t fl = fixed_len ? fixed_len[i] : -1;
    b.n_samples = bs[i];
    b.staged = true;
    // a query's weights go to block i of the slot's weight storage, laid out like its index rows; enqueue_forward then plans
    // the set as it plans a set of staged batches of which the same ones carry weights
    const void* w = d.weights_of(i);
    b.weighted = w != nullptr;
    b.wgt = w ? s.d_wgt + (size_t)i * e->blk.idx_elems() : nullptr;
    b.uniform_len = bs[i] > 0 ? fl : -1;
    for (int t = 0; t < T; ++t) b.h_off[e->blk.h_off_at(t, bs[i])] = (int32_t)d.n_idx_per_table[i];   // (all the byte accounting reads)
    bts[i] = &b;
    if (bs[i] == 0) continue;
    InQuery& q = a.q[a.n_q++];
    q.ids = d.d_ids[i]; q.len = d.d_lengths[i]; q.dense = e->m_den > 0 ? d.d_dense[i] : nullptr;
    q.ids_stride = d.ids_row_stride[i]; q.len_stride = d.len_row_stride[i];
    q.idx = b.idx; q.off = b.off; q.dst_dense = b.dense;
    q.bs = bs[i]; q.n_idx = (int32_t)d.n_idx_per_table[i];
    q.fixed_len = fl;
    q.store_off = !e->sls_uniform || fl < 0;     // (enqueue_forward's predicate for handing the kernels uniform_len = -1)
    if (w) {
      InWgt& iw = aw.w[a.n_q - 1];
      iw.src = w; iw.stride = d.wgt_row_stride[i]; iw.dst = b.wgt; iw.dtype = d.weight_type(i);
    }
  }
  const int64_t grid = pass_w ? plan_input_pass_weighted(aw) : plan_input_pass(a);
  if (grid < 0) return fail(e, DRS_ERR_BAD_ARG, "the set's inputs do not fit one input pass");
  if (grid > 0) {
    if (behind) {
      // the engine's streams are non-blocking: the edge from the caller's stream (the null stream too) is an event
      HIP_TRY(e, hipEventRecord(s.ev_caller, *behind));
      HIP_TRY(e, hipStreamWaitEvent(e->stream_h2d, s.ev_caller, 0));
    }
    if (pass_w) HIP_TRY(e, launch_input_pass_weighted(aw, grid, e->stream_h2d));
    else HIP_TRY(e, launch_input_pass(a, grid, e->stream_h2d));
    if ((rc = order_behind_inputs(e, s, Mv))) return rc;
  }
  rc = enqueue_forward(e, s, n, bts, bs);
  if (rc == DRS_OK && grid > 0 && e->dispatch_log) {
    // the pass's own entry, in FRONT of the entries enqueue_forward has just noted for the set (it starts the record)
    char head[64];
    const int hl = snprintf(head, sizeof head, "input_pass[%lld x %d%s] ", (long long)grid, kInPassThreads, pass_w ? ",w" : "");
    DispatchLog& lg = s.dlog;
    if (hl > 0 && lg.len + hl < (int)sizeof(lg.text)) {
      memmove(lg.text + hl, lg.text, (size_t)lg.len + 1);
      memcpy(lg.text, head, (size_t)hl);
      lg.len += hl;
    }
  }
  return rc;
}

}  // namespace eng
}  // namespace drs

extern "C" {

int32_t drs_run_queues_device_multi_async(drs_handle e, int32_t slot, int32_t n, const int32_t* bs,
                                          const float* const* d_dense, const int64_t* const* d_ids,
                                          const int64_t* ids_row_stride, const int64_t* n_idx_per_table,
                                          const int32_t* const* d_lengths, const int64_t* len_row_stride,
                                          const int32_t* fixed_len) {
  const DeviceSet d = {n, bs, d_dense, d_ids, ids_row_stride, n_idx_per_table, d_lengths, len_row_stride, fixed_len};
  int64_t Mv = 0;
  const int32_t rc = check_device_set(e, slot, d, &Mv);
  return rc ? rc : enqueue_device_set(e, slot, d, Mv, nullptr);
}

int32_t drs_run_queues_device_async(drs_handle e, int32_t slot, int32_t bs, const float* d_dense, const int64_t* d_ids,
                                    int64_t ids_row_stride, int64_t n_idx_per_table, const int32_t* d_lengths,
                                    int64_t len_row_stride, int32_t fixed_len) {
  return drs_run_queues_device_multi_async(e, slot, 1, &bs, &d_dense, &d_ids, &ids_row_stride, &n_idx_per_table, &d_lengths,
                                           &len_row_stride, &fixed_len);
}

}  // extern "C"
