// libdrs_hip.so, host side: staged input sets and the per-call input path -- drs_stage_batch, drs_forward_inputs*,
// drs_run_queues*.  A query's arrays go through ONE host pass (convert_item per table and for the dense rows, then
// seal_query; int64 -> int32 + Caffe2's ENFORCEs: input_block.h) into one packed block [dense | idx | off] whose layout is
// e->blk, and the copies plan_block_copies lists move what was used of it: a query alone converts its one block, a launch
// set converts its n blocks in one fork-join and ships them on the copy stream.
#include "engine.h"

namespace drs {
namespace eng {

// One query's per-call arrays: per-table lists (drs_forward_inputs*), or with ids non-null 2-D arrays with a row stride (drs_run_queues*)
struct QueryIn {
  int32_t bs;
  const float* dense;
  const int64_t* const* idx_list;
  const int64_t* n_idx_list;
  const int32_t* const* len_list;
  const int64_t* ids;
  const int32_t* lens;
  int64_t ids_stride, len_stride, n_idx_all;
  const int64_t* idx(int t) const { return ids ? ids + (int64_t)t * ids_stride : idx_list[t]; }
  const int32_t* len(int t) const { return ids ? lens + (int64_t)t * len_stride : len_list[t]; }
  int64_t n_idx(int t) const { return ids ? n_idx_all : n_idx_list[t]; }
};

// "query 3: " in front of what a launch set refuses (i < 0, a query alone: nothing)
struct Who {
  char s[32];
  explicit Who(int i) { s[0] = 0; if (i >= 0) snprintf(s, sizeof s, "query %d: ", i); }
};
int32_t check_bs(drs_engine* e, int i, int32_t bs) {
  if (bs < 0 || bs > e->max_batch) return fail(e, DRS_ERR_BAD_ARG, "%sn_samples=%d exceeds max_batch=%d", Who(i).s, bs, e->max_batch);
  return DRS_OK;
}
int32_t check_dense(drs_engine* e, int i, const float* dense, int32_t bs) {
  if (e->m_den > 0 && !dense && bs > 0) return fail(e, DRS_ERR_BAD_ARG, "%snull dense input", Who(i).s);
  return DRS_OK;
}
int32_t check_set_rows(drs_engine* e, int64_t Mv) {
  if (Mv > e->max_rows) return fail(e, DRS_ERR_BAD_ARG, "%lld coalesced rows exceed the slot capacity %lld", (long long)Mv, (long long)e->max_rows);
  return DRS_OK;
}

// the workers of the host pass (created on first use)
static HostPool* host_pool(drs_engine* e) {
  if (!e->pool) {
    int w = e->host_threads >= 0 ? e->host_threads : (e->T < 7 ? e->T : 7);   // T tables + the dense rows
    const int hw = (int)std::thread::hardware_concurrency();
    if (hw > 0 && w > hw - 1) w = hw - 1;
    e->pool.reset(new HostPool(w < 0 ? 0 : w));
  }
  return e->pool.get();
}

// Work item t of a query's host pass into the block v (host addresses): table t, or with t == T the dense rows (v.dense
// null: they travel another way).  h_off (optional): the batch's host copy of the prefix sums, filled table by table.
static void convert_item(const drs_engine* e, const QueryIn& q, int t, const BlockView& v, int32_t* h_off, ConvRes* res) {
  const BlockLayout& L = e->blk;
  if (t == e->T) {
    if (v.dense && e->m_den > 0 && q.bs > 0) memcpy(v.dense, q.dense, sizeof(float) * (size_t)q.bs * e->m_den);
    return;
  }
  int32_t* off_t = v.off + L.h_off_at(t, 0);
  convert_table(L, e->rows[t], q.bs, q.idx(t), q.n_idx(t), q.len(t), v.idx + (size_t)t * L.cap, off_t, res[t]);
  if (h_off) memcpy(h_off + L.h_off_at(t, 0), off_t, sizeof(int32_t) * L.off_stride());
}

// Seal a converted query: what its lowest failing table reports (what a sequential pass would have hit first), else the
// batch is staged -- uniform_len from every table's ConvRes::same and first length.
static int32_t seal_query(drs_engine* e, Batch& b, const QueryIn& q, const ConvRes* res, int i) {
  for (int t = 0; t < e->T; ++t) {
    const ConvRes& r = res[t];
    if (r.code == DRS_OK) continue;
    const Who who(i);
    if (r.code == DRS_ERR_BAD_ARG) {
      if (r.pos == -1) return fail(e, DRS_ERR_BAD_ARG, "%sh_idx[%d] is NULL", who.s, t);
      if (r.pos == -2) return fail(e, DRS_ERR_BAD_ARG, "%sh_len[%d] is NULL", who.s, t);
      return fail(e, DRS_ERR_BAD_ARG, "%stable %d: %lld indices exceed staging capacity %lld", who.s, t,
                  (long long)r.n_idx, (long long)e->cap);
    }
    if (r.code == DRS_ERR_LENGTHS_SUM) {
      if (r.pos == -1) return fail(e, DRS_ERR_LENGTHS_SUM, "%stable %d bag %d: negative length", who.s, t, r.bag);
      return fail(e, DRS_ERR_LENGTHS_SUM, "%stable %d: sum(lengths)=%lld != len(indices)=%lld", who.s, t,
                  (long long)r.total, (long long)r.n_idx);
    }
    return fail(e, DRS_ERR_INDEX_RANGE, "%stable %d: index %lld at position %lld outside [0, %lld)", who.s, t,
                (long long)r.val, (long long)r.pos, (long long)e->rows[t]);
  }
  b.n_samples = q.bs;
  b.staged = true;
  b.uniform_len = -1;
  if (q.bs > 0) {
    const int32_t L0 = q.len(0)[0];
    bool same = true;
    for (int t = 0; t < e->T && same; ++t) same = res[t].same && q.len(t)[0] == L0;
    if (same) b.uniform_len = L0;
  }
  return DRS_OK;
}

// record that the set's blocks are filled (stream_h2d) and order its gather and MLP streams behind that
int32_t order_behind_inputs(drs_engine* e, Slot& s, int64_t Mv) {
  HIP_TRY(e, hipEventRecord(s.ev_in, e->stream_h2d));
  const hipStream_t ms = job_stream(e, s, Mv), gs = job_gather_stream(e, s, Mv);
  HIP_TRY(e, hipStreamWaitEvent(gs, s.ev_in, 0));
  if (ms != gs) HIP_TRY(e, hipStreamWaitEvent(ms, s.ev_in, 0));   // the MLP side reads the dense rows
  return DRS_OK;
}

// Everything of a per-call-input query that is a HIP call: the one DMA copy of its converted block
// (copy mode 2), the cross-stream events, the launches.  Runs on the calling thread or, with
// "launch_thread" 1, on the launcher thread.
int32_t finish_inputs(drs_engine* e, Slot& s, int mode, int32_t bs, size_t used, bool need_off) {
  const Batch* bt = mode == 2 ? &s.dc : mode == 1 ? &s.zc : &s.scratch;
  if (mode != 1) {
    const hipStream_t gstream = job_gather_stream(e, s, padded_rows(bs));
    if (mode == 2) {
      // the used prefix and, for ragged bags -- or "sls_uniform" 0, which makes enqueue_forward hand the kernels
      // uniform_len = -1 for fixed-length bags too -- the prefix sums as well (same predicate)
      BlockCopy cp[2];
      const int n_cp = plan_block_copies(e->blk, 0, 1, &used, &need_off, false, cp);
      for (int k = 0; k < n_cp; ++k)
        HIP_TRY(e, hipMemcpyAsync(s.d_stage + cp[k].at, static_cast<char*>(s.h_stage) + cp[k].at, cp[k].bytes, hipMemcpyHostToDevice, gstream));
    }
    // mode 2 copied on the gather's stream and the MLP side reads the dense rows; mode 0 copied on the MLP side's stream
    // and the gather runs on another: order the one behind the other
    if (gstream != s.stream) {
      HIP_TRY(e, hipEventRecord(s.ev_in, mode == 2 ? gstream : s.stream));
      HIP_TRY(e, hipStreamWaitEvent(mode == 2 ? s.stream : gstream, s.ev_in, 0));
    }
  }
  return enqueue_forward(e, s, 1, &bt, &bs);
}

// The per-query blocks of a slot's launch sets with per-call inputs, allocated on first use: the HBM blocks (s.d_multi,
// viewed as s.mq) and, for the host form alone (host_side), their pinned twins -- the device form
// (engine_device_inputs.hip) never needs the pinned half.  What THIS call allocated is all there or all gone (the slot
// takes the two over only once both exist); blocks an earlier call of the other form made stay.
int32_t multi_blocks(drs_engine* e, Slot& s, bool host_side) {
  const bool need_d = !s.d_multi, need_h = host_side && !s.h_multi;
  if (!need_d && !need_h) return DRS_OK;
  const size_t block = e->blk.padded;
  PinnedBuf<char> h;
  DeviceBuf<char> d;
  hipError_t r = hipSuccess;
  if (need_h) r = h.alloc(block * DRS_MAX_COALESCE, hipHostMallocDefault);
  if (r == hipSuccess && need_d) r = d.alloc(block * DRS_MAX_COALESCE);
  if (r != hipSuccess)
    return fail(e, r == hipErrorOutOfMemory ? DRS_ERR_OOM : DRS_ERR_HIP, "per-call input blocks of a launch set: %s", hipGetErrorString(r));
  if (need_h) s.h_multi = std::move(h);
  if (need_d) {
    s.d_multi = std::move(d);
    s.mq.assign(DRS_MAX_COALESCE, Batch());
    for (int i = 0; i < DRS_MAX_COALESCE; ++i) view_as(s.mq[i], e->blk, s.d_multi + (size_t)i * block);
  }
  return DRS_OK;
}

// Convert one query into `b`.  pinned: the slot's pinned block -- in_place, `b` is a view of that block (or of its HBM twin,
// which finish_inputs copies it to) and nothing is copied here; else `b` gets per-array copies from it (copy mode 0).
// No pinned block (drs_stage_batch): the pass runs into temporaries, since a failure part-way (index range on table 3)
// must leave a previously staged batch exactly as it was.
static int32_t stage_into(drs_engine* e, Batch& b, const QueryIn& q, hipStream_t stream, void* pinned, bool in_place = false) {
  const BlockLayout& L = e->blk;
  const int32_t n = q.bs;
  int32_t rc;
  if ((rc = check_bs(e, -1, n))) return rc;
  if (!q.ids && (!q.idx_list || !q.n_idx_list || !q.len_list)) return fail(e, DRS_ERR_BAD_ARG, "null index/length arrays");
  if ((rc = check_dense(e, -1, q.dense, n))) return rc;
  std::vector<int32_t> tmp_idx, tmp_off;
  BlockView v;
  if (pinned) {
    v = view_block(L, pinned);
  } else {
    tmp_idx.resize(L.idx_elems());
    tmp_off.resize(L.off_elems());
    v = BlockView{nullptr, tmp_idx.data(), tmp_off.data()};
  }
  HostPool* pool = pinned ? host_pool(e) : nullptr;
  // zero-copy path: the dense rows' copy into the pinned block rides along as one more work item
  const int n_items = e->T + (in_place && e->m_den > 0 && n > 0 ? 1 : 0);
  std::vector<ConvRes> res((size_t)e->T);
  auto item = [&](int t) { convert_item(e, q, t, v, pinned ? b.h_off.data() : nullptr, res.data()); };
  int64_t work = 0;
  for (int t = 0; t < e->T; ++t) work += q.n_idx(t) > 0 ? q.n_idx(t) : 0;
  if (pool && work >= 32768) pool->run(n_items, item);
  else for (int i = 0; i < n_items; ++i) item(i);
  if ((rc = seal_query(e, b, q, res.data(), -1))) {
    if (pinned) { b.staged = false; b.n_samples = 0; }   // the slot's pinned block was overwritten: nothing valid in it
    return rc;
  }
  if (in_place) return DRS_OK;   // the converted inputs are already where the kernels (or the one DMA copy) will read them
  if (!pinned) memcpy(b.h_off.data(), v.off, L.off_bytes);
  // copy only what is used of each table's index row
  for (int t = 0; t < e->T; ++t)
    if (q.n_idx(t) > 0)
      HIP_TRY(e, hipMemcpyAsync(b.idx + (size_t)t * L.cap, v.idx + (size_t)t * L.cap, sizeof(int32_t) * (size_t)q.n_idx(t), hipMemcpyHostToDevice, stream));
  HIP_TRY(e, hipMemcpyAsync(b.off, v.off, L.off_bytes, hipMemcpyHostToDevice, stream));
  if (e->m_den > 0 && n > 0) {
    const float* src = q.dense;
    if (pinned) {
      memcpy(v.dense, q.dense, sizeof(float) * (size_t)n * e->m_den);
      src = v.dense;
    }
    HIP_TRY(e, hipMemcpyAsync(b.dense, src, sizeof(float) * (size_t)n * e->m_den, hipMemcpyHostToDevice, stream));
  }
  if (!pinned) HIP_TRY(e, hipStreamSynchronize(stream));
  return DRS_OK;
}

static int32_t forward_query_async(drs_engine* e, int32_t slot, const QueryIn& q) {
  int32_t rc = check_handle(e, true);
  if (rc) return rc;
  if (slot < 0 || slot >= e->n_slots) return fail(e, DRS_ERR_BAD_ARG, "slot %d of %d", slot, e->n_slots);
  Slot& s = e->slots[slot];
  const int32_t bs = q.bs;
  if (s.busy && (rc = wait_slot(e, s, nullptr))) return rc;
  // the copies below must go on the stream the job's MLP side will use
  if (bs >= 0) s.stream = job_stream(e, s, padded_rows(bs));
  // how the converted inputs reach the kernels: 1 = read in place from the pinned block over PCIe
  // (no copy: best for small queries, kernel-issued PCIe reads top out near 20 GB/s), 2 = ONE
  // DMA copy of the packed block into its HBM twin (the copy engine moves it at PCIe rate beside
  // the kernels of the other slots), 3 = 2 when the query carries >= 128 KB, else 1 (default: 1)
  int mode = e->zero_copy_inputs;
  if (mode == 3) {
    int64_t bytes = (int64_t)bs * e->m_den * 4;
    for (int t = 0; t < e->T && (q.ids || q.n_idx_list); ++t) bytes += q.n_idx(t) * 4;
    mode = bytes >= 128 * 1024 ? 2 : 1;
  }
  size_t used = 0;
  bool need_off = false;
  // 1: no H2D copies at all -- convert straight into the slot's host-mapped pinned block and let the gather / first MLP
  // layer read it in place (795 KB per RMC1 query, read once); 2: the same block, then its used prefix to the HBM twin
  Batch& b = mode == 2 ? s.dc : mode == 1 ? s.zc : s.scratch;
  if ((rc = stage_into(e, b, q, s.stream, s.h_stage, mode != 0))) return rc;
  if (mode == 2) {
    used = e->blk.used_prefix(q.n_idx(e->T - 1));
    need_off = !e->sls_uniform || b.uniform_len < 0;
  }
  // the arrays are consumed; what is left are HIP calls
  if (e->launch_thread && bs > 0 && mode != 0) {
    if (!e->launcher) {          // (created on first use)
      e->launch_state.reset(new std::atomic<int>[e->slots.size()]);
      for (size_t i = 0; i < e->slots.size(); ++i) e->launch_state[i].store(0, std::memory_order_relaxed);
      e->launcher.reset(new Launcher(e));
    }
    s.busy = true;                 // (enqueue_forward sets it too; wait_slot needs it before that ran)
    s.launch_rc = 0;
    e->launcher->push(slot, mode, bs, used, need_off);
    return DRS_OK;
  }
  return finish_inputs(e, s, mode, bs, used, need_off);
}

}  // namespace eng
}  // namespace drs

extern "C" {

int32_t drs_stage_batch(drs_handle e, int32_t batch_id, int32_t n_samples, const float* h_dense,
                        const int64_t* const* h_idx, const int64_t* n_idx,
                        const int32_t* const* h_len) {
  int32_t rc = check_handle(e);
  if (rc) return rc;
  if (batch_id < 0 || batch_id >= e->n_batches) return fail(e, DRS_ERR_BAD_ARG, "batch_id %d of %d", batch_id, e->n_batches);
  // make sure no in-flight query still reads this batch
  for (auto& s : e->slots) if (s.busy) HIP_TRY(e, hipStreamSynchronize(s.stream));
  const QueryIn q = {n_samples, h_dense, h_idx, n_idx, h_len, nullptr, nullptr, 0, 0, 0};
  rc = stage_into(e, e->batches[batch_id], q, e->slots[0].stream, nullptr);
  if (rc == DRS_OK) e->batches[batch_id].weighted = false;   // new indices: the weights of the old ones are dropped (a failed call changed nothing)
  return rc;
}

// Per-sample weights of a staged batch (SparseLengthsWeightedSum): one fp32 per staged index, laid out like the indices
// ([T, cap]); a table without weights gets 1.0f throughout, so the kernels read one array whatever the mix.  The batch then
// makes every launch set it is part of a weighted one (launch_gather, plan_sls).
int32_t drs_stage_batch_weights(drs_handle e, int32_t batch_id, const float* const* h_wgt, const int64_t* n_idx) {
  int32_t rc = check_handle(e);
  if (rc) return rc;
  if (batch_id < 0 || batch_id >= e->n_batches) return fail(e, DRS_ERR_BAD_ARG, "batch_id %d of %d", batch_id, e->n_batches);
  if (e->kind == DRS_MODEL_DIN || e->kind == DRS_MODEL_DIEN)
    return fail(e, DRS_ERR_UNSUPPORTED, "drs_stage_batch_weights: DIN and DIEN pool their bags by the plain sum only");
  if (e->sls_pool) return fail(e, DRS_ERR_UNSUPPORTED, "drs_stage_batch_weights: \"sls_pool\" 1 has no weighted form (there is no weighted mean)");
  if (!h_wgt || !n_idx) return fail(e, DRS_ERR_BAD_ARG, "null weight/count arrays");
  Batch& b = e->batches[batch_id];
  if (!b.staged) return fail(e, DRS_ERR_STATE, "batch %d is not staged", batch_id);
  const BlockLayout& L = e->blk;
  for (int t = 0; t < e->T; ++t) {
    const int64_t staged = b.h_off[L.h_off_at(t, b.n_samples)];
    if (h_wgt[t] && n_idx[t] != staged)
      return fail(e, DRS_ERR_LENGTHS_SUM, "table %d: %lld weights for %lld staged indices", t, (long long)n_idx[t], (long long)staged);
  }
  // make sure no in-flight query still reads this batch
  for (auto& s : e->slots) if (s.busy) HIP_TRY(e, hipStreamSynchronize(s.stream));
  if (!b.wgt) {
    HIP_TRY(e, e->batch_mem[batch_id].wgt.alloc(L.idx_elems()));
    b.wgt = e->batch_mem[batch_id].wgt;
  }
  std::vector<float> ones;
  for (int t = 0; t < e->T; ++t) {
    const int64_t n = b.h_off[L.h_off_at(t, b.n_samples)];
    if (n <= 0) continue;
    const float* src = h_wgt[t];
    if (!src) {
      if ((int64_t)ones.size() < n) ones.assign((size_t)n, 1.0f);
      src = ones.data();
    }
    HIP_TRY(e, hipMemcpy(b.wgt + (size_t)t * L.cap, src, sizeof(float) * (size_t)n, hipMemcpyHostToDevice));
  }
  b.weighted = true;
  return DRS_OK;
}

int32_t drs_forward_inputs_async(drs_handle e, int32_t slot, int32_t bs, const float* h_dense,
                                 const int64_t* const* h_idx, const int64_t* n_idx,
                                 const int32_t* const* h_len) {
  return forward_query_async(e, slot, QueryIn{bs, h_dense, h_idx, n_idx, h_len, nullptr, nullptr, 0, 0, 0});
}

int32_t drs_run_queues_async(drs_handle e, int32_t slot, int32_t bs, const float* h_dense,
                             const int64_t* h_ids, int64_t ids_row_stride, int64_t n_idx_per_table,
                             const int32_t* h_lengths, int64_t len_row_stride) {
  if (!e) return fail(nullptr, DRS_ERR_BAD_ARG, "null handle");
  if (!h_ids || !h_lengths || n_idx_per_table < 0) return fail(e, DRS_ERR_BAD_ARG, "bad 2-D input arrays");
  return forward_query_async(e, slot, QueryIn{bs, h_dense, nullptr, nullptr, nullptr, h_ids, h_lengths, ids_row_stride, len_row_stride, n_idx_per_table});
}

// n queries' per-call arrays as ONE launch set: every query is narrowed / ENFORCE-checked into its
// own block of the slot's multi-block pinned allocation, the blocks cross the bus in one DMA copy on
// a copy stream of their own (so the copy of this set runs under the gathers of the sets before it),
// and the set is launched like a coalesced set of staged batches.
int32_t drs_run_queues_multi_async(drs_handle e, int32_t slot, int32_t n, const int32_t* bs,
                                   const float* const* h_dense, const int64_t* const* h_ids,
                                   const int64_t* ids_row_stride, const int64_t* n_idx_per_table,
                                   const int32_t* const* h_lengths, const int64_t* len_row_stride) {
  int32_t rc = check_handle(e);
  if (rc) return rc;
  if (slot < 0 || slot >= e->n_slots) return fail(e, DRS_ERR_BAD_ARG, "slot %d of %d", slot, e->n_slots);
  if (n < 1 || n > DRS_MAX_COALESCE) return fail(e, DRS_ERR_BAD_ARG, "1..%d queries per launch", DRS_MAX_COALESCE);
  if (!bs || !h_dense || !h_ids || !ids_row_stride || !n_idx_per_table || !h_lengths || !len_row_stride)
    return fail(e, DRS_ERR_BAD_ARG, "bad per-query array tables");
  Slot& s = e->slots[slot];
  if (s.busy && (rc = wait_slot(e, s, nullptr))) return rc;
  const BlockLayout& L = e->blk;
  if ((rc = multi_blocks(e, s, true))) return rc;
  if ((rc = copy_stream(e))) return rc;
  QueryIn qs[DRS_MAX_COALESCE];
  for (int i = 0; i < n; ++i) {
    if ((rc = check_bs(e, i, bs[i]))) return rc;
    if (!h_ids[i] || !h_lengths[i] || n_idx_per_table[i] < 0) return fail(e, DRS_ERR_BAD_ARG, "bad 2-D input arrays of query %d", i);
    if ((rc = check_dense(e, i, h_dense[i], bs[i]))) return rc;
    qs[i] = QueryIn{bs[i], h_dense[i], nullptr, nullptr, nullptr, h_ids[i], h_lengths[i], ids_row_stride[i], len_row_stride[i], n_idx_per_table[i]};
  }
  // host pass: ONE fork-join over the tables (and dense rows) of every query of the set
  const int T = e->T, per_q = T + 1;
  std::vector<ConvRes> res((size_t)n * T);
  auto item = [&](int k) {
    const int i = k / per_q;
    convert_item(e, qs[i], k % per_q, view_block(L, s.h_multi + (size_t)i * L.padded), s.mq[i].h_off.data(), res.data() + (size_t)i * T);
  };
  host_pool(e)->run(n * per_q, item);
  const Batch* bts[DRS_MAX_COALESCE];
  int64_t Mv = 0;
  size_t used[DRS_MAX_COALESCE];
  bool need_off[DRS_MAX_COALESCE];
  for (int i = 0; i < n; ++i) {
    Batch& b = s.mq[i];
    b.weighted = false;       // (the slot's last set may have been a device set with per-sample weights: the host arrays carry none)
    if ((rc = seal_query(e, b, qs[i], res.data() + (size_t)i * T, i))) {
      for (int k = 0; k < n; ++k) { s.mq[k].staged = false; s.mq[k].n_samples = 0; }
      return rc;
    }
    bts[i] = &b;
    Mv += padded_rows(bs[i]);
    used[i] = L.used_prefix(n_idx_per_table[i]);
    need_off[i] = !e->sls_uniform || b.uniform_len < 0;
  }
  if ((rc = check_set_rows(e, Mv))) return rc;
  BlockCopy cp[2 * DRS_MAX_COALESCE];
  const int n_cp = plan_block_copies(L, L.padded, n, used, need_off, true, cp);
  for (int k = 0; k < n_cp; ++k)
    HIP_TRY(e, hipMemcpyAsync(s.d_multi + cp[k].at, s.h_multi + cp[k].at, cp[k].bytes, hipMemcpyHostToDevice, e->stream_h2d));
  if ((rc = order_behind_inputs(e, s, Mv))) return rc;
  return enqueue_forward(e, s, n, bts, bs);
}

int32_t drs_forward_inputs(drs_handle e, int32_t slot, int32_t bs, const float* h_dense,
                           const int64_t* const* h_idx, const int64_t* n_idx,
                           const int32_t* const* h_len, float* h_out) {
  int32_t rc = drs_forward_inputs_async(e, slot, bs, h_dense, h_idx, n_idx, h_len);
  if (rc) return rc;
  return wait_slot(e, e->slots[slot], h_out);
}

}  // extern "C"
