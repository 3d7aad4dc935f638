// libdrs_hip.so, host side: ONE launch set -- which kernels, on which streams, in which order (enqueue_forward), its completion
// (wait_slot), and the entry points on top: drs_forward*, drs_wait, drs_sync, drs_fetch_interaction, the operator-level calls.
#include "engine.h"
#include "mlp_stream.h"

namespace drs {
namespace eng {

int32_t mlp_ready(drs_engine* e, const Mlp& m, const char* name) {
  for (size_t i = 0; i < m.layers.size(); ++i)
    if (!m.layers[i].set) return fail(e, DRS_ERR_STATE, "%s layer %zu has no weights", name, i);
  return DRS_OK;
}

int act_of(const Mlp& m, int l) { return (l + 1 == m.sigmoid_layer) ? DRS_ACT_SIGMOID : DRS_ACT_RELU; }

// A layer big enough to deserve its own 2-D launch (many workgroups, W streamed once per
// 16-row slab would be too much traffic): RM3's 2560x1024.  RM1's 576x256 is not.
bool is_wide(const drs_engine* e, const Mlp& m, int l) {
  return e->mlp_split && (int64_t)m.ln[l] * m.ln[l + 1] >= e->mlp_wide_kn;
}

// "mlp_dtype" 2: layer l of m runs on the bf16 matrix cores -- as a launch of its own (gemm_bf16.hip), or inside DLRM's
// or NCF's one-launch form ("mlp_bf16_fuse" 1: dlrm_one_launch, mlp_ncf)
bool is_bf16(const drs_engine* e, const Mlp& m, int l) { return bf16_shape(e, m.ln[l], m.ln[l + 1]); }

void fill_chain(ChainArgs& c, const Mlp& m, int l0, int cnt, const float* x, int64_t ldx, int64_t M,
                float* y, int64_t ldy) {
  memset(&c, 0, sizeof c);
  c.x = x; c.ldx = ldx; c.M = M; c.n_layers = cnt; c.y = y; c.ldy = ldy;
  for (int i = 0; i <= cnt; ++i) c.width[i] = m.ln[l0 + i];
  for (int i = 0; i < cnt; ++i) {
    c.W[i] = m.layers[l0 + i].W;
    c.b[i] = m.layers[l0 + i].b;
    c.act[i] = act_of(m, l0 + i);
  }
}

// The stream the set's next MLP launch goes on.  "mlp_layout" 0: the set's own MLP stream.  1: wide-layer
// GEMMs of full launch sets on the gather stream, everything else on the set's MLP stream; when the kind
// changes inside a set, the new stream waits for an event recorded behind the set's previous launch.
hipError_t mlp_launch_stream(drs_engine* e, Slot& s, bool wide, int64_t M, hipStream_t* out) {
  hipStream_t want = s.stream;
  if (e->mlp_layout == 1 && e->shared_stream == 2 && wide && M > e->mlp_small_rows) want = e->stream_g;
  if (s.cur && s.cur != want) {
    hipEvent_t ev = s.ev_k[s.n_ev];
    s.n_ev = (s.n_ev + 1) & 3;
    hipError_t r = hipEventRecord(ev, s.cur);
    if (r == hipSuccess) r = hipStreamWaitEvent(want, ev, 0);
    if (r != hipSuccess) return r;
  }
  s.cur = want;
  *out = want;
  return hipSuccess;
}

// "mlp_layout" 1: a launch or copy that goes straight on s.stream (interaction, row copies, DIN attention, the
// output copy and flag write, the timing event) must sit behind the set's latest MLP launch, which may have gone
// on the gather's stream (a wide layer): bring the set back to s.stream first.  A no-op otherwise.
hipError_t rejoin_stream(drs_engine* e, Slot& s) {
  hipStream_t st;
  return mlp_launch_stream(e, s, false, 0, &st);
}


// Run all layers of `m` on x -> y.  A huge layer and a bf16 layer ("mlp_dtype" 2) run as their own 2-D launch; runs of
// ordinary layers between them are fused into one LDS-resident chain.  Segment outputs that are not
// the final one ping-pong between s.H and s.Hb.  first (optional): the caller's plan of layer 0 alone.
int32_t run_mlp(drs_engine* e, Slot& s, const Mlp& m, const float* x, int64_t ldx, int64_t M, float* y, int64_t ldy,
                const Done* done = nullptr, const XSrc* xs = nullptr, const MlpPlan* first = nullptr) {
  const int n_layers = (int)m.layers.size();
  const float* in = x;
  int64_t ldin = ldx;
  for (int l0 = 0, cnt = 1; l0 < n_layers; l0 += cnt) {
    MlpPlan own;
    // layers [l0, l0 + n) as one chain; n == 0: layer l0 alone
    auto plan = [&](int n) {
      const bool last = l0 + (n ? n : 1) == n_layers;
      float* out = last ? y : (in == s.H ? s.Hb : s.H);
      const int64_t ldo = last ? ldy : e->ldH;
      const Done* d = last ? done : nullptr;
      const XSrc* x0 = l0 == 0 ? xs : nullptr;
      if (!n)
        return plan_layer(in, ldin, M, m.ln[l0], m.layers[l0].W, m.layers[l0].b, m.ln[l0 + 1], act_of(m, l0), out, ldo,
                          e->tune, d, x0, &own, is_bf16(e, m, l0) ? m.layers[l0].Wb : nullptr);
      ChainArgs c;
      fill_chain(c, m, l0, n, in, ldin, M, out, ldo);
      return plan_chains(c, nullptr, e->tune, d, x0, nullptr, nullptr, &own);
    };
    const bool given = l0 == 0 && first;
    cnt = 0;
    auto alone = [&](int l) { return is_wide(e, m, l) || is_bf16(e, m, l); };
    if (!given && !alone(l0))
      while (l0 + cnt < n_layers && cnt < DRS_MAX_CHAIN && !alone(l0 + cnt)) ++cnt;
    while (cnt > 0 && !plan(cnt)) --cnt;   // the longest run that a chain kernel holds, else the layer alone
    const bool ok = given || cnt > 0 || plan(0);
    cnt = cnt > 0 ? cnt : 1;
    const MlpPlan& p = given ? *first : own;
    hipStream_t st = s.stream;
    HIP_TRY(e, mlp_launch_stream(e, s, is_wide(e, m, l0), M, &st));
    if (!ok) return fail(e, DRS_ERR_HIP, "no kernel takes the %dx%d layer %d", m.ln[l0], m.ln[l0 + 1], l0);
    HIP_TRY(e, launch_plan(p, e->tune, st));
    in = p.a.y; ldin = p.a.ldy;
  }
  return DRS_OK;
}

// What a one-launch form asks of an MLP's layers: none wide; under "mlp_dtype" 2 which are bf16 layers, each with its twin.
struct LayerScan {
  bool wide = false, bf16 = false, twins = true;
  const uint16_t* wb[DRS_MAX_CHAIN] = {};   // per layer its bf16 twin (a bf16 layer) or null
};
LayerScan scan_layers(const drs_engine* e, const Mlp& m) {
  LayerScan r;
  for (int l = 0; l < (int)m.layers.size() && l < DRS_MAX_CHAIN; ++l) {
    r.wide = r.wide || is_wide(e, m, l);
    if (!is_bf16(e, m, l)) continue;
    r.bf16 = true;
    r.twins = r.twins && (r.wb[l] = m.layers[l].Wb);
  }
  return r;
}
bool bf16_fuse_on(const drs_engine* e) { return e->mlp_bf16_fuse && e->mlp_dtype == DRS_MLP_BF16; }

// DLRM: bottom MLP, interaction and top MLP of a 16-row slab in ONE launch (the slab's dense_out never waits for a kernel
// boundary): fusing on, enough rows, no wide layer, chains of at most DRS_MAX_CHAIN layers, slabs that fit LDS.  "cat":
// the top chain reads the buffer the bottom chain wrote; "dot": the kernel computes T.T^T in LDS between the chains.
// All layers fp32: a stream kernel or chain_kernel (plan_chains).  Some of them bf16 layers: fused_bf16_kernel, under
// "mlp_bf16_fuse" 1 with "mlp_dtype" 2 and every bf16 layer with its twin.  false: the set runs launch by launch.
bool dlrm_one_launch(const drs_engine* e, const Slot& s, int64_t Mv, float* out, const Done* dp, const XSrc* xs, MlpPlan* p) {
  if (!e->mlp_fuse || Mv < e->mlp_fuse_rows || e->kind != DRS_MODEL_DLRM) return false;
  const int nb = (int)e->bot.layers.size(), nt = (int)e->top.layers.size();
  if (nb < 1 || nt < 1 || nb > DRS_MAX_CHAIN || nt > DRS_MAX_CHAIN) return false;
  const LayerScan sa = scan_layers(e, e->bot), sb = scan_layers(e, e->top);
  if (sa.wide || sb.wide) return false;
  const bool cat = e->interaction_op == DRS_INTERACT_CAT;
  ChainArgs a, b;
  fill_chain(a, e->bot, 0, nb, nullptr, e->m_den, Mv, s.T, e->ldT);
  fill_chain(b, e->top, 0, nt, cat ? s.T : s.R, cat ? e->ldT : e->ldR, Mv, out, e->n_out);
  const DotArgs dot = {s.T, e->ldT, e->T + 1, e->D, e->itself, s.R, e->ldR};
  if (!sa.bf16 && !sb.bf16) return plan_chains(a, &b, e->tune, dp, xs, cat ? nullptr : &dot, nullptr, p);
  if (!bf16_fuse_on(e) || !sa.twins || !sb.twins) return false;
  return plan_fused_bf16(a, b, sa.wb, sb.wb, cat ? nullptr : &dot, dp, xs, p);
}

// shared_stream: 1 = one stream for everything (launch sets strictly back to back);
// 0 = one stream per slot; 2 = pipelined: every gather on stream_g, everything else on the
// first slot's stream behind an event, so the HBM-bound gather of set i+1 runs under the
// latency-bound MLP of set i and the gathers themselves never overlap each other.
void apply_stream_mode(drs_engine* e) {
  // pipelined mode: the MLP launches may alternate between `mlp_streams` streams, so that the
  // latency-bound tail of one set's MLP launch (completion hand-off: one workgroup active)
  // overlaps the start of the next set's
  const int nm = e->mlp_streams < 1 ? 1 : (e->mlp_streams > (int)e->slots.size() ? (int)e->slots.size() : e->mlp_streams);
  int k = 0;
  for (auto& s : e->slots) {
    if (e->shared_stream == 2) s.stream = e->slots[k % nm].own_stream;
    else s.stream = e->shared_stream ? e->slots[0].own_stream : s.own_stream;
    s.base_stream = s.stream;
    s.gather_stream = e->shared_stream == 2 ? e->stream_g : s.stream;
#ifdef DRS_LAB
    if (e->shared_stream == 2 && e->gather_streams == 2 && e->stream_g2 && (k & 1)) s.gather_stream = e->stream_g2;
#endif
    ++k;
  }
}

// the stream the MLP side of a job of Mv virtual rows goes on (see enqueue_forward)
hipStream_t job_stream(const drs_engine* e, const Slot& s, int64_t Mv) {
  return (e->shared_stream == 2 && Mv <= e->mlp_small_rows) ? s.own_stream : s.base_stream;
}
// ... and the stream its gather goes on: a small set runs entirely on the slot's own stream (no
// cross-stream event; short gathers of different slots may overlap -- they are latency-bound,
// by PCIe when the inputs are read in place from host memory)
hipStream_t job_gather_stream(const drs_engine* e, const Slot& s, int64_t Mv) {
  return (e->shared_stream == 2 && Mv <= e->mlp_small_rows && !e->small_piped) ? s.own_stream : s.gather_stream;
}


static int32_t weights_ready(drs_engine* e) {
  for (int t = 0; t < e->T; ++t)
    if (!e->table_set[t]) return fail(e, DRS_ERR_STATE, "table %d has no data", t);
  int32_t rc;
  if ((rc = mlp_ready(e, e->bot, "bottom")) || (rc = mlp_ready(e, e->top, "top")) ||
      (rc = mlp_ready(e, e->fin, "final")))
    return rc;
  for (auto& tk : e->tasks)
    if ((rc = mlp_ready(e, tk, "task"))) return rc;
  for (auto& au : e->att)
    if ((rc = mlp_ready(e, au, "attention"))) return rc;
  for (auto& rn : e->rnn)
    if ((rc = mlp_ready(e, rn, "rnn"))) return rc;
  return DRS_OK;
}

// e->d_att: {W, b} of the first `layers` layers (0: all) of every unit, as a device table of pointers
static hipError_t upload_weight_table(drs_engine* e, const std::vector<Mlp>& units, size_t layers) {
  std::vector<const float*> hp;
  for (auto& u : units)
    for (size_t l = 0; l < (layers ? layers : u.layers.size()); ++l) { hp.push_back(u.layers[l].W); hp.push_back(u.layers[l].b); }
  hipError_t r = e->d_att.alloc(hp.size());
  if (r == hipSuccess) r = hipMemcpy(e->d_att, hp.data(), sizeof(float*) * hp.size(), hipMemcpyHostToDevice);
  return r;
}

// The DIEN recurrence's and the DIN attention units' weights in the form their kernels read: rebuilt after drs_set_fc
// changed them (att_dirty).  (drs_set_fc is synchronous; nothing of this engine is in flight while weights change)
static int32_t pack_weights(drs_engine* e) {
  if (!e->att_dirty) return DRS_OK;
  if (!e->rnn.empty()) {
    const int H = e->rnn[0].ln[1];
    if (!e->d_att) {
      HIP_TRY(e, upload_weight_table(e, e->rnn, 2));
      HIP_TRY(e, e->d_att_packed.alloc((size_t)dien_packed_floats(e->D, H)));
    }
    HIP_TRY(e, launch_dien_pack(e->d_att, e->d_att_packed, e->D, H, nullptr));
    HIP_TRY(e, hipStreamSynchronize(nullptr));
  } else if (!e->att.empty() && e->din_any) {
    // any-shape units (din_any.hip): the kernel reads the layers where drs_set_fc put them
    if (!e->d_att) {
      HIP_TRY(e, upload_weight_table(e, e->att, 0));
      HIP_TRY(e, e->d_att_ln.alloc(e->att[0].ln.size()));
      HIP_TRY(e, hipMemcpy(e->d_att_ln, e->att[0].ln.data(), sizeof(int32_t) * e->att[0].ln.size(), hipMemcpyHostToDevice));
    }
  } else if (!e->att.empty()) {
    const int U = (int)e->att.size(), h = e->att[0].ln[1];
    if (!e->d_att) {
      HIP_TRY(e, upload_weight_table(e, e->att, 2));
      HIP_TRY(e, e->d_att_packed.alloc((size_t)U * din_unit_stride(e->D, h)));
    }
    HIP_TRY(e, launch_din_pack(e->d_att, e->d_att_packed, U, e->D, h, nullptr));
    HIP_TRY(e, hipStreamSynchronize(nullptr));
  } else {
    return DRS_OK;
  }
  e->att_dirty = false;
  return DRS_OK;
}

// One launch set being enqueued: what its steps hand on to each other.
struct SetCtx {
  drs_engine* e;
  Slot& s;
  QTable q;
  const Batch* qb[DRS_MAX_COALESCE];
  int64_t Mv;
  int32_t c;              // valid samples
  hipStream_t gstream;    // the gather's stream
  bool piped, joined;     // does s.stream differ from it / has it been made to wait for the gather yet?
  bool din_fused;
  Done done;
  const Done* dp;         // the set's completion hand-off (zero copy), or null
  float* out;
  bool out_dma;
  XSrc xs;                // the queries' dense rows
  hipError_t join() {
    if (joined) return hipSuccess;
    joined = true;
    return hipStreamWaitEvent(s.stream, s.ev_sls, 0);
  }
};

// layout of the set: zero-sized queries take no rows
static int32_t lay_out_set(SetCtx& x, int n, const Batch* const* bts, const int32_t* bss) {
  QTable& q = x.q;
  memset(&q, 0, sizeof q);
  int32_t v = 0, c = 0;
  for (int i = 0; i < n; ++i) {
    if (bss[i] < 0 || bss[i] > bts[i]->n_samples)
      return fail(x.e, DRS_ERR_BAD_ARG, "bs=%d outside [0, %d]", bss[i], bts[i]->n_samples);
    x.s.q_bs[i] = bss[i];
    x.s.q_vstart[i] = v;
    if (bss[i] == 0) continue;
    x.qb[q.n_q] = bts[i];
    q.vstart[q.n_q] = v;
    q.cum[q.n_q] = c;
    q.bs[q.n_q] = bss[i];
    q.n_q++;
    v += (bss[i] + 63) / 64 * 64;   // whole 64-row MLP blocks per query
    c += bss[i];
  }
  q.vstart[q.n_q] = v;
  q.cum[q.n_q] = c;
  if (v > x.e->max_rows) return fail(x.e, DRS_ERR_BAD_ARG, "%d coalesced rows exceed the slot capacity %lld", v, (long long)x.e->max_rows);
  x.Mv = v;
  x.c = c;
  return DRS_OK;
}

// The gather (the fused DIN launch: gather + attention units) on the gather's stream.
static int32_t launch_gather(SetCtx& x) {
  drs_engine* e = x.e;
  Slot& s = x.s;
  const QTable& q = x.q;
  const int64_t Mv = x.Mv;
  log_launch(e->tune.log, "set[%d queries, %d rows, gather on %s, mlp on %s]", q.n_q, (int)Mv,
             job_gather_stream(e, s, Mv) == e->stream_g ? "stream_g" : "own", s.stream == s.own_stream ? "own" : "shared");
  const hipStream_t gstream = x.gstream = job_gather_stream(e, s, Mv);
  const bool prof = e->profiling >= 1;
  const bool evts = e->profiling >= 2;
  const bool piped = x.piped = gstream != s.stream;
  if (evts) HIP_TRY(e, hipEventRecord(s.ev[0], gstream));

  SlsArgs a;
  memset(&a, 0, sizeof a);
  a.tables = e->tables; a.tab_off = e->d_tab_off; a.tab_rows = e->d_tab_rows;
  a.q = q;
  for (int i = 0; i < q.n_q; ++i) {
    a.idx[i] = x.qb[i]->idx;
    a.off[i] = x.qb[i]->off;
    a.wgt[i] = x.qb[i]->weighted ? x.qb[i]->wgt : nullptr;   // (staged batches, and device sets that carry weights: drs_device_weights.h; the host per-call paths carry none)
    a.uniform_len[i] = e->sls_uniform ? x.qb[i]->uniform_len : -1;
  }
  a.idx_stride = e->blk.cap; a.off_stride = (int64_t)e->blk.off_stride();
  a.out = s.T; a.ld_out = e->ldT; a.col0 = e->kind == DRS_MODEL_NCF ? 0 : e->w0;
  a.T = e->T; a.D = e->D; a.err = reinterpret_cast<int32_t*>(s.d_err.get());
  a.ts = prof ? s.d_ts : nullptr;
  a.ln_mul = e->i8l.mul; a.ln_shift = e->i8l.shift; a.ln_pad = e->i8l.pad;   // ("table_int8_lines" / "table_int4_lines": zeros for every other layout)
  a.tab_scale = e->table_dtype == DRS_TABLE_FP8_E4M3 ? e->d_tab_scale : nullptr;   // (read by the fp8 instances alone)
  a.pool = e->sls_pool;      // ("sls_pool": DIN and DIEN refuse 1, so the fused DIN launch never sees it)
  // short bags (W&D / NCF: one lookup per table) take the sequential lane-group-per-bag form (plan_sls); the queries'
  // own bag lengths count here, also when "sls_uniform" 0 keeps them from the kernels
  bool short_bags = true;
  for (int i = 0; i < q.n_q; ++i) short_bags = short_bags && x.qb[i]->uniform_len >= 0 && x.qb[i]->uniform_len <= e->sls_short_bag;
  const SlsPlan plan = plan_sls(a, e->sls_exact, short_bags, e->tune, e->table_dtype);
  // DIN, default mode: the attention units are fused into the gather launch (din.hip)
  const bool din_fused = x.din_fused = e->kind == DRS_MODEL_DIN && !e->sls_exact && e->din_fused && !e->din_any &&
                                       din_fused_applicable(e->D, e->att[0].ln[1]);
  s.ts_blocks = prof ? (din_fused ? din_fused_grid(a, e->tune) : plan.grid) : 0;
  if (prof) {
    // algorithmic bytes of THIS launch (rows + int32 indices + length + pooled output
    // per bag), so that achieved GB/s = sum(bytes) / sum(duration) over exactly the timed launches
    int64_t bytes = 0;
    for (int i = 0; i < q.n_q; ++i)
      for (int t = 0; t < e->T; ++t)
        bytes += (int64_t)x.qb[i]->h_off[e->blk.h_off_at(t, q.bs[i])] * (table_row_bytes(e->table_dtype, e->D) + 4 + (x.qb[i]->weighted ? 4 : 0)) +
                 (int64_t)q.bs[i] * (4 + (int64_t)e->D * 4);
    // (the fused DIN launch writes the 4 D floats of the top MLP's input row per sample instead
    // of T pooled vectors)
    if (din_fused) bytes -= (int64_t)x.c * (e->T - 4) * e->D * 4;
    s.ts_bytes = bytes;
  }
  // pipelined mode: the event the MLP stream waits for is recorded by the gather dispatch itself
  // (hipExtLaunchKernel's stop event = the packet's completion signal): no marker packet sits
  // between consecutive gathers (a hipEventRecord there costs ~2 us per set)
  if (din_fused)
    HIP_TRY(e, launch_din_fused(a, e->att[0].ln[1], e->d_att_packed, s.R, e->ldR, e->tune, gstream, piped ? s.ev_sls : nullptr));
  else
    HIP_TRY(e, launch_sls(a, plan, e->tune, gstream, piped ? s.ev_sls : nullptr));
  if (evts) HIP_TRY(e, hipEventRecord(s.ev[1], gstream));
  x.joined = !piped;
  return DRS_OK;
}

// last kernel of the job: outputs either go straight to host-mapped pinned memory
// followed by a flag store (zero copy, no stream sync), or to a device buffer + memcpy
static void arm_hand_off(SetCtx& x) {
  drs_engine* e = x.e;
  Slot& s = x.s;
  s.seq += 1;
  if (s.seq == 0) s.seq = 1;
  Done& done = x.done;
  memset(&done, 0, sizeof done);
  done.counter = s.d_counter; done.host_flag = s.dm_out; done.host_err = s.dm_out + 1;
  done.dev_err = s.d_err; done.seq = s.seq;
  if (e->profiling >= 1 && e->zero_copy) { done.ts = s.d_ts; done.ts_blocks = (uint32_t)s.ts_blocks; done.span_acc = s.d_span_acc; done.host_span = s.dm_span; }
  x.dp = e->zero_copy ? &done : nullptr;
  x.out = s.d_out;          // kernels store to the device buffer; see Done::host_out
  done.dev_out = s.d_out; done.host_out = reinterpret_cast<float*>(s.dm_out + kOutOffset);
  done.out_words = (uint32_t)(x.Mv * e->n_out);
  // "out_dma": the outputs leave through a copy-engine transfer queued behind the last kernel, and the flag through
  // a stream-ordered 32-bit write behind that -- the last workgroup then hands over the error word only
  x.out_dma = e->zero_copy && e->out_dma && (int64_t)done.out_words * 4 >= e->out_dma;
  if (x.out_dma) { done.out_words = 0; done.host_flag = nullptr; }
  memset(&x.xs, 0, sizeof x.xs);
  x.xs.q = x.q;
  for (int i = 0; i < x.q.n_q; ++i) x.xs.x[i] = x.qb[i]->dense;
}

// DIEN: the two recurrent layers over the pooled behaviour rows -> top MLP input R [rows, H + 3D] -> top MLP
static int32_t mlp_dien(SetCtx& x) {
  drs_engine* e = x.e;
  Slot& s = x.s;
  HIP_TRY(e, x.join());
  const float* rw[8];
  for (int l = 0; l < 2; ++l) {
    rw[4 * l + 0] = e->rnn[l].layers[0].W; rw[4 * l + 1] = e->rnn[l].layers[0].b;
    rw[4 * l + 2] = e->rnn[l].layers[1].W; rw[4 * l + 3] = e->rnn[l].layers[1].b;
  }
  // the top MLP in the recurrence's own launch when it fits ("dien_fuse_top", default on): one workgroup per 16
  // samples instead of two, one launch less per set
  const int Hh = e->rnn[0].ln[1], c = x.c;
  DienTop tp;
  memset(&tp, 0, sizeof tp);
  const int nt = (int)e->top.layers.size();
  // 3: the any-shape form (din_any.hip) -- every shape without an instance in dien.hip, or on request
  const int form = dien_applicable(e->D, Hh) ? e->dien_mfma : 3;
  const bool mfma_form = form != 3 && form && Hh % 16 == 0;
  if (e->dien_fuse_top && mfma_form && nt >= 1 && nt <= 4 && e->top.layers[0].packed &&
      dien_top_fusable(nt, e->top.ln.data(), Hh) && e->top.ln[0] == Hh + 3 * e->D) {
    tp.n = nt; tp.sc1 = x.dp ? 1 : 0; tp.out = x.out; tp.ldo = e->n_out;
    for (int l = 0; l < nt; ++l) {
      const Layer& L = e->top.layers[l];
      tp.Wp[l] = L.W + ((size_t)L.m * L.n + 63) / 64 * 64; tp.b[l] = L.b;
      tp.K[l] = e->top.ln[l]; tp.N[l] = e->top.ln[l + 1]; tp.act[l] = act_of(e->top, l);
    }
    tp.kmax = dien_top_kmax(nt, e->top.ln.data());
  }
  log_launch(e->tune.log, "%s<%d,%d%s>[%d wg]", form == 3 ? "dien_rnn_any_kernel" : mfma_form ? "dien_rnn_mfma_kernel" : "dien_rnn_kernel",
             e->D, Hh, tp.n ? ",top" : "", form == 3 ? c : mfma_form ? (c + 15) / 16 : (c + 3) / 4);
  HIP_TRY(e, launch_dien_rnn(s.T, e->ldT, x.q, e->T, e->D, Hh, e->d_att_packed, rw, form, s.R,
                             e->ldR, s.stream, tp.n ? &tp : nullptr, x.dp));
  return tp.n ? DRS_OK : run_mlp(e, s, e->top, s.R, e->ldR, x.Mv, x.out, e->n_out, x.dp);
}

// DIN: attention units over the pooled rows -> top MLP input R [rows, 4D] -> top MLP (all ReLU)
static int32_t mlp_din(SetCtx& x) {
  drs_engine* e = x.e;
  Slot& s = x.s;
  const int64_t Mv = x.Mv;
  HIP_TRY(e, x.join());
  if (e->din_any) {
    log_launch(e->tune.log, "din_attention_any_kernel[%lld wg]", (long long)Mv);
    HIP_TRY(e, launch_din_attention_any(s.T, e->ldT, Mv, e->T, e->D, (int)e->att[0].ln.size(), e->d_att_ln, e->d_att, e->din_maxw,
                                        s.R, e->ldR, s.stream));
  } else if (!x.din_fused) {
    log_launch(e->tune.log, "din_attention_kernel[%lld wg]", (long long)((Mv + 3) / 4));
    HIP_TRY(e, launch_din_attention(s.T, e->ldT, Mv, e->T, e->D, e->att[0].ln[1], e->d_att_packed, s.R, e->ldR, s.stream));
  }
  return run_mlp(e, s, e->top, s.R, e->ldR, Mv, x.out, e->n_out, x.dp);
}

// NCF: mf = Sum(sls0, sls1); mlp = Concat(sls2, sls3) -> MLP; Concat(mf, mlp_out) -> FC+Relu
static int32_t mlp_ncf(SetCtx& x) {
  drs_engine* e = x.e;
  Slot& s = x.s;
  const int64_t Mv = x.Mv;
  const int D = e->D;
  const int wl = e->top.ln.back();
  const int64_t ldc = D + wl;
  HIP_TRY(e, x.join());
  // one launch when it fits: Sum, MLP branch and predictor of a 16-row slab in the stream kernel
  const int nt = (int)e->top.layers.size();
  if (e->mlp_fuse && nt >= 1 && nt <= DRS_MAX_CHAIN && e->fin.layers.size() == 1) {
    ChainArgs ca, cb;
    fill_chain(ca, e->top, 0, nt, s.T + 2 * D, e->ldT, Mv, s.H2 + D, ldc);
    fill_chain(cb, e->fin, 0, 1, s.H2, ldc, Mv, x.out, e->n_out);
    const SumArgs sum = {s.T, e->ldT, 0, D, D, s.H2, ldc};
    const LayerScan st = scan_layers(e, e->top), sf = scan_layers(e, e->fin);
    MlpPlan p;
    // (... or, with "mlp_bf16_fuse" 1, in fused_bf16_sum_kernel when some of the layers are bf16 layers, each with its twin)
    const bool one = st.wide || sf.wide ? false
                     : !st.bf16 && !sf.bf16 ? plan_chains(ca, &cb, e->tune, x.dp, nullptr, nullptr, &sum, &p)
                     : bf16_fuse_on(e) && st.twins && sf.twins && plan_fused_bf16_sum(ca, cb, st.wb, sf.wb[0], sum, x.dp, &p);
    if (one) {
      HIP_TRY(e, launch_plan(p, e->tune, s.stream));
      return DRS_OK;
    }
  }
  log_launch(e->tune.log, "add_rows_kernel");
  HIP_TRY(e, launch_add_rows(s.T, e->ldT, s.T + D, e->ldT, s.H2, ldc, Mv, D, s.stream));
  int32_t rc;
  if ((rc = run_mlp(e, s, e->top, s.T + 2 * D, e->ldT, Mv, s.H2 + D, ldc))) return rc;
  return run_mlp(e, s, e->fin, s.H2, ldc, Mv, x.out, e->n_out, x.dp);
}

// DLRM, W&D, MT-WnD: bottom MLP (DLRM) beside the gather, interaction, top MLP (and MT-WnD's task heads)
static int32_t mlp_dense(SetCtx& x) {
  drs_engine* e = x.e;
  Slot& s = x.s;
  const int64_t Mv = x.Mv;
  float* out = x.out;
  int32_t rc;
  MlpPlan p;                   // the fused DLRM launch, or W&D's / MT-WnD's first top layer reading a split row
  bool split = false;          // (the latter: it reads the dense columns in place)
  s.split_last = false;
  const bool dot = e->kind == DRS_MODEL_DLRM && e->interaction_op == DRS_INTERACT_DOT;
  const float* top_in = dot ? s.R : s.T;
  const int64_t ld_top = dot ? e->ldR : e->ldT;
  if (!e->bot.layers.empty()) {
    bool fused = false;
    // "mlp_early": a small set of staged queries (gather on the slot's own stream, nothing else of the set there) whose
    // bottom + top MLP is ONE stream4_kernel launch: the launch goes on a second stream WITHOUT waiting for the gather,
    // runs its prologue and the bottom chain beside it and polls the slot's flag -- a 32-bit write queued behind the
    // gather -- before it fetches the pooled rows (mlp.hip, Done::wait_flag).  <= 512 rows: at most 32 workgroups spin.
#ifdef DRS_LAB
    if (e->mlp_early && e->shared_stream == 2 && !x.piped && x.gstream == s.own_stream && Mv <= 512 && x.dp && s.early_stream &&
        e->kind == DRS_MODEL_DLRM) {
      bool staged = true;
      for (int i = 0; i < x.q.n_q; ++i)
        staged = staged && x.qb[i] >= e->batches.data() && x.qb[i] < e->batches.data() + e->batches.size();
      x.done.wait_flag = staged ? s.d_gflag : nullptr;
      x.done.wait_val = staged ? s.seq : 0;
      // (a waiting launch is planned only where it can wait: plan_fused_bf16 takes none, this is the fp32 attempt alone)
      fused = staged && dlrm_one_launch(e, s, Mv, out, x.dp, &x.xs, &p);
      if (!fused) { x.done.wait_flag = nullptr; x.done.wait_val = 0; }
    }
    if (fused) {
      HIP_TRY(e, hipStreamWriteValue32(x.gstream, s.d_gflag, s.seq, 0));
      s.stream = s.early_stream;
      log_launch(e->tune.log, "early");
    }
#endif
    fused = fused || dlrm_one_launch(e, s, Mv, out, x.dp, &x.xs, &p);
    if (fused) {
      HIP_TRY(e, x.join());
      HIP_TRY(e, launch_plan(p, e->tune, s.stream));
      return DRS_OK;
    }
    if ((rc = run_mlp(e, s, e->bot, nullptr, e->m_den, Mv, s.T, e->ldT, nullptr, &x.xs))) return rc;
  } else {
    // W&D / MT-WnD: Concat(dense, pooled embeddings) feeds the first top layer.  When that layer goes to a GEMM form
    // that can read a split row ("gemm_split", gemm_plan) it takes the dense columns from the queries' own arrays;
    // otherwise the dense rows are copied in front of the embeddings first (so does a bf16 first layer: gemm_bf16_kernel
    // reads whole rows).
    if (e->gemm_split && !e->top.layers.empty() && is_wide(e, e->top, 0) && !is_bf16(e, e->top, 0)) {
      XSrc xsp = x.xs;
      xsp.ksplit = e->m_den;
      // (the layer's output as run_mlp would place it: the model's output, or s.H ahead of further layers)
      const bool one = e->top.layers.size() == 1, mt = e->kind == DRS_MODEL_MTWND;
      float* y = !one ? s.H : mt ? s.H3 : out;
      const int64_t ldy = !one ? e->ldH : mt ? e->top.ln.back() : e->n_out;
      split = plan_layer(top_in, ld_top, Mv, e->top.ln[0], e->top.layers[0].W, e->top.layers[0].b, e->top.ln[1], act_of(e->top, 0),
                         y, ldy, e->tune, one && !mt ? x.dp : nullptr, &xsp, &p);
    }
    s.split_last = split;
    if (!split) {
      log_launch(e->tune.log, "copy_rows_multi_kernel");
      HIP_TRY(e, launch_copy_rows_multi(x.xs, e->m_den, s.T, e->ldT, s.stream));
      s.cur = s.stream;          // ("mlp_layout" 1: a wide first layer routed to the gather's stream must wait for this copy)
    }
  }
  HIP_TRY(e, x.join());   // (the bottom MLP above ran beside the gather)
  if (dot) {
    HIP_TRY(e, rejoin_stream(e, s));
    log_launch(e->tune.log, "interact_dot_kernel[%lld wg]", (long long)((Mv + 3) / 4));
    HIP_TRY(e, launch_interact_dot(s.T, e->ldT, Mv, e->T + 1, e->D, e->itself, s.R, e->ldR, s.stream));
  }
  const MlpPlan* first = split ? &p : nullptr;
  if (e->kind != DRS_MODEL_MTWND) return run_mlp(e, s, e->top, top_in, ld_top, Mv, out, e->n_out, x.dp, nullptr, first);
  // shared top MLP (all ReLU) -> H3, then every task head reads H3 and writes its block of
  // the output row; the last head's last launch carries the completion hand-off
  const int wt = e->top.ln.back(), wo = e->tasks[0].ln.back();
  if ((rc = run_mlp(e, s, e->top, top_in, ld_top, Mv, s.H3, wt, nullptr, nullptr, first))) return rc;
  for (size_t k = 0; k < e->tasks.size(); ++k)
    if ((rc = run_mlp(e, s, e->tasks[k], s.H3, wt, Mv, out + k * wo, e->n_out, k + 1 == e->tasks.size() ? x.dp : nullptr)))
      return rc;
  return DRS_OK;
}

// the set's outputs to the host: behind its last launch, back on s.stream
static int32_t hand_off(SetCtx& x) {
  drs_engine* e = x.e;
  Slot& s = x.s;
  const int64_t Mv = x.Mv;
  HIP_TRY(e, rejoin_stream(e, s));     // ("mlp_layout" 1: the tail below is ordered behind a last launch on the gather's stream)
  if (e->profiling >= 2) {
    HIP_TRY(e, hipEventRecord(s.ev[2], s.stream));
    s.ev_pending = true;
  }
  if (!e->zero_copy) {
    HIP_TRY(e, hipMemcpyAsync(s.h_out + kOutOffset, s.d_out, sizeof(float) * (size_t)Mv * e->n_out,
                              hipMemcpyDeviceToHost, s.stream));
    HIP_TRY(e, hipMemcpyAsync(s.h_out + 1, s.d_err, sizeof(uint32_t), hipMemcpyDeviceToHost, s.stream));
  }
  if (x.out_dma) {
    log_launch(e->tune.log, "out_dma[%lld B]", (long long)(sizeof(float) * (size_t)Mv * e->n_out));
    // ... on the engine's copy stream, behind an event: queued on s.stream itself, the transfer (2 MB = ~40 us of PCIe
    // per MT-WnD set) held up the NEXT set's launches on that MLP stream -- the chip idled 13.5 % of the time
    // (profiles/r06_mtwnd_kernel_overlap_before.txt)
    HIP_TRY(e, hipEventRecord(s.ev_dma, s.stream));
    HIP_TRY(e, hipStreamWaitEvent(e->stream_dma, s.ev_dma, 0));
    HIP_TRY(e, hipMemcpyAsync(s.h_out + kOutOffset, s.d_out, sizeof(float) * (size_t)Mv * e->n_out,
                              hipMemcpyDeviceToHost, e->stream_dma));
    HIP_TRY(e, hipStreamWriteValue32(e->stream_dma, s.dm_out, s.seq, 0));
  }
  s.on_dma = x.out_dma;
  s.polled = e->zero_copy != 0;
  return DRS_OK;
}

// Enqueue n >= 1 coalesced queries (query i = first bs[i] samples of *bts[i]) as ONE set of
// launches on the slot's stream.
int32_t enqueue_forward(drs_engine* e, Slot& s, int n, const Batch* const* bts, const int32_t* bss) {
  if (n < 1 || n > DRS_MAX_COALESCE) return fail(e, DRS_ERR_BAD_ARG, "1..%d queries per launch, got %d", DRS_MAX_COALESCE, n);
  int32_t rc;
  if ((rc = weights_ready(e)) || (rc = pack_weights(e))) return rc;
  SetCtx x{e, s};
  if ((rc = lay_out_set(x, n, bts, bss))) return rc;
  s.last_n = n;
  s.last_bs = x.c;
  s.busy = true;
  s.polled = false;
  s.out_pass = false;            // (engine_device_outputs.hip sets it behind this call, for its own sets alone)
  if (x.c == 0) return DRS_OK;
  // Pipelined mode, small launch set (a single query: 256 rows = 16 MLP workgroups on a 256-CU
  // chip): its latency-bound MLP launch goes on the SLOT's own stream, so the MLP launches of
  // consecutive sets overlap each other instead of queueing on the one shared MLP stream
  // (one query per launch set: 23 k -> see DESIGN 3.5).  Full sets (8 queries, 128 workgroups)
  // keep the shared stream: there the extra concurrency only takes CUs from the gather.
  // Safe: a slot is reused only after its previous job was observed complete on the host.
  s.stream = job_stream(e, s, x.Mv);
  s.cur = nullptr;               // (the set's first MLP launch needs no event: join() orders it behind the gather)
  s.dlog.len = 0; s.dlog.text[0] = 0;
  // ("dispatch_log" 1: the launch functions note what they choose for this set -- drs_last_dispatch; off by default: four
  //  to eight vsnprintf per set are ~1 us of the ~11 us a small set costs the host)
  e->tune.log = e->dispatch_log ? &s.dlog : nullptr;
  e->tune.xbuf = s.xbuf; e->tune.xcnt = s.xcnt; e->tune.xbuf_rows = s.xrows; e->tune.xbuf_cols = s.xcols;
  // (both belong to THIS slot: launches made outside this function -- the operator-level entry points -- must not see them)
  struct TuneScope { Tune& t; ~TuneScope() { t.log = nullptr; t.xbuf = nullptr; t.xcnt = nullptr; } } tune_scope{e->tune};
  if ((rc = launch_gather(x))) return rc;
  arm_hand_off(x);
  if (e->kind == DRS_MODEL_DIEN) rc = mlp_dien(x);
  else if (e->kind == DRS_MODEL_DIN) rc = mlp_din(x);
  else if (e->kind == DRS_MODEL_NCF) rc = mlp_ncf(x);
  else rc = mlp_dense(x);
  return rc ? rc : hand_off(x);
}



int32_t wait_slot(drs_engine* e, Slot& s, float* h_out, int64_t h_cap) {
  if (!s.busy) return DRS_OK;
  if (e->launch_state) {
    // the job's launches may still be with the launcher thread
    std::atomic<int>& st = e->launch_state[&s - e->slots.data()];
    if (st.load(std::memory_order_acquire) != 0) {
      while (st.load(std::memory_order_acquire) == 1) __builtin_ia32_pause();
      st.store(0, std::memory_order_relaxed);
      if (s.launch_rc) {
        s.busy = false;
        const int32_t rc = s.launch_rc;
        s.launch_rc = 0;
        return fail(e, rc, "%s", s.launch_err.c_str());
      }
    }
  }
  // the caller's buffer must hold what was SUBMITTED on this slot (a mismatched bs
  // after a multi-query submit used to overflow the heap silently); the job stays in flight
  if (h_out && h_cap >= 0 && h_cap < (int64_t)s.last_bs * e->n_out)
    return fail(e, DRS_ERR_BAD_ARG, "output buffer holds %lld floats, the %d queries on this slot produce %lld",
                (long long)h_cap, s.last_n, (long long)s.last_bs * e->n_out);
  if (s.polled && s.last_bs > 0) {
    // spin on the flag the last kernel publishes (bounded: fall back to a stream sync)
    volatile uint32_t* flag = s.h_out;
    const auto t0 = std::chrono::steady_clock::now();
    uint64_t spins = 0;
    while (*flag != s.seq) {
      __builtin_ia32_pause();
      // 8 ranks on a node share its cores with each other's runtime threads: do not starve them
      if ((++spins & 0xfff) == 0) sched_yield();
      if ((spins & 0xfffff) == 0 &&
          std::chrono::steady_clock::now() - t0 > std::chrono::seconds(10)) {
        HIP_TRY(e, hipStreamSynchronize(s.stream));
        if (s.on_dma) HIP_TRY(e, hipStreamSynchronize(e->stream_dma));
        if (*flag != s.seq) {
          s.busy = false;
          return fail(e, DRS_ERR_HIP, "completion flag never arrived (seq %u, flag %u)", s.seq, *flag);
        }
      }
    }
    std::atomic_thread_fence(std::memory_order_acquire);
  } else {
    HIP_TRY(e, hipStreamSynchronize(s.stream));
  }
  if (s.out_pass) {
    // device outputs: the flag above is published by the set's last MLP kernel, BEFORE the output pass behind it reads
    // s.d_out and the error word -- and the next set on this slot may launch on another stream (job_stream goes by Mv)
    s.out_pass = false;
    HIP_TRY(e, hipEventSynchronize(s.ev_out));
  }
  s.busy = false;
  if (s.ev_pending) {
    HIP_TRY(e, hipEventSynchronize(s.ev[2]));
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, s.ev[0], s.ev[1]) == hipSuccess) { e->k_ms[DRS_KERNEL_SLS] += ms; e->k_n[DRS_KERNEL_SLS]++; e->k_bytes[DRS_KERNEL_SLS] += s.ts_bytes; }
    if (hipEventElapsedTime(&ms, s.ev[1], s.ev[2]) == hipSuccess) { e->k_ms[DRS_KERNEL_MLP] += ms; e->k_n[DRS_KERNEL_MLP]++; }
    s.ev_pending = false;
  }
  if (s.ts_blocks > 0) {
    uint64_t lo = ~0ull, hi = 0;
    if (s.polled) {
      lo = s.h_span[0]; hi = s.h_span[1];       // reduced on the device, see Done
    } else {
      HIP_TRY(e, hipMemcpy(s.h_ts.data(), s.d_ts, sizeof(uint64_t) * 2 * (size_t)s.ts_blocks, hipMemcpyDeviceToHost));
      for (int64_t i = 0; i < s.ts_blocks; ++i) {
        lo = s.h_ts[2 * i] < lo ? s.h_ts[2 * i] : lo;
        hi = s.h_ts[2 * i + 1] > hi ? s.h_ts[2 * i + 1] : hi;
      }
    }
    if (hi > lo) {
      e->k_ms[DRS_KERNEL_SLS_CLOCK] += (double)(hi - lo) / e->wall_clock_khz;
      e->k_n[DRS_KERNEL_SLS_CLOCK]++;
      e->k_bytes[DRS_KERNEL_SLS_CLOCK] += s.ts_bytes;
    }
    s.ts_blocks_done = s.ts_blocks;
    s.ts_blocks = 0;
  }
  if (s.last_bs > 0 && s.h_out[1] != 0) {
    const uint32_t bits = s.h_out[1];
    s.h_out[1] = 0;
    HIP_TRY(e, hipMemsetAsync(s.d_err, 0, sizeof(uint32_t), s.stream));
    HIP_TRY(e, hipStreamSynchronize(s.stream));
    if (bits & kErrMlpEarly) return fail(e, DRS_ERR_HIP, "mlp_early: the gather's flag never reached the MLP launch");
    if (bits & kErrLengths)    // (the device input pass, input_pass.hip: the device keeps one word, no position or value)
      return fail(e, DRS_ERR_LENGTHS_SUM, "device inputs: a negative length, sum(lengths) != len(indices), or a length that differs from the promised fixed_len");
    return fail(e, DRS_ERR_INDEX_RANGE, "an embedding index was out of range on the device");
  }
  if (h_out && s.last_bs > 0) {
    // queries sit at 16-row aligned virtual offsets: pack them back to back
    const float* src = reinterpret_cast<const float*>(s.h_out + kOutOffset);
    size_t o = 0;
    for (int i = 0; i < s.last_n; ++i) {
      memcpy(h_out + o, src + (size_t)s.q_vstart[i] * e->n_out, sizeof(float) * (size_t)s.q_bs[i] * e->n_out);
      o += (size_t)s.q_bs[i] * e->n_out;
    }
  }
  return DRS_OK;
}

// (hot = the per-call input path itself, which may have jobs with the launcher thread; every other
// entry point first lets that thread finish what it was handed)
int32_t check_handle(drs_engine* e, bool hot) {
  if (!e) return fail(nullptr, DRS_ERR_BAD_ARG, "null handle");
  if (!hot && e->launcher) e->launcher->drain();
  return set_device(e);
}


}  // namespace eng
}  // namespace drs

extern "C" {

int32_t drs_forward_async(drs_handle e, int32_t slot, int32_t batch_id, int32_t bs) {
  int32_t rc = check_handle(e);
  if (rc) return rc;
  if (slot < 0 || slot >= e->n_slots) return fail(e, DRS_ERR_BAD_ARG, "slot %d of %d", slot, e->n_slots);
  if (batch_id < 0 || batch_id >= e->n_batches || !e->batches[batch_id].staged)
    return fail(e, DRS_ERR_STATE, "batch %d is not staged", batch_id);
  Slot& s = e->slots[slot];
  if (s.busy && (rc = wait_slot(e, s, nullptr))) return rc;
  const Batch* bt = &e->batches[batch_id];
  return enqueue_forward(e, s, 1, &bt, &bs);
}

int32_t drs_forward_multi_async(drs_handle e, int32_t slot, int32_t n, const int32_t* batch_ids,
                                const int32_t* bs) {
  int32_t rc = check_handle(e);
  if (rc) return rc;
  if (slot < 0 || slot >= e->n_slots) return fail(e, DRS_ERR_BAD_ARG, "slot %d of %d", slot, e->n_slots);
  if (!batch_ids || !bs || n < 1 || n > DRS_MAX_COALESCE) return fail(e, DRS_ERR_BAD_ARG, "1..%d queries per launch", DRS_MAX_COALESCE);
  const Batch* bts[DRS_MAX_COALESCE];
  for (int i = 0; i < n; ++i) {
    if (batch_ids[i] < 0 || batch_ids[i] >= e->n_batches || !e->batches[batch_ids[i]].staged)
      return fail(e, DRS_ERR_STATE, "batch %d is not staged", batch_ids[i]);
    bts[i] = &e->batches[batch_ids[i]];
  }
  Slot& s = e->slots[slot];
  if (s.busy && (rc = wait_slot(e, s, nullptr))) return rc;
  return enqueue_forward(e, s, n, bts, bs);
}

int32_t drs_wait(drs_handle e, int32_t slot, float* h_out, int64_t h_out_floats) {
  int32_t rc = check_handle(e, true);
  if (rc) return rc;
  if (slot < 0 || slot >= e->n_slots) return fail(e, DRS_ERR_BAD_ARG, "slot %d of %d", slot, e->n_slots);
  if (h_out && h_out_floats < 0) return fail(e, DRS_ERR_BAD_ARG, "negative output capacity");
  return wait_slot(e, e->slots[slot], h_out, h_out_floats);
}

int32_t drs_forward(drs_handle e, int32_t batch_id, int32_t bs, float* h_out) {
  int32_t rc = drs_forward_async(e, 0, batch_id, bs);
  if (rc) return rc;
  return wait_slot(e, e->slots[0], h_out);
}

int32_t drs_sync(drs_handle e) {
  int32_t rc = check_handle(e);
  if (rc) return rc;
  int32_t first = DRS_OK;
  for (auto& s : e->slots) {
    rc = wait_slot(e, s, nullptr);
    if (rc && !first) first = rc;
  }
  return first;
}

int32_t drs_fetch_interaction(drs_handle e, int32_t slot, int32_t bs, float* h_R) {
  int32_t rc = check_handle(e);
  if (rc) return rc;
  // rows are VIRTUAL rows of the slot: coalesced query i sits at the 64-row aligned offset
  // sum of round_up(bs_j, 64) over j < i; a single query starts at row 0
  if (slot < 0 || slot >= e->n_slots || !h_R || bs < 0 || bs > e->max_rows) return fail(e, DRS_ERR_BAD_ARG, "bad arguments");
  Slot& s = e->slots[slot];
  HIP_TRY(e, hipStreamSynchronize(s.stream));
  if (e->mlp_layout == 1) HIP_TRY(e, hipStreamSynchronize(e->stream_g));
  const float* src;
  int64_t ld;
  if (e->kind == DRS_MODEL_NCF) { src = s.H2; ld = e->num_int; }
  else if (e->kind == DRS_MODEL_DIN || e->kind == DRS_MODEL_DIEN) { src = s.R; ld = e->ldR; }
  else if (e->kind == DRS_MODEL_DLRM && e->interaction_op == DRS_INTERACT_DOT) { src = s.R; ld = e->ldR; }
  else {
    if (s.split_last)
      return fail(e, DRS_ERR_STATE, "the set's dense columns were read in place (\"gemm_split\" 1): set it to 0 to materialise the interaction tensor");
    src = s.T; ld = e->ldT;
  }
  HIP_TRY(e, hipMemcpy2D(h_R, sizeof(float) * e->num_int, src, sizeof(float) * ld,
                         sizeof(float) * e->num_int, bs, hipMemcpyDeviceToHost));
  return DRS_OK;
}

int32_t drs_out_width(drs_handle e, int32_t* n_out) {
  if (!e || !n_out) return DRS_ERR_BAD_ARG;
  *n_out = e->n_out;
  return DRS_OK;
}

int32_t drs_interaction_width(drs_handle e, int32_t* num_int) {
  if (!e || !num_int) return DRS_ERR_BAD_ARG;
  *num_int = e->num_int;
  return DRS_OK;
}

// ---- operator-level entry points ---------------------------------------------
// drs_sls and drs_sls_weighted (d_wgt: one weight per index, or nullptr)
static int32_t sls_op(drs_handle e, const float* d_W, int64_t rows, int32_t D, const int32_t* d_idx, const float* d_wgt,
                      const int32_t* d_len, int64_t n_bags, int64_t n_idx, float* d_out, int32_t exact_order) {
  int32_t rc = check_handle(e);
  if (rc) return rc;
  if (!d_W || !d_len || !d_out || (!d_idx && n_idx > 0) || n_bags < 0 || n_idx < 0 || rows <= 0)
    return fail(e, DRS_ERR_BAD_ARG, "bad arguments");
  if (D <= 0 || D > 4096) return fail(e, DRS_ERR_UNSUPPORTED, "D=%d must be in [1, 4096]", D);
  if (rows * (int64_t)D >= (1ll << 33) || n_bags >= (1ll << 31) || n_idx >= (1ll << 31))
    return fail(e, DRS_ERR_UNSUPPORTED, "operand too large");
  if (n_bags == 0) return n_idx == 0 ? DRS_OK : fail(e, DRS_ERR_LENGTHS_SUM, "indices without bags");
  Slot& s = e->slots[0];
  if (s.busy && (rc = wait_slot(e, s, nullptr))) return rc;
  std::vector<int32_t> len((size_t)n_bags), off((size_t)n_bags + 1);
  HIP_TRY(e, hipMemcpy(len.data(), d_len, sizeof(int32_t) * (size_t)n_bags, hipMemcpyDeviceToHost));
  int64_t total = 0;
  off[0] = 0;
  for (int64_t b = 0; b < n_bags; ++b) {
    if (len[b] < 0) return fail(e, DRS_ERR_LENGTHS_SUM, "negative length");
    total += len[b];
    if (total > n_idx) return fail(e, DRS_ERR_LENGTHS_SUM, "sum(lengths) exceeds len(indices)");
    off[b + 1] = (int32_t)total;
  }
  if (total != n_idx) return fail(e, DRS_ERR_LENGTHS_SUM, "sum(lengths)=%lld != len(indices)=%lld", (long long)total, (long long)n_idx);
  DeviceBuf<int32_t> d_off, d_err;
  HIP_TRY(e, d_off.alloc((size_t)n_bags + 1));
  hipError_t r = d_err.alloc(1);
  if (r != hipSuccess) return fail(e, DRS_ERR_OOM, "hipMalloc");
  const int64_t tab[2] = {0, rows};
  int32_t h_err = 0;
  r = hipMemcpy(d_off, off.data(), sizeof(int32_t) * ((size_t)n_bags + 1), hipMemcpyHostToDevice);
  if (r == hipSuccess) r = hipMemcpy(e->d_op_tab, tab, sizeof tab, hipMemcpyHostToDevice);
  if (r == hipSuccess) r = hipMemset(d_err, 0, sizeof(int32_t));
  if (r == hipSuccess) {
    SlsArgs a;
    memset(&a, 0, sizeof a);
    a.tables = d_W; a.tab_off = e->d_op_tab; a.tab_rows = e->d_op_tab + 1;
    a.q.n_q = 1; a.q.vstart[1] = (int32_t)n_bags; a.q.cum[1] = (int32_t)n_bags; a.q.bs[0] = (int32_t)n_bags;
    a.idx[0] = d_idx; a.off[0] = d_off; a.uniform_len[0] = -1;
    a.wgt[0] = d_wgt;        // (null: drs_sls; the table is one table, so the weights line up with the indices)
    a.out = d_out; a.ld_out = D; a.col0 = 0; a.T = 1; a.D = D; a.err = d_err; a.ts = nullptr;
    a.pool = e->sls_pool;    // the operator follows the handle: SparseLengthsMean under "sls_pool" 1
    r = launch_sls(a, plan_sls(a, exact_order != 0, false, e->tune, DRS_TABLE_FP32), e->tune, s.stream);
  }
  if (r == hipSuccess) r = hipStreamSynchronize(s.stream);
  if (r == hipSuccess) r = hipMemcpy(&h_err, d_err, sizeof(int32_t), hipMemcpyDeviceToHost);
  if (r != hipSuccess) return fail(e, DRS_ERR_HIP, "drs_sls: %s", hipGetErrorString(r));
  if (h_err) return fail(e, DRS_ERR_INDEX_RANGE, "an index is outside [0, %lld)", (long long)rows);
  return DRS_OK;
}

int32_t drs_sls(drs_handle e, const float* d_W, int64_t rows, int32_t D, const int32_t* d_idx,
                const int32_t* d_len, int64_t n_bags, int64_t n_idx, float* d_out, int32_t exact_order) {
  return sls_op(e, d_W, rows, D, d_idx, nullptr, d_len, n_bags, n_idx, d_out, exact_order);
}

int32_t drs_sls_weighted(drs_handle e, const float* d_W, int64_t rows, int32_t D, const int32_t* d_idx, const float* d_wgt,
                         const int32_t* d_len, int64_t n_bags, int64_t n_idx, float* d_out, int32_t exact_order) {
  int32_t rc = check_handle(e);
  if (rc) return rc;
  if (!d_wgt && n_idx > 0) return fail(e, DRS_ERR_BAD_ARG, "drs_sls_weighted: null weights");
  if (e->sls_pool) return fail(e, DRS_ERR_UNSUPPORTED, "drs_sls_weighted: \"sls_pool\" 1 has no weighted form (there is no weighted mean)");
  return sls_op(e, d_W, rows, D, d_idx, d_wgt, d_len, n_bags, n_idx, d_out, exact_order);
}

int32_t drs_fc(drs_handle e, const float* d_x, int64_t M, int32_t K, const float* d_W, const float* d_b,
               int32_t N, int32_t act, float* d_y) {
  int32_t rc = check_handle(e);
  if (rc) return rc;
  if (!d_x || !d_W || !d_y || M < 0 || K <= 0 || N <= 0 || act < 0 || act > 2) return fail(e, DRS_ERR_BAD_ARG, "bad arguments");
  Slot& s = e->slots[0];
  if (s.busy && (rc = wait_slot(e, s, nullptr))) return rc;
  MlpPlan p;
  // "mlp_dtype" 2: a bf16 layer by its shape, as in a launch set -- d_W rounded into a scratch twin first
  DeviceBuf<uint16_t> wb;
  if (M > 0 && bf16_shape(e, K, N)) {
    if (wb.alloc((size_t)N * bf16_kpad(K)) != hipSuccess) {
      (void)hipGetLastError();
      return fail(e, DRS_ERR_OOM, "drs_fc: no room for the bf16 twin of the %dx%d layer", K, N);
    }
    hipError_t r = launch_bf16_twin(d_W, K, N, wb, s.stream);
    if (r != hipSuccess) return fail(e, DRS_ERR_HIP, "drs_fc: %s", hipGetErrorString(r));
  }
  hipError_t r = hipSuccess;
  const bool ok = M <= 0 || plan_layer(d_x, K, M, K, d_W, d_b, N, act, d_y, N, e->tune, nullptr, nullptr, &p, wb);
  if (ok && M > 0) r = launch_plan(p, e->tune, s.stream);
  if (r == hipSuccess) r = hipStreamSynchronize(s.stream);
  if (!ok) return fail(e, DRS_ERR_HIP, "no kernel takes the %dx%d layer", K, N);
  HIP_TRY(e, r);
  return DRS_OK;
}

int32_t drs_interact_dot(drs_handle e, const float* d_T, int64_t B, int32_t F, int32_t D, int32_t itself, float* d_R) {
  int32_t rc = check_handle(e);
  if (rc) return rc;
  if (!d_T || !d_R || B < 0 || F <= 0 || D <= 0) return fail(e, DRS_ERR_BAD_ARG, "bad arguments");
  Slot& s = e->slots[0];
  if (s.busy && (rc = wait_slot(e, s, nullptr))) return rc;
  const int P = itself ? F * (F + 1) / 2 : F * (F - 1) / 2;
  hipError_t r = launch_interact_dot(d_T, (int64_t)F * D, B, F, D, itself, d_R, D + P, s.stream);
  if (r == hipErrorInvalidValue) return fail(e, DRS_ERR_UNSUPPORTED, "F=%d D=%d does not fit LDS", F, D);
  HIP_TRY(e, r);
  HIP_TRY(e, hipStreamSynchronize(s.stream));
  return DRS_OK;
}

// ---- tuning / measurement ------------------------------------------------------

}  // extern "C"
