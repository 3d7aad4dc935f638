// Internal declarations shared by the HIP translation units of libdrs_hip.so.
// Public surface: include/drs.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/drs.h"
#include "weight_plan.h"

namespace drs {

// Up to this many queries can be coalesced into one set of launches.  A query q owns the
// virtual rows [vstart[q], vstart[q] + bs[q]) of the slot's activation buffers; vstart[]
// is kept a multiple of 64 so a 16- or 64-row MLP block never straddles two queries.
// (DRS_MAX_COALESCE: include/drs.h)
struct QTable {
  int32_t n_q;
  int32_t vstart[DRS_MAX_COALESCE + 1];   // virtual first row per query; [n_q] = total virtual rows
  int32_t cum[DRS_MAX_COALESCE + 1];      // prefix sums of bs (valid samples before query q)
  int32_t bs[DRS_MAX_COALESCE];
};

// One launch of the multi-table gather-reduce (SparseLengthsSum x T tables).
// Bags are numbered sample-major: bag = b * T + t, so the T pooled vectors of a
// sample land next to each other in the interaction buffer
//   out[b * ld_out + col0 + t * D + d]
// which is the [B, F, D] / Concat(axis=1) layout of
// models/dlrm_s_caffe2.py:337-342,358-360 with the dense slot in front.
struct SlsArgs {
  const float* tables;        // base of the table arena
  const int64_t* tab_off;     // [T] offset of table t in the arena, in units of its type (table_unit_bytes)
  const int64_t* tab_rows;    // [T]
  // fp8 e4m3 tables ("table_dtype" 4): [T] each table's 2^-k (fp8_exponent below).  The fp8 instances multiply a bag's
  // finished sum of decoded codes by it; no other instance reads it (null for every other type).
  const float* tab_scale;
  QTable q;                   // which query a bag belongs to
  const int32_t* idx[DRS_MAX_COALESCE];   // per query: [T][idx_stride] int32 indices (Cast op done)
  const int32_t* off[DRS_MAX_COALESCE];   // per query: [T][off_stride] exclusive prefix sums of lengths
  // per query: [T][idx_stride] fp32 per-sample weights, laid out like idx (SparseLengthsWeightedSum), or nullptr: the query is
  // unweighted, every weight 1.0f.  A launch with at least one non-null entry is a WEIGHTED launch (SlsPlan::weighted).
  const float* wgt[DRS_MAX_COALESCE];
  int32_t uniform_len[DRS_MAX_COALESCE];  // per query: >= 0 -> every bag has this many indices
  int64_t idx_stride;
  int64_t off_stride;
  float* out;
  int64_t ld_out;             // floats between consecutive (virtual) samples
  int32_t col0;               // first output column of table 0
  int32_t T;
  int32_t D;
  int32_t* err;               // device error word: bit0 = index out of range
  uint64_t* ts;               // optional [2 * gridDim.x] start/end wall_clock64() per workgroup
  int32_t nt;                 // fused DIN launch: table rows by non-temporal loads ("sls_nt"; set by launch_din_fused)
  int32_t pool;               // "sls_pool": 0 a bag's sum | 1 its mean, the finished sum / (float)length (sls_dev.h pool_finish)
  // int8 / int4 rowwise tables in the line-packed layout ("table_int8_lines" / "table_int4_lines", I8Lines below): row r
  // starts r * PR + (r / n) * ln_pad pieces into its table, r / n == ln_mul ? umulhi(r, ln_mul) >> ln_shift : r.  ln_pad == 0: every other layout.
  uint32_t ln_mul, ln_shift, ln_pad;
};

// What the launch functions chose for the launch set being enqueued ("which kernel serves which shape"):
// each launch appends "name<template args>[grid x block] " to the log of the slot (drs_last_dispatch).
// Host-side bookkeeping only; nothing on the device reads it.
struct DispatchLog {
  char text[768];
  int len;
};
void log_launch(DispatchLog* log, const char* fmt, ...) __attribute__((format(printf, 2, 3)));

// Per-engine tunables (drs_set_option) and the per-device resources every launch needs.
// Nothing here is process-global: two engines in one process (the mixed-model accelerator
// engine; engines on different GPUs) keep their own copy.
struct Tune {
  int device = 0;
  const float* zero = nullptr;   // 256 B of zeros on `device`: source of out-of-range float4 loads
  const float* w_arena = nullptr;   // the engine's FC weight arena (biases + weights, one allocation) ...
  uint64_t w_arena_floats = 0;
  uint64_t w_packed_lo = 0, w_packed_hi = 0;   // float range of the arena whose layers carry a packed twin
  uint32_t w_zero_off = 0;          // ... whose first 64 floats are zeros (float offset of them)
  int sls_flat = 1;              // fixed-length bags: all row loads of a wave in flight at once
  int sls_bpw = 0;               // ... bags per wave of that variant (0 = auto | 1 | 2 | 4)
  int sls_nt = 1;                // table rows are read with non-temporal loads (every gather kernel of sls.hip and sls_wflat.hip)
  int sls_weighted_flat = 0;     // a WEIGHTED launch may take the flat, flatc and one-lookup forms (their weighted instances: sls_wflat.hip); 0: the ring walk or the any-width form only
  int sls_one = 1;               // fixed bags of ONE row (W&D, MT-WnD, NCF, DIEN): the copy form (sls_one_kernel); 1 = 64 samples per wave, 16 for small launches | 64 | 16 | 0 off
  int din_nt = 1;                // fused DIN launch: non-temporal row loads ("din_nt": +2.5 % queries/s, 0.527 -> 0.545 of peak)
  int din_pipe = 1;              // fused DIN launch, hidden width 1: indices staged in LDS, units pipelined (din_pipe_kernel)
  int din_s = 0;                 // fused DIN launch: samples per workgroup (0 = by launch size | 1 | 2 | 4)
  int mlp_preload = 0, mlp_kc = 0, mlp_stream = 2, mlp_stream_2cu = 0, mlp_gemm = 1, gemm_tile = 0, gemm_2cu = 0, mlp_debug = 0;
  int gemm32 = 1;                // wide layers through the v_mfma_f32_32x32x2_f32 kernel (gemm.hip gemm32_kernel) ...
  int gemm32_small_blocks = 0;   // ... when that shape gives at least this many workgroups
  int gemm32_small = 0;          // ... and smaller launches this gemm32 shape (0 = gemm_kernel | 22 | 21 | 12 | 11)
  int gemm32_blocks = 512;       // ... when its 128 x 128 workgroups number at least this many (two per CU)
  int bf16_tile = 0;             // gemm_bf16_kernel's tile shape (0 = by workgroup count | 44 | 22 | 12; gemm_bf16.hip gemm_bf16_plan)
  int64_t mlp_rows32 = 0;        // stream4_kernel: launches of at least this many rows take 32 rows per workgroup (0 = never)
  DispatchLog* log = nullptr;    // where the launch functions note what they chose (the slot being enqueued; may be null)
  // stream4_kernel's column-split form (mlp.hip SArgs::ns): launches of at most mlp_nsplit_rows rows spread the first
  // layer of the second chain over mlp_nsplit (0 = never | 2 | 4) workgroups per slab of rows.  xbuf / xcnt: the
  // exchange buffer ([xbuf_rows, xbuf_cols] floats) and ticket words of the slot being enqueued (like `log`).
  int mlp_nsplit = 0;
  int64_t mlp_nsplit_rows = 0;
  float* xbuf = nullptr;
  uint32_t* xcnt = nullptr;
  int64_t xbuf_rows = 0;
  int32_t xbuf_cols = 0;
};
// Once per DEVICE (thread-safe): the > 64 KB dynamic-LDS attribute of every kernel that needs
// it (HIP function attributes are per device) and the device's zero page.
hipError_t device_init(int device, const float** zero_page);
hipError_t mlp_set_attrs();    // mlp.hip's kernels, on the current device
hipError_t gemm_set_attrs();   // gemm.hip's kernels, on the current device
hipError_t gemm_bf16_set_attrs();   // gemm_bf16.hip's kernels, on the current device
hipError_t fused_bf16_set_attrs();  // mlp_fused_bf16.hip's kernels, on the current device

// One gather launch, decided once by plan_sls and run by launch_sls (sls.hip, sls_wflat.hip).  Host-only.
//   form: any (any row width) | ring (sls_kernel) | one (one lookup per bag) | flat | flatc (fixed-length bags)
//   exact: the sequential summation order (bit-identical to Caffe2's SparseLengthsSum)
//   G, NL, BPW, BW, L, nt: the instance -- lanes per row, loads per lane, bags per wave, samples per wave, bag length,
//   non-temporal row loads; tiles: one-lookup sample tiles per table; grid: workgroups (0: nothing to launch)
//   weighted: a query of the launch carries per-sample weights (SlsArgs::wgt): the weighted instance of the form.  With
//   "sls_weighted_flat" 0 (the default) that is the ring walk or the any-width form, never flat, flatc or one; with 1 the
//   form is the one the unweighted launch would take
//   dtype: element type of the tables a.tables points at (DRS_TABLE_*; a.tab_off counts units of that type:
//   table_unit_bytes) -- the same decisions and grids for every type, rows widened to fp32 before they are summed
enum class SlsForm { any, ring, one, flat, flatc };
struct SlsPlan {
  SlsForm form = SlsForm::ring;
  bool exact = false;
  int G = 0, NL = 0, BPW = 1, BW = 0, L = 0, nt = 0;
  int tiles = 0;
  int64_t grid = 0;
  int dtype = DRS_TABLE_FP32;
  bool weighted = false;
};
// exact: the caller asks for the sequential order ("sls_exact", drs_sls's exact_order); short_bags: every bag of the
// launch is short ("sls_short_bag"), so the sequential order is taken unless the flat variant takes the launch
SlsPlan plan_sls(const SlsArgs& a, bool exact, bool short_bags, const Tune& tune, int dtype);
// stop_event (optional): recorded by the gather dispatch itself when it completes
hipError_t launch_sls(const SlsArgs& a, const SlsPlan& plan, const Tune& tune, hipStream_t stream,
                      hipEvent_t stop_event = nullptr);
// the weighted flat, flatc and one-lookup launches of launch_sls (sls_wflat.hip; plan.weighted, plan.grid > 0)
hipError_t launch_sls_wflat(const SlsArgs& a, const SlsPlan& plan, hipStream_t stream, hipEvent_t stop_event);
// "table_dtype" layouts.  Stored bytes of one row: D elements of 4 (fp32) or 2 (fp16 / bf16) bytes; int8 rowwise: D codes,
// zero padding to round_up(D, 8), fp32 scale, fp32 bias (every row 8-byte aligned); int4 rowwise: D / 2 code bytes, zero
// padding to round_up(D / 2, 4), fp16 scale, fp16 bias (every row 4-byte aligned; D even); fp8 e4m3: D codes of one byte,
// no header (the table's power-of-two scale lives beside tab_off: SlsArgs::tab_scale)
inline bool table_rowwise(int dtype) { return dtype == DRS_TABLE_INT8_ROWWISE || dtype == DRS_TABLE_INT4_ROWWISE; }
// the types whose arena is laid out in bytes, table by table (table_unit_bytes 1): conversions into or out of them run per table
inline bool table_bytewise(int dtype) { return table_rowwise(dtype) || dtype == DRS_TABLE_FP8_E4M3; }
inline int64_t table_row_stride(int dtype, int64_t D) {
  if (dtype == DRS_TABLE_INT4_ROWWISE) return (D / 2 + 3) / 4 * 4 + 4;
  if (dtype == DRS_TABLE_FP8_E4M3) return D;
  return dtype == DRS_TABLE_INT8_ROWWISE ? (D + 7) / 8 * 8 + 8 : D * (dtype == DRS_TABLE_FP32 ? 4 : 2);
}
// bytes a gathered row moves (the algorithmic count of drs_gather_bytes and of the launch-form choice): int8 rowwise D + 8,
// int4 rowwise D / 2 + 4
inline int64_t table_row_bytes(int dtype, int64_t D) {
  if (dtype == DRS_TABLE_INT4_ROWWISE) return D / 2 + 4;
  return dtype == DRS_TABLE_INT8_ROWWISE ? D + 8 : table_row_stride(dtype, D);
}
// what a table offset (SlsArgs::tab_off, drs_engine::tab_off) counts: elements (4 / 2 bytes), or bytes for the rowwise types and fp8
inline int64_t table_unit_bytes(int dtype) { return dtype == DRS_TABLE_FP32 ? 4 : table_bytewise(dtype) ? 1 : 2; }

// fp8 e4m3 tables: the scale exponent of a table whose largest finite |x| is absmax -- the largest k with
// absmax * 2^k <= 448 = 0.875 * 2^9, clamped to [-64, 64]; 0 for an all-zero table
inline int32_t fp8_exponent(float absmax) {
  if (!(absmax > 0.0f) || __builtin_isinf(absmax)) return 0;
  int e = 0;
  const float m = __builtin_frexpf(absmax, &e);           // absmax = m * 2^e, m in [0.5, 1)
  const int k = m <= 0.875f ? 9 - e : 8 - e;
  return k < -64 ? -64 : k > 64 ? 64 : k;
}
inline float fp8_pow2(int32_t k) { return __builtin_ldexpf(1.0f, k); }

// "table_int8_lines" / "table_int4_lines": rowwise rows that never cross a 128-byte line.  When the row stride S =
// table_row_stride(dtype, D) < 128 does not divide 128, n = 128 / S rows share a line: row r starts at byte
// (r / n) * 128 + (r % n) * S of its table and the last 128 - n * S bytes of every line are zero.  Any other S keeps the
// plain layout (n == 0 here).  The kernels count in pieces of `piece` bytes (int8: 4, int4: 2): r * (S / piece) +
// (r / n) * pad, with r / n == umulhi(r, mul) >> shift for every 32-bit r (n == 1: mul == 0 and the quotient is r itself;
// n == 2: 2^31, 0; n == 3: 0xAAAAAAAB, 1; n == 4: 2^31, 1; n == 5: 0xCCCCCCCD, 2; n == 6: 0xAAAAAAAB, 2; n == 10:
// 0xCCCCCCCD, 3 -- the 64-bit product shifted by 32 + shift).
struct I8Lines {
  int32_t n = 0;                   // rows per line; 0: the plain layout
  uint32_t mul = 0, shift = 0, pad = 0;
};
inline I8Lines row_lines(int64_t S, int64_t piece, int lines) {
  I8Lines l;
  if (!lines || S >= 128 || 128 % S == 0) return l;
  l.n = (int32_t)(128 / S);
  l.pad = (uint32_t)(128 / piece - l.n * (S / piece));
  if (l.n > 1) {
    int lg = 0;                    // ceil(log2(n))
    while ((1 << lg) < l.n) ++lg;
    l.shift = (uint32_t)(lg - 1);
    l.mul = (uint32_t)((((uint64_t)1 << (31 + lg)) + (uint64_t)l.n - 1) / (uint64_t)l.n);   // ceil(2^(31 + lg) / n)
  }
  return l;
}
inline I8Lines i8_lines(int64_t D, int lines) { return row_lines(table_row_stride(DRS_TABLE_INT8_ROWWISE, D), 4, lines); }
inline I8Lines i4_lines(int64_t D, int lines) { return row_lines(table_row_stride(DRS_TABLE_INT4_ROWWISE, D), 2, lines); }
// the layout of an arena of type dtype under its own option's value (fp32 / fp16 / bf16: plain)
inline I8Lines table_lines(int dtype, int64_t D, int lines) {
  return dtype == DRS_TABLE_INT8_ROWWISE ? i8_lines(D, lines) : dtype == DRS_TABLE_INT4_ROWWISE ? i4_lines(D, lines) : I8Lines();
}
// byte offset of row r inside its int8 / int4 rowwise table, and the bytes `rows` rows occupy (before the 256-byte rounding)
__host__ __device__ inline int64_t i8_row_offset(int64_t r, int64_t S, int32_t n) { return n ? r / n * 128 + r % n * S : r * S; }
inline int64_t i8_table_bytes(int64_t rows, int64_t S, int32_t n) { return n ? (rows + n - 1) / n * 128 : rows * S; }

// Completion hand-off to the host without a copy or a stream sync: the LAST kernel of a
// query stores its outputs straight into host-mapped pinned memory and, once every one
// of its workgroups has done so (device-scope arrival counter), the last arriver copies
// the device error word and publishes `seq` in a host flag the CPU is polling.
struct Done {
  uint32_t* counter;        // device arrival counter (zero between uses); nullptr = disabled
  uint32_t* host_flag;      // host-mapped: receives seq
  uint32_t* host_err;       // host-mapped: receives *dev_err
  const uint32_t* dev_err;  // device error word written by earlier kernels of the query
  uint32_t seq;
  // live timing of the gather launch: its per-workgroup [start, end] clock stamps are
  // reduced to (min start, max end) by the same last-arriving workgroup and stored in
  // host-mapped memory, so profiling adds no copy, no sync and no extra launch
  const uint64_t* ts;       // [2 * ts_blocks] or nullptr
  uint32_t ts_blocks;
  uint64_t* span_acc;       // device [2 * workgroups of the last kernel]: per-workgroup (min, max)
  uint64_t* host_span;      // host-mapped [2]
  // the outputs themselves: every workgroup stores to the DEVICE buffer; only the last
  // arriver streams them to host-mapped memory (8 KB for 2048 rows) behind ONE system-scope
  // release.  (Letting all workgroups store to host memory and fence at system scope cost
  // 20 us per launch: measured 56 us vs 36 us.)
  const float* dev_out;
  float* host_out;
  uint32_t out_words;
  // early start (stream4_kernel, "mlp_early"): the launch does NOT wait for the gather on its stream; it runs its
  // prologue and the first chain, then polls `wait_flag` for `wait_val` (a stream-ordered 32-bit write queued behind the
  // gather) before it fetches the second chain's pooled rows.  nullptr: the stream orders the launch behind the gather.
  uint32_t wait_val;
  const uint32_t* wait_flag;
};

// y[M, N] (ld = ldy) = act(x[M, K] (ld = ldx) . W[N, K]^T + b), k-ordered fp32 MFMA chain
// Optional per-query sources of the FIRST layer's input rows (dense features live in the
// staged batches, one array per query); rows of y are always virtual rows.
struct XSrc {
  QTable q;
  const float* x[DRS_MAX_COALESCE];
  // > 0 (gemm32_kernel's scalar-base forms only, gemm.hip gemm_plan): columns [0, ksplit) of an input row come from the
  // queries' own staged arrays (rows ksplit floats apart), columns from ksplit on from `x` at the VIRTUAL row -- W&D's and
  // MT-WnD's first layer reads Concat(dense, pooled embeddings) without the dense rows ever being copied next to the
  // embeddings (models/wide_and_deep.py:271-281).  A multiple of 32, >= 64, < K.
  int32_t ksplit;
};


// Fused chain of up to DRS_MAX_CHAIN FC layers on 16-row slabs; intermediate
// activations never leave LDS.
#define DRS_MAX_CHAIN 6
struct ChainArgs {
  const float* x;
  int64_t ldx;
  int64_t M;
  int32_t n_layers;
  int32_t width[DRS_MAX_CHAIN + 1];   // width[0] = K of first layer
  const float* W[DRS_MAX_CHAIN];
  const float* b[DRS_MAX_CHAIN];
  int32_t act[DRS_MAX_CHAIN];
  float* y;
  int64_t ldy;
};
// Two chains on the same rows in one launch (bottom MLP, then the top MLP that reads the
// buffer the first one wrote its last layer into), mlp.hip plan_chains.
// Optional dot interaction BETWEEN the two chains (DLRM "dot",
// models/dlrm_s_caffe2.py:334-354): the first chain writes the dense_out slot of T, the
// interaction turns T [M, F*D] into R [M, D + P], the second chain reads R.
struct DotArgs {
  const float* T;   // == a.y: [M, F*D] sample-major (dense_out | emb_0 | ...), ld = ldt
  int64_t ldt;
  int32_t F, D, itself;
  float* R;         // == b->x: interaction output, ld = ldr (also kept for drs_fetch_interaction)
  int64_t ldr;
};
// Optional NCF-style join (models/ncf.py:301-305,317-346): the second chain's input buffer is
// [ src[:, col_a:col_a+cols] + src[:, col_b:col_b+cols] | output of the first chain ], i.e.
// Sum of two pooled embeddings in front of the MLP branch.  dst (== b->x) receives the summed
// block as well (the first chain stores its output right behind it, a.y == dst + cols).
struct SumArgs {
  const float* src;
  int64_t ld;
  int32_t col_a, col_b, cols;
  float* dst;
  int64_t ldd;
};

// T [B, F, D] (sample stride ldt) -> R [B, D + P] (ld = ldr), see drs_interact_dot
hipError_t launch_interact_dot(const float* T, int64_t ldt, int64_t B, int32_t F, int32_t D,
                               int32_t itself, float* R, int64_t ldr, hipStream_t stream);

// out[i] = a[i] + b[i] rows of width D (NCF Sum, models/ncf.py:301-305) and strided copies
hipError_t launch_add_rows(const float* a, int64_t lda, const float* b, int64_t ldb, float* out,
                           int64_t ldo, int64_t M, int32_t D, hipStream_t stream);
// dense rows of all coalesced queries (xs.x[q], m_den wide) -> their virtual rows of `out`
hipError_t launch_copy_rows_multi(const XSrc& xs, int32_t m_den, float* out, int64_t ldo, hipStream_t stream);
hipError_t launch_copy_rows(const float* a, int64_t lda, float* out, int64_t ldo, int64_t M,
                            int32_t D, hipStream_t stream);

// DIN (din.hip; models/din.py:247-330).  packed: the attention units' weights, one block of
// din_unit_stride(D, h) floats per unit, built by launch_din_pack from 4 device pointers per unit
// (W1 [h, 3D], b1 [h], W2 [D, h], b2 [D]).  launch_din_attention: T [M, Tn*D] pooled rows ->
// R [M, 4*D] = [ profile | Sum_i unit_i(u_i, ad) | ad | context ], bit-identical to the oracle.
// launch_din_fused: gather + units + Concat in one launch (a: the gather's arguments; a.out unused).
int64_t din_unit_stride(int D, int h);
hipError_t launch_din_pack(const float* const* att, float* packed, int32_t U, int32_t D, int32_t h, hipStream_t stream);
hipError_t launch_din_attention(const float* T, int64_t ldt, int64_t M, int32_t Tn, int32_t D, int32_t h,
                                const float* packed, float* R, int64_t ldr, hipStream_t stream);
bool din_fused_applicable(int32_t D, int32_t h);
int64_t din_fused_grid(const SlsArgs& a, const Tune& tune);
hipError_t launch_din_fused(const SlsArgs& a, int32_t h, const float* packed, float* R, int64_t ldr,
                            const Tune& tune, hipStream_t stream, hipEvent_t stop);

// DIEN (dien.hip; models/dien.py:308-432).  w: 8 device pointers {i2h_w, i2h_b, gates_t_w, gates_t_b} of
// layer 1 then layer 2; launch_dien_rnn: T [rows, Tn*D] pooled rows of the coalesced queries q ->
// R [rows, H + 3*D] = [ last state of layer 2 | profile | ad | context ].
// Any-shape forms (din_any.hip): attention units of any depth and width -- d_ln: the unit's n_ln widths on the device,
// d_att: per unit and layer {W, b}, maxw: the widest hidden layer -- and the recurrence for any D and H (packed as
// launch_dien_pack lays it out).  *_fits: the sample's activations fit the 160 KB of LDS.
bool din_any_fits(int32_t D, int32_t maxw);
bool dien_any_fits(int32_t D, int32_t H);
hipError_t launch_din_attention_any(const float* T, int64_t ldt, int64_t M, int32_t Tn, int32_t D, int32_t n_ln,
                                    const int32_t* d_ln, const float* const* d_att, int32_t maxw, float* R, int64_t ldr,
                                    hipStream_t stream);
hipError_t launch_dien_rnn_any(const float* T, int64_t ldt, const QTable& q, int32_t Tn, int32_t D, int32_t H,
                               const float* packed, float* R, int64_t ldr, hipStream_t stream);
bool dien_applicable(int32_t D, int32_t H);
int64_t dien_packed_floats(int32_t D, int32_t H);
hipError_t launch_dien_pack(const float* const* w, float* packed, int32_t D, int32_t H, hipStream_t stream);
// (mfma: the 16-samples-per-workgroup matrix-core form when H % 16 == 0, reading the row-major
// weights w[8] (host array of device pointers); else one wave per sample on `packed`; same bits)
// top (optional, matrix-core form only): the model's top MLP over R's rows in the same launch -- n <= 4 layers,
// every K a multiple of 4 and <= 256 (dien_top_fusable) -- written to out [rows, ldo]; `done`
// then makes the launch sign off the launch set (mlp_dev.h signal_done).  Same bits as the stream kernels' chains.
struct DienTop {
  int32_t n, kmax, sc1, pad_;      // layers (0: none) | rows of an LDS activation buffer (dien_top_kmax) | write-through output stores
  const float* Wp[4];              // the layers' PACKED twins (mlp.hip pack_stream_kernel; W + roundup64(K N) in the arena)
  const float* b[4];
  int32_t K[4], N[4], act[4];
  float* out;
  int64_t ldo;
};
bool dien_top_fusable(int32_t n_layers, const int32_t* widths /* n_layers + 1 */, int32_t H);
int32_t dien_top_kmax(int32_t n_layers, const int32_t* widths);
hipError_t launch_dien_rnn(const float* T, int64_t ldt, const QTable& q, int32_t Tn, int32_t D, int32_t H,
                           const float* packed, const float* const* w, int mfma, float* R, int64_t ldr,
                           hipStream_t stream, const DienTop* top = nullptr, const Done* done = nullptr);

// Weights of one FC layer (W [N, K] row-major) in the stream kernel's MFMA-operand order (mlp.hip):
// per 128-column pass and 64-k chunk, per wave (16 columns), four float4 per lane.
int64_t stream_packed_floats(int K, int N);
hipError_t launch_pack_stream_weights(const float* W, int32_t K, int32_t N, float* Wp, hipStream_t stream);

// "mlp_dtype" 2: the bf16 twin of one FC layer (gemm_bf16.hip): W [N, K] fp32 -> Wb [N, bf16_kpad(K)] bf16, rounded to
// nearest even (NaN stays NaN), zeros from K on
inline int32_t bf16_kpad(int32_t K) { return (K + 63) / 64 * 64; }
hipError_t launch_bf16_twin(const float* W, int32_t K, int32_t N, uint16_t* Wb, hipStream_t stream);

// random 128- / 256- / 512-byte row reads over [base, base + bytes) in the gather's access shape, timed with events on `s`
// (sls_probe.hip probe_rows_kernel, lab build only); sink: >= 1 KiB of device memory nobody reads
hipError_t probe_rows(const void* base, size_t bytes, int waves, int reps, float* sink, hipStream_t s, double* gbs,
                      int windows = 0, int sorted = 0, int row_bytes = 256, int nt = 1, int loads = 20);

// dependent-load walk through each of n_chunks chunks of chunk_bytes (one lane per chunk); d_ticks[k] = 100 MHz ticks
hipError_t probe_latency(const void* base, size_t chunk_bytes, int n_chunks, int steps, uint64_t* d_ticks, hipStream_t s);

// Writing tables (table_convert.hip).  One side of a pass: rows of D columns stored as `dtype` (DRS_TABLE_*).  A rowwise
// side (int8 / int4) is the TABLE's first byte in the layout lines_n (I8Lines::n of its own type; 0: plain), and the window
// names its rows first .. first + rows - 1 of `total` (the table's last row clears the rest of its line); a side of any
// other type points at the window's first row.  scale: an fp8 side's decode scale 2^-k (source) or multiplier 2^k (destination).
struct TableSide { void* base; int dtype; int32_t lines_n = 0; float scale = 1.0f; };
struct RowWindow { int64_t first, rows, total; };
// The window's rows of src, stored as dst asks: rounded to nearest even (widening is exact), quantized per row, encoded
// as e4m3_rne(x * scale) (torch's float8_e4m3fn conversion bit for bit; NaN and +-inf: 0x7F with the sign bit), or -- the
// same rowwise type on both sides -- the rows' bytes moved to the other layout.  A rowwise or fp8 source gives each row's
// value (fmaf(scale, q, 0.0f + bias); decode(code) * scale).  hipErrorInvalidValue: fp8 from fp8 or a rowwise type, an
// int4 side with odd D, an fp8 source with first != 0.
hipError_t launch_convert_rows(const TableSide& src, const TableSide& dst, const RowWindow& w, int D, hipStream_t stream);
// the uniform fill's values of table t (oracle/drs_oracle.c fill_value), stored as dst asks
hipError_t launch_fill_rows(const TableSide& dst, int64_t rows, int D, int32_t t, float lo, float hi, uint64_t seed, hipStream_t stream);
// atomicMax of the bits of |x| over the FINITE values of an fp32 / fp16 / bf16 source into *d_bits (a device word the caller zeroed)
hipError_t launch_absmax_rows(const TableSide& src, int64_t rows, int D, uint32_t* d_bits, hipStream_t stream);
// n elements of type src_dtype -> dst_dtype, fp32 / fp16 / bf16 only: a whole arena in one pass
hipError_t launch_convert_table(const void* src, int src_dtype, void* dst, int dst_dtype, int64_t n, hipStream_t stream);
// Single rows (table_rows.hip): `rows` rows of S bytes between a packed buffer (row r at r * S) and rows d_ids[r] of the table
// whose first byte is `table` (lines_n: I8Lines::n of a line-packed rowwise table, else 0) -- into the table (distinct ids)
// or out of it.  Only the rows' own S bytes are touched.
hipError_t launch_move_rows(void* buf, void* table, const int64_t* d_ids, int64_t rows, int64_t S, int32_t lines_n, bool to_table, hipStream_t stream);

// The per-call input pass on the device (input_pass.hip; include/drs_device_inputs.h): what convert_table does on the host
// for a launch set whose arrays are device arrays -- ONE launch narrows every query's int64 indices into its int32 index
// rows, turns its lengths into prefix sums and copies its dense rows.  A query's workgroups are numbered lengths first
// (one per table), then nb_idx per table of kInPassIdx indices each, then nb_dense of kInPassDense floats each; query i
// owns workgroups [wg0[i], wg0[i + 1]).
constexpr int kInPassThreads = 256;
constexpr int kInPassIdx = 2048;      // indices per narrowing workgroup: four 16-byte loads (two int64 each) per lane
constexpr int kInPassDense = 4096;    // floats per dense-row workgroup: four float4 per lane
constexpr uint32_t kErrIndex = 1u, kErrMlpEarly = 2u, kErrLengths = 4u;   // bits of a slot's device error word
struct InQuery {
  const int64_t* ids;         // [T] rows of n_idx, ids_stride elements apart (8-byte aligned, no more)
  const int32_t* len;         // [T] rows of bs, len_stride elements apart
  const float* dense;         // [bs * m_den], or null
  int64_t ids_stride, len_stride;
  int32_t* idx;               // -> Batch::idx [T][cap]
  int32_t* off;               // -> Batch::off [T][max_batch + 1]
  float* dst_dense;           // -> Batch::dense
  int32_t bs, n_idx;
  int32_t fixed_len;          // >= 0: every length must equal it | -1
  int32_t store_off;          // the gather will read this query's prefix sums (ragged bags, or "sls_uniform" 0)
  int32_t nb_idx, nb_dense;
};
struct InPassArgs {
  int32_t n_q, T, m_den, max_batch;
  int64_t cap;
  const int64_t* rows;        // [T] rows of every table (device)
  uint32_t* err;              // the slot's device error word
  int32_t wg0[DRS_MAX_COALESCE + 1];
  InQuery q[DRS_MAX_COALESCE];
};
// fills nb_idx / nb_dense / wg0 from the rest and returns the grid (0: nothing to do)
int64_t plan_input_pass(InPassArgs& a);
hipError_t launch_input_pass(const InPassArgs& a, int64_t grid, hipStream_t stream);

// The same pass for a set in which at least one query carries per-sample weights (include/drs_device_weights.h): a second
// instance of the kernel with a fourth kind of work item, kInPassWgt weights of one (query, table) row copied or widened into
// the query's [T, cap] fp32 weight block.  A query's weight workgroups are numbered behind its dense ones (weight_plan.h),
// so the other three kinds keep their numbers.  A set without weights launches input_pass_kernel as before.
struct InWgt {
  const void* src;            // [T] rows of n_idx weights of `dtype`, `stride` elements apart (aligned to the element, no more); null: unweighted
  int64_t stride;
  float* dst;                 // -> Batch::wgt [T][cap]
  int32_t dtype;              // DRS_TABLE_FP32 | DRS_TABLE_FP16 | DRS_TABLE_BF16
  int32_t nb_wgt;
};
struct InPassWgtArgs {
  InPassArgs in;
  InWgt w[DRS_MAX_COALESCE];  // entry i belongs to in.q[i]
};
// fills nb_idx / nb_dense / nb_wgt / wg0 from the rest and returns the grid (0: nothing to do; -1: beyond 32-bit block numbers)
int64_t plan_input_pass_weighted(InPassWgtArgs& a);
hipError_t launch_input_pass_weighted(const InPassWgtArgs& a, int64_t grid, hipStream_t stream);

// The output pass on the device (output_pass.hip; include/drs_device_outputs.h), its mirror: ONE launch moves every query's
// scores from the slot's device buffer to the caller's device arrays.  OutPassArgs, its planner and the owner lookup are
// plain C++ (output_plan.h).
struct OutPassArgs;
hipError_t launch_output_pass(const OutPassArgs& a, int64_t grid, hipStream_t stream);

// The top-k pass on the device (topk_pass.hip; include/drs_device_topk.h): ONE launch, workgroup i ranks query i of TopKArgs
// by one score column and writes its k winners' row numbers and score rows.  TopKArgs and the order are plain C++ (topk_plan.h).
struct TopKArgs;
hipError_t launch_topk_pass(const TopKArgs& a, hipStream_t stream);

}  // namespace drs
