// The MLP launch planners: which kernel form serves a launch and how its LDS is laid out.  Host code only -- no kernel
// lives here; the kernels, their attributes and launch_plan are in mlp.hip, mlp_stream8.hip, mlp_stream4.hip and
// mlp_fused_bf16.hip (gemm_plan / gemm_bf16_plan stay beside their kernels: they encode those kernels' tile shapes).
//   plan_layer            one layer: a GEMM form, else fc_kernel
//   plan_chains           one or two chains: a stream kernel (stream_plan), else chain_kernel (chain_plan)
//   plan_fused_bf16       DLRM in one launch with its bf16 layers (fused_bf16_kernel)
//   plan_fused_bf16_sum   NCF likewise (fused_bf16_sum_kernel)
// The three one-launch forms keep a slab of rows in LDS from the first input to the last layer: X0 (the first chain's
// input) | RS (what the first chain's last layer writes and the second chain reads, beside the pooled rows) | RI (dot: the
// interaction's output, the second chain's input) | P | Q (ping-pong outputs of the other layers).  lay_slabs places them,
// hop tells a layer which two it reads and writes.
#include <string.h>

#include "mlp_stream.h"

namespace drs {
namespace {

constexpr size_t kLdsBudget = 156 * 1024;
// copies of SArgs::tiles and SArgs::L the packed stream kernels keep in LDS, in floats
constexpr int kTableFloats = 4 * DRS_MAX_STREAM_TILES + (int)(sizeof(SLayer) / 4) * DRS_MAX_STREAM_LAYERS;

inline int pad64(int n) { return (n + 63) & ~63; }
inline int pad4(int n) { return (n + 3) & ~3; }
inline int chunks64(int K) { return (K + 63) / 64; }

// ---- chain_kernel / fc_kernel: K chunks staged through LDS ----

size_t stage_bytes(int kc, int nbuf) { return sizeof(float) * (size_t)nbuf * (16 + kFcPassCols) * (kc + 4); }

// Fewest K rounds that fit the LDS budget next to `extra` bytes of slabs.
// force_kc: drs_set_option "mlp_kc" (0 = fewest rounds that fit)
bool pick_kc(int maxK, size_t extra, int force_kc, int* kc_out, int* nbuf_out) {
  const int cands[4] = {256, 192, 128, 64};
  int best_kc = 0, best_nbuf = 0, best_rounds = 1 << 30;
  for (int kc : cands) {
    if (force_kc && kc != force_kc) continue;
    const int rounds = (maxK + kc - 1) / kc;
    const int nbuf = rounds > 1 ? 2 : 1;
    if (stage_bytes(kc, nbuf) + extra > kLdsBudget) continue;
    if (rounds < best_rounds || (rounds == best_rounds && kc < best_kc)) {
      best_rounds = rounds; best_kc = kc; best_nbuf = nbuf;
    }
  }
  if (!best_kc) return false;
  *kc_out = best_kc; *nbuf_out = best_nbuf;
  return true;
}

int chain_slab_ld2(const ChainArgs& a, const ChainArgs* b) {
  int w = 4;
  for (int l = 1; l < a.n_layers; ++l) w = a.width[l] > w ? a.width[l] : w;  // slabs hold layer outputs
  if (b) for (int l = 1; l < b->n_layers; ++l) w = b->width[l] > w ? b->width[l] : w;
  return pad4(w) + 4;
}

// ldA > 0: the chains' input slab (16 x K0) is preloaded into LDS (see run_chain)
bool chain_plan(const ChainArgs& a, const ChainArgs* b, const Tune& tune, int* kc, int* nbuf, size_t* lds, int* ldA) {
  int maxK = 1, k0 = a.width[0];
  for (int l = 0; l < a.n_layers; ++l) maxK = a.width[l] > maxK ? a.width[l] : maxK;
  if (b) {
    for (int l = 0; l < b->n_layers; ++l) maxK = b->width[l] > maxK ? b->width[l] : maxK;
    k0 = b->width[0] > k0 ? b->width[0] : k0;
  }
  const size_t slabs = sizeof(float) * (size_t)2 * 16 * chain_slab_ld2(a, b);
  const int lda = pad4(k0) + 4;
  const size_t pre = (tune.mlp_preload && k0 <= 640) ? sizeof(float) * (size_t)16 * lda : 0;
  if (pre && pick_kc(maxK, slabs + pre, tune.mlp_kc, kc, nbuf)) {
    *lds = stage_bytes(*kc, *nbuf) + slabs + pre;
    *ldA = lda;
    return true;
  }
  if (!pick_kc(maxK, slabs, tune.mlp_kc, kc, nbuf)) return false;
  *lds = stage_bytes(*kc, *nbuf) + slabs;
  *ldA = 0;
  return true;
}

// ---- the one-launch forms: slabs ----

struct Slab { int off, ld; };                     // LDS float offset (-1: no such slab), floats between two rows
struct Slabs { Slab x0, rs, ri, p, q; int end; };

// `rows` (16 | 32) rows per slab, 64 m + lpad (4 | 8) floats apart, from float offset `base` on.  rs_cols / ri_cols 0: no
// RS / RI.  mids: the widths of the layer outputs that ping-pong between P and Q, in layer order (the first goes to P).
// q_may_share_x0 (a single chain): X0 is dead once layer 0 has run (the barrier behind it) and Q is first written by
// layer 1 -- Q lives in X0's space when it fits there (RM3's 416-512-256-1 top chain at 32 rows: 164 KB -> 130 KB).
Slabs lay_slabs(int base, int rows, int lpad, int k0, int rs_cols, int ri_cols, const int* mids, int n_mids,
                bool q_may_share_x0) {
  Slabs s;
  int off = base;
  auto take = [&](Slab& b, int cols, bool on) {
    b.off = on ? off : -1; b.ld = on ? pad64(cols) + lpad : 0;
    off += rows * b.ld;
  };
  take(s.x0, k0, true);
  take(s.rs, rs_cols, rs_cols > 0);
  take(s.ri, ri_cols, ri_cols > 0);
  int w[2] = {0, 0};
  for (int i = 0; i < n_mids; ++i) w[i & 1] = pad64(mids[i]) > w[i & 1] ? pad64(mids[i]) : w[i & 1];
  s.p.ld = w[0] + lpad; s.q.ld = w[1] + lpad;
  s.p.off = off; off += w[0] ? rows * s.p.ld : 0;
  const bool share = q_may_share_x0 && w[1] && s.q.ld <= s.x0.ld;
  s.q.off = share ? s.x0.off : off; off += w[1] && !share ? rows * s.q.ld : 0;
  s.end = off;
  return s;
}

// the ping-pong widths of chain a, then b (may be null): every layer's output but a chain's last
int mid_widths(const ChainArgs& a, const ChainArgs* b, int* mids) {
  int n = 0;
  for (int l = 0; l + 1 < a.n_layers; ++l) mids[n++] = a.width[l + 1];
  if (b) for (int l = 0; l + 1 < b->n_layers; ++l) mids[n++] = b->width[l + 1];
  return n;
}

// columns of its output slab that layer i of n (the first na: the first chain) fills, zeros from N on: a chain's last layer
// writes exactly N, any other up to the next multiple of 64 (the next layer's padded k reads zeros)
inline int hop_pad(int i, int na, int n, int N) { return i == na - 1 || i == n - 1 ? N : pad64(N); }

// What layer i reads and writes.  An intermediate layer writes P or Q in turn; the last layer of the first chain writes
// RS (from column 0: a caller with something in front of it moves on) and the second chain then reads RI behind the dot
// interaction, else RS; the last layer of all writes no slab.
struct Hop { Slab in, out; int out_pad; bool last_of_chain, last_of_all; };
Hop hop(const Slabs& s, int i, int na, int n, int N) {
  const int m = i - (i >= na ? 1 : 0);              // intermediate layers before this one
  Hop h;
  h.last_of_all = i == n - 1;
  h.last_of_chain = h.last_of_all || i == na - 1;
  h.in = i == 0 ? s.x0 : i == na ? (s.ri.off >= 0 ? s.ri : s.rs) : ((m - 1) & 1) ? s.q : s.p;
  h.out = h.last_of_all ? Slab{-1, 0} : h.last_of_chain ? s.rs : (m & 1) ? s.q : s.p;
  h.out_pad = hop_pad(i, na, n, N);
  return h;
}

// The dot join: the first chain writes the dense_out slot of T, the interaction turns T [F x D per row] into R [D + P per
// row], the second chain reads R.  *P: the pairs.
bool check_dot_join(const ChainArgs& a, const ChainArgs& b, const DotArgs& dot, int* P) {
  const int d_out = a.width[a.n_layers];
  *P = dot.F * (dot.F - 1) / 2 + (dot.itself ? dot.F : 0);
  return dot.T == a.y && dot.ldt == a.ldy && dot.R == b.x && dot.ldr == b.ldx && dot.D == d_out && !(d_out & 3) &&
         b.width[0] == d_out + *P && dot.F >= 2;
}

// ---- stream_kernel / stream4_kernel ----

// What the steps of stream_plan share: the launch, then the form (choose_form).
struct StreamJob {
  const ChainArgs& a;
  const ChainArgs* b;
  const Tune& tune;
  const DotArgs* dot;
  const SumArgs* sum;
  int na, n, d_out, dotP;      // layers of the first chain | of both
  bool pk, f3;                 // packed twins | stream4_kernel and its step table
  int ns, SR, lpad;            // column slices of the split layer (0: none) | rows per workgroup | slab row padding
  const ChainArgs& chain(int i) const { return i < na ? a : *b; }
  int at(int i) const { return i < na ? i : i - na; }
  int K(int i) const { return chain(i).width[at(i)]; }
  int N(int i) const { return chain(i).width[at(i) + 1]; }
  const float* W(int i) const { return chain(i).W[at(i)]; }
  // NCF's join: the branch's last layer writes behind the summed block and zero-fills the predictor's padded k
  int out_pad(int i) const { return sum && i == na - 1 ? pad64(b->width[0]) - sum->cols : hop_pad(i, na, n, N(i)); }
  int bias_floats() const { int f = 0; for (int i = 0; i < n; ++i) f += pad4(N(i)); return f; }
};

// Join geometry, arena residency, alignment, back-to-back biases.
bool stream_eligible(StreamJob& j, const XSrc& xs) {
  const ChainArgs &a = j.a, *b = j.b;
  const SumArgs* sum = j.sum;
  const Tune& tune = j.tune;
  const int d_out = j.d_out;
  // second chain must read the buffer the first one writes (dense_out slot in front)
  if (j.dot) {
    if (!b || !check_dot_join(a, *b, *j.dot, &j.dotP)) return false;
  } else if (sum) {
    // [ sum of two column blocks | first chain's output ] -> second chain
    if (!b || sum->cols <= 0 || (sum->cols & 3) || (sum->col_a & 3) || (sum->col_b & 3) || (sum->ld & 3) ||
        (sum->ldd & 3) || !aligned16(sum->src) || !aligned16(sum->dst) || b->x != sum->dst ||
        b->ldx != sum->ldd || a.y != sum->dst + sum->cols || a.ldy != sum->ldd ||
        b->width[0] != sum->cols + d_out || (d_out & 3))
      return false;
  } else if (b && (b->x != a.y || b->ldx != a.ldy || d_out > b->width[0] || (d_out & 3))) {
    return false;
  }
  // every weight matrix must live inside the engine's arena (tile addresses are 32-bit byte offsets from its base),
  // 16-byte aligned like every input; every K a multiple of 4
  if (!tune.w_arena || tune.w_arena_floats >= (1ull << 30)) return false;
  for (int i = 0; i < j.n; ++i) {
    const float* w = j.W(i);
    if (w < tune.w_arena || w + (int64_t)j.K(i) * j.N(i) > tune.w_arena + tune.w_arena_floats) return false;
    if (!aligned16(w) || (j.K(i) & 3)) return false;
  }
  if (!aligned16(a.x) || (a.ldx & 3) || (b && (!aligned16(b->x) || (b->ldx & 3)))) return false;
  for (int i = 0; i < xs.q.n_q; ++i) if (!aligned16(xs.x[i])) return false;
  // biases back to back, each padded to 4 floats (how the engine's arena lays them out)
  const float* expect = a.b[0];
  if (!expect) return false;
  for (int i = 0; i < j.n; ++i) {
    if (j.chain(i).b[j.at(i)] != expect) return false;
    expect += pad4(j.N(i));
  }
  return true;
}

// stream4_kernel's cut of layer i into steps: a pass is four waves x tpw (1 / 2 / 4) tiles of 16 columns, a step one
// 64-k chunk of a pass.  The split layer: slice 0's tiles, one pass.
struct Steps4 { int tpw, tpp, npass, nch; };
Steps4 steps4(const StreamJob& j, int i) {
  const int nch = chunks64(j.K(i));
  if (j.ns && i == j.na) { const int tpw = j.N(i) / j.ns / 64; return {tpw, 4 * tpw, 1, nch}; }
  const int etl = (j.out_pad(i) + 15) / 16;         // (out_pad >= N)
  int t = 1;
  while (t < 4 && etl > 4 * t) t *= 2;
  return {t, 4 * t, (etl + 4 * t - 1) / (4 * t), nch};
}
inline int tiles8(int K, int N) { return ((N + 127) / 128) * chunks64(K); }   // stream_kernel: 128-column passes

Slabs stream_slabs(const StreamJob& j, int rows) {
  int mids[DRS_MAX_STREAM_LAYERS];
  const int n_mids = mid_widths(j.a, j.b, mids);
  const int rs_cols = !j.b ? 0 : j.dot ? j.dot->F * j.dot->D : j.b->width[0];
  // LDS layout (floats): [sB 2x128x68 (LDS-staged form only)][X0][RS][RI][P][Q][biases][tables]
  return lay_slabs(j.pk ? 0 : 2 * 128 * 68, rows, j.lpad, j.a.width[0], rs_cols, j.dot ? j.b->width[0] : 0, mids, n_mids,
                   rows == 32 && !j.b);
}

// Form choice: pk, stream4 or stream8, ns, SR.  false: no stream form.  d_wait: the launch polls Done::wait_flag.
bool choose_form(StreamJob& j, bool d_wait) {
  const Tune& tune = j.tune;
  const ChainArgs* b = j.b;
  // the packed form ("mlp_stream" 2): every layer must carry its packed twin (engine layers of the
  // bottom / top / final / task MLPs do: drs_set_fc)
  j.pk = tune.mlp_stream >= 2 && tune.w_packed_hi > tune.w_packed_lo;
  for (int i = 0; i < j.n; ++i) {
    const uint64_t o = (uint64_t)(j.W(i) - tune.w_arena);
    j.pk = j.pk && o >= tune.w_packed_lo && o < tune.w_packed_hi;
  }
  // "mlp_stream" 4: stream4_kernel -- four waves x up to four tiles, b128 activation operands, a step table run segment
  // by segment; its steps must fit the descriptor table
  j.f3 = j.pk && tune.mlp_stream == 4;
  // Column-split form ("mlp_nsplit"; SArgs::ns): the first layer of the second chain over ns workgroups per slab of rows.
  // A slice is ONE pass of the four waves: N / ns in {64, 128, 256} columns (1 / 2 / 4 tiles per wave), N a multiple of
  // 64 (no zero pad in the slab), and the layer must hand its outputs on through LDS (not the chain's last).
  j.ns = 0;
  if (j.f3 && b && !j.sum && b->n_layers >= 2 && tune.mlp_nsplit >= 2 && tune.xbuf && tune.xcnt && !d_wait &&
      j.a.M <= tune.mlp_nsplit_rows && j.a.M <= tune.xbuf_rows && b->width[1] <= tune.xbuf_cols && !(b->width[1] & 63)) {
    for (int S = tune.mlp_nsplit >= 4 ? 4 : 2; S >= 2 && !j.ns; S >>= 1) {
      const int cw = b->width[1] / S;
      if (b->width[1] % S == 0 && (cw == 64 || cw == 128 || cw == 256)) j.ns = S;
    }
  }
  if (j.f3) {
    int st = 0;
    for (int i = 0; i < j.n; ++i) {
      const Steps4 s = steps4(j, i);
      st += s.npass * s.nch;
      j.f3 = j.f3 && j.N(i) <= 4080 && j.K(i) <= 4096;
    }
    j.f3 = j.f3 && st <= DRS_MAX_STREAM_TILES;
  }
  if (!j.f3) j.ns = 0;
  // stream_kernel: the zero pad behind the summed block must fall in an existing pass
  if (j.sum && !j.f3 && pad64(b->width[0]) - j.sum->cols > ((j.d_out + 127) / 128) * 128) return false;
  j.lpad = j.f3 ? 8 : 4;      // slab rows: 64 m + 8 floats apart in the b128 form, 64 m + 4 else
  // rows per workgroup: 16, or 32 for stream4_kernel's two-halves form ("mlp_rows32": launches of at
  // least that many rows, no summed input, slabs that still fit LDS)
  j.SR = 16;
  if (j.f3 && !j.sum && tune.mlp_rows32 > 0 && j.a.M >= tune.mlp_rows32) {
    // (+ 4: 16 bytes stricter than the layout stream_plan then checks -- kept so that every launch decides as it always did)
    const size_t fl = (size_t)stream_slabs(j, 32).end + j.bias_floats() + kTableFloats + 4;
    if (sizeof(float) * fl <= kLdsBudget) j.SR = 32;
  }
  return true;
}

void fill_layers(const StreamJob& j, const Slabs& S, bool publish, SArgs& p) {
  int boff = p.bias_off;
  for (int i = 0; i < j.n; ++i) {
    const ChainArgs& c = j.chain(i);
    const int l = j.at(i);
    const Hop h = hop(S, i, j.na, j.n, j.N(i));
    SLayer& L = p.L[i];
    L.W = c.W[l]; L.w_off = (uint32_t)(c.W[l] - j.tune.w_arena);
    L.wp_off = L.w_off + (uint32_t)(((uint64_t)c.width[l] * c.width[l + 1] + 63) / 64 * 64);   // twin right behind W
    L.b = c.b[l]; L.K = c.width[l]; L.N = c.width[l + 1]; L.act = c.act[l];
    L.in_off = h.in.off; L.in_ld = h.in.ld;
    L.out_off = h.out.off; L.out_ld = h.out.ld; L.out_pad = j.out_pad(i);
    L.out_col0 = j.sum && i == j.na - 1 ? j.sum->cols : 0;      // behind the summed block
    L.b_off = boff; boff += pad4(L.N);
    if (h.last_of_chain) { L.g_out = c.y; L.g_ld = c.ldy; L.g_sc1 = h.last_of_all && publish; }
  }
  p.n_layers = j.n;
}

// stream4_kernel: one descriptor per STEP (layer, pass of 4 x tpw tiles, 64-k chunk), and the arena range of the twins.
// wp_off: chunk c of the twin's first 128-column pass; in_ld: floats between two such passes;
// a_off: low half = LDS offset of (row 0, k = 64 c) of the input slab, high half = its leading dimension
void write_steps4(const StreamJob& j, SArgs& p, NSplit* nsp) {
  int ti = 0, inter_at = j.dot ? 0 : -1;
  for (int l = 0; l < p.n_layers; ++l) {
    const SLayer& L = p.L[l];
    const Steps4 s = steps4(j, l);
    const int ntl = (L.N + 15) / 16;
    if (j.dot && l < j.na) inter_at += s.npass * s.nch;
    if (j.b && !j.sum && l == j.na) p.wait_tile = ti;
    if (j.ns && l == j.na) {                 // this launch's split layer
      p.ns = j.ns;
      nsp->t0 = ti; nsp->t1 = ti + s.nch; nsp->tps = s.tpp; nsp->n = L.N; nsp->off = L.out_off; nsp->ld = L.out_ld;
      nsp->xbuf = j.tune.xbuf; nsp->xcnt = j.tune.xcnt;
    }
    for (int ps = 0; ps < s.npass; ++ps)
      for (int c = 0; c < s.nch; ++c) {
        STile& t = p.tiles[ti++];
        t.wp_off = L.wp_off + (uint32_t)c * 8192u;
        t.a_off = (L.in_off + c * 64) | (L.in_ld << 16);
        t.in_ld = s.nch * 8192;
        const bool last_of_layer = c == s.nch - 1 && ps == s.npass - 1;
        t.info = (ps * s.tpp) | (ntl << 8) | (c == s.nch - 1 ? S3_LAST : 0) | (last_of_layer ? S3_BARRIER : 0) |
                 (last_of_layer ? 0 : S3_ANEXT) | (s.tpw << S3_TPW_SHIFT) | (c == 0 ? S3_FIRST : 0) | (l << 24);
      }
  }
  if (inter_at >= 0 && inter_at < ti) p.tiles[inter_at].info |= S3_INTERACT;
  p.n_table = p.n_tiles = ti;
  // the arena range that holds the packed twins of this launch's layers (L2 warm-up)
  uint64_t lo = ~0ull, hi = 0;
  for (int l = 0; l < p.n_layers; ++l) {
    const uint64_t b = p.L[l].wp_off, e = b + (uint64_t)stream_packed_floats(p.L[l].K, p.L[l].N);
    lo = b < lo ? b : lo; hi = e > hi ? e : hi;
  }
  lo &= ~1023ull;                                          // 4-KB granules
  hi = (hi + 1023) & ~1023ull;
  if (hi > j.tune.w_arena_floats) hi = j.tune.w_arena_floats & ~1023ull;
  if (hi < lo + 1024) { lo = 0; hi = 1024; }
  p.warm_off = (uint32_t)lo;
  p.warm_bytes = (int32_t)((hi - lo) * 4);
}

// stream_kernel<packed>: one descriptor per round (layer, 128-column pass, 64-k chunk); inter_at: SArgs::inter_tile or -1
void write_tiles8(SArgs& p, int inter_at) {
  int ti = 0;
  for (int l = 0; l < p.n_layers; ++l) {
    const SLayer& L = p.L[l];
    const int nch = chunks64(L.K), npass = (L.N + 127) / 128;
    for (int ps = 0; ps < npass; ++ps)
      for (int c = 0; c < nch; ++c) {
        STile& t = p.tiles[ti];
        t.wp_off = L.wp_off + (uint32_t)(ps * nch + c) * 8192u;
        t.a_off = L.in_off + c * 64;
        t.in_ld = L.in_ld;
        const int ncols = L.N - ps * 128;
        t.info = (ncols > 0xffff ? 0xffff : ncols) | (c == nch - 1 ? 1 << 16 : 0) |
                 (c == nch - 1 && ps == npass - 1 ? 1 << 17 : 0) | (ti == inter_at ? 1 << 18 : 0) | (l << 24);
        ++ti;
      }
  }
  p.n_table = ti;
}

// SInput 0 / 1 and the dot block.
void fill_inputs(const StreamJob& j, const Slabs& S, const XSrc& xs, SArgs& p) {
  const ChainArgs &a = j.a, *b = j.b;
  SInput& i0 = p.in[0];
  i0.src = a.x; i0.ld = a.ldx; i0.col0 = 0; i0.cols = a.width[0]; i0.cols_pad = pad64(a.width[0]);
  i0.lds_off = S.x0.off; i0.lds_ld = S.x0.ld; i0.lds_col0 = 0; i0.use_xs = xs.q.n_q > 0;
  p.in[0].col2 = p.in[1].col2 = -1;
  p.n_inputs = b ? 2 : 1;
  if (b) {           // the pooled rows beside the dense_out slot of RS, or NCF's two summed blocks in front of it
    const int rs_cols = j.dot ? j.dot->F * j.dot->D : b->width[0];
    SInput& i1 = p.in[1];
    i1.src = j.dot ? j.dot->T : b->x; i1.ld = j.dot ? j.dot->ldt : b->ldx; i1.col0 = j.d_out; i1.cols = rs_cols - j.d_out;
    i1.cols_pad = pad64(rs_cols) - j.d_out;
    i1.lds_off = S.rs.off; i1.lds_ld = S.rs.ld; i1.lds_col0 = j.d_out; i1.use_xs = 0;
    if (j.sum) {
      i1.src = j.sum->src; i1.ld = j.sum->ld; i1.col0 = j.sum->col_a; i1.col2 = j.sum->col_b;
      i1.cols = i1.cols_pad = j.sum->cols; i1.lds_col0 = 0;
      i1.g_dst = j.sum->dst; i1.g_ldd = j.sum->ldd;
    }
  }
  if (j.dot) {
    p.inter_on = 1; p.F = j.dot->F; p.D = j.dot->D; p.itself = j.dot->itself ? 1 : 0; p.P = j.dotP;
    p.t_off = S.rs.off; p.t_ld = S.rs.ld; p.r_off = S.ri.off; p.r_ld = S.ri.ld; p.r_pad = pad64(b->width[0]);
    p.g_R = j.dot->R; p.g_ldr = j.dot->ldr;
    for (int l = 0; l < j.na; ++l) p.inter_tile += tiles8(a.width[l], a.width[l + 1]);
  }
}

// the kernel instance: stream4_kernel (the packed step table), else stream_kernel (packed twins | weights staged in LDS)
MlpForm stream_form(const StreamJob& j, const SArgs& p) {
  const bool two = j.tune.mlp_stream_2cu;
  if (p.ns) return j.SR == 32 ? (p.ns == 4 ? MlpForm::stream4_rows32_nsplit4 : MlpForm::stream4_rows32_nsplit2)
                              : (p.ns == 4 ? MlpForm::stream4_nsplit4 : MlpForm::stream4_nsplit2);
  if (j.f3) return j.SR == 32 ? MlpForm::stream4_rows32 : j.sum ? MlpForm::stream4_sum : two ? MlpForm::stream4_2cu : MlpForm::stream4;
  return !j.pk ? MlpForm::stream_lds : (two && p.n_table > 0) ? MlpForm::stream_packed_2cu : MlpForm::stream_packed;
}

// Lay the chain(s) out for a stream kernel (pl: its Done and XSrc set).  false = not applicable.
bool stream_plan(const ChainArgs& a, const ChainArgs* b, const Tune& tune, const DotArgs* dot, const SumArgs* sum,
                 MlpPlan* pl) {
  SArgs& p = pl->sa;
  memset(&pl->ns, 0, sizeof pl->ns);
  memset(&p, 0, sizeof p);
  StreamJob j = {a, b, tune, dot, sum, a.n_layers, a.n_layers + (b ? b->n_layers : 0), a.width[a.n_layers]};
  if (j.n > DRS_MAX_STREAM_LAYERS) return false;
  if (!stream_eligible(j, pl->xs) || !choose_form(j, pl->done.wait_flag != nullptr)) return false;
  // layout: slabs, biases, the packed forms' copies of the step / tile table and of the layers
  const Slabs S = stream_slabs(j, j.SR);
  const int n_bias = j.bias_floats();
  p.sB_off = 0;
  p.tab_off = pad4(S.end + n_bias);
  p.lay_off = p.tab_off + (j.pk ? 4 * DRS_MAX_STREAM_TILES : 0);
  const int off = j.pk ? p.tab_off + kTableFloats : p.tab_off;
  if (sizeof(float) * (size_t)off > kLdsBudget) return false;
  pl->lds = sizeof(float) * (size_t)off;
  p.lds_floats = off;
  p.bias_off = S.end; p.n_bias = n_bias; p.bias = a.b[0]; p.wait_tile = -1;
  fill_layers(j, S, pl->done.counter != nullptr, p);
  // tables: stream4_kernel's steps, or stream_kernel's rounds when they fit the table (else its iterator form)
  for (int i = 0; i < j.n; ++i) p.n_tiles += tiles8(j.K(i), j.N(i));
  fill_inputs(j, S, pl->xs, p);
  if (j.f3) write_steps4(j, p, &pl->ns);
  else if (j.pk && p.n_tiles <= DRS_MAX_STREAM_TILES) write_tiles8(p, dot ? p.inter_tile : -1);
  p.M = a.M; p.zero = tune.zero; p.wbase = tune.w_arena; p.zero_off = tune.w_zero_off; p.dbg = tune.mlp_debug;
  pl->form = stream_form(j, p);
  pl->grid_x = (unsigned)((a.M + j.SR - 1) / j.SR) * (p.ns ? (unsigned)p.ns : 1u);
  pl->grid_y = 1;
  return true;
}

// ---- fused_bf16_kernel / fused_bf16_sum_kernel ----

// X0 | RS | RI | P | Q of 16 rows, 64 m + 4 floats apart, for the fused bf16 forms; false: beyond LDS
bool lay_fused(const ChainArgs& a, const ChainArgs& b, int rs_cols, int ri_cols, MlpPlan* p, Slabs* S) {
  int mids[DRS_MAX_STREAM_LAYERS];
  const int n_mids = mid_widths(a, &b, mids);
  *S = lay_slabs(0, 16, 4, a.width[0], rs_cols, ri_cols, mids, n_mids, false);
  FArgs& f = p->fa;
  f.k0 = a.width[0];
  f.x0_ld = S->x0.ld; f.x0_off = S->x0.off;
  f.rs_ld = S->rs.ld; f.rs_off = S->rs.off;
  if (ri_cols) { f.ri_ld = S->ri.ld; f.ri_off = S->ri.off; }
  if (sizeof(float) * (size_t)S->end > kLdsBudget) return false;
  p->lds = sizeof(float) * (size_t)S->end;
  return true;
}

// layer i of the chains a, b (wb: its bf16 twin or null) between the slabs hop names; returns the hop
Hop fill_flayer(FArgs& f, const Slabs& S, const ChainArgs& a, const ChainArgs& b, int i, const uint16_t* wb, bool publish) {
  const int na = a.n_layers;
  const ChainArgs& c = i < na ? a : b;
  const int l = i < na ? i : i - na;
  const Hop h = hop(S, i, na, na + b.n_layers, c.width[l + 1]);
  FLayer& L = f.L[i];
  L.W = c.W[l]; L.Wb = wb; L.b = c.b[l]; L.K = c.width[l]; L.N = c.width[l + 1]; L.act = c.act[l];
  L.in_off = h.in.off; L.in_ld = h.in.ld;
  L.out_off = h.out.off; L.out_ld = h.out.ld; L.out_pad = h.out_pad;
  if (h.last_of_chain) { L.g_out = c.y; L.g_ld = c.ldy; L.g_sc1 = h.last_of_all && publish; }
  f.n_bf16 += wb ? 1 : 0;
  return h;
}

void fused_grid(MlpPlan* p, MlpForm form) {
  p->form = form;
  p->grid_x = (unsigned)((p->a.M + 15) / 16);
  p->grid_y = 1;
}

}  // namespace

// One layer: a GEMM form (gemm.hip) when the layer has one, else fc_kernel.  A split input row (XSrc::ksplit) is for
// the GEMM forms only.  Wb: a bf16 layer ("mlp_dtype" 2) -- the bf16 GEMM form (gemm_bf16.hip) and no other.
bool plan_layer(const float* x, int64_t ldx, int64_t M, int32_t K, const float* W, const float* b, int32_t N, int32_t act,
                float* y, int64_t ldy, const Tune& tune, const Done* done, const XSrc* xs, MlpPlan* p, const uint16_t* Wb) {
  memset(p, 0, sizeof *p);
  if (done) p->done = *done;
  if (xs) p->xs = *xs;
  ChainArgs& L = p->a;
  L.x = x; L.ldx = ldx; L.M = M; L.n_layers = 1; L.width[0] = K; L.width[1] = N;
  L.W[0] = W; L.b[0] = b; L.act[0] = act; L.y = y; L.ldy = ldy;
  if (Wb) { p->wb = Wb; return gemm_bf16_plan(tune, p); }
  if (N >= 64 && K >= 64 && gemm_plan(tune, p)) return true;
  if (p->xs.ksplit > 0 || !pick_kc(K, 0, tune.mlp_kc, &p->kc, &p->nbuf)) return false;
  p->form = MlpForm::fc;
  p->lds = stage_bytes(p->kc, p->nbuf);
  p->grid_x = (unsigned)((M + 15) / 16);
  p->grid_y = (unsigned)((N + kFcPassCols - 1) / kFcPassCols);
  bool vec = aligned16(x) && aligned16(W) && (ldx & 3) == 0 && (K & 3) == 0;
  for (int i = 0; i < p->xs.q.n_q; ++i) vec = vec && aligned16(p->xs.x[i]);
  p->vec = vec;
  return true;
}

// One or two chains in one launch: the stream kernel when it takes them, else chain_kernel -- which has neither the
// interaction nor the summed input nor the late start.  A single chain is planned only where chain_kernel holds it
// (run_mlp cuts a run of layers shorter until it does).
bool plan_chains(const ChainArgs& a, const ChainArgs* b, const Tune& tune, const Done* done, const XSrc* xs,
                 const DotArgs* dot, const SumArgs* sum, MlpPlan* p) {
  memset(p, 0, sizeof *p);
  if (done) p->done = *done;
  if (xs) p->xs = *xs;
  if (a.n_layers < 1 || a.n_layers > DRS_MAX_CHAIN || (b && (b->n_layers < 1 || b->n_layers > DRS_MAX_CHAIN)))
    return false;
  p->a = a;
  if (b) p->b = *b;
  const bool chain_ok = !dot && !sum && !p->done.wait_flag && chain_plan(a, b, tune, &p->kc, &p->nbuf, &p->lds, &p->lda);
  if (!b && !chain_ok) return false;
  if (tune.mlp_stream && tune.zero && stream_plan(a, b, tune, dot, sum, p))
    return !p->done.wait_flag || can_defer(*p);
  if (!chain_ok) return false;
  bool vec = aligned16(a.x) && (a.ldx & 3) == 0;
  for (int l = 0; l < a.n_layers; ++l) vec = vec && aligned16(a.W[l]) && (a.width[l] & 3) == 0;
  if (b) {
    vec = vec && aligned16(b->x) && (b->ldx & 3) == 0;
    for (int l = 0; l < b->n_layers; ++l) vec = vec && aligned16(b->W[l]) && (b->width[l] & 3) == 0;
  }
  for (int i = 0; i < p->xs.q.n_q; ++i) vec = vec && aligned16(p->xs.x[i]);
  p->form = MlpForm::chain;
  p->vec = vec;
  p->sld = chain_slab_ld2(a, b);
  p->grid_x = (unsigned)((a.M + 15) / 16);
  p->grid_y = 1;
  return true;
}

// Lay the bottom chain a, the interaction and the top chain b out for fused_bf16_kernel.  wb_a / wb_b: per layer its bf16
// twin, or null for an fp32 layer.  false: the form does not take the launch (no bf16 layer, a launch that waits for the
// gather by itself, D not a multiple of 4 under the dot interaction, slabs beyond LDS).  Any K and N otherwise.
bool plan_fused_bf16(const ChainArgs& a, const ChainArgs& b, const uint16_t* const* wb_a, const uint16_t* const* wb_b,
                     const DotArgs* dot, const Done* done, const XSrc* xs, MlpPlan* p) {
  memset(p, 0, sizeof *p);
  if (done) p->done = *done;
  if (!xs || xs->q.n_q < 1 || p->done.wait_flag) return false;
  p->xs = *xs;
  p->a = a; p->b = b;
  const int na = a.n_layers, nb = b.n_layers;
  if (na < 1 || nb < 1 || na > DRS_MAX_CHAIN || nb > DRS_MAX_CHAIN) return false;
  const int d_out = a.width[na];
  int dotP = 0;
  if (dot ? !check_dot_join(a, b, *dot, &dotP) : (b.x != a.y || b.ldx != a.ldy || d_out >= b.width[0])) return false;
  // RS: the dot interaction's T slab, or the top input itself (cat)
  const int rs_cols = dot ? dot->F * dot->D : b.width[0];
  const float* T = dot ? dot->T : b.x;
  const int64_t ldt = dot ? dot->ldt : b.ldx;
  FArgs& f = p->fa;
  Slabs S;
  if (!lay_fused(a, b, rs_cols, dot ? b.width[0] : 0, p, &S)) return false;
  for (int i = 0; i < na + nb; ++i) fill_flayer(f, S, a, b, i, i < na ? wb_a[i] : wb_b[i - na], p->done.counter != nullptr);
  if (!f.n_bf16) return false;
  f.n_layers = na + nb; f.n_bot = na;
  f.M = a.M; f.ldx = a.ldx;
  f.T = T; f.ldt = ldt; f.p_col0 = d_out; f.p_cols = rs_cols - d_out;
  f.p_cols_pad = dot ? f.p_cols : pad64(rs_cols) - d_out;
  bool vx = !(f.k0 & 3) && !(a.ldx & 3);
  for (int i = 0; i < xs->q.n_q; ++i) vx = vx && aligned16(xs->x[i]);
  f.vec_x = vx;
  f.vec_t = aligned16(T) && !(ldt & 3) && !(d_out & 3) && !(f.p_cols & 3);
  if (dot) { f.dot = 1; f.F = dot->F; f.D = dot->D; f.itself = dot->itself ? 1 : 0; f.R = dot->R; f.ldr = dot->ldr; }
  fused_grid(p, MlpForm::fused_bf16);
  return true;
}

// NCF: the MLP branch a (its input: columns of sum.src, the gather's output, behind the two summed blocks), the Sum and
// the one-layer predictor b for fused_bf16_sum_kernel.  wb_a / wb_b as above.  false: the form does not take the launch
// (no bf16 layer, a launch that waits for the gather by itself, buffers that are not laid out as NCF's, slabs beyond
// LDS).  Any D, K and N otherwise.
bool plan_fused_bf16_sum(const ChainArgs& a, const ChainArgs& b, const uint16_t* const* wb_a, const uint16_t* wb_b,
                         const SumArgs& sum, const Done* done, MlpPlan* p) {
  memset(p, 0, sizeof *p);
  if (done) p->done = *done;
  if (p->done.wait_flag) return false;
  p->a = a; p->b = b;
  const int na = a.n_layers, D = sum.cols;
  if (na < 1 || na > DRS_MAX_CHAIN || b.n_layers != 1 || D < 1 || a.M < 1) return false;
  const int wl = a.width[na];
  const int64_t col_x = a.x - sum.src;
  // T = [ emb0 | emb1 | ... branch input ... ], R = [ mf | branch output ] = the predictor's input
  if (sum.col_a != 0 || sum.col_b < D || col_x < (int64_t)sum.col_b + D || col_x + a.width[0] > sum.ld || a.ldx != sum.ld ||
      a.y != sum.dst + D || a.ldy != sum.ldd || b.x != sum.dst || b.ldx != sum.ldd || b.width[0] != D + wl || D + wl > sum.ldd)
    return false;
  FArgs& f = p->fa;
  Slabs S;
  if (!lay_fused(a, b, D + wl, 0, p, &S)) return false;
  for (int i = 0; i <= na; ++i) {
    const Hop h = fill_flayer(f, S, a, b, i, i < na ? wb_a[i] : wb_b, p->done.counter != nullptr);
    if (h.last_of_chain && !h.last_of_all) {   // behind mf; a bf16 predictor reads zeros up to its padded K
      f.L[i].out_off += D;
      f.L[i].out_pad = wb_b ? pad64(D + wl) - D : wl;
    }
  }
  if (!f.n_bf16) return false;
  f.n_layers = na + 1; f.n_bot = na;
  f.M = a.M;
  f.T = sum.src; f.ldt = sum.ld; f.p_col0 = (int)col_x; f.p_cols = sum.col_b;
  f.D = D; f.R = sum.dst; f.ldr = sum.ldd;
  f.vec_t = aligned16(sum.src) && !(sum.ld & 3) && !(D & 3) && !(sum.col_b & 3) && !(col_x & 3) && !(f.k0 & 3);
  f.vec_x = f.vec_t && aligned16(sum.dst) && !(sum.ldd & 3);
  fused_grid(p, MlpForm::fused_bf16_sum);
  return true;
}

}  // namespace drs
