// Multi-table SparseLengthsSum gather-reduce for gfx950 (MI355X).
//
// Replaces the T x SparseLengthsSum([tbl, idx, len]) operators emitted by
// create_emb (reference models/dlrm_s_caffe2.py:281-329, op at :317-325) with ONE
// launch over all B*T bags of a query.  HBM-bound: every pooled row is a random
// D*4-byte read (128 B at D=32, 256 B at D=64) out of multi-GB tables.
//
// Mapping to CDNA4
//   - a row is read by G = D/4 adjacent lanes, 4 floats (16 B) per lane:
//     one global_load_dwordx4 per lane, 64/G whole rows per wave-instruction,
//     each row a single contiguous, aligned segment (tables are 256-B aligned and
//     D*4 is a multiple of 16).
//   - EXACT variant: each G-lane group owns one bag and walks its rows in index
//     order, so every output column is the sequential fp32 sum
//     ((r0 + r1) + r2) + ... -- bit-identical to the Caffe2 CPU perfkernel the
//     reference runs.  64/G bags progress concurrently in a wave; U independent
//     row loads are kept in flight per lane to cover the ~0.5-1 us HBM latency.
//   - SPLIT variant: the wave owns one bag, lane group g takes rows g, g+64/G, ...
//     and the partial sums are combined with a wave-wide xor butterfly
//     (different fp32 summation order -> tolerance compare, not bitwise).
//   - FLAT variant (fixed-length bags -- every shipped reference config generates
//     num_indices_per_lookup_fixed inputs): a wave owns BPW consecutive bags of one sample
//     (R = BPW*L flattened rows), lane group g takes rows g, g+64/G, ... and ALL of a
//     lane's NL = ceil(R / (64/G)) row loads are issued before the first one is consumed;
//     the indices come from ONE coalesced read (lane i owns row i) and reach the loading
//     lanes through the cross-lane network (ds_bpermute), not LDS.  Two dependent HBM round
//     trips per wave (indices, rows) instead of the five or more of a ring walk: short bags
//     (RM3: 20 x 128 B) and single-query launches spend their time streaming, not waiting.
//   - the bag's offsets come from the staged prefix-sum vector; its indices are
//     staged in LDS by one coalesced read per wave (CH at a time) and then
//     broadcast-read by the lanes of the group; no __syncthreads: a wave only
//     reads what it wrote itself.
//   - 64-thread workgroups: B*T bags of a single query are few (2048 at RMC1
//     b=256), so the launch is cut into as many workgroups as possible to cover
//     all 256 CUs; workgroups never cooperate.
//   - index range is checked per row (Caffe2 ENFORCEs it): an out-of-range index
//     raises bit 0 of *err and contributes zero instead of faulting.
//   - WEIGHTED launches (SparseLengthsWeightedSum, SlsArgs::wgt): the ring walk (sequential and split) and the any-width
//     form have a weighted instance (template parameter WGT) in which a row's weight travels with its index -- staged in a
//     second LDS array by the same coalesced read, read beside the index when the row load is issued, and applied as
//     acc = fma(w, x, acc) per column (rowwise types: s = w * scale, b = w * bias into the same row step).  The unweighted
//     instances are the code they were.  The flat and one-lookup forms take a weighted launch under "sls_weighted_flat" 1
//     only; their kernel templates (sls_dev.h) become weighted through the element type Wgt<policy>, and sls_wflat.hip
//     holds those instances.
#include "drs_internal.h"
#include "launch_host.h"
#include "owner_dev.h"
#include "sls_dev.h"

namespace drs {
namespace {

constexpr int kChunk = 128;  // indices staged in LDS per bag per round

// NT: the hint must be a COMPILE-TIME property of the load: a run-time `nt ? ld_nt(p) : *p` is if-converted
// into one plain load (the hint is metadata the merge drops): measured in the ISA, 0 of 5 / 2 of 14 loads kept it.
// G lanes per row, 4 elements per lane.  U (row loads per register ring and lane) is 4: two rings, so 4..8 loads in
// flight per lane, the waves per CU provide the rest of the memory-level parallelism.  (8, 16 and 20 were options until
// round 4 -- measured equal or slower on every shape -- as was a 16-lane x 8-byte form for D == 32.)
// WGT: the weighted instance (a.wgt; a query whose entry is null weighs every row 1.0f and keeps its unweighted bits).  With
// WGT == false nothing below that names a weight exists: the unweighted instances compile to what they were.
template <int G, bool EXACT, bool NT = false, class E = F32, bool WGT = false>
__global__ __launch_bounds__(64) void sls_kernel(SlsArgs a) {
  using piece = typename E::piece;
  using sbt = typename E::sb;
  using wt = std::conditional_t<WGT, float, NoSb>;   // a row's weight beside its piece in the rings
  constexpr int U = 4;
  constexpr int NG = 64 / G;                  // lane groups per wave
  constexpr int BAGS = EXACT ? NG : 1;        // bags per wave
  constexpr int STEP = EXACT ? 1 : NG;        // row stride between a lane's loads
  constexpr int OWNERS = EXACT ? G : 64;      // lanes that stage one bag's indices
  __shared__ __attribute__((aligned(16))) int32_t s_idx[BAGS][kChunk];
  __shared__ __attribute__((aligned(16))) float s_wgt[WGT ? BAGS : 1][WGT ? kChunk : 1];   // (never referenced without WGT)

  // live timing (bench.py roofline leg): first/last constant-rate clock tick of every
  // workgroup; the host takes max(end) - min(start) as the launch duration
  if (a.ts && threadIdx.x == 0) a.ts[2 * blockIdx.x] = wall_clock64();

  const int lane = threadIdx.x;
  const int g = lane / G;
  const int gl = lane - g * G;
  const int col = min(gl * 4, a.D - 4);       // clamp idle lanes onto valid columns
  const bool col_ok = gl * 4 < a.D;

  const int64_t n_bags = (int64_t)a.q.cum[a.q.n_q] * a.T;
  const int64_t bag = (int64_t)blockIdx.x * BAGS + (EXACT ? g : 0);
  const bool bag_ok = bag < n_bags;
  const int smp = bag_ok ? (int)(bag / a.T) : 0;            // valid-sample number over all queries
  const int t = bag_ok ? (int)(bag - (int64_t)smp * a.T) : 0;
  DRS_OWNER_OF(a, smp, b, vrow, ulen, qidx, qoff)   // which coalesced query owns this sample

  // fixed-length bags (every shipped reference config: num_indices_per_lookup_fixed) need
  // no offsets: one dependent HBM round trip less before the first row load can issue
  int beg, end;
  if (ulen >= 0) {
    beg = bag_ok ? b * ulen : 0;
    end = bag_ok ? beg + ulen : 0;
  } else {
    const int32_t* __restrict__ offp = qoff + (int64_t)t * a.off_stride;
    beg = bag_ok ? offp[b] : 0;
    end = bag_ok ? offp[b + 1] : 0;
  }
  const int32_t* __restrict__ ip = qidx + (int64_t)t * a.idx_stride;
  // the owning query's weights, laid out like its indices (null: an unweighted query inside a weighted launch)
  [[maybe_unused]] const float* wp = nullptr;
  if constexpr (WGT) {
    const float* qwgt = a.wgt[0];
    DRS_OWNER_CHAIN(a.q, smp, qwgt = in ? a.wgt[i] : qwgt;)
    wp = qwgt ? qwgt + (int64_t)t * a.idx_stride : nullptr;
  }
  const typename E::elem* __restrict__ W = table_base<E>(a.tables) + a.tab_off[t] + col_elems<E>(col);
  const uint32_t rows = (uint32_t)a.tab_rows[t];
  const int64_t D = a.D;
  // row stride in load-width units: rows * D / 4 < 2^32 (rows * D < 2^33 is enforced at table creation; int8 rowwise:
  // rows * S / 4 < 2^32, int4 rowwise: rows * S / 2 < 2^32, enforced by the conversion)
  const uint32_t Dv = E::pieces_per_row(a.D);
  const int sbd = sb_delta<E>(a.D, col);
  DRS_ROW_LINES(E, a, ln)

  int32_t* my_idx = s_idx[EXACT ? g : 0];
  [[maybe_unused]] float* my_wgt = s_wgt[WGT && EXACT ? g : 0];
  const int me = EXACT ? gl : lane;           // my slot among the owners
  const int first = EXACT ? 0 : g;            // first row (within a chunk) of this lane
  float4 acc = vzero4();
  bool bad = false;

  // Control flow is kept WAVE-UNIFORM: every lane runs as many rounds as the
  // longest bag in the wave needs (shorter bags re-read their last row, an L1
  // hit, and add +0.0f in its place, weighted or not: the row's value is dropped).  With scalar branches each pipeline arm below is one
  // straight-line block, so the compiler's s_waitcnt vmcnt(N) counts stay exact
  // and U..2U row loads per lane remain outstanding.
  const int len = end - beg;
  int len_max = len;
#pragma unroll
  for (int m = G; m < 64; m <<= 1) len_max = max(len_max, __shfl_xor(len_max, m));
  len_max = __builtin_amdgcn_readfirstlane(len_max);

  for (int c = 0; c < len_max; c += kChunk) {
    const int n = min(kChunk, len - c);            // this lane's rows in the chunk (may be <= 0)
    const int n_u = min(kChunk, len_max - c);      // uniform: rounds the wave runs
    const int last = max(n - 1, 0);
    const int j0 = beg + c;
    // stage the next indices of each bag in LDS: coalesced, clamped (branch-free)
    for (int c0 = 0; c0 < n_u; c0 += 4 * OWNERS) {
      int32_t tmp[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) tmp[q] = n > 0 ? ip[j0 + min(c0 + q * OWNERS + me, last)] : 0;
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (c0 + q * OWNERS + me < kChunk) my_idx[c0 + q * OWNERS + me] = tmp[q];
      if constexpr (WGT) {   // the weights of the same positions (< n only, like the indices), by the same coalesced read
        float wtmp[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) wtmp[q] = n > 0 && wp ? wp[j0 + min(c0 + q * OWNERS + me, last)] : 1.0f;
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (c0 + q * OWNERS + me < kChunk) my_wgt[c0 + q * OWNERS + me] = wtmp[q];
      }
    }
    __builtin_amdgcn_wave_barrier();

    // U independent, unconditional row loads
    // (weighted: a row's weight is read beside its index, and an out-of-range row takes the weight 0)
    auto issue = [&](piece (&ring)[U], sbt (&rsb)[U], wt (&rw)[U], int pos) {
      uint32_t r[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        r[u] = (uint32_t)my_idx[min(pos + u * STEP, last)];
        if constexpr (WGT) rw[u] = my_wgt[min(pos + u * STEP, last)];
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        bad |= (pos + u * STEP < n) && (r[u] >= rows);
        if constexpr (WGT) rw[u] = r[u] < rows ? rw[u] : 0.0f;
        r[u] = r[u] < rows ? r[u] : 0u;
        const piece* rp_ = reinterpret_cast<const piece*>(W) + (uint64_t)E::row_piece(r[u], Dv, ln);
        if constexpr (NT) ring[u] = ld_nt(rp_); else ring[u] = *rp_;
        rsb[u] = E::template load_sb<NT>(rp_, sbd);
      }
    };
    // (weighted: the clamped re-reads past the bag's end, and row 0 read for an empty bag, are dropped by keep like the
    // unweighted ones -- masking the weight would turn an inf or NaN element of such a row into fma(0, x, acc) == NaN)
    auto consume = [&](const piece (&ring)[U], const sbt (&rsb)[U], const wt (&rw)[U], int pos) {
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if constexpr (WGT) E::addw(acc, pos + u * STEP < n, rw[u], ring[u], rsb[u]);
        else E::add(acc, pos + u * STEP < n, ring[u], rsb[u]);
      }
    };

    // software pipeline over two register rings: while ring A (round k) is summed
    // in index order, ring B (round k+1) is already in flight, and vice versa.
    // Each arm holds its own issue+consume pair; the distinct asm comments keep
    // SimplifyCFG from sinking the common tails into a join.
    constexpr int R = U * STEP;
    piece ringA[U], ringB[U];
    sbt sbA[U], sbB[U];
    wt wA[U], wB[U];
    int jj = first;                                 // per-lane row position
    int ju = 0;                                     // uniform round position
    issue(ringA, sbA, wA, jj);
    for (;;) {
      if (ju + R < n_u) {
        issue(ringB, sbB, wB, jj + R);
        __builtin_amdgcn_sched_barrier(0);   // loads first, then the sums
        consume(ringA, sbA, wA, jj);
        asm volatile("; drs sls: A summed, B in flight" ::: "memory");
      } else {
        consume(ringA, sbA, wA, jj);
        asm volatile("; drs sls: A summed, tail" ::: "memory");
        break;
      }
      if (ju + 2 * R < n_u) {
        issue(ringA, sbA, wA, jj + 2 * R);
        __builtin_amdgcn_sched_barrier(0);
        consume(ringB, sbB, wB, jj + R);
        asm volatile("; drs sls: B summed, A in flight" ::: "memory");
      } else {
        consume(ringB, sbB, wB, jj + R);
        asm volatile("; drs sls: B summed, tail" ::: "memory");
        break;
      }
      jj += 2 * R;
      ju += 2 * R;
    }
    __builtin_amdgcn_wave_barrier();
  }

  if (!EXACT) {
#pragma unroll
    for (int m = G; m < 64; m <<= 1) vadd(acc, vshfl_xor(acc, m));
  }
  if (bad) atomicOr(a.err, 1);
  scale_finish<E>(acc, a, t);
  pool_finish(acc, a.pool, len);   // (behind the loops and the butterfly: the pipeline arms above keep their waitcnt counts)
  if (bag_ok && col_ok && (EXACT || g == 0)) {
    float* o = a.out + (int64_t)vrow * a.ld_out + a.col0 + (int64_t)t * D + col;
    *reinterpret_cast<float4*>(o) = acc;
  }
  if (a.ts) {
    __builtin_amdgcn_s_waitcnt(0);   // include the output store in the span
    if (threadIdx.x == 0) a.ts[2 * blockIdx.x + 1] = wall_clock64();
  }
}



// ANY row width: the generic form behind the ABI's total boundary.  The reference only asks m_spa == ln_bot[-1]
// (models/dlrm_s_caffe2.py:435-437); every kernel above reads a row as 16-byte pieces (D % 4 == 0, D <= 256), which
// every shipped config satisfies.  Other widths -- D = 10, 50, 300 -- take this one: a wave per bag, lane c takes columns
// c, c + 64, ... (dword loads: rows need no alignment), rows strictly in index order, i.e. Caffe2's own summation order
// (bit-identical to the oracle), ragged bags through the prefix sums.  Slow by design (one row at a time), never wrong.
// WGT: the weighted instance -- row j's weight is read beside its index (1.0f for a query without weights, 0.0f for an
// out-of-range row) and the row adds acc = fma(w, x, acc), or with s = w * scale, b = w * bias for the rowwise types.
template <class E = F32, bool WGT = false>
__global__ __launch_bounds__(64) void sls_any_kernel(SlsArgs a) {
  if (a.ts && threadIdx.x == 0) a.ts[2 * blockIdx.x] = wall_clock64();
  const int lane = threadIdx.x;
  const int64_t bag = blockIdx.x;
  const int smp = (int)(bag / a.T);
  const int t = (int)(bag - (int64_t)smp * a.T);
  DRS_OWNER_OF(a, smp, b, vrow, ulen, qidx, qoff)
  int beg, end;
  if (ulen >= 0) {
    beg = b * ulen;
    end = beg + ulen;
  } else {
    const int32_t* __restrict__ offp = qoff + (int64_t)t * a.off_stride;
    beg = offp[b];
    end = offp[b + 1];
  }
  const int32_t* __restrict__ ip = qidx + (int64_t)t * a.idx_stride;
  [[maybe_unused]] const float* wp = nullptr;
  if constexpr (WGT) {
    const float* qwgt = a.wgt[0];
    DRS_OWNER_CHAIN(a.q, smp, qwgt = in ? a.wgt[i] : qwgt;)
    wp = qwgt ? qwgt + (int64_t)t * a.idx_stride : nullptr;
  }
  const typename E::elem* __restrict__ W = table_base<E>(a.tables) + a.tab_off[t];
  const uint32_t rows = (uint32_t)a.tab_rows[t];
  const int D = a.D;
  DRS_ROW_LINES(E, a, ln)
  float* o = a.out + (int64_t)vrow * a.ld_out + a.col0 + (int64_t)t * D;
  bool bad = false;
  for (int c0 = 0; c0 < D; c0 += 64 * 4) {          // four columns per lane and pass
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int j = beg; j < end; ++j) {
      uint32_t r = (uint32_t)ip[j];
      bad |= r >= rows;
      [[maybe_unused]] float w = 1.0f;
      if constexpr (WGT) {
        w = wp ? wp[j] : 1.0f;
        w = r < rows ? w : 0.0f;
      }
      r = r < rows ? r : 0u;
      if constexpr (E::rowwise) {
        // byte loads of the codes; every lane of the wave reads the row's scale and bias
        const uint8_t* row;
        if constexpr (E::lines) row = W + (int64_t)E::row_piece(r, E::pieces_per_row(D), ln) * kPieceElems<E>;
        else row = W + (int64_t)r * (int64_t)E::pieces_per_row(D) * kPieceElems<E>;
        float2 sb = E::row_sb(row, D);
        if constexpr (WGT) sb = make_float2(__fmul_rn(w, sb.x), __fmul_rn(w, sb.y));
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int c = c0 + lane + 64 * k;
          if (c < D) acc[k] = E::row1(sb.x, sb.y, E::code(row, c), acc[k]);
        }
      } else {
        const typename E::elem* row = W + (int64_t)r * D;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int c = c0 + lane + 64 * k;
          if constexpr (WGT) acc[k] = c < D ? E::addw1(acc[k], w, E::up1(row[c])) : acc[k];
          else acc[k] += c < D ? E::up1(row[c]) : 0.f;
        }
      }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int c = c0 + lane + 64 * k;
      if constexpr (E::scaled) acc[k] = __fmul_rn(acc[k], a.tab_scale[t]);
      if (c < D) o[c] = pool_finish(acc[k], a.pool, end - beg);
    }
  }
  if (bad) atomicOr(a.err, 1);
  if (a.ts) {
    __builtin_amdgcn_s_waitcnt(0);
    if (threadIdx.x == 0) a.ts[2 * blockIdx.x + 1] = wall_clock64();
  }
}

int lanes_per_row(int D) { return D <= 8 ? 2 : D <= 16 ? 4 : D <= 32 ? 8 : D <= 64 ? 16 : D <= 128 ? 32 : 64; }

// the launch for tables of element type E (F32 / F16 / BF16 / F8 / I8 / I8L / I4 / I4L): the plan's dispatch-log line, then its instance
template <class E>
hipError_t launch_sls_e(const SlsArgs& a, const SlsPlan& p, const Tune& tune, hipStream_t s, hipEvent_t stop) {
  // dispatch log: the dtype token ("" for fp32), then "mean" under "sls_pool" 1 (nothing for sum), then "w" on a weighted
  // launch (nothing otherwise)
  char tags[24];
  snprintf(tags, sizeof tags, "%s%s%s%s%s", E::tag, *E::tag && a.pool ? "," : "", a.pool ? "mean" : "",
           p.weighted && (*E::tag || a.pool) ? "," : "", p.weighted ? "w" : "");
  const char* dt = tags;
  const char* sep = *dt ? "," : "";
  const long long wg = (long long)p.grid;
  if (!wg && (p.form == SlsForm::any || p.form == SlsForm::one)) return hipSuccess;   // (an empty launch of these is not logged)
  switch (p.form) {
    case SlsForm::any:
      log_launch(tune.log, "sls_any_kernel%s%s%s[%lld wg, D=%d]", *dt ? "<" : "", dt, *dt ? ">" : "", wg, a.D);
      break;
    case SlsForm::flat:
    case SlsForm::flatc:
      log_launch(tune.log, "%s<%d,%d%s%s%s%s>[%lld wg, L=%d]", p.form == SlsForm::flatc ? "sls_flatc_kernel" : "sls_flat_kernel",
                 p.G, p.NL, p.form == SlsForm::flatc ? "" : (p.BPW == 4 ? ",bpw4" : p.BPW == 2 ? ",bpw2" : ",bpw1"),
                 p.nt ? ",nt" : "", sep, dt, wg, p.L);
      break;
    case SlsForm::one:
      log_launch(tune.log, "sls_one_kernel<%d,%d%s%s>[%lld wg]", p.G, p.BW, sep, dt, wg);
      break;
    case SlsForm::ring:
      log_launch(tune.log, "sls_kernel<%d,%s%s%s>[%lld wg]", p.G, p.exact ? "sequential" : (p.nt ? "split,nt" : "split"), sep, dt, wg);
      break;
  }
  if (!wg) return hipSuccess;             // an empty launch enqueues nothing
  // (the weighted instances of the flat and one-lookup forms: sls_wflat.hip)
  if (p.weighted && p.form != SlsForm::any && p.form != SlsForm::ring) return launch_sls_wflat(a, p, s, stop);
  const dim3 grid((unsigned)p.grid);
  switch (p.form) {
    case SlsForm::any:
      if (p.weighted) launch_k(sls_any_kernel<E, true>, grid, s, stop, a);
      else launch_k(sls_any_kernel<E>, grid, s, stop, a);
      break;
    case SlsForm::flatc:
      with_int<8, 16, 32>(p.G, [&](auto G) { with_int<5, 10, 20>(p.NL, [&](auto NL) { with_int<0, 1>(p.nt, [&](auto NT) {
        launch_k(sls_flatc_kernel<G, NL, NT != 0, E>, grid, s, stop, a, p.L);
      }); }); });
      break;
    case SlsForm::flat:   // (xcd_order 1: every launch deals the work list to the XCDs in slices)
      with_int<8, 16, 32>(p.G, [&](auto G) { with_int<5, 10, 20>(p.NL, [&](auto NL) { with_int<0, 1>(p.nt, [&](auto NT) {
        with_int<1, 2, 4>(p.BPW, [&](auto BPW) {
          if constexpr (BPW == 1 || NL <= 10) launch_k(sls_flat_kernel<G, NL, BPW, NT != 0, E>, grid, s, stop, a, p.L, 1);
        });
      }); }); });
      break;
    case SlsForm::one:
      with_int<4, 8, 16, 32>(p.G, [&](auto G) { with_int<64, 16>(p.BW, [&](auto BW) {
        launch_k(sls_one_kernel<G, BW, E>, grid, s, stop, a, p.tiles);
      }); });
      break;
    case SlsForm::ring:
      with_int<2, 4, 8, 16, 32, 64>(p.G, [&](auto G) { with_int<0, 1>(p.exact, [&](auto EXACT) { with_int<0, 1>(p.nt, [&](auto NT) {
        if constexpr (!(EXACT && NT)) {
          if (p.weighted) launch_k(sls_kernel<G, EXACT != 0, NT != 0, E, true>, grid, s, stop, a);
          else launch_k(sls_kernel<G, EXACT != 0, NT != 0, E>, grid, s, stop, a);
        }
      }); }); });
      break;
  }
  return hipGetLastError();
}

}  // namespace

// Tunables (drs_set_option, kept per engine in Tune): "sls_flat" / "sls_bpw" the flat variant and its bags
// per wave (0 = auto), "sls_nt" non-temporal row loads, "sls_one" the one-lookup copy form and its samples per wave,
// "sls_weighted_flat" whether a weighted launch may take those forms.
SlsPlan plan_sls(const SlsArgs& a, bool exact, bool short_bags, const Tune& tune, int dtype) {
  SlsPlan p;
  p.dtype = dtype;
  const int D = a.D, n_q = a.q.n_q, n_smp = a.q.cum[n_q];
  const int64_t n_bags = (int64_t)n_smp * a.T;
  // a weighted launch: at least one of its queries carries per-sample weights.  By default ("sls_weighted_flat" 0) it
  // takes the any-width form or the ring walk below -- sequential or split by the same rule as ever -- and never the flat
  // or the one-lookup forms; under "sls_weighted_flat" 1 the weights play no part in the choice: the launch takes the form
  // its unweighted twin takes, in its weighted instance.
  for (int i = 0; i < n_q; ++i) p.weighted = p.weighted || a.wgt[i] != nullptr;
  const bool wflat = !p.weighted || tune.sls_weighted_flat;
  // widths that are not whole 16-byte pieces, or wider than a wave: the generic form (sequential order)
  if ((D & 3) || D > 256) {
    p.form = SlsForm::any;
    p.exact = true;
    p.grid = n_bags;
    return p;
  }
  // the flat variant, in split order only: every coalesced query must have the same fixed bag length L >= 2 (L == 1
  // is a copy), G must be one of the instantiated widths, BPW must divide T (a wave's bags belong to one sample) and
  // BPW * L rows must fit NL loads per lane
  const int G = lanes_per_row(D), NG = 64 / G;
  const int L = n_q >= 1 ? a.uniform_len[0] : -1;
  bool flat = wflat && !exact && tune.sls_flat && n_q >= 1 && L >= 2 && (G == 8 || G == 16 || G == 32);
  for (int i = 1; flat && i < n_q; ++i) flat = a.uniform_len[i] == L;
  int bpw = 1;
  if (flat && tune.sls_bpw > 0) {
    bpw = tune.sls_bpw;
    flat = (bpw == 1 || bpw == 2 || bpw == 4) && a.T % bpw == 0;
  } else if (flat) {
    // short bags share a wave until it has five loads per lane to issue (measured on RM3,
    // 12 x 10M x 32, L = 20, beside its GEMM launches: 2 bags per wave 0.48 of peak, 1 or 4 bags
    // 0.44; the chip to itself: 0.60 / 0.55 / 0.59)
    for (int c : {4, 2})
      if (a.T % c == 0 && c * L <= 5 * NG) { bpw = c; break; }
  }
  const int need = (bpw * L + NG - 1) / NG;
  // (30 loads per lane -- RM2: L = 120, D = 64 -- in the one-bag-per-wave form was measured in round 4: 497.6 us per
  // launch against the ring walk's 497.4 us; not kept)
  const int nl = need <= 5 ? 5 : need <= 10 ? 10 : need <= 20 ? 20 : 0;
  if (flat && nl && (bpw == 1 || nl <= 10)) {
    p.form = bpw == 1 && tune.sls_flat == 1 ? SlsForm::flatc : SlsForm::flat;   // "sls_flat" 2 forces the phased form
    p.G = G; p.NL = nl; p.BPW = bpw; p.L = L; p.nt = tune.sls_nt != 0;
    const unsigned n_work = (unsigned)n_smp * (unsigned)(a.T / bpw);
    p.grid = p.form == SlsForm::flatc ? n_work : 8u * ((n_work + 7u) / 8u);   // (the phased form: whole rounds of 8 XCDs)
    return p;
  }
  // Bags of a few rows (W&D / NCF: one lookup per table) would leave most of a wave idle in the wave-per-bag variant: a
  // lane group per bag is both faster there and bit-exact -- unless the flat variant took the launch above
  p.exact = exact || short_bags;
  // the one-lookup copy form: every coalesced query has fixed bags of ONE row, a row is 4 / 8 / 16 / 32 lanes x 16 B
  bool one = wflat && p.exact && tune.sls_one && n_q >= 1 && (D == 16 || D == 32 || D == 64 || D == 128);
  for (int i = 0; one && i < n_q; ++i) one = a.uniform_len[i] == 1;
  if (one) {
    p.form = SlsForm::one;
    p.G = D / 4;
    // samples per wave: 64, unless that leaves the launch under 1 024 waves ("sls_one" 64 / 16 force one)
    p.BW = tune.sls_one == 64 || tune.sls_one == 16 ? tune.sls_one : (int64_t)a.T * ((n_smp + 63) / 64) < 1024 ? 16 : 64;
    p.tiles = (n_smp + p.BW - 1) / p.BW;
    p.grid = (int64_t)a.T * p.tiles;
    return p;
  }
  // the ring walk.  The non-temporal hint is for bags of many rows out of big tables; the one-lookup models (W&D, NCF,
  // MT-WnD: the sequential form) keep their rows cacheable -- NCF's tables live in the Infinity Cache (measured: -3 % with it)
  p.form = SlsForm::ring;
  p.G = G;
  p.nt = !p.exact && tune.sls_nt;
  p.grid = p.exact ? (n_bags + NG - 1) / NG : n_bags;
  return p;
}

hipError_t launch_sls(const SlsArgs& a, const SlsPlan& p, const Tune& tune, hipStream_t s, hipEvent_t stop) {
  if (a.D <= 0) return hipErrorInvalidValue;
  switch (p.dtype) {
    case DRS_TABLE_FP16: return launch_sls_e<F16>(a, p, tune, s, stop);
    case DRS_TABLE_BF16: return launch_sls_e<BF16>(a, p, tune, s, stop);
    case DRS_TABLE_FP8_E4M3: return a.tab_scale ? launch_sls_e<F8>(a, p, tune, s, stop) : hipErrorInvalidValue;
    case DRS_TABLE_INT8_ROWWISE: return a.ln_pad ? launch_sls_e<I8L>(a, p, tune, s, stop) : launch_sls_e<I8>(a, p, tune, s, stop);
    case DRS_TABLE_INT4_ROWWISE: return a.ln_pad ? launch_sls_e<I4L>(a, p, tune, s, stop) : launch_sls_e<I4>(a, p, tune, s, stop);
    default: return launch_sls_e<F32>(a, p, tune, s, stop);
  }
}

}  // namespace drs
