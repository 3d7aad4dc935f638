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

// ---------------------------------------------------------------------------
// device-side table fill, bit-identical to oracle/drs_oracle.c fill_value()
__device__ __forceinline__ float fill_value(int64_t i, int32_t t, float lo, float span, uint64_t seed) {
  uint64_t z = seed + 0x9E3779B97F4A7C15ull * ((uint64_t)i + ((uint64_t)(uint32_t)t << 40) + 1ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  const float u = (float)(uint32_t)(z >> 40) * (1.0f / 16777216.0f);
  return __fmaf_rn(u, span, lo);
}
__global__ void fill_uniform_kernel(float* W, int64_t n, int32_t t, float lo, float hi,
                                    uint64_t seed) {
  const float span = hi - lo;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    W[i] = fill_value(i, t, lo, span, seed);
  }
}

// "table_dtype": an fp32 value as it is stored in a table of element type dt (fp16 / bf16: the hardware's
// round-to-nearest-even conversions, v_cvt_f16_f32 / v_cvt_pk_bf16_f32 -- NaN stays NaN, overflow gives +-inf, fp16
// subnormals are kept), and back (exact)
__device__ __forceinline__ void store_elem(void* W, int dt, int64_t i, float x) {
  if (dt == DRS_TABLE_FP16) static_cast<_Float16*>(W)[i] = (_Float16)x;
  else if (dt == DRS_TABLE_BF16) static_cast<__bf16*>(W)[i] = (__bf16)x;
  else static_cast<float*>(W)[i] = x;
}
__device__ __forceinline__ float load_elem(const void* W, int dt, int64_t i) {
  if (dt == DRS_TABLE_FP16) return F16::up1(static_cast<const uint16_t*>(W)[i]);
  if (dt == DRS_TABLE_BF16) return BF16::up1(static_cast<const uint16_t*>(W)[i]);
  return static_cast<const float*>(W)[i];
}
// n elements of type sdt -> type ddt (the arena conversion of "table_dtype", drs_set_table's staged rows)
__global__ void convert_table_kernel(const void* src, int sdt, void* dst, int ddt, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    store_elem(dst, ddt, i, load_elem(src, sdt, i));
}
// fill_uniform_kernel's fp32 value, rounded to the table's element type
__global__ void fill_uniform_round_kernel(void* W, int dt, int64_t n, int32_t t, float lo, float hi, uint64_t seed) {
  const float span = hi - lo;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    store_elem(W, dt, i, fill_value(i, t, lo, span, seed));
  }
}

// ---------------------------------------------------------------------------
// "table_dtype" 8, 8-bit rowwise tables (layout: struct I8).  Quantizing a row, FBGEMM's embedding_bag_byte_prepack in
// IEEE fp32 without contraction: mn = min, mx = max, range = mx - mn, scale = range / 255, bias = mn,
// inv = 255 / (range + 1e-8), q = rint((x - mn) * inv).  One wave per row, any D; the row is read twice (the second
// time from the cache).  Rows holding inf or NaN are outside the contract: the clamp keeps every code a byte.  A finite
// row with mx - mn = inf (+3e38 beside -3e38) is inside it: scale = inf, inv = 0 and every code 0 (fminf(fmaxf(NaN, 0), 255)
// is 0 for the element whose x - mn is inf) -- embedding_bag_byte_prepack's bytes; the row decodes to inf * 0 = NaN and
// the gather keeps that NaN to the bags that name it (I8::addw).
struct SrcElems {      // row r of a table of element type dt at src (D elements per row)
  const void* src;
  int dt;
  __device__ __forceinline__ float operator()(int64_t r, int D, int c) const { return load_elem(src, dt, r * D + c); }
};
struct SrcFill {       // fill_uniform_kernel's values of table t
  int32_t t;
  float lo, span;
  uint64_t seed;
  __device__ __forceinline__ float operator()(int64_t r, int D, int c) const { return fill_value(r * D + c, t, lo, span, seed); }
};
// Where the int8 rows of a launch go, or come from: `base` is the TABLE's first byte, the launch's row r is the table's row
// first + r (drs_set_table stages a table in chunks) of `total`, n = I8Lines::n of the layout (0: plain).
struct I8Rows {
  uint8_t* base;
  int64_t first, total;
  int32_t n;
  __device__ __forceinline__ uint8_t* row(int64_t r, int64_t S) const { return base + i8_row_offset(first + r, S, n); }
  // line-packed layout: the bytes of its line behind row r that belong to no row -- the line's last 128 - n S bytes after
  // its last slot, and the unused slots too after the table's last row
  __device__ __forceinline__ int tail(int64_t r, int64_t S) const {
    if (!n) return 0;
    const int slot = (int)((first + r) % n);
    return slot == n - 1 || first + r == total - 1 ? 128 - (slot + 1) * (int)S : 0;
  }
};
struct SrcI8 {         // each int8 rowwise row's value, fmaf(scale, q, 0.0f + bias)
  I8Rows rows;
  __device__ __forceinline__ float operator()(int64_t r, int D, int c) const {
    const uint8_t* row = rows.row(r, I8::padded(D) + 8);
    const float2 sb = I8::row_sb(row, D);
    return I8::row1(sb.x, sb.y, I8::code(row, c), 0.0f);
  }
};
// int4 rowwise rows (layout: struct I4), as I8Rows: `base` is the TABLE's first byte, the launch's row r its row first + r of
// `total`, n = I8Lines::n of the layout ("table_int4_lines"; 0: plain)
struct I4Rows {
  uint8_t* base;
  int64_t first, total;
  int32_t n;
  __device__ __forceinline__ uint8_t* row(int64_t r, int D) const { return base + i8_row_offset(first + r, I4::padded(D) + 4, n); }
  // the bytes of its line behind row r that belong to no row (I8Rows::tail; a multiple of 4 here)
  __device__ __forceinline__ int tail(int64_t r, int D) const { return I8Rows{base, first, total, n}.tail(r, I4::padded(D) + 4); }
};
struct SrcI4 {         // each int4 rowwise row's value
  I4Rows rows;
  __device__ __forceinline__ float operator()(int64_t r, int D, int c) const {
    const uint8_t* row = rows.row(r, D);
    const float2 sb = I4::row_sb(row, D);
    return I4::row1(sb.x, sb.y, I4::code(row, c), 0.0f);
  }
};
template <class Src>
__device__ __forceinline__ void quantize_rows8(Src src, I8Rows dst, int64_t rows, int D) {
  const int lane = threadIdx.x & 63;
  const int D8 = I8::padded(D);
  const int64_t S = D8 + 8;
  for (int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < rows; r += (int64_t)gridDim.x * 4) {
    float mn = INFINITY, mx = -INFINITY;
    for (int c = lane; c < D; c += 64) {
      const float x = src(r, D, c);
      mn = fminf(mn, x);
      mx = fmaxf(mx, x);
    }
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
      mn = fminf(mn, __shfl_xor(mn, m));
      mx = fmaxf(mx, __shfl_xor(mx, m));
    }
    const float range = __fsub_rn(mx, mn);
    const float inv = __fdiv_rn(255.0f, __fadd_rn(range, 1e-8f));
    uint8_t* row = dst.row(r, S);
    for (int c = lane; c < D8; c += 64) {
      const float q = c < D ? rintf(__fmul_rn(__fsub_rn(src(r, D, c), mn), inv)) : 0.f;
      row[c] = (uint8_t)fminf(fmaxf(q, 0.f), 255.f);
    }
    if (lane == 0) *reinterpret_cast<float2*>(row + D8) = make_float2(__fdiv_rn(range, 255.0f), mn);
    for (int c = lane * 8, z = dst.tail(r, S); c < z; c += 64 * 8) *reinterpret_cast<uint2*>(row + S + c) = make_uint2(0u, 0u);
  }
}
template <class Src>
__global__ __launch_bounds__(256) void quantize_rows_kernel(Src src, I8Rows dst, int64_t rows, int D) {
  quantize_rows8(src, dst, rows, D);
}
// int4 rowwise rows -> int8 rowwise rows ("table_dtype" 9 -> 8): each row's value, quantized again
__global__ __launch_bounds__(256) void rows4_to_rows8_kernel(SrcI4 src, I8Rows dst, int64_t rows, int D) {
  quantize_rows8(src, dst, rows, D);
}
// int8 rows -> elements of type dt: each row's value fmaf(scale, q, 0.0f + bias) (the one-row bag), rounded to dt
__global__ __launch_bounds__(256) void dequantize_rows_kernel(I8Rows src, void* dst, int dt, int64_t rows, int D) {
  const int lane = threadIdx.x & 63;
  const int D8 = I8::padded(D);
  for (int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < rows; r += (int64_t)gridDim.x * 4) {
    const uint8_t* row = src.row(r, D8 + 8);
    const float2 sb = *reinterpret_cast<const float2*>(row + D8);
    for (int c = lane; c < D; c += 64) store_elem(dst, dt, r * D + c, I8::row1(sb.x, sb.y, (float)row[c], 0.0f));
  }
}
// int8 rows from one layout to the other ("table_int8_lines" set on an int8 arena): the rows' bytes as they are
__global__ __launch_bounds__(256) void relayout_rows_kernel(I8Rows src, I8Rows dst, int64_t rows, int D) {
  const int lane = threadIdx.x & 63;
  const int64_t S = I8::padded(D) + 8;
  for (int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < rows; r += (int64_t)gridDim.x * 4) {
    const uint8_t* from = src.row(r, S);
    uint8_t* to = dst.row(r, S);
    for (int c = lane * 8; c < S; c += 64 * 8) *reinterpret_cast<uint2*>(to + c) = *reinterpret_cast<const uint2*>(from + c);
    for (int c = lane * 8, z = dst.tail(r, S); c < z; c += 64 * 8) *reinterpret_cast<uint2*>(to + S + c) = make_uint2(0u, 0u);
  }
}

// ---------------------------------------------------------------------------
// "table_dtype" 9, 4-bit rowwise tables (layout: struct I4).  Quantizing a row, torch's embedding_bag_4bit_prepack in IEEE
// fp32 without contraction: bias = fp16(min), scale = fp16((max - (float)bias) / 15), a zero scale becomes 1,
// inv = 1 / (float)scale (infinite: scale = inv = 1), q = clamp(rint((x - (float)bias) * inv), 0, 15).  One wave per row,
// any even D; the row is read twice (the second time from the cache).  Rows holding inf or NaN, or values beyond fp16's
// range, are outside the contract: the clamp keeps every code a nibble.  A finite row with (max - bias) / 15 >= 65520 --
// one element of 1e6 -- takes the scale +inf, inv = 0 and every code 0, embedding_bag_4bit_prepack's bytes: it decodes to
// inf * 0 = NaN in every column, and the gather keeps that NaN to the bags that name it (I4::addw).
template <class Src>
__device__ __forceinline__ void pack4_rows(Src src, I4Rows dst, int64_t rows, int D) {
  const int lane = threadIdx.x & 63;
  const int P = I4::padded(D);
  for (int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < rows; r += (int64_t)gridDim.x * 4) {
    float mn = INFINITY, mx = -INFINITY;
    for (int c = lane; c < D; c += 64) {
      const float x = src(r, D, c);
      mn = fminf(mn, x);
      mx = fmaxf(mx, x);
    }
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
      mn = fminf(mn, __shfl_xor(mn, m));
      mx = fmaxf(mx, __shfl_xor(mx, m));
    }
    const _Float16 bias_h = (_Float16)mn;
    const float bias = (float)bias_h;
    _Float16 scale_h = (_Float16)__fdiv_rn(__fsub_rn(mx, bias), 15.0f);
    if (scale_h == (_Float16)0.0f) scale_h = (_Float16)1.0f;
    float inv = __fdiv_rn(1.0f, (float)scale_h);
    if (isinf(inv)) { scale_h = (_Float16)1.0f; inv = 1.0f; }
    uint8_t* row = dst.row(r, D);
    for (int j = lane; j < P; j += 64) {          // byte j: columns 2 j (low nibble) and 2 j + 1
      uint32_t b = 0;
      if (2 * j < D) {
        const float q0 = rintf(__fmul_rn(__fsub_rn(src(r, D, 2 * j), bias), inv));
        const float q1 = rintf(__fmul_rn(__fsub_rn(src(r, D, 2 * j + 1), bias), inv));
        b = (uint32_t)fminf(fmaxf(q0, 0.f), 15.f) | ((uint32_t)fminf(fmaxf(q1, 0.f), 15.f) << 4);
      }
      row[j] = (uint8_t)b;
    }
    if (lane == 0)
      *reinterpret_cast<uint32_t*>(row + P) = (uint32_t)__builtin_bit_cast(uint16_t, scale_h) | ((uint32_t)__builtin_bit_cast(uint16_t, bias_h) << 16);
    for (int c = lane * 4, z = dst.tail(r, D); c < z; c += 64 * 4) *reinterpret_cast<uint32_t*>(row + P + 4 + c) = 0u;
  }
}
template <class Src>
__global__ __launch_bounds__(256) void pack4_rows_kernel(Src src, I4Rows dst, int64_t rows, int D) {
  pack4_rows(src, dst, rows, D);
}
// int4 rows -> elements of type dt: each row's value fmaf(scale, q, 0.0f + bias) (the one-row bag), rounded to dt
__global__ __launch_bounds__(256) void unpack4_rows_kernel(SrcI4 src, void* dst, int dt, int64_t rows, int D) {
  const int lane = threadIdx.x & 63;
  for (int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < rows; r += (int64_t)gridDim.x * 4)
    for (int c = lane; c < D; c += 64) store_elem(dst, dt, r * D + c, src(r, D, c));
}
// int4 rows from one layout to the other ("table_int4_lines" set on an int4 arena): the rows' bytes as they are
__global__ __launch_bounds__(256) void relayout4_rows_kernel(I4Rows src, I4Rows dst, int64_t rows, int D) {
  const int lane = threadIdx.x & 63;
  const int S = I4::padded(D) + 4;
  for (int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < rows; r += (int64_t)gridDim.x * 4) {
    const uint8_t* from = src.row(r, D);
    uint8_t* to = dst.row(r, D);
    for (int c = lane * 4; c < S; c += 64 * 4) *reinterpret_cast<uint32_t*>(to + c) = *reinterpret_cast<const uint32_t*>(from + c);
    for (int c = lane * 4, z = dst.tail(r, D); c < z; c += 64 * 4) *reinterpret_cast<uint32_t*>(to + S + c) = 0u;
  }
}
static unsigned row_grid(int64_t rows) {
  const int64_t want = (rows + 3) / 4;
  return (unsigned)(want < 16384 ? want : 16384);
}

// ---------------------------------------------------------------------------
// "table_dtype" 4, fp8 e4m3 tables (layout: struct F8).  e4m3_rne: an fp32 value as its OCP e4m3 code, torch's
// float8_e4m3fn conversion in integer arithmetic, bit for bit: round to nearest even, the subnormal codes (multiples of
// 2^-9 below 2^-6) through the add of 2^14 whose ulp they are, 0x7F (NaN) with the sign bit for NaN, +-inf and everything
// that rounds beyond 448 -- which no finite element does after the table's scale.
__device__ __forceinline__ uint8_t e4m3_rne(float x) {
  uint32_t b = __float_as_uint(x);
  const uint32_t sign = b & 0x80000000u;
  b ^= sign;
  uint32_t q;
  if (b >= 0x43F00000u) {                           // >= 480, +-inf, NaN
    q = 0x7Fu;
  } else if (b < (121u << 23)) {                    // below 2^-6
    q = __float_as_uint(__fadd_rn(__uint_as_float(b), __uint_as_float(141u << 23))) - (141u << 23);
  } else {
    const uint32_t odd = (b >> 20) & 1u;
    b += ((uint32_t)(7 - 127) << 23) + 0x7FFFFu + odd;
    q = b >> 20;
  }
  return (uint8_t)(q | (sign >> 24));
}
struct SrcF8 {         // each fp8 code's value, decode(code) * 2^-k of its table
  const uint8_t* codes;
  float scale;
  __device__ __forceinline__ float operator()(int64_t r, int D, int c) const { return __fmul_rn(F8::up1(codes[r * D + c]), scale); }
};
// the largest |x| over the source's finite values, as its bits: one atomicMax per wave into *out (zeroed by the caller)
template <class Src>
__global__ __launch_bounds__(256) void absmax_rows_kernel(Src src, int64_t rows, int D, uint32_t* out) {
  const int64_t n = rows * D;
  uint32_t m = 0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / D;
    const uint32_t b = __float_as_uint(src(r, D, (int)(i - r * D))) & 0x7fffffffu;
    m = b < 0x7f800000u && b > m ? b : m;
  }
#pragma unroll
  for (int k = 1; k < 64; k <<= 1) {
    const uint32_t o = (uint32_t)__shfl_xor((int)m, k);
    m = o > m ? o : m;
  }
  if ((threadIdx.x & 63) == 0 && m) atomicMax(out, m);
}
// rows x D source values -> codes: dst[r * D + c] = e4m3_rne(x * mul), mul = 2^k
template <class Src>
__global__ __launch_bounds__(256) void to_fp8_rows_kernel(Src src, uint8_t* dst, int64_t rows, int D, float mul) {
  const int64_t n = rows * D;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / D;
    dst[i] = e4m3_rne(__fmul_rn(src(r, D, (int)(i - r * D)), mul));
  }
}
// fp8 rows -> int8 / int4 rowwise rows ("table_dtype" 4 -> 8, 4 -> 9): each code's value, through that type's quantizer
__global__ __launch_bounds__(256) void fp8_to_rows8_kernel(SrcF8 src, I8Rows dst, int64_t rows, int D) {
  quantize_rows8(src, dst, rows, D);
}
__global__ __launch_bounds__(256) void fp8_to_rows4_kernel(SrcF8 src, I4Rows dst, int64_t rows, int D) {
  pack4_rows(src, dst, rows, D);
}
// fp8 rows -> elements of type dt: each code's value, rounded to dt
__global__ __launch_bounds__(256) void from_fp8_rows_kernel(SrcF8 src, void* dst, int dt, int64_t rows, int D) {
  const int64_t n = rows * D;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / D;
    store_elem(dst, dt, i, src(r, D, (int)(i - r * D)));
  }
}
static unsigned elem_grid(int64_t n) {
  const int64_t want = (n + 255) / 256;
  return (unsigned)(want < 16384 ? want : 16384);
}
static bool plain_dtype(int dtype) { return dtype == DRS_TABLE_FP32 || dtype == DRS_TABLE_FP16 || dtype == DRS_TABLE_BF16; }

#ifdef DRS_LAB   // probes of tools/placement_lab.py (libdrs_hip_lab.so: make lab-lib); not in the product library
// ---------------------------------------------------------------------------
// Row-read probe of a range of device memory: the access shape of the many-rows-per-bag gather (a wave =
// 80 random 256-byte rows, 4 per load instruction, all 20 loads of a lane in flight, non-temporal) without
// index arrays or outputs.  What it is for: DESIGN.md 5 -- the same gather runs up to 9 % faster on some
// gigabytes of HBM than on others, and the arena builder keeps the gigabytes this probe reads fastest.
// G lanes per row (16 bytes each): 16 = RMC1's 256-byte rows (a wave = 80 rows), 8 = 128-byte rows (dlrm_rm1.json / RM3:
// a wave = 160 rows, eight per load instruction), 32 = 512-byte rows; NT: non-temporal loads (a compile-time property).
template <int G, bool NT, int NLD>
__global__ __launch_bounds__(64) void probe_rows_kernel(const float4* __restrict__ base, uint32_t rows, uint32_t seed,
                                                        float4* __restrict__ sink, uint32_t windows, uint32_t stride_rows, int sorted) {
  // windows == 0: the wave's 80 rows anywhere in [0, rows).  windows > 0: wave w reads inside window w % windows
  // (window k = rows [k * stride_rows, k * stride_rows + rows)), like a bag of one table; sorted: ascending, one row per
  // eightieth of the window (what np.unique leaves of a bag's indices)
  constexpr int NG = 64 / G;                       // rows per load instruction
  constexpr uint32_t RW = NLD * NG;                 // rows per wave
  const int lane = threadIdx.x, g = lane / G, gl = lane % G;
  const uint64_t w0 = windows ? (uint64_t)(blockIdx.x % windows) * stride_rows : 0;
  uint32_t r[NLD];
#pragma unroll
  for (int u = 0; u < NLD; ++u) {
    uint32_t z = (blockIdx.x * RW + (uint32_t)(NG * u + g)) * 0x9E3779B1u + seed;
    z = (z ^ (z >> 16)) * 0x85EBCA6Bu;
    z = (z ^ (z >> 13)) * 0xC2B2AE35u;
    z ^= z >> 16;
    if (sorted) {
      const uint32_t lo = (uint32_t)(((uint64_t)(NG * u + g) * rows) / RW), hi = (uint32_t)(((uint64_t)(NG * u + g + 1) * rows) / RW);
      r[u] = lo + (uint32_t)(((uint64_t)z * (hi > lo ? hi - lo : 1)) >> 32);
    } else {
      r[u] = (uint32_t)(((uint64_t)z * rows) >> 32);
    }
  }
  float4 v[NLD];
#pragma unroll
  for (int u = 0; u < NLD; ++u) {
    if constexpr (NT) v[u] = ld_nt(base + (w0 + r[u]) * G + gl);
    else v[u] = base[(w0 + r[u]) * G + gl];
  }
  float4 acc = vzero4();
#pragma unroll
  for (int u = 0; u < NLD; ++u) vadd(acc, v[u]);
  if (acc.x == 1.2345e-30f) sink[lane] = acc;      // (keeps the loads alive; never true for table data)
}

// time `reps` launches of `waves` waves over [base, base + bytes); GB/s of row bytes in *gbs
hipError_t probe_rows(const void* base, size_t bytes, int waves, int reps, float* sink, hipStream_t s, double* gbs,
                      int windows, int sorted, int row_bytes, int nt, int loads) {
  *gbs = 0;
  if (row_bytes != 128 && row_bytes != 256 && row_bytes != 512) return hipErrorInvalidValue;
  uint64_t rows = bytes / (uint64_t)row_bytes, stride = 0;
  if (windows > 0) { stride = rows / (uint64_t)windows; rows = stride; }
  if (loads != 10 && loads != 20) return hipErrorInvalidValue;
  const int G = row_bytes / 16, rw = loads * (64 / G);
  if (rows < (uint64_t)rw || rows > 0xffffffffull) return hipErrorInvalidValue;
  auto launch = [&](uint32_t seed) {
#define DRS_PROBE(G_, NT_)                                                                                                               \
  do {                                                                                                                                     \
    if (loads == 10) hipLaunchKernelGGL((probe_rows_kernel<G_, NT_, 10>), dim3((unsigned)waves), dim3(64), 0, s, static_cast<const float4*>(base), \
                                        (uint32_t)rows, seed, reinterpret_cast<float4*>(sink), (uint32_t)windows, (uint32_t)stride, sorted); \
    else hipLaunchKernelGGL((probe_rows_kernel<G_, NT_, 20>), dim3((unsigned)waves), dim3(64), 0, s, static_cast<const float4*>(base),       \
                            (uint32_t)rows, seed, reinterpret_cast<float4*>(sink), (uint32_t)windows, (uint32_t)stride, sorted);            \
  } while (0)
    if (G == 8) { if (nt) DRS_PROBE(8, true); else DRS_PROBE(8, false); }
    else if (G == 16) { if (nt) DRS_PROBE(16, true); else DRS_PROBE(16, false); }
    else { if (nt) DRS_PROBE(32, true); else DRS_PROBE(32, false); }
#undef DRS_PROBE
  };
  hipEvent_t e0, e1;
  hipError_t r = hipEventCreate(&e0);
  if (r != hipSuccess) return r;
  r = hipEventCreate(&e1);
  if (r != hipSuccess) { (void)hipEventDestroy(e0); return r; }
  launch(1u);
  r = hipEventRecord(e0, s);
  for (int i = 0; i < reps && r == hipSuccess; ++i) {
    launch(0x51ED27u * (uint32_t)(i + 2));
    r = hipGetLastError();
  }
  if (r == hipSuccess) r = hipEventRecord(e1, s);
  if (r == hipSuccess) r = hipEventSynchronize(e1);
  float ms = 0.f;
  if (r == hipSuccess) r = hipEventElapsedTime(&ms, e0, e1);
  if (r == hipSuccess && ms > 0.f) *gbs = (double)waves * (double)rw * (double)row_bytes * reps / (ms * 1e-3) / 1e9;
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  return r;
}

// Latency probe: workgroup k walks `steps` DEPENDENT 16-byte loads through random 256-byte rows of chunk k
// ([base + k * chunk_bytes, + chunk_bytes)); out[k] = device-clock ticks (100 MHz) for the walk.  One lane per
// chunk, all chunks at once: the walks do not disturb each other, and a launch is steps x ~1 us long.
__global__ __launch_bounds__(64) void probe_latency_kernel(const float4* __restrict__ base, uint64_t chunk_rows, uint32_t rows,
                                                           int steps, uint32_t seed, uint64_t* __restrict__ out) {
  if (threadIdx.x != 0) return;
  const float4* b = base + (uint64_t)blockIdx.x * chunk_rows * 16;
  uint32_t z = seed + blockIdx.x * 0x9E3779B1u;
  float sink = 0.f;
  const uint64_t t0 = wall_clock64();
  for (int i = 0; i < steps; ++i) {
    z = (z ^ (z >> 16)) * 0x85EBCA6Bu;
    z = (z ^ (z >> 13)) * 0xC2B2AE35u;
    z ^= z >> 16;
    const uint32_t r = (uint32_t)(((uint64_t)z * rows) >> 32);
    const float4 v = ld_nt(b + (uint64_t)r * 16 + (z & 15));
    z += __float_as_uint(v.x) | 1u;                  // the next address depends on the loaded value
    sink += v.y;
  }
  const uint64_t t1 = wall_clock64();
  out[blockIdx.x] = t1 - t0 + (sink == 1.2345e-30f ? 1 : 0);
}

hipError_t probe_latency(const void* base, size_t chunk_bytes, int n_chunks, int steps, uint64_t* d_ticks, hipStream_t s) {
  const uint64_t rows = chunk_bytes / 256;
  if (rows < 1 || rows > 0xffffffffull || n_chunks < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(probe_latency_kernel, dim3((unsigned)n_chunks), dim3(64), 0, s, static_cast<const float4*>(base), rows,
                     (uint32_t)rows, steps, 12345u, d_ticks);
  return hipGetLastError();
}

#endif  // DRS_LAB

hipError_t launch_fill_uniform(float* W, int64_t n, int32_t t, float lo, float hi, uint64_t seed,
                               hipStream_t s) {
  if (n <= 0) return hipSuccess;
  const int64_t want = (n + 255) / 256;
  const unsigned grid = (unsigned)(want < 8192 ? want : 8192);
  hipLaunchKernelGGL(fill_uniform_kernel, dim3(grid), dim3(256), 0, s, W, n, t, lo, hi, seed);
  return hipGetLastError();
}

hipError_t launch_fill_uniform_dtype(void* W, int dtype, int64_t rows, int D, int32_t t, float lo, float hi, uint64_t seed,
                                     hipStream_t s, int32_t n_lines) {
  const int64_t n = rows * D;
  if (dtype == DRS_TABLE_FP32) return launch_fill_uniform(static_cast<float*>(W), n, t, lo, hi, seed, s);
  if (n <= 0) return hipSuccess;
  if (dtype == DRS_TABLE_INT4_ROWWISE) {
    if (D & 1) return hipErrorInvalidValue;   // (internal guard: the engine refuses table_dtype 9 on odd D before any launch)
    hipLaunchKernelGGL(pack4_rows_kernel<SrcFill>, dim3(row_grid(rows)), dim3(256), 0, s, SrcFill{t, lo, hi - lo, seed},
                       I4Rows{static_cast<uint8_t*>(W), 0, rows, n_lines}, rows, D);
    return hipGetLastError();
  }
  if (dtype == DRS_TABLE_INT8_ROWWISE) {
    hipLaunchKernelGGL(quantize_rows_kernel<SrcFill>, dim3(row_grid(rows)), dim3(256), 0, s, SrcFill{t, lo, hi - lo, seed},
                       I8Rows{static_cast<uint8_t*>(W), 0, rows, n_lines}, rows, D);
    return hipGetLastError();
  }
  const int64_t want = (n + 255) / 256;
  const unsigned grid = (unsigned)(want < 8192 ? want : 8192);
  hipLaunchKernelGGL(fill_uniform_round_kernel, dim3(grid), dim3(256), 0, s, W, dtype, n, t, lo, hi, seed);
  return hipGetLastError();
}

hipError_t launch_absmax_rows(const void* src, int src_dtype, int64_t rows, int D, uint32_t* d_bits, hipStream_t s) {
  if (rows <= 0) return hipSuccess;
  if (!plain_dtype(src_dtype)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(absmax_rows_kernel<SrcElems>, dim3(elem_grid(rows * D)), dim3(256), 0, s, SrcElems{src, src_dtype}, rows, D, d_bits);
  return hipGetLastError();
}

hipError_t launch_rows_to_fp8(const void* src, int src_dtype, uint8_t* dst, int64_t rows, int D, float mul, hipStream_t s) {
  if (rows <= 0) return hipSuccess;
  if (!plain_dtype(src_dtype)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(to_fp8_rows_kernel<SrcElems>, dim3(elem_grid(rows * D)), dim3(256), 0, s, SrcElems{src, src_dtype}, dst, rows, D, mul);
  return hipGetLastError();
}

hipError_t launch_fill_uniform_fp8(uint8_t* dst, int64_t rows, int D, int32_t t, float lo, float hi, uint64_t seed, float mul, hipStream_t s) {
  if (rows <= 0) return hipSuccess;
  hipLaunchKernelGGL(to_fp8_rows_kernel<SrcFill>, dim3(elem_grid(rows * D)), dim3(256), 0, s, SrcFill{t, lo, hi - lo, seed}, dst, rows, D, mul);
  return hipGetLastError();
}

hipError_t launch_convert_rows(const void* src, int src_dtype, void* dst, int dst_dtype, int64_t rows, int D, hipStream_t s,
                               int32_t n_src, int32_t n_dst, int64_t first, int64_t total, float src_scale) {
  if (rows <= 0) return hipSuccess;
  if (total < 0) total = first + rows;
  if (src_dtype == DRS_TABLE_FP8_E4M3) {   // (whole tables only: first == 0)
    const SrcF8 from8{static_cast<const uint8_t*>(src), src_scale};
    const dim3 grid(row_grid(rows)), block(256);
    if (first != 0 || dst_dtype == DRS_TABLE_FP8_E4M3 || (dst_dtype == DRS_TABLE_INT4_ROWWISE && (D & 1))) return hipErrorInvalidValue;
    if (dst_dtype == DRS_TABLE_INT8_ROWWISE)
      hipLaunchKernelGGL(fp8_to_rows8_kernel, grid, block, 0, s, from8, I8Rows{static_cast<uint8_t*>(dst), 0, total, n_dst}, rows, D);
    else if (dst_dtype == DRS_TABLE_INT4_ROWWISE)
      hipLaunchKernelGGL(fp8_to_rows4_kernel, grid, block, 0, s, from8, I4Rows{static_cast<uint8_t*>(dst), 0, total, n_dst}, rows, D);
    else
      hipLaunchKernelGGL(from_fp8_rows_kernel, dim3(elem_grid(rows * D)), block, 0, s, from8, dst, dst_dtype, rows, D);
    return hipGetLastError();
  }
  if (dst_dtype == DRS_TABLE_FP8_E4M3) return hipErrorInvalidValue;   // (launch_rows_to_fp8: it needs the table's scale first)
  const I8Rows from{static_cast<uint8_t*>(const_cast<void*>(src)), first, total, n_src}, to{static_cast<uint8_t*>(dst), first, total, n_dst};
  const bool si8 = src_dtype == DRS_TABLE_INT8_ROWWISE, di8 = dst_dtype == DRS_TABLE_INT8_ROWWISE;
  const bool si4 = src_dtype == DRS_TABLE_INT4_ROWWISE, di4 = dst_dtype == DRS_TABLE_INT4_ROWWISE;
  if (si4 || di4) {
    // (internal guard, unreachable through the engine: convert_tables refuses odd D)
    if (D & 1) return hipErrorInvalidValue;
    const dim3 grid(row_grid(rows)), block(256);
    const SrcI4 from4{I4Rows{from.base, first, total, n_src}};
    const I4Rows to4{to.base, first, total, n_dst};
    if (si4 && di4) hipLaunchKernelGGL(relayout4_rows_kernel, grid, block, 0, s, from4.rows, to4, rows, D);
    else if (si4 && di8) hipLaunchKernelGGL(rows4_to_rows8_kernel, grid, block, 0, s, from4, to, rows, D);
    else if (si4) hipLaunchKernelGGL(unpack4_rows_kernel, grid, block, 0, s, from4, dst, dst_dtype, rows, D);
    else if (si8) hipLaunchKernelGGL(pack4_rows_kernel<SrcI8>, grid, block, 0, s, SrcI8{from}, to4, rows, D);
    else hipLaunchKernelGGL(pack4_rows_kernel<SrcElems>, grid, block, 0, s, SrcElems{src, src_dtype}, to4, rows, D);
    return hipGetLastError();
  }
  if (di8 && !si8)
    hipLaunchKernelGGL(quantize_rows_kernel<SrcElems>, dim3(row_grid(rows)), dim3(256), 0, s, SrcElems{src, src_dtype}, to, rows, D);
  else if (si8 && !di8)
    hipLaunchKernelGGL(dequantize_rows_kernel, dim3(row_grid(rows)), dim3(256), 0, s, from, dst, dst_dtype, rows, D);
  else if (si8 && di8)
    hipLaunchKernelGGL(relayout_rows_kernel, dim3(row_grid(rows)), dim3(256), 0, s, from, to, rows, D);
  else
    return hipErrorInvalidValue;
  return hipGetLastError();
}

hipError_t launch_convert_table(const void* src, int src_dtype, void* dst, int dst_dtype, int64_t n, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  const int64_t want = (n + 255) / 256;
  const unsigned grid = (unsigned)(want < 16384 ? want : 16384);
  hipLaunchKernelGGL(convert_table_kernel, dim3(grid), dim3(256), 0, s, src, src_dtype, dst, dst_dtype, n);
  return hipGetLastError();
}

}  // namespace drs
