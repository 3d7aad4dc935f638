// Max pooling ("sls_max" 1, SlsArgs::pool == 2): a bag's pooled vector is the element-wise maximum of the rows it names,
// torch's EmbeddingBag(mode="max") with torch.amax's rule for NaN.  A row counts as its stored value widened to fp32:
// fp32 as it is, fp16 / bf16 widened, fp8 its decoded code times the table's 2^-k, int8 / int4 rowwise fmaf(scale, q, bias).
// A maximum has no order and no rounding: there is no sequential / split distinction, every form and launch shape serves
// the same value (the sign of a zero maximum is open when +0 and -0 both occur), and re-reading a row is harmless -- so the
// clamped re-read of a bag's last row, which costs the sum kernels a `keep` select per add, needs no mask here.  What does
// need care:
//   * an empty bag is +0.0 (torch's rule) and loads no row;
//   * an out-of-range index sets the error bit and its row is replaced by -inf, the maximum's identity;
//   * NaN must reach the result.  The hardware's float maximum, and the compare-and-select used here, drop a NaN operand,
//     so every accumulator column carries a second word: the unsigned maximum of the rows' |x| bit patterns.  A pattern
//     above +inf's is a NaN; it survives the per-lane maxima and the butterfly as an integer and turns the stored value
//     into a quiet NaN at the end.  -inf's own pattern is +inf's: dropped and masked rows raise no flag.
// Accumulators start at -inf, never at 0 or at "the first row".
#include "drs_internal.h"
#include "launch_host.h"
#include "owner_dev.h"
#include "sls_dev.h"

namespace drs {
namespace {

constexpr uint32_t kInfBits = 0x7f800000u;   // |x| patterns above it: NaN
constexpr uint32_t kDropped = 0xffffffffu;   // a row offset no row has (rows * row pieces < 2^32): the index was out of range

__device__ __forceinline__ float neg_inf() { return __uint_as_float(0xff800000u); }

// the running maximum of four columns and the NaN word of each
struct MaxAcc {
  float4 v;
  uint32_t nx, ny, nz, nw;
};
__device__ __forceinline__ MaxAcc max_identity() { return MaxAcc{make_float4(neg_inf(), neg_inf(), neg_inf(), neg_inf()), 0u, 0u, 0u, 0u}; }
__device__ __forceinline__ float max1(float acc, float x) { return x > acc ? x : acc; }   // (a NaN x is not taken: the NaN word has it)
__device__ __forceinline__ uint32_t abs_bits(float x) { return __float_as_uint(x) & 0x7fffffffu; }
__device__ __forceinline__ void take(MaxAcc& m, const float4& x) {
  m.v = make_float4(max1(m.v.x, x.x), max1(m.v.y, x.y), max1(m.v.z, x.z), max1(m.v.w, x.w));
  m.nx = max(m.nx, abs_bits(x.x)); m.ny = max(m.ny, abs_bits(x.y)); m.nz = max(m.nz, abs_bits(x.z)); m.nw = max(m.nw, abs_bits(x.w));
}
// the lanes m apart exchange what they hold: afterwards both hold the maximum of the two
__device__ __forceinline__ void take_xor(MaxAcc& m, int mask) {
  const float4 o = vshfl_xor(m.v, mask);
  const uint32_t ox = (uint32_t)__shfl_xor((int)m.nx, mask), oy = (uint32_t)__shfl_xor((int)m.ny, mask);
  const uint32_t oz = (uint32_t)__shfl_xor((int)m.nz, mask), ow = (uint32_t)__shfl_xor((int)m.nw, mask);
  m.v = make_float4(max1(m.v.x, o.x), max1(m.v.y, o.y), max1(m.v.z, o.z), max1(m.v.w, o.w));
  m.nx = max(m.nx, ox); m.ny = max(m.ny, oy); m.nz = max(m.nz, oz); m.nw = max(m.nw, ow);
}
__device__ __forceinline__ float finish1(float v, uint32_t n) { return n > kInfBits ? __uint_as_float(0x7fc00000u) : v; }
__device__ __forceinline__ float4 finish(const MaxAcc& m) {
  return make_float4(finish1(m.v.x, m.nx), finish1(m.v.y, m.ny), finish1(m.v.z, m.nz), finish1(m.v.w, m.nw));
}
__device__ __forceinline__ float4 or_neg_inf(bool keep, const float4& x) {
  return make_float4(keep ? x.x : neg_inf(), keep ? x.y : neg_inf(), keep ? x.z : neg_inf(), keep ? x.w : neg_inf());
}

// A lane's piece of a row as its four fp32 values -- decoding only, what E::add folds into its sum: the plain types
// widened (fp8: still in the code domain, scale_finish multiplies the finished maximum, and a positive power of two keeps
// the order), the rowwise types fmaf(scale, q, bias), the value the row reads back as.
template <class E>
__device__ __forceinline__ float4 row_values(const typename E::piece& p, const typename E::sb& sb) {
  if constexpr (!E::rowwise) {
    return E::up(p);
  } else if constexpr (std::is_base_of<I8, E>::value) {
    const uint32_t c = p;
    return make_float4(__fmaf_rn(sb.x, (float)(c & 0xffu), sb.y), __fmaf_rn(sb.x, (float)((c >> 8) & 0xffu), sb.y),
                       __fmaf_rn(sb.x, (float)((c >> 16) & 0xffu), sb.y), __fmaf_rn(sb.x, (float)(c >> 24), sb.y));
  } else {
    const float2 f = E::up_sb(sb);
    const uint32_t c = p;
    return make_float4(__fmaf_rn(f.x, (float)(c & 15u), f.y), __fmaf_rn(f.x, (float)((c >> 4) & 15u), f.y),
                       __fmaf_rn(f.x, (float)((c >> 8) & 15u), f.y), __fmaf_rn(f.x, (float)(c >> 12), f.y));
  }
}

// ---------------------------------------------------------------------------
// D % 4 == 0, D <= 256.  One wave per workgroup, G lanes per row (16 B of fp32 per lane), NG = 64 / G rows per load
// instruction, NL loads per lane in flight: the wave moves in rounds of NL * NG rows.
//
// BPW 1 -- one bag per wave, fixed or ragged.  The bag's begin and length are SCALARS (the query's fixed length, or two
// words of its prefix sums), so a ragged launch keeps wave-uniform control flow: no "longest bag of the wave".  A round is
// one coalesced index read (lane i owns the round's row i, clamped onto the bag's last row: a re-read, harmless for a
// maximum), the range check and row offset by the owner, the offsets handed to the loading lanes over the cross-lane
// network, all NL row loads back to back, then the maxima.  A bag longer than a round loops, and the NEXT round's index read
// is issued before this round's row loads, so a further round costs no further dependent index round trip (RM2's 120 rows
// at D 64 are two rounds of NL 20).
//
// BPW 2 / 4 -- fixed-length bags, T % BPW == 0, BPW * L <= NL * NG (plan_sls_max): the wave takes one sample's bags of BPW
// consecutive tables as one round of BPW * L flattened rows, row j belonging to bag j / L; each accumulator takes a row by
// select (-inf otherwise).  The accumulators are indexed by unrolled constants only: registers, never scratch.
//
// Then the butterfly over the lane groups, the NaN words' verdict, fp8's scale, and lane group 0 stores BPW rows.
template <int G, int NL, int BPW, bool NT, class E>
__global__ __launch_bounds__(64) void sls_max_kernel(SlsArgs a) {
  using elem = typename E::elem;
  using piece = typename E::piece;
  constexpr int NG = 64 / G;                       // lane groups = rows per load instruction
  constexpr int R = NL * NG;                       // rows per round
  constexpr int NI = (R + 63) / 64;                // index registers per lane and round
  if (a.ts && threadIdx.x == 0) a.ts[2 * blockIdx.x] = wall_clock64();

  const int lane = threadIdx.x;
  const int g = lane / G;
  const int gl = lane - g * G;
  const int col = min(gl * 4, a.D - 4);            // clamp idle lanes onto valid columns
  const bool col_ok = gl * 4 < a.D;

  // the wave's bags: sample smp, tables t0 .. t0 + BPW - 1 -- uniform
  const int64_t bag0 = (int64_t)blockIdx.x * BPW;
  const int smp = (int)(bag0 / a.T);
  const int t0 = (int)(bag0 - (int64_t)smp * a.T);
  DRS_OWNER_OF(a, smp, b, vrow, ulen, qidx, qoff)
  int beg_v, len_v;
  if (ulen >= 0) {
    beg_v = b * ulen;
    len_v = ulen;
  } else if (BPW == 1) {
    const int32_t* __restrict__ offp = qoff + (int64_t)t0 * a.off_stride;
    beg_v = offp[b];
    len_v = offp[b + 1] - beg_v;
  } else {
    beg_v = len_v = 0;                             // (several bags per wave are planned for fixed lengths only)
  }
  const int beg = __builtin_amdgcn_readfirstlane(beg_v), len = __builtin_amdgcn_readfirstlane(len_v);
  const int n = BPW * len;                         // flattened rows of the wave
  float* __restrict__ o = a.out + (int64_t)vrow * a.ld_out + a.col0 + (int64_t)t0 * a.D + col;

  if (n <= 0) {                                    // empty: +0.0 in every column, no row is loaded
    if (col_ok && g == 0) {
#pragma unroll
      for (int k = 0; k < BPW; ++k) *reinterpret_cast<float4*>(o + (int64_t)k * a.D) = vzero4();
    }
    if (a.ts) {
      __builtin_amdgcn_s_waitcnt(0);
      if (threadIdx.x == 0) a.ts[2 * blockIdx.x + 1] = wall_clock64();
    }
    return;
  }

  const uint32_t D4 = E::pieces_per_row(a.D);      // row stride in pieces: rows * D / 4 < 2^32 (enforced at table creation)
  const int sbd = sb_delta<E>(a.D, col);
  DRS_ROW_LINES(E, a, ln)
  const elem* Wk[BPW];
  uint32_t rows_k[BPW];
#pragma unroll
  for (int k = 0; k < BPW; ++k) {
    Wk[k] = table_base<E>(a.tables) + a.tab_off[t0 + k] + col_elems<E>(col);
    rows_k[k] = (uint32_t)a.tab_rows[t0 + k];
  }
  // which of the wave's bags does flattened row j belong to (j < n)
  auto bag_of = [&](int j) {
    int k = 0;
#pragma unroll
    for (int q = 1; q < BPW; ++q) k += j >= q * len ? 1 : 0;
    return k;
  };
  // the coalesced index read of the round that starts at flattened row r0: lane i owns rows r0 + i, r0 + i + 64, ...
  auto read_indices = [&](int r0, uint32_t (&raw)[NI]) {
#pragma unroll
    for (int q = 0; q < NI; ++q) {
      const int ii = min(r0 + lane + 64 * q, n - 1);
      const int k = bag_of(ii);
      raw[q] = (uint32_t)qidx[(int64_t)(t0 + k) * a.idx_stride + beg + (ii - k * len)];
    }
  };

  MaxAcc acc[BPW];
#pragma unroll
  for (int k = 0; k < BPW; ++k) acc[k] = max_identity();
  bool bad = false;
  uint32_t raw[NI];
  read_indices(0, raw);
  for (int r0 = 0;;) {
    // the owners: range check (Caffe2's ENFORCE: flag it, drop the row) and the row's offset inside its table
    uint32_t roff[NI];
#pragma unroll
    for (int q = 0; q < NI; ++q) {
      uint32_t rk = rows_k[0];
      if (BPW > 1) {
        const int k = bag_of(min(r0 + lane + 64 * q, n - 1));
#pragma unroll
        for (int z = 1; z < BPW; ++z) rk = k == z ? rows_k[z] : rk;
      }
      const bool out = raw[q] >= rk;
      bad |= out;
      roff[q] = out ? kDropped : E::row_piece(raw[q], D4, ln);
    }
    // a further round: its indices are on their way before this round's rows are
    const int r1 = r0 + R;
    const bool more = BPW == 1 && r1 < n;
    if (more) read_indices(r1, raw);

    // every row load of the round, back to back
    piece v[NL];
    typename E::sb sb[NL];
    bool keep[NL];
    [[maybe_unused]] int kj[NL];
#pragma unroll
    for (int u = 0; u < NL; ++u) {
      const int j = g + NG * u;                    // (j >> 6) == (NG * u) >> 6: compile time
      uint32_t ro = (uint32_t)__shfl((int)roff[(NG * u) >> 6], j & 63);
      keep[u] = ro != kDropped;
      ro = keep[u] ? ro : 0u;                      // (a dropped row reads row 0: valid memory, never looked at)
      const elem* W = Wk[0];
      if (BPW > 1) {
        kj[u] = bag_of(min(j, n - 1));
#pragma unroll
        for (int z = 1; z < BPW; ++z) W = kj[u] == z ? Wk[z] : W;
      }
      const piece* rp = reinterpret_cast<const piece*>(W) + (uint64_t)ro;
      if constexpr (NT) v[u] = ld_nt(rp);          // "sls_nt" 1: the rows are read once
      else v[u] = *rp;
      sb[u] = E::template load_sb<NT>(rp, sbd);
    }
    __builtin_amdgcn_sched_barrier(0);             // loads first, then the maxima

#pragma unroll
    for (int u = 0; u < NL; ++u) {
      const float4 x = or_neg_inf(keep[u], row_values<E>(v[u], sb[u]));
      if (BPW == 1) {
        take(acc[0], x);
      } else {
#pragma unroll
        for (int k = 0; k < BPW; ++k) take(acc[k], or_neg_inf(kj[u] == k, x));
      }
    }
    if (!more) break;
    r0 = r1;
  }
#pragma unroll
  for (int k = 0; k < BPW; ++k)
#pragma unroll
    for (int m = G; m < 64; m <<= 1) take_xor(acc[k], m);

  if (bad) atomicOr(a.err, 1);
  // every group holds every maximum after the butterfly; group 0 stores them, one row per bag
  if (col_ok && g == 0) {
#pragma unroll
    for (int k = 0; k < BPW; ++k) {
      float4 r = finish(acc[k]);
      scale_finish<E>(r, a, t0 + k);
      *reinterpret_cast<float4*>(o + (int64_t)k * a.D) = r;
    }
  }
  if (a.ts) {
    __builtin_amdgcn_s_waitcnt(0);                 // include the output store in the span
    if (threadIdx.x == 0) a.ts[2 * blockIdx.x + 1] = wall_clock64();
  }
}

// ANY other row width (D % 4 != 0 or D > 256): sls_any_kernel's walk -- a wave per bag, lane c takes columns c, c + 64, ...
// (dword / byte loads: rows need no alignment), rows one at a time, ragged bags through the prefix sums.  Every lane reads
// the same index, so an out-of-range row is skipped by a uniform branch.
template <class E>
__global__ __launch_bounds__(64) void sls_max_any_kernel(SlsArgs a) {
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
  const typename E::elem* __restrict__ W = table_base<E>(a.tables) + a.tab_off[t];
  const uint32_t rows = (uint32_t)a.tab_rows[t];
  const int D = a.D;
  DRS_ROW_LINES(E, a, ln)
  float* o = a.out + (int64_t)vrow * a.ld_out + a.col0 + (int64_t)t * D;
  bool bad = false;
  for (int c0 = 0; c0 < D; c0 += 64 * 4) {          // four columns per lane and pass
    float acc[4] = {neg_inf(), neg_inf(), neg_inf(), neg_inf()};
    uint32_t nan[4] = {0u, 0u, 0u, 0u};
    for (int j = beg; j < end; ++j) {
      const uint32_t r = (uint32_t)ip[j];
      if (r >= rows) {                               // (uniform)
        bad = true;
        continue;
      }
      if constexpr (E::rowwise) {
        const uint8_t* row;
        if constexpr (E::lines) row = W + (int64_t)E::row_piece(r, E::pieces_per_row(D), ln) * kPieceElems<E>;
        else row = W + (int64_t)r * (int64_t)E::pieces_per_row(D) * kPieceElems<E>;
        const float2 sb = E::row_sb(row, D);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int c = c0 + lane + 64 * k;
          if (c < D) {
            const float x = __fmaf_rn(sb.x, E::code(row, c), sb.y);
            acc[k] = max1(acc[k], x);
            nan[k] = max(nan[k], abs_bits(x));
          }
        }
      } else {
        const typename E::elem* row = W + (int64_t)r * D;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int c = c0 + lane + 64 * k;
          if (c < D) {
            const float x = E::up1(row[c]);
            acc[k] = max1(acc[k], x);
            nan[k] = max(nan[k], abs_bits(x));
          }
        }
      }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int c = c0 + lane + 64 * k;
      float r = end > beg ? finish1(acc[k], nan[k]) : 0.0f;   // an empty bag: +0.0
      if constexpr (E::scaled) r = __fmul_rn(r, a.tab_scale[t]);
      if (c < D) o[c] = r;
    }
  }
  if (bad) atomicOr(a.err, 1);
  if (a.ts) {
    __builtin_amdgcn_s_waitcnt(0);
    if (threadIdx.x == 0) a.ts[2 * blockIdx.x + 1] = wall_clock64();
  }
}

int max_lanes_per_row(int D) { return D <= 8 ? 2 : D <= 16 ? 4 : D <= 32 ? 8 : D <= 64 ? 16 : D <= 128 ? 32 : 64; }

// the launch for tables of element type E: the plan's dispatch-log line, then its instance
template <class E>
hipError_t launch_max_e(const SlsArgs& a, const SlsPlan& p, const Tune& tune, hipStream_t s, hipEvent_t stop) {
  const char* dt = E::tag;
  const long long wg = (long long)p.grid;
  const dim3 grid((unsigned)p.grid);
  if (p.form == SlsForm::any) {
    if (!wg) return hipSuccess;             // (an empty launch of this form is not logged, as sls_any_kernel's is not)
    log_launch(tune.log, "sls_max_any_kernel%s%s%s[%lld wg, D=%d]", *dt ? "<" : "", dt, *dt ? ">" : "", wg, a.D);
    launch_k(sls_max_any_kernel<E>, grid, s, stop, a);
    return hipGetLastError();
  }
  log_launch(tune.log, "sls_max_kernel<%d,%d,bpw%d%s%s%s>[%lld wg, L=%d]", p.G, p.NL, p.BPW, p.nt ? ",nt" : "", *dt ? "," : "", dt, wg, p.L);
  if (!wg) return hipSuccess;               // an empty launch enqueues nothing
  with_int<2, 4, 8, 16, 32, 64>(p.G, [&](auto G) { with_int<5, 10, 20>(p.NL, [&](auto NL) { with_int<0, 1>(p.nt, [&](auto NT) {
    with_int<1, 2, 4>(p.BPW, [&](auto BPW) {
      if constexpr (BPW == 1 || NL == 5) launch_k(sls_max_kernel<G, NL, BPW, NT != 0, E>, grid, s, stop, a);
    });
  }); }); });
  return hipGetLastError();
}

}  // namespace

// The plan of a max launch (a.pool == 2).  SlsForm::any: sls_max_any_kernel; SlsForm::one: the existing one-lookup copy form,
// handed over unchanged -- a one-row bag's maximum is its row; SlsForm::flat: sls_max_kernel<G, NL, BPW, nt>.  The rules are
// the sum forms' (their measurements; none of them measured for max): queries that share a fixed length L
// take the smallest NL of {5, 10, 20} with NL * NG >= BPW * L, else 20 and the kernel loops; short fixed bags share a wave
// under sls_flat_kernel's rule (T % BPW == 0, BPW * L <= 5 * NG: one round of NL 5); ragged bags, or fixed lengths that
// differ between the queries, NL 10.  "sls_exact", "sls_flat" and "sls_bpw" play no part: a maximum has one value.  The
// uniform "sls_nt" is honoured; a mixed "sls_nt_mask" falls back to it.  Weights play no part either (the engine refuses
// them under "sls_max" 1 before a launch is planned).
SlsPlan plan_sls_max(const SlsArgs& a, const Tune& tune, int dtype) {
  SlsPlan p;
  p.dtype = dtype;
  const int D = a.D, n_q = a.q.n_q, n_smp = a.q.cum[n_q];
  const int64_t n_bags = (int64_t)n_smp * a.T;
  if ((D & 3) || D > 256) {
    p.form = SlsForm::any;
    p.exact = true;
    p.grid = n_bags;
    return p;
  }
  int L = n_q >= 1 ? a.uniform_len[0] : -1;
  for (int i = 1; i < n_q; ++i) L = a.uniform_len[i] == L ? L : -1;
  if (L == 1 && tune.sls_one && (D == 16 || D == 32 || D == 64 || D == 128)) {
    p.form = SlsForm::one;
    p.exact = true;
    p.G = D / 4;
    p.BW = tune.sls_one == 64 || tune.sls_one == 16 ? tune.sls_one : (int64_t)a.T * ((n_smp + 63) / 64) < 1024 ? 16 : 64;
    p.tiles = (n_smp + p.BW - 1) / p.BW;
    p.grid = (int64_t)a.T * p.tiles;
    return p;
  }
  const int G = max_lanes_per_row(D), NG = 64 / G;
  p.form = SlsForm::flat;
  p.G = G;
  p.L = L < 0 ? -1 : L;
  p.nt = tune.sls_nt != 0;
  p.BPW = 1;
  p.NL = 10;
  if (L >= 1) {
    for (int c : {4, 2})
      if (a.T % c == 0 && c * L <= 5 * NG) { p.BPW = c; break; }
    const int need = (p.BPW * L + NG - 1) / NG;
    p.NL = need <= 5 ? 5 : need <= 10 ? 10 : 20;
  } else if (L == 0) {
    p.NL = 5;
  }
  p.grid = (int64_t)n_smp * (a.T / p.BPW);
  return p;
}

hipError_t launch_sls_max(const SlsArgs& a, const SlsPlan& p, const Tune& tune, hipStream_t s, hipEvent_t stop) {
  if (a.D <= 0 || a.pool != 2 || (p.form != SlsForm::any && p.form != SlsForm::one && p.form != SlsForm::flat)) return hipErrorInvalidValue;
  if (p.form == SlsForm::one) {             // the copy form never sees pool 2: it stores 0.0f + row
    SlsArgs a1 = a;
    a1.pool = 0;
    return launch_sls(a1, p, tune, s, stop);
  }
  switch (p.dtype) {
    case DRS_TABLE_FP16: return launch_max_e<F16>(a, p, tune, s, stop);
    case DRS_TABLE_BF16: return launch_max_e<BF16>(a, p, tune, s, stop);
    case DRS_TABLE_FP8_E4M3: return a.tab_scale ? launch_max_e<F8>(a, p, tune, s, stop) : hipErrorInvalidValue;
    case DRS_TABLE_INT8_ROWWISE: return a.ln_pad ? launch_max_e<I8L>(a, p, tune, s, stop) : launch_max_e<I8>(a, p, tune, s, stop);
    case DRS_TABLE_INT4_ROWWISE: return a.ln_pad ? launch_max_e<I4L>(a, p, tune, s, stop) : launch_max_e<I4>(a, p, tune, s, stop);
    default: return launch_max_e<F32>(a, p, tune, s, stop);
  }
}

}  // namespace drs
