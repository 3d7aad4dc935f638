// The one-bag-per-wave gathers with a cache policy PER TABLE ("sls_nt_mask"): sls_flatc_kernel's walk (and, below, the split
// ring walk) on fp32 rows, unweighted, whose row loads are non-temporal for the tables whose bit of SlsArgs::nt_mask is set and plain for the
// others.  Which policy is fast depends on the physical memory a table lies in, and a model's tables lie in
// different gigabytes of the arena.  A wave reads rows of ONE table, so the bit is a scalar: one branch per wave into two
// copies of the loads and sums, one of ld_nt loads only, one of plain loads only -- a select between the two inside one
// copy is merged into a plain load (sls.hip).  The same rows, the same sums in the same order, the same butterfly, store,
// error word and stamps as sls_flatc_kernel<G, NL, *, F32>: the same bits under every mask.
#include "drs_internal.h"
#include "launch_host.h"
#include "owner_dev.h"
#include "sls_dev.h"

namespace drs {
namespace {

template <int G, int NL>
__global__ __launch_bounds__(64) void sls_flatc_ntm_kernel(SlsArgs a, int L) {
  constexpr int NG = 64 / G;                       // lane groups = rows per load instruction
  constexpr int NI = (NL * NG + 63) / 64;          // index registers per lane
  if (a.ts && threadIdx.x == 0) a.ts[2 * blockIdx.x] = wall_clock64();

  const int lane = threadIdx.x;
  const int g = lane / G;
  const int gl = lane - g * G;
  const int col = min(gl * 4, a.D - 4);            // clamp idle lanes onto valid columns
  const bool col_ok = gl * 4 < a.D;

  // the wave's bag: sample smp, table t -- uniform
  const int64_t bag = (int64_t)blockIdx.x;
  const int smp = (int)(bag / a.T);
  const int t = (int)(bag - (int64_t)smp * a.T);
  DRS_OWNER_OF(a, smp, b, vrow, ulen, qidx, qoff)
  const uint32_t D4 = F32::pieces_per_row(a.D);    // row stride in pieces: rows * D / 4 < 2^32 (enforced at table creation)
  const float* W = a.tables + a.tab_off[t] + col;
  const uint32_t rows = (uint32_t)a.tab_rows[t];

  // ONE coalesced index read: lane i owns rows i, i+64, ...; range check (Caffe2 ENFORCE) by the owner; an out-of-range
  // index reads row 0 and is dropped from nothing: it is flagged, as in sls_flatc_kernel
  uint32_t roff[NI];
  bool bad = false;
#pragma unroll
  for (int q = 0; q < NI; ++q) {
    const int i = lane + 64 * q;
    const int ii = min(i, L - 1);
    uint32_t r = (uint32_t)qidx[(int64_t)t * a.idx_stride + (int64_t)b * L + ii];
    bad |= i < L && r >= rows;
    r = r < rows ? r : 0u;
    roff[q] = r * D4;
  }

  float4 acc = vzero4();
  // every row load of the wave, then the sums in u order; nt: the loads' policy, a compile-time constant of the copy
  auto rows_in = [&](auto nt) {
    float4 v[NL];
#pragma unroll
    for (int u = 0; u < NL; ++u) {
      const int j = g + NG * u;                      // (j >> 6) == (NG * u) >> 6: compile time
      const uint32_t ro = (uint32_t)__shfl((int)roff[(NG * u) >> 6], j & 63);
      if constexpr (decltype(nt)::value) v[u] = ld_nt(reinterpret_cast<const float4*>(W) + (uint64_t)ro);
      else v[u] = reinterpret_cast<const float4*>(W)[(uint64_t)ro];
    }
#pragma unroll
    for (int u = 0; u < NL; ++u) F32::add(acc, g + NG * u < L, v[u], NoSb{});
  };
  // (the distinct comments at both ends of each arm keep the optimiser from hoisting or sinking the arms' common
  // instructions into one, which drops the hint)
  if ((a.nt_mask >> (uint32_t)__builtin_amdgcn_readfirstlane(t)) & 1u) {
    asm volatile("; drs sls: table read nt" ::: "memory");
    rows_in(std::true_type{});
    asm volatile("; drs sls: nt rows summed" ::: "memory");
  } else {
    asm volatile("; drs sls: table read plain" ::: "memory");
    rows_in(std::false_type{});
    asm volatile("; drs sls: plain rows summed" ::: "memory");
  }
#pragma unroll
  for (int m = G; m < 64; m <<= 1) vadd(acc, vshfl_xor(acc, m));

  if (bad) atomicOr(a.err, 1);
  pool_finish(acc, a.pool, L);
  if (col_ok && g == 0) *reinterpret_cast<float4*>(a.out + (int64_t)vrow * a.ld_out + a.col0 + (int64_t)t * a.D + col) = acc;
  if (a.ts) {
    __builtin_amdgcn_s_waitcnt(0);   // include the output store in the span
    if (threadIdx.x == 0) a.ts[2 * blockIdx.x + 1] = wall_clock64();
  }
}

// The split ring walk with a policy per table: sls_kernel<G, false, *, F32>'s wave-per-bag walk (sls.hip), unweighted.  The
// wave walks ONE bag, i.e. one table: the walk over the bag's chunks exists twice, with ld_nt loads only and with plain
// loads only, and the wave branches once on its table's bit.  The same staging, rings, sums in the same order, butterfly,
// store, error word and stamps: the same bits under every mask.
constexpr int kChunk = 128;  // indices staged in LDS per bag per round (as sls.hip)

template <int G>
__global__ __launch_bounds__(64) void sls_ntm_kernel(SlsArgs a) {
  constexpr int U = 4;
  constexpr int NG = 64 / G;                  // lane groups per wave = row stride between a lane's loads
  __shared__ __attribute__((aligned(16))) int32_t s_idx[kChunk];
  if (a.ts && threadIdx.x == 0) a.ts[2 * blockIdx.x] = wall_clock64();

  const int lane = threadIdx.x;
  const int g = lane / G;
  const int gl = lane - g * G;
  const int col = min(gl * 4, a.D - 4);       // clamp idle lanes onto valid columns
  const bool col_ok = gl * 4 < a.D;

  const int64_t n_bags = (int64_t)a.q.cum[a.q.n_q] * a.T;
  const int64_t bag = (int64_t)blockIdx.x;
  const bool bag_ok = bag < n_bags;
  const int smp = bag_ok ? (int)(bag / a.T) : 0;
  const int t = bag_ok ? (int)(bag - (int64_t)smp * a.T) : 0;
  DRS_OWNER_OF(a, smp, b, vrow, ulen, qidx, qoff)
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
  const float* __restrict__ W = a.tables + a.tab_off[t] + col;
  const uint32_t rows = (uint32_t)a.tab_rows[t];
  const uint32_t Dv = F32::pieces_per_row(a.D);   // rows * D / 4 < 2^32 (enforced at table creation)
  float4 acc = vzero4();
  bool bad = false;
  const int len = end - beg;
  const int len_max = __builtin_amdgcn_readfirstlane(len);   // (one bag per wave: every lane's length)

  // the walk over the bag's chunks; nt: the row loads' policy, a compile-time constant of the copy
  auto walk = [&](auto nt) {
    for (int c = 0; c < len_max; c += kChunk) {
      const int n = min(kChunk, len - c);
      const int n_u = min(kChunk, len_max - c);
      const int last = max(n - 1, 0);
      const int j0 = beg + c;
      // stage the next indices of the bag in LDS: coalesced, clamped (branch-free)
      for (int c0 = 0; c0 < n_u; c0 += 4 * 64) {
        int32_t tmp[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) tmp[q] = n > 0 ? ip[j0 + min(c0 + q * 64 + lane, last)] : 0;
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (c0 + q * 64 + lane < kChunk) s_idx[c0 + q * 64 + lane] = tmp[q];
      }
      __builtin_amdgcn_wave_barrier();

      auto issue = [&](float4 (&ring)[U], int pos) {
        uint32_t r[U];
#pragma unroll
        for (int u = 0; u < U; ++u) r[u] = (uint32_t)s_idx[min(pos + u * NG, last)];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          bad |= (pos + u * NG < n) && (r[u] >= rows);
          r[u] = r[u] < rows ? r[u] : 0u;
          const float4* rp_ = reinterpret_cast<const float4*>(W) + (uint64_t)(r[u] * Dv);
          if constexpr (decltype(nt)::value) ring[u] = ld_nt(rp_); else ring[u] = *rp_;
        }
      };
      auto consume = [&](const float4 (&ring)[U], int pos) {
#pragma unroll
        for (int u = 0; u < U; ++u) F32::add(acc, pos + u * NG < n, ring[u], NoSb{});
      };
      // two register rings: while ring A (round k) is summed in index order, ring B (round k + 1) is in flight
      constexpr int R = U * NG;
      float4 ringA[U], ringB[U];
      int jj = g;                                     // per-lane row position
      int ju = 0;                                     // uniform round position
      issue(ringA, jj);
      for (;;) {
        if (ju + R < n_u) {
          issue(ringB, jj + R);
          __builtin_amdgcn_sched_barrier(0);   // loads first, then the sums
          consume(ringA, jj);
          asm volatile("; drs sls: A summed, B in flight" ::: "memory");
        } else {
          consume(ringA, jj);
          asm volatile("; drs sls: A summed, tail" ::: "memory");
          break;
        }
        if (ju + 2 * R < n_u) {
          issue(ringA, jj + 2 * R);
          __builtin_amdgcn_sched_barrier(0);
          consume(ringB, jj + R);
          asm volatile("; drs sls: B summed, A in flight" ::: "memory");
        } else {
          consume(ringB, jj + R);
          asm volatile("; drs sls: B summed, tail" ::: "memory");
          break;
        }
        jj += 2 * R;
        ju += 2 * R;
      }
      __builtin_amdgcn_wave_barrier();
    }
  };
  if ((a.nt_mask >> (uint32_t)__builtin_amdgcn_readfirstlane(t)) & 1u) {
    asm volatile("; drs sls: table read nt" ::: "memory");
    walk(std::true_type{});
    asm volatile("; drs sls: nt rows summed" ::: "memory");
  } else {
    asm volatile("; drs sls: table read plain" ::: "memory");
    walk(std::false_type{});
    asm volatile("; drs sls: plain rows summed" ::: "memory");
  }
#pragma unroll
  for (int m = G; m < 64; m <<= 1) vadd(acc, vshfl_xor(acc, m));
  if (bad) atomicOr(a.err, 1);
  pool_finish(acc, a.pool, len);
  if (bag_ok && col_ok && g == 0) *reinterpret_cast<float4*>(a.out + (int64_t)vrow * a.ld_out + a.col0 + (int64_t)t * a.D + col) = acc;
  if (a.ts) {
    __builtin_amdgcn_s_waitcnt(0);   // include the output store in the span
    if (threadIdx.x == 0) a.ts[2 * blockIdx.x + 1] = wall_clock64();
  }
}

}  // namespace

hipError_t launch_sls_ntm(const SlsArgs& a_in, const SlsPlan& p, hipStream_t s, hipEvent_t stop) {
  if ((p.form != SlsForm::flatc && p.form != SlsForm::ring) || p.exact || p.nt != 2 || p.dtype != DRS_TABLE_FP32 || p.weighted)
    return hipErrorInvalidValue;
  SlsArgs a = a_in;
  a.nt_mask = p.nt_mask;
  const dim3 grid((unsigned)p.grid);
  if (p.form == SlsForm::ring) {
    with_int<2, 4, 8, 16, 32, 64>(p.G, [&](auto G) { launch_k(sls_ntm_kernel<G>, grid, s, stop, a); });
  } else {
    with_int<8, 16, 32>(p.G, [&](auto G) { with_int<5, 10, 20>(p.NL, [&](auto NL) {
      launch_k(sls_flatc_ntm_kernel<G, NL>, grid, s, stop, a, p.L);
    }); });
  }
  return hipGetLastError();
}

}  // namespace drs
