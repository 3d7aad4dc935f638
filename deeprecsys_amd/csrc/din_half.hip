// DIN over narrow tables ("din_table_dtype" 1 | 2 | 4): the pipelined fused launch of din.hip -- gather + attention units +
// Concat, hidden width 1, fixed bags of at most 3 rows, D 32 or 64 -- over the fp16, bf16 and fp8 e4m3 row policies of
// sls_dev.h.  A translation unit of its own: din.hip's kernels keep their register allocation (tools/kernel_isa_diff.py).
//
// The contract is the project's invariant for narrow tables: the launch returns, bit for bit, what din_pipe_kernel returns
// on an fp32 engine that holds the upcast (fp8: decoded x 2^-k_t) tables.  So the association is din_pipe_kernel's: G = D / 4
// lanes per row, lane gl owns columns 4 gl .. 4 gl + 3; kWaves waves serve S samples; lane group gg takes units gg,
// gg + NGB, ... in rising order; a bag is pooled from +0 in index order (a slot past the bag's end adds the zero page's +0);
// the unit's arithmetic is din_pipe_kernel's line by line; the lane-group butterfly runs m = G .. 32 and the waves add
// through LDS in wave order.  Nothing is masked by a multiplication: the zero page, `have`, the kNone slots and the live
// masks are selects and addresses, as there.
//
// Inside that contract the rows are a half or a quarter as wide, and the kernel is laid out for that:
//   * a slot keeps its row pieces in the STORED type (uint2 per piece for fp16 / bf16, one dword for fp8) and widens them
//     with E::up when the unit is applied -- exact.  At S 4 the rows of one slot are 24 VGPRs (12 at fp8) against fp32's 48;
//   * the depth P is a template parameter (2 and 4 are instantiated; narrow_depth below says which one a launch takes);
//   * fp8: thread t also stages its table's 2^-k_t; a pooled bag is multiplied by it once, after its last add and before
//     anything reads it (scale_finish's rule: a power of two commutes with the adds, so the twin's bits hold).
#include "drs_internal.h"
#include "launch_host.h"
#include "owner_dev.h"
#include "sls_dev.h"

namespace drs {
namespace {

__device__ __forceinline__ float4 ld4w(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ float dot4(const float4& a, const float4& b, float acc) {
  acc = fmaf(a.x, b.x, acc); acc = fmaf(a.y, b.y, acc); acc = fmaf(a.z, b.z, acc); acc = fmaf(a.w, b.w, acc);
  return acc;
}
__device__ __forceinline__ float4 relu4(float4 v) {
  return make_float4(fmaxf(v.x, 0.f), fmaxf(v.y, 0.f), fmaxf(v.z, 0.f), fmaxf(v.w, 0.f));
}
// a row piece in its stored type: read once per launch -- non-temporal when NT ("din_nt", a compile-time property)
template <bool NT, class P>
__device__ __forceinline__ P ld_piece(const P* p) {
  if constexpr (NT) return ld_nt(p); else return *p;
}
// which S samples a workgroup serves: din.hip's xcd_group (contiguous runs of sample groups per XCD; a renumbering only)
__device__ __forceinline__ unsigned xcd_group() {
  const unsigned nb_ = gridDim.x, xcd_ = blockIdx.x & 7u, per_ = nb_ >> 3, rem_ = nb_ & 7u;
  return xcd_ * per_ + (xcd_ < rem_ ? xcd_ : rem_) + (blockIdx.x >> 3);
}
// din.hip's group_sum: the butterfly of __shfl_xor(., 1 / 2 / 4 / 8) on the DPP network -- same pairs, same bits
template <int CTRL>
__device__ __forceinline__ float dpp_f(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, false));
}
template <int G>
__device__ __forceinline__ float group_sum(float v) {
  static_assert(G == 8 || G == 16, "lane groups of 8 or 16");
  v += dpp_f<0xB1>(v);                     // quad_perm [1,0,3,2]
  v += dpp_f<0x4E>(v);                     // quad_perm [2,3,0,1]
  v += dpp_f<0x141>(v);                    // row_half_mirror
  if (G == 16) v += dpp_f<0x140>(v);       // row_mirror
  return v;
}
// a pooled bag out of the code domain (fp8): times its table's 2^-k, a product of its own (never folded into a later add)
__device__ __forceinline__ float4 times_scale(const float4& v, float s) {
#pragma clang fp contract(off)
  return make_float4(v.x * s, v.y * s, v.z * s, v.w * s);
}

template <int G, int S, int NW, int P, bool NT, class E>
__global__ __launch_bounds__(64 * NW, 2) void din_pipe_narrow_kernel(SlsArgs a, const float* __restrict__ packed,
                                                                     int64_t stride, const float* __restrict__ zero,
                                                                     float* __restrict__ R, int64_t ldr) {
  using elem = typename E::elem;
  using piece = typename E::piece;
  constexpr int NG = 64 / G, NGB = NW * NG, D = 4 * G, C = 3;
  constexpr uint32_t kNone = 0xffffffffu;            // staged "no row here": the load reads the zero page
  static_assert(S <= NW, "wave s finishes sample s");
  static_assert(kPieceElems<E> == 4 && !E::rowwise, "a piece is four plain elements");
  __shared__ float4 s_z[S][NW][G];
  extern __shared__ int64_t s_dyn[];
  const int T = a.T;
  int64_t* s_off = s_dyn;                                         // [T] offset of the table, in elements (fp8: bytes)
  uint32_t* s_r = reinterpret_cast<uint32_t*>(s_off + T);         // [T][S * C] row numbers (kNone past the bag's end)
  [[maybe_unused]] float* s_scale = reinterpret_cast<float*>(s_r + (size_t)T * (S * C));   // fp8: [T] the table's 2^-k
  if (a.ts && threadIdx.x == 0) a.ts[2 * blockIdx.x] = wall_clock64();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane / G, gl = lane - g * G, gg = wave * NG + g;
  const int n_smp = a.q.cum[a.q.n_q];
  const int U = T - 3;
  const int col = gl * 4;

  const unsigned grp = xcd_group();
  bool live[S];
  int vrow[S];
  {
    // ---- stage: thread t takes table t (the owners of the S samples are only needed here) ----------
    Owner ow[S];
#pragma unroll
    for (int s = 0; s < S; ++s) {
      const int smp = (int)grp * S + s;
      live[s] = smp < n_smp;
      ow[s] = owner_of(a, live[s] ? smp : 0);
      vrow[s] = ow[s].vrow;
    }
    bool bad = false;
    for (int t = threadIdx.x; t < T; t += 64 * NW) {
      const uint32_t rows = (uint32_t)a.tab_rows[t];
      s_off[t] = a.tab_off[t];
      if constexpr (E::scaled) s_scale[t] = a.tab_scale[t];
      uint32_t r[S][C];
#pragma unroll
      for (int s = 0; s < S; ++s) {
        const int len = live[s] ? ow[s].ulen : 0;
        const int32_t* ip = ow[s].idx + (int64_t)t * a.idx_stride;
        if (len == C) {                        // (uniform per sample) the whole bag with one 12-byte load
          typedef int32_t I3 __attribute__((ext_vector_type(3), aligned(4)));
          const I3 i3 = *reinterpret_cast<const I3*>(ip + ow[s].b * C);
          r[s][0] = (uint32_t)i3.x; r[s][1] = (uint32_t)i3.y; r[s][2] = (uint32_t)i3.z;
        } else {
#pragma unroll
          for (int c = 0; c < C; ++c) r[s][c] = (uint32_t)ip[c < len ? ow[s].b * ow[s].ulen + c : 0];
        }
      }
#pragma unroll
      for (int s = 0; s < S; ++s) {
        const int len = live[s] ? ow[s].ulen : 0;
#pragma unroll
        for (int c = 0; c < C; ++c) {
          const bool in = c < len;
          bad |= in && r[s][c] >= rows;
          s_r[t * (S * C) + s * C + c] = !in ? kNone : r[s][c] < rows ? r[s][c] : 0u;
        }
      }
    }
    if (bad) atomicOr(a.err, 1);
  }
  __syncthreads();

  // the zero page, through the piece type: this lane's piece of an all-zero row
  const piece* zcol = reinterpret_cast<const piece*>(zero) + gl;
  // the staged rows of the S bags of table t -> v, still in the stored type
  auto issue_rows = [&](int t, bool have, piece (&v)[S][C]) {
    const elem* __restrict__ W = table_base<E>(a.tables) + s_off[t] + col_elems<E>(col);
    uint32_t r[S * C];
#pragma unroll
    for (int x = 0; x < S * C; ++x) r[x] = s_r[t * (S * C) + x];
#pragma unroll
    for (int s = 0; s < S; ++s)
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const uint32_t rr = r[s * C + c];
        const elem* p = W + (uint64_t)(rr * ((uint32_t)D >> 2)) * kPieceElems<E>;
        v[s][c] = ld_piece<NT>(have && rr != kNone ? reinterpret_cast<const piece*>(p) : zcol);
      }
  };
  // widen and pool: from +0 in index order, then (fp8) out of the code domain with table t's scale
  auto pool = [&](const piece (&v)[S][C], [[maybe_unused]] int t, float4 (&acc)[S]) {
#pragma unroll
    for (int s = 0; s < S; ++s) {
      acc[s] = vzero4();
#pragma unroll
      for (int c = 0; c < C; ++c) vadd(acc[s], E::up(v[s][c]));
    }
    if constexpr (E::scaled) {
      const float sc = s_scale[t];
#pragma unroll
      for (int s = 0; s < S; ++s) acc[s] = times_scale(acc[s], sc);
    }
  };
  // one unit's weights, this lane's pieces: [ W1 : 3D | W2 : D | b2 : D | b1 ] (h = 1) -- fp32, as in din_pipe_kernel
  struct Wt {
    float4 w1u, w1a, w1s, w2, b2;
    float b1;
  };
  auto issue_w = [&](int i, Wt& w) {
    const float* __restrict__ wp = packed + (int64_t)i * stride;
    w.w1u = ld4w(wp + col);
    w.w1a = ld4w(wp + D + col);
    w.w1s = ld4w(wp + 2 * D + col);
    w.w2 = ld4w(wp + 3 * D + col);
    w.b2 = ld4w(wp + 4 * D + col);
    w.b1 = wp[5 * D];
  };

  // slots: the candidate ad goes out together with the group's first P units
  const int K = (U + NGB - 1) / NGB;        // units per lane group (the last one may be missing: `have`)
  piece v[P][S][C];
  Wt w[P];
  float4 ad[S];
  {
    piece vad[S][C];
    issue_rows(T - 2, true, vad);
#pragma unroll
    for (int j = 0; j < P; ++j) {
      const int i = gg + j * NGB;
      const bool have = j < K && i < U;
      issue_rows(have ? 1 + i : T - 2, have, v[j]);
      issue_w(have ? i : 0, w[j]);
    }
    pool(vad, T - 2, ad);
  }

  // pass-through features of the top MLP's input row: lane group 0 of waves 0..2 takes one each
  // (profile, candidate ad, context)
  if (wave < 3 && g == 0) {
    const int dst = wave == 0 ? 0 : wave == 1 ? 2 * D : 3 * D;
    float4 pv[S];
    if (wave == 1) {
#pragma unroll
      for (int s = 0; s < S; ++s) pv[s] = ad[s];
    } else {
      const int tp = wave == 0 ? 0 : T - 1;
      piece vp[S][C];
      issue_rows(tp, true, vp);
      pool(vp, tp, pv);
    }
#pragma unroll
    for (int s = 0; s < S; ++s)
      if (live[s]) *reinterpret_cast<float4*>(R + (int64_t)vrow[s] * ldr + dst + col) = pv[s];
  }

  float4 z[S];
#pragma unroll
  for (int s = 0; s < S; ++s) z[s] = vzero4();
  // unit k of this lane group out of slot j; then the slot takes unit k + P (into the SAME registers, after the unit's
  // arithmetic, as in din_pipe_kernel)
  auto step = [&](int j, int k, bool refill) {
    __builtin_amdgcn_sched_barrier(0);
    const int i = gg + k * NGB;
    const bool have = i < U;
    float4 u[S];
    pool(v[j], have ? 1 + i : T - 2, u);     // (a missing unit's slot holds the zero page: +0 under any table's scale)
    const Wt& wt = w[j];
#pragma unroll
    for (int s = 0; s < S; ++s) {
      const float4 sum = make_float4(u[s].x + ad[s].x, u[s].y + ad[s].y, u[s].z + ad[s].z, u[s].w + ad[s].w);
      float pd = dot4(u[s], wt.w1u, 0.f);
      pd = dot4(ad[s], wt.w1a, pd);
      pd = dot4(sum, wt.w1s, pd);
      pd = group_sum<G>(pd);
      const float y = fmaxf(pd + wt.b1, 0.f);
      float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
      o.x = fmaf(y, wt.w2.x, o.x); o.y = fmaf(y, wt.w2.y, o.y);
      o.z = fmaf(y, wt.w2.z, o.z); o.w = fmaf(y, wt.w2.w, o.w);
      vadd(o, wt.b2);
      o = relu4(o);
      z[s].x += have ? o.x : 0.f; z[s].y += have ? o.y : 0.f;
      z[s].z += have ? o.z : 0.f; z[s].w += have ? o.w : 0.f;
    }
    if (refill) {
      const int in_ = gg + (k + P) * NGB;
      const bool hn = in_ < U;
      issue_rows(hn ? 1 + in_ : T - 2, hn, v[j]);
      issue_w(hn ? in_ : 0, w[j]);
    }
    __builtin_amdgcn_sched_barrier(0);
  };
  // rounds in which every slot is refilled (no branch around the loads) ...
  int k0 = 0;
  for (; k0 + 2 * P <= K; k0 += P) {
#pragma unroll
    for (int j = 0; j < P; ++j) step(j, k0 + j, true);
  }
  // ... and the last ones
  for (; k0 < K; k0 += P) {
#pragma unroll
    for (int j = 0; j < P; ++j) {
      const int k = k0 + j;
      if (k >= K) break;                       // (uniform)
      step(j, k, k + P < K);
    }
  }
  // partial sums: the lane groups of a wave over the cross-lane network, the waves through LDS
#pragma unroll
  for (int s = 0; s < S; ++s) {
#pragma unroll
    for (int m = G; m < 64; m <<= 1) vadd(z[s], vshfl_xor(z[s], m));
    if (g == 0) s_z[s][wave][gl] = z[s];
  }
  __syncthreads();
#pragma unroll
  for (int s = 0; s < S; ++s)
    if (wave == s && g == 0 && live[s]) {          // wave s finishes sample s (S <= NW)
      float4 t = s_z[s][0][gl];
#pragma unroll
      for (int w_ = 1; w_ < NW; ++w_) vadd(t, s_z[s][w_][gl]);
      *reinterpret_cast<float4*>(R + (int64_t)vrow[s] * ldr + D + col) = t;
    }
  if (a.ts) {
    __builtin_amdgcn_s_waitcnt(0);
    __syncthreads();
    if (threadIdx.x == 0) a.ts[2 * blockIdx.x + 1] = wall_clock64();
  }
}

// Units in flight per lane group.  With half-width rows depth 4 keeps the bytes in flight per lane that fp32's depth 2 has
// (kPipeNarrow).  Measured on the din workload (profiles/r37_din_narrow_tables.md: three alternating runs per arm), depth 4
// against 2: fp16 170.4 k against 166.9 k queries/s (launch 45.5 against 46.4 us), bf16 169.6 k against 167.8 k, fp8 174.0 k
// against 171.1 k -- 4 for every stored type; no instance of either depth spills (256 VGPRs at the most: bf16, D 32, S 4).
constexpr int kPipeNarrow = 4;
#ifndef DRS_DIN_NARROW_PIPE
#define DRS_DIN_NARROW_PIPE 0   // (a lab build's -DDRS_DIN_NARROW_PIPE=2|4 forces one depth for every launch: the A/B of the record)
#endif
int narrow_depth(int /*dtype*/, int /*S*/) { return DRS_DIN_NARROW_PIPE ? DRS_DIN_NARROW_PIPE : kPipeNarrow; }

size_t narrow_lds(int T, int S, int dtype) { return din_pipe_lds(T, S) + (dtype == DRS_TABLE_FP8_E4M3 ? (size_t)T * 4 : 0); }

template <class F>
void with_policy(int dtype, F&& f) {
  if (dtype == DRS_TABLE_FP16) f(F16{});
  else if (dtype == DRS_TABLE_BF16) f(BF16{});
  else f(F8{});
}

}  // namespace

// The narrow pipe form takes a launch set of a DIN engine whose arena is fp16, bf16 or fp8 where din_pipe_kernel would take
// its fp32 twin: D 32 or 64, hidden width 1, every bag of one fixed length <= 3, "din_pipe" 1, the staged indices inside 48 KB.
bool din_narrow_applicable(const SlsArgs& a, int32_t h, int dtype, const Tune& tune) {
  if (dtype != DRS_TABLE_FP16 && dtype != DRS_TABLE_BF16 && dtype != DRS_TABLE_FP8_E4M3) return false;
  if (!tune.din_pipe || h != 1 || (a.D != 32 && a.D != 64)) return false;
  const FusedShape f = fused_shape(a, tune);
  return f.C == 3 && narrow_lds(a.T, f.S, dtype) <= 48 * 1024;
}

hipError_t launch_din_narrow(const SlsArgs& a_in, int dtype, const float* packed, float* R, int64_t ldr, const Tune& tune,
                             hipStream_t s, hipEvent_t stop) {
  SlsArgs a = a_in;
  a.nt = tune.din_nt;
  const int64_t n_smp = a.q.cum[a.q.n_q];
  if (n_smp <= 0) return hipSuccess;
  if (!din_narrow_applicable(a, 1, dtype, tune)) return hipErrorInvalidValue;
  const int64_t stride = din_unit_stride(a.D, 1);
  const FusedShape f = fused_shape(a, tune);
  const unsigned grid = (unsigned)din_fused_grid(a, tune);
  const int depth = narrow_depth(dtype, f.S);
  const size_t lds = narrow_lds(a.T, f.S, dtype);
  with_policy(dtype, [&](auto e) {
    using E = decltype(e);
    log_launch(tune.log, "din_pipe_narrow_kernel<%d,S%d,P%d%s,%s>[%u wg]", a.D == 32 ? 8 : 16, f.S, depth, a.nt ? ",nt" : "", E::tag, grid);
    with_int<8, 16>(a.D / 4, [&](auto G) { with_int<4, 2, 1>(f.S, [&](auto S) { with_int<2, 4>(depth, [&](auto P) {
      with_int<0, 1>(a.nt != 0, [&](auto NT) {
        launch_kb(din_pipe_narrow_kernel<G, S, kWaves, P, NT != 0, E>, dim3(grid), dim3(64 * kWaves), lds, s, stop,
                  a, packed, stride, tune.zero, R, ldr);
      });
    }); }); });
  });
  return hipGetLastError();
}

}  // namespace drs
