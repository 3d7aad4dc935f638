// DIEN's recurrence on the bf16 matrix cores ("dien_bf16" 1): dien.hip's dien_rnn_mfma_kernel with every product of
// the two BasicRNN layers on v_mfma_f32_16x16x32_bf16 -- 32 k per instruction, so a layer's step is a chain of
// ceil((D + H) / 32) or 2 H / 32 instructions (3 and 4 at D 32 / H 64) where the fp32 form issues (D + H) / 4 and H / 2.
//
// The arithmetic contract (docs/OPTIONS.md), for both layers and every step:
//   h = tanh_rnn((Sum_k bf16(W_i2h[j][k]) bf16(in[k]) + Sum_k bf16(W_gates[j][k]) bf16(h_prev[k])) + (b_i2h[j] + b_gates[j]))
// exact products, ONE fp32 accumulation over both k ranges (the instruction's order; input range first, from a zero
// accumulator), fp32 biases added to each other and then to the sum, rnn_dev.h's tanh.  A state stays fp32 for the
// result -- the last layer-2 state goes to R as computed -- and is rounded to bf16 (nearest even, NaN stays NaN:
// v_cvt_pk_bf16_f32) only where it becomes an operand of a later product; so are the embeddings.  The top MLP is not
// part of this launch: it runs over R in fp32 as under "dien_fuse_top" 0.
//
// Work split: dien_rnn_mfma_kernel's SPLIT form.  A workgroup of 2 H / 16 waves serves 16 samples; wave w of the first
// set owns hidden units [16 w, 16 w + 16) of layer 1, wave w of the second set the same units of layer 2, which runs one
// step behind; D[m = hidden 4 g + q][n = sample r].  (With 3-4 MFMAs to a chain a step is the 4 tanh per lane and the
// LDS round trip, not the matrix cores: two wave sets let one layer's tanh run under the other's operand reads.  One
// set running both layers was not measured: profiles/r38_dien_bf16.md.)
// A operands: the wave's 16 weight rows, read once from the fp32 matrices and packed to bf16 in registers -- lane (r, g)
// holds k = 32 c + 8 g .. + 7 of row 16 w + r for every chunk c: (D + H) / 8 or 2 H / 8 VGPRs; no weight twin.
// B operands: ONE LDS row per sample and parity, Z[2][16][ x (D) | h0 (H) | h1 (H) | pad 8 ] in bf16, k contiguous, so a
// lane's 8 k of a chunk are one ds_read_b128.  A row is (D + 2 H) / 8 + 1 16-byte groups long -- an odd number: the 16
// samples of a read phase start in 16 different groups of the 16 that make up the 64 banks.  In iteration t row t & 1 holds
// x_{t+1}, h0_t and h1_{t-1}: layer 1 of step t + 1 is the k range [0, D + H), layer 2 of step t the range [D, D + 2 H).
// Both write their tanh to the OTHER row (4 hidden units of a sample: one 8-byte store of packed bf16), the loaders put
// x_{t+2} there, and ONE workgroup barrier per step orders everything.
// K padding: D + H = 48 or 80 leaves half of layer 1's last chunk beyond K; those lanes hold zero weights AND take a
// zero operand by value -- what lies there is h1, and a NaN in it must not reach layer 1 through 0 x NaN.
#include <string.h>

#include "drs_internal.h"
#include "launch_host.h"
#include "owner_dev.h"
#include "rnn_dev.h"

namespace drs {
namespace {

typedef float f32x4_ __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
struct DienW { const float* w[8]; };   // {i2h_w, i2h_b, gates_t_w, gates_t_b} x 2 layers, row-major [out, in]

// fp32 -> bf16, nearest even, NaN stays NaN: the plain cast (v_cvt_pk_bf16_f32)
__device__ __forceinline__ bf16x4 to_bf16x4(const f32x4_ v) {
  bf16x4 o;
  o[0] = (__bf16)v[0]; o[1] = (__bf16)v[1]; o[2] = (__bf16)v[2]; o[3] = (__bf16)v[3];
  return o;
}

// 8 consecutive weights of a row as one A operand; in [k0, k0 + 8): the first matrix below K0, the second up to K0 + K1,
// zeros beyond (k0, K0, K1: multiples of 8 -- the 8 never straddle)
__device__ __forceinline__ bf16x8 weights8(const float* __restrict__ Wa, int K0, const float* __restrict__ Wb, int K1, int row, int k0) {
  bf16x8 o;
  const bool first = k0 < K0, any = k0 < K0 + K1;
  const float* p = first ? Wa + (int64_t)row * K0 + k0 : Wb + (int64_t)row * K1 + (any ? k0 - K0 : 0);
#pragma unroll
  for (int e = 0; e < 8; ++e) o[e] = (__bf16)(any ? p[e] : 0.f);
  return o;
}

template <int D, int H>
__global__ __launch_bounds__(128 * (H / 16)) void dien_rnn_bf16_kernel(const float* __restrict__ T, int64_t ldt, QTable q, int Tn,
                                                                       DienW W, float* __restrict__ R, int64_t ldr) {
  static_assert(D % 16 == 0 && H % 16 == 0 && D <= 64 && H <= 64, "16 hidden units per wave, 8 k per lane and chunk");
  constexpr int NW = H / 16, NT = 128 * NW;
  constexpr int K1 = D + H, K2 = 2 * H;                 // layer 1: [x | h0]; layer 2: [h0 | h1]
  constexpr int C1 = (K1 + 31) / 32, C2 = K2 / 32;      // MFMAs per step
  constexpr int CM = C1 > C2 ? C1 : C2;
  constexpr int ZLD = D + 2 * H + 8;                    // bf16 per row: an odd number of 16-byte groups
  __shared__ __attribute__((aligned(16))) __bf16 Z[2][16][ZLD];
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));   // (scalar: `role` indexes the kernel's arguments)
  const int wave = wv % NW, role = wv / NW;
  const int r = lane & 15, g = lane >> 4;
  const int n_smp = q.cum[q.n_q];
  const int smp_base = (int)blockIdx.x * 16;
  const int smp = min(smp_base + r, n_smp - 1);
  const bool live = smp_base + r < n_smp;
  DRS_QOWNER_OF(q, smp, b, bs, v0)
  const int U = Tn - 3;
  // A operands and the 4 output rows' bias sums (hidden 16 w + 4 g + qd) of the layer this wave runs
  const int row = 16 * wave + r;
  bf16x8 wa[CM];
#pragma unroll
  for (int c = 0; c < CM; ++c) {
    if (role == 0) wa[c] = weights8(W.w[0], D, W.w[2], H, row, c < C1 ? 32 * c + 8 * g : K1);
    else wa[c] = weights8(W.w[4], H, W.w[6], H, row, c < C2 ? 32 * c + 8 * g : K2);
  }
  float bsum[4];
#pragma unroll
  for (int qd = 0; qd < 4; ++qd) {
    const int hid = 16 * wave + 4 * g + qd;
    bsum[qd] = W.w[4 * role + 1][hid] + W.w[4 * role + 3][hid];
  }
  for (int i = threadIdx.x; i < 2 * 16 * ZLD / 2; i += NT) reinterpret_cast<uint32_t*>(&Z[0][0][0])[i] = 0u;   // initial_h = 0; pads
  // The embeddings, as in dien_rnn_mfma_kernel: step t of "sample" b is embedding n % U of sample n / U, n = t * bs + b
  // (the reference's Reshape, models/dien.py:316-320); the 16 rows of a step are fetched once per workgroup by the
  // layer-1 waves, 16 bytes per loader lane (lane f: piece f % (D / 4) of sample f / (D / 4)), NB steps ahead into a
  // register ring, and converted to bf16 on their way into Z.
  constexpr int NB = 4;
  constexpr int NF = 16 * D / 4;
  constexpr int NLD = 64 * NW;
  constexpr int NL = (NF + NLD - 1) / NLD;
  f32x4_ xr[NB][NL];
  const float* xsrc[NL];
  int xb_[NL], xbs[NL];
  if (role == 0) {
#pragma unroll
    for (int i = 0; i < NL; ++i) {
      const int f = min(wave * 64 + lane + i * NLD, NF - 1);
      const int ls = f / (D / 4), piece = f - ls * (D / 4);
      const int sm = min(smp_base + ls, n_smp - 1);
      DRS_QOWNER_OF(q, sm, bb, bsz, vv)
      xb_[i] = bb; xbs[i] = bsz;
      xsrc[i] = T + (int64_t)vv * ldt + D + 4 * piece;
    }
  }
  auto fetch_x = [&](int t, f32x4_ (&xq)[NL]) {
    if (role != 0) return;
    const int tt = min(t, U - 1);
#pragma unroll
    for (int i = 0; i < NL; ++i) {
      const int n = tt * xbs[i] + xb_[i];
      const int src = n / U, unit = n - src * U;
      xq[i] = *reinterpret_cast<const f32x4_*>(xsrc[i] + (int64_t)src * ldt + (int64_t)unit * D);
    }
  };
  auto stash_x = [&](int buf, const f32x4_ (&xq)[NL]) {            // ring slot -> Z[buf][.][0 .. D)
    if (role != 0) return;
#pragma unroll
    for (int i = 0; i < NL; ++i) {
      const int f = wave * 64 + lane + i * NLD;
      if (f < NF) {
        const int ls = f / (D / 4), piece = f - ls * (D / 4);
        *reinterpret_cast<bf16x4*>(&Z[buf][ls][4 * piece]) = to_bf16x4(xq[i]);
      }
    }
  };
  // one layer's step: the chain over NC chunks of row Z[rd][r] from column k0 on; the tanh of the wave's 16 units, fp32
  // in the return value, bf16 into Z[wr][r][dst + ...]
  auto step = [&](auto NC_, int KV, int rd, int wr, int k0, int dst) {
    constexpr int NC = decltype(NC_)::value;
    const __bf16* zr = &Z[rd][r][k0 + 8 * g];
    const bf16x8 zero8 = {};
    bf16x8 bv[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      bv[c] = *reinterpret_cast<const bf16x8*>(zr + 32 * c);
      if (32 * c + 32 > KV && 32 * c + 8 * g >= KV) bv[c] = zero8;   // k >= K: zero by value
    }
    f32x4_ acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < NC; ++c) acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wa[c], bv[c], acc, 0, 0, 0);
#pragma unroll
    for (int qd = 0; qd < 4; ++qd) acc[qd] = tanh_rnn(acc[qd] + bsum[qd]);
    *reinterpret_cast<bf16x4*>(&Z[wr][r][dst + 16 * wave + 4 * g]) = to_bf16x4(acc);
    return acc;
  };
  using IC1 = std::integral_constant<int, C1>;
  using IC2 = std::integral_constant<int, C2>;
#pragma unroll
  for (int j = 0; j < NB; ++j) fetch_x(j, xr[j]);              // slot j % NB holds x_j
  __syncthreads();                                             // (the zeros, before the first rows go in)
  stash_x(1, xr[0]);
  __syncthreads();
  // step 0 of layer 1: Z[1] holds x_0 and zero states; Z[0] gets h0_0 and x_1
  if (role == 0) step(IC1{}, K1, 1, 0, 0, D);
  stash_x(0, xr[1 % NB]);
  fetch_x(NB, xr[0]);
  fetch_x(NB + 1, xr[1 % NB]);
  __syncthreads();
  f32x4_ h1v = {0.f, 0.f, 0.f, 0.f};
  for (int t0 = 0; t0 < U; t0 += NB) {
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      const int t = t0 + j;
      if (t >= U) break;                                 // (uniform)
      const int cur = t & 1, nxt = cur ^ 1;
      f32x4_ (&xn)[NL] = xr[(j + 2) % NB];               // x_{t+2} (t0 is a multiple of NB)
      // Z[cur] = x_{t+1} | h0_t | h1_{t-1}.  Layer 1, step t + 1 -> h0_{t+1}; layer 2, step t -> h1_t; both into Z[nxt],
      // which nobody reads before the barrier.  (After the last step layer 1 computes one step too many into the unused
      // row: cheaper than a divergent tail.)
      if (role == 0) {
        step(IC1{}, K1, cur, nxt, 0, D);
        stash_x(nxt, xn);
        fetch_x(t + 2 + NB, xn);
      } else {
        h1v = step(IC2{}, K2, cur, nxt, D, D + H);
      }
      __syncthreads();
    }
  }
  // top MLP input rows: [ last state (fp32) | user profile | candidate ad | context ] (:411-421)
  if (live && role == 1) {
    float* out = R + (int64_t)(v0 + b) * ldr;
#pragma unroll
    for (int qd = 0; qd < 4; ++qd) out[16 * wave + 4 * g + qd] = h1v[qd];
  }
  for (int i = threadIdx.x; i < 16 * 3 * D; i += NT) {
    const int smp_i = smp_base + i / (3 * D), c = i % (3 * D);
    if (smp_i >= n_smp) break;
    DRS_QOWNER_OF(q, smp_i, bi, bsi, vi)
    const int tab = c < D ? 0 : c < 2 * D ? Tn - 2 : Tn - 1;
    R[(int64_t)(vi + bi) * ldr + H + c] = T[(int64_t)(vi + bi) * ldt + (int64_t)tab * D + c % D];
  }
}

}  // namespace

// Shapes dien_rnn_bf16_kernel is instantiated for: dien.hip's, with 16 hidden units to a wave
bool dien_bf16_applicable(int32_t D, int32_t H) { return dien_applicable(D, H) && H % 16 == 0; }

hipError_t launch_dien_rnn_bf16(const float* T, int64_t ldt, const QTable& q, int32_t Tn, int32_t D, int32_t H,
                                const float* const* w, float* R, int64_t ldr, hipStream_t s) {
  const int64_t n = q.cum[q.n_q];
  if (n <= 0) return hipSuccess;
  if (!dien_bf16_applicable(D, H)) return hipErrorInvalidValue;   // (the engine refuses "dien_bf16" 1 on such a model)
  DienW W;
  for (int i = 0; i < 8; ++i) W.w[i] = w[i];
  const unsigned g16 = (unsigned)((n + 15) / 16);
  with_int<16, 32, 64>(D, [&](auto D_) { with_int<16, 32, 64>(H, [&](auto H_) {
    launch_kb(dien_rnn_bf16_kernel<D_, H_>, dim3(g16), dim3(128 * (H_ / 16)), 0, s, nullptr, T, ldt, q, Tn, W, R, ldr);
  }); });
  return hipGetLastError();
}

}  // namespace drs
