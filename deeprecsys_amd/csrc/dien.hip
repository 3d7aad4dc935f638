// DIEN (models/dien.py:308-432): two caffe2 rnn_cell.BasicRNN layers over the behaviour
// embeddings of a query.  One wave per sample, lane j = hidden unit j (H <= 64): the lane keeps
// row j of the four weight matrices in registers for all U steps (D + 3 H values), the step's
// input and the two states are broadcast through 3 x 64 floats of LDS per wave (ds_read_b128 of one
// address for all lanes; no VALU cross-lane traffic), every product-sum is the oracle's k-ordered
// fmaf chain with the bias added after it, and the next step's input row is fetched while the
// current step computes.  VALU work: the recurrence is U = 40 dependent steps of 64-wide
// mat-vecs per sample -- an MFMA form would tile 16 samples x 16 hidden units per wave and
// exchange states through LDS with a barrier per step; at 1.1 MFLOP per sample the VALU form
// already runs a launch set in tens of microseconds, next to ~10 us of gather.
// Packed weights (dien_pack_kernel), transposed so that lane j's loads coalesce:
//   [ i2h_0^T : D x H | gates_0^T : H x H | i2h_1^T : H x H | gates_1^T : H x H | 4 biases : 4 x H ]
#include <string.h>

#include "drs_internal.h"
#include "launch_host.h"
#include "mlp_dev.h"
#include "owner_dev.h"
#include "rnn_dev.h"

namespace drs {
namespace {

__global__ __launch_bounds__(256) void dien_pack_kernel(const float* const* __restrict__ w, float* __restrict__ packed,
                                                        int D, int H) {
  // w: {i2h_w, i2h_b, gates_w, gates_b} of layer 1, then of layer 2 (row-major [out, in])
  const int K[4] = {D, H, H, H};
  const int src[4] = {0, 2, 4, 6};
  int64_t off = 0;
  for (int m = 0; m < 4; ++m) {
    const float* W = w[src[m]];
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < (int64_t)K[m] * H; i += (int64_t)gridDim.x * blockDim.x) {
      const int k = (int)(i / H), j = (int)(i - (int64_t)k * H);
      packed[off + i] = W[(int64_t)j * K[m] + k];
    }
    off += (int64_t)K[m] * H;
  }
  const int bsrc[4] = {1, 3, 5, 7};
  for (int m = 0; m < 4; ++m)
    for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < H; j += gridDim.x * blockDim.x) packed[off + (int64_t)m * H + j] = w[bsrc[m]][j];
}

template <int K>
__device__ __forceinline__ float chain_lds(const float* __restrict__ sv, const float (&w)[K]) {
  float acc = 0.f;
#pragma unroll
  for (int k4 = 0; k4 < K / 4; ++k4) {
    const float4 v = *reinterpret_cast<const float4*>(sv + 4 * k4);
    acc = fmaf(v.x, w[4 * k4 + 0], acc); acc = fmaf(v.y, w[4 * k4 + 1], acc);
    acc = fmaf(v.z, w[4 * k4 + 2], acc); acc = fmaf(v.w, w[4 * k4 + 3], acc);
  }
  return acc;
}

template <int D, int H>
__global__ __launch_bounds__(256) void dien_rnn_kernel(const float* __restrict__ T, int64_t ldt, QTable q, int Tn,
                                                       const float* __restrict__ packed, float* __restrict__ R,
                                                       int64_t ldr) {
  static_assert(D % 4 == 0 && H % 4 == 0 && D <= 64 && H <= 64, "lane j = hidden unit j");
  __shared__ __attribute__((aligned(16))) float sx[4][64], sh0[4][64], sh1[4][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int smp = blockIdx.x * 4 + wave;
  if (smp >= q.cum[q.n_q]) return;                       // (no workgroup barrier below)
  DRS_QOWNER_OF(q, smp, b, bs, v0)
  const int U = Tn - 3;
  const int j = min(lane, H - 1);
  float wi0[D], wg0[H], wi1[H], wg1[H];
  const float* p = packed;
#pragma unroll
  for (int k = 0; k < D; ++k) wi0[k] = p[k * H + j];
  p += D * H;
#pragma unroll
  for (int k = 0; k < H; ++k) wg0[k] = p[k * H + j];
  p += H * H;
#pragma unroll
  for (int k = 0; k < H; ++k) wi1[k] = p[k * H + j];
  p += H * H;
#pragma unroll
  for (int k = 0; k < H; ++k) wg1[k] = p[k * H + j];
  p += H * H;
  const float bi0 = p[j], bg0 = p[H + j], bi1 = p[2 * H + j], bg1 = p[3 * H + j];

  // step t of "sample" b reads embedding n % U of sample n / U, n = t * bs + b (the reference's
  // Reshape of [bs, U*D] to [U, bs, D], models/dien.py:316-320)
  auto x_of = [&](int t) {
    const int n = t * bs + b;
    const int src = n / U, unit = n - src * U;
    return T[(int64_t)(v0 + src) * ldt + (int64_t)(1 + unit) * D + min(lane, D - 1)];
  };
  float* mx = sx[wave];
  float* m0 = sh0[wave];
  float* m1 = sh1[wave];
  m0[lane] = 0.f;                                        // initial_h = 0 (:498-499)
  m1[lane] = 0.f;
  float xv = x_of(0), h1 = 0.f;
  // every weight load has landed before the loop: inside it only the input prefetch is in flight,
  // and nothing waits for it before the next step's LDS write (with the weights still pending at
  // the loop header the waitcnt pass put a vmcnt(0) right behind the prefetch: 3 800 cycles a step)
  __builtin_amdgcn_s_waitcnt(0);
  for (int t = 0; t < U; ++t) {
    mx[lane] = xv;
    __builtin_amdgcn_wave_barrier();
    xv = x_of(min(t + 1, U - 1));                       // (unconditional: one more read of the last row)
    // layer 1: Tanh(Sum(FC(h_prev, gates_t), FC(x_t, i2h)))
    const float a0 = chain_lds<D>(mx, wi0) + bi0;
    const float g0 = chain_lds<H>(m0, wg0) + bg0;
    const float h0 = tanh_rnn(g0 + a0);
    __builtin_amdgcn_wave_barrier();
    m0[lane] = h0;
    __builtin_amdgcn_wave_barrier();
    // layer 2 on layer 1's new state
    const float a1 = chain_lds<H>(m0, wi1) + bi1;
    const float g1 = chain_lds<H>(m1, wg1) + bg1;
    h1 = tanh_rnn(g1 + a1);
    __builtin_amdgcn_wave_barrier();
    m1[lane] = h1;
    __builtin_amdgcn_wave_barrier();
  }
  // top MLP input row: [ last state | user profile | candidate ad | context ] (:411-421)
  float* out = R + (int64_t)(v0 + b) * ldr;
  const float* e = T + (int64_t)(v0 + b) * ldt;
  if (lane < H) out[lane] = h1;
  if (lane < D) {
    out[H + lane] = e[lane];
    out[H + D + lane] = e[(int64_t)(Tn - 2) * D + lane];
    out[H + 2 * D + lane] = e[(int64_t)(Tn - 1) * D + lane];
  }
}

// The MFMA form (H a multiple of 16).  A workgroup of H / 16 waves serves 16 samples; wave w owns
// hidden units [16 w, 16 w + 16) of BOTH layers.  Per step and layer the pre-activations are two
// v_mfma_f32_16x16x4_f32 chains (bit-for-bit k-ordered fp32 fma chains, as in mlp.hip): A = the
// wave's 16 weight rows (registers for the whole launch: (D + 3 H) / 4 VGPRs), B = the step's input
// [k][sample] -- the embeddings through LDS (one coalesced fetch of the 16 rows per workgroup and step,
// four steps ahead: round 5), the states from LDS ([hidden][sample], double-buffered so ONE workgroup
// barrier per step orders everything) -- D[m = hidden 4 g + q][n = sample r].  Same bits as dien_rnn_kernel.
// Cost: (D + 3 H) / 4 = 56 MFMAs of 32 cycles per wave and step at D 32 / H 64, 16 samples at a
// time, against 2 x 112 dependent VALU fmas per SAMPLE in the one-wave-per-sample form.
// Measured on dien.json's shape (40 steps, 2048 samples per launch = 128 workgroups): every wave
// running both layers 76 us per launch (the VALU form: 112 us); per step 1.9 us = 0.8 MFMA + 0.2 tanh
// + 0.2 barrier + 0.7 LDS / issue latency that one wave per SIMD cannot hide.  One wave set per
// layer (SPLIT, the default: 24 / 32 MFMAs per wave and step, two waves per SIMD): 66 us.  The engine
// also lets the launches of consecutive sets overlap on separate streams (each covers half the
// chip): 51 k -> 127 k (both layers per wave) -> 141 k queries/s (SPLIT).
typedef float f32x4_ __attribute__((ext_vector_type(4)));
struct DienW { const float* w[8]; };   // {i2h_w, i2h_b, gates_t_w, gates_t_b} x 2 layers, row-major [out, in]

template <int D, int H, int SPLIT>
__global__ __launch_bounds__(64 * (SPLIT ? 2 : 1) * (H / 16)) void dien_rnn_mfma_kernel(const float* __restrict__ T, int64_t ldt,
                                                                                     QTable q, int Tn, DienW W,
                                                                                     float* __restrict__ R, int64_t ldr,
                                                                                     DienTop top, Done done) {
  static_assert(D % 4 == 0 && H % 16 == 0 && H <= 64, "16 hidden units per wave");
  // SPLIT = 1: 2 x H / 16 waves; the first H / 16 run layer 1 (of step t + 1), the others layer 2
  // (of step t) -- the two layers of an iteration are independent, so the per-step critical path of
  // a wave is 24 or 32 MFMAs instead of 56, at two waves per SIMD.  SPLIT = 0: every wave runs both
  // layers of its 16 hidden units (four interleaved chains).  Same bits.
  // (Two independent 16-sample groups per workgroup, the other way to put two waves on a SIMD, was
  // measured as well: 130 us on half as many CUs instead of 76 us, no gain in queries/s.)
  constexpr int NW = H / 16, NT = 64 * (SPLIT ? 2 : 1) * NW;
  __shared__ float s0[2][H][16], s1[2][H][16];
  // x_t of the 16 samples, [sample][k] with rows 4 floats apart from a multiple of 64: the B operand read
  // sx[.][r][4 s + g] touches 64 different banks, the loaders' 16-byte writes are aligned
  constexpr int XLD = D + 4;
  __shared__ __attribute__((aligned(16))) float sx[2][16][XLD];
  extern __shared__ __attribute__((aligned(16))) float dien_top_lds[];   // fused top MLP: 2 x [kmax][16] (none otherwise)
  const int lane = threadIdx.x & 63, wave = (threadIdx.x >> 6) % NW, role = (threadIdx.x >> 6) / NW;
  const bool do1 = !SPLIT || role == 0, do2 = !SPLIT || role == 1;   // (wave-uniform)
  const int r = lane & 15, g = lane >> 4;
  const int n_smp = q.cum[q.n_q];
  const int smp_base = (int)blockIdx.x * 16;
  const int smp = min(smp_base + r, n_smp - 1);
  const bool live = smp_base + r < n_smp;
  DRS_QOWNER_OF(q, smp, b, bs, v0)
  const int U = Tn - 3;
  // A operands: lane (r, g) holds W[16 w + r][4 s + g] of every MFMA step s -- the i2h and gates_t
  // rows of the layer(s) this wave runs
  const int row = 16 * wave + r;
  float wia[SPLIT ? (D > H ? D : H) / 4 : D / 4], wga[H / 4];      // layer 1 (or, SPLIT role 1, layer 2)
  float wib[SPLIT ? 1 : H / 4], wgb[SPLIT ? 1 : H / 4];            // layer 2 when one wave runs both
  float bia[4], bga[4], bib[4], bgb[4];
  const int la = (SPLIT && role == 1) ? 1 : 0;                       // layer held in the "a" set
  const int Ka = la == 0 ? D : H;
#pragma unroll
  for (int s = 0; s < (int)(sizeof(wia) / sizeof(float)); ++s) wia[s] = 4 * s < Ka ? W.w[4 * la + 0][row * Ka + 4 * s + g] : 0.f;
#pragma unroll
  for (int s = 0; s < H / 4; ++s) wga[s] = W.w[4 * la + 2][row * H + 4 * s + g];
  if (!SPLIT) {
#pragma unroll
    for (int s = 0; s < H / 4; ++s) {
      wib[s] = W.w[4][row * H + 4 * s + g];
      wgb[s] = W.w[6][row * H + 4 * s + g];
    }
  }
  // biases of the 4 output rows this lane holds: hidden 16 w + 4 g + qd
#pragma unroll
  for (int qd = 0; qd < 4; ++qd) {
    const int hid = 16 * wave + 4 * g + qd;
    bia[qd] = W.w[4 * la + 1][hid]; bga[qd] = W.w[4 * la + 3][hid];
    bib[qd] = SPLIT ? 0.f : W.w[5][hid]; bgb[qd] = SPLIT ? 0.f : W.w[7][hid];
  }
  for (int i = threadIdx.x; i < 2 * H * 16; i += NT) {         // initial_h = 0 (models/dien.py:498-499)
    (&s0[0][0][0])[i] = 0.f;
    (&s1[0][0][0])[i] = 0.f;
  }
  // B operand of the input product: x_t[sample r][k = 4 s + g]; step t of "sample" b is embedding
  // n % U of sample n / U, n = t * bs + b (the reference's Reshape, models/dien.py:316-320).
  // Round 5: the 16 rows of a step (D floats each, contiguous in the gather's buffer) are fetched ONCE per
  // workgroup, 16 bytes per lane (loader lane f takes piece f % (D/4) of sample f / (D/4): a row per 128-byte
  // line), NB steps ahead into a register ring, and handed to the layer-1 waves through sx -- until then every
  // layer-1 wave fetched the operand itself, a dword per lane and MFMA step: 8 requests of 16 lines each per wave
  // and step, 32 per workgroup, and the texture path of a CU with two workgroups was the bound (the recurrence
  // with the fetch compiled out: 179 k -> 203 k queries/s; with a second workgroup on the CU a launch took twice
  // as long).  (Rounds 3-4 on the wait counters across the loop's back edge: docs/DESIGN_rounds_1-4.md.)
  constexpr int NB = 4;
  constexpr int NF = 16 * D / 4;                                  // float4 pieces of a step
  constexpr int NLD = 64 * NW;                                    // loader lanes: the waves that run layer 1
  constexpr int NL = (NF + NLD - 1) / NLD;
  f32x4_ xr[NB][NL];
  const float* xsrc[NL];                                          // this loader lane's sample: row 0 of its query ...
  int xb_[NL], xbs[NL];                                           // ... its number in the query, the query's size
  if (do1) {
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
    if (!do1) return;
    const int tt = min(t, U - 1);
#pragma unroll
    for (int i = 0; i < NL; ++i) {
      const int n = tt * xbs[i] + xb_[i];
      const int src = n / U, unit = n - src * U;
      xq[i] = *reinterpret_cast<const f32x4_*>(xsrc[i] + (int64_t)src * ldt + (int64_t)unit * D);
    }
  };
  auto stash_x = [&](int buf, const f32x4_ (&xq)[NL]) {            // ring slot -> sx[buf]
    if (!do1) return;
#pragma unroll
    for (int i = 0; i < NL; ++i) {
      const int f = wave * 64 + lane + i * NLD;
      if (f < NF) {
        const int ls = f / (D / 4), piece = f - ls * (D / 4);
        *reinterpret_cast<f32x4_*>(&sx[buf][ls][4 * piece]) = xq[i];
      }
    }
  };
#pragma unroll
  for (int j = 0; j < NB; ++j) fetch_x(j, xr[j]);              // slot j % NB holds x_j
  stash_x(0, xr[0]);
  stash_x(1, xr[1 % NB]);
  fetch_x(NB, xr[0]);
  fetch_x(NB + 1, xr[1 % NB]);
  __syncthreads();
  // Layer 2 runs one step behind layer 1: an iteration holds layer 2 of step t and layer 1 of step
  // t + 1, which do not depend on each other, and ONE barrier per iteration orders the
  // double-buffered state exchange.
  //   s0[t & 1] = layer-1 state after step t,  s1[t & 1] = layer-2 state after step t
  auto layer1 = [&](int rd, int wr, int xbuf) {   // x_t in sx[xbuf], state s0[rd] -> s0[wr]
    f32x4_ aa = {0.f, 0.f, 0.f, 0.f}, ag = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < H / 4; ++s) {
      ag = __builtin_amdgcn_mfma_f32_16x16x4f32(wga[s], s0[rd][4 * s + g][r], ag, 0, 0, 0);
      if (s < D / 4) aa = __builtin_amdgcn_mfma_f32_16x16x4f32(wia[s], sx[xbuf][r][4 * s + g], aa, 0, 0, 0);
    }
#pragma unroll
    for (int s = H / 4; s < D / 4; ++s) aa = __builtin_amdgcn_mfma_f32_16x16x4f32(wia[s], sx[xbuf][r][4 * s + g], aa, 0, 0, 0);
#pragma unroll
    for (int qd = 0; qd < 4; ++qd)
      s0[wr][16 * wave + 4 * g + qd][r] = tanh_rnn((ag[qd] + bga[qd]) + (aa[qd] + bia[qd]));
  };
  f32x4_ h1v = {0.f, 0.f, 0.f, 0.f};
  if (do1) layer1(1, 0, 0);         // step 0 of layer 1: its previous state is the zero buffer s0[1]
  __syncthreads();
  for (int t0 = 0; t0 < U; t0 += NB) {
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      const int t = t0 + j;
      if (t >= U) break;                                 // (uniform)
      const int cur = t & 1, prv = cur ^ 1;
      f32x4_ (&xn)[NL] = xr[(j + 2) % NB];               // x_{t+2} (t0 is a multiple of NB): into sx[t & 1], whose x_t
                                                         // was read an iteration ago; x_{t+1} sits in sx[prv]
      // layer 2, step t: input = layer-1 state of step t (s0[cur]), previous own state s1[prv];
      // layer 1, step t + 1: input x_{t+1}, previous state s0[cur]; writes s0[prv].  (After the last
      // step layer 1 computes one step too many into the unused buffer: cheaper than a divergent tail.)
      if (SPLIT) {
        if (role == 0) {
          layer1(cur, prv, prv);
          stash_x(cur, xn);
          fetch_x(t + 2 + NB, xn);
        } else {
          f32x4_ ba = {0.f, 0.f, 0.f, 0.f}, bg = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int s = 0; s < H / 4; ++s) {
            ba = __builtin_amdgcn_mfma_f32_16x16x4f32(wia[s], s0[cur][4 * s + g][r], ba, 0, 0, 0);
            bg = __builtin_amdgcn_mfma_f32_16x16x4f32(wga[s], s1[prv][4 * s + g][r], bg, 0, 0, 0);
          }
#pragma unroll
          for (int qd = 0; qd < 4; ++qd) {
            h1v[qd] = tanh_rnn((bg[qd] + bga[qd]) + (ba[qd] + bia[qd]));
            s1[cur][16 * wave + 4 * g + qd][r] = h1v[qd];
          }
        }
      } else {
        // one wave, four chains issued round-robin (independent MFMAs back to back)
        f32x4_ ba = {0.f, 0.f, 0.f, 0.f}, bg = {0.f, 0.f, 0.f, 0.f};
        f32x4_ aa = {0.f, 0.f, 0.f, 0.f}, ag = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < H / 4; ++s) {
          const float h0k = s0[cur][4 * s + g][r];
          ba = __builtin_amdgcn_mfma_f32_16x16x4f32(wib[s], h0k, ba, 0, 0, 0);
          bg = __builtin_amdgcn_mfma_f32_16x16x4f32(wgb[s], s1[prv][4 * s + g][r], bg, 0, 0, 0);
          ag = __builtin_amdgcn_mfma_f32_16x16x4f32(wga[s], h0k, ag, 0, 0, 0);
          if (s < D / 4) aa = __builtin_amdgcn_mfma_f32_16x16x4f32(wia[s], sx[prv][r][4 * s + g], aa, 0, 0, 0);
        }
#pragma unroll
        for (int s = H / 4; s < D / 4; ++s) aa = __builtin_amdgcn_mfma_f32_16x16x4f32(wia[s], sx[prv][r][4 * s + g], aa, 0, 0, 0);
        stash_x(cur, xn);
        fetch_x(t + 2 + NB, xn);
#pragma unroll
        for (int qd = 0; qd < 4; ++qd) {
          h1v[qd] = tanh_rnn((bg[qd] + bgb[qd]) + (ba[qd] + bib[qd]));
          s1[cur][16 * wave + 4 * g + qd][r] = h1v[qd];
          s0[prv][16 * wave + 4 * g + qd][r] = tanh_rnn((ag[qd] + bga[qd]) + (aa[qd] + bia[qd]));
        }
      }
      __syncthreads();
    }
  }
  // top MLP input rows: [ last state | user profile | candidate ad | context ] (:411-421)
  if (live && do2) {
    float* out = R + (int64_t)(v0 + b) * ldr;
#pragma unroll
    for (int qd = 0; qd < 4; ++qd) out[16 * wave + 4 * g + qd] = h1v[qd];
  }
  for (int i = threadIdx.x; i < 16 * 3 * D; i += NT) {
    const int smp_i = smp_base + i / (3 * D), c = i % (3 * D);
    if (smp_i >= n_smp) break;
    DRS_QOWNER_OF(q, smp_i, bi, bsi, vi)
    const int tab = c < D ? 0 : c < 2 * D ? Tn - 2 : Tn - 1;
    const float ev = T[(int64_t)(vi + bi) * ldt + (int64_t)tab * D + c % D];
    R[(int64_t)(vi + bi) * ldr + H + c] = ev;
    if (top.n > 0) dien_top_lds[(H + c) * 16 + i / (3 * D)] = ev;
  }
  if (top.n <= 0) return;                              // (uniform: a kernel argument)

  // ---- the top MLP of the workgroup's 16 samples, in the same launch (round 4) ----------------------------
  // Every CU holds two workgroups of this model at a time (the recurrence: 2 x 120 registers per SIMD; the
  // stream kernel that ran the top MLP: 256), so a set cost each CU t_rnn + t_top of workgroup time at two
  // in flight -- and the top launch, 19 us alone, took 60-110 us beside recurrences.  Here its three small
  // layers (160-200-80-2: 0.1 MFLOP per sample) follow the last step as MFMA chains of the same form:
  // A = 16 rows of W [N, K] (lane (r, g): W[16 t + r][4 s + g], every 64-k chunk of them requested up front),
  // B = the layer's input [k][sample] in LDS, D[m = unit 4 g + qd][n = sample r]; k ascending from a zero
  // accumulator (through the zero-padded end of the last 64-k chunk, like theirs), bias, activation: the bits of
  // the stream kernels' chains (mlp.hip).  Tiles of 16 units go
  // round the workgroup's waves; the last layer stores to the output buffer and the workgroup signs off the
  // launch set itself (signal_done).
  {
    constexpr int NWV = NT / 64;
    const int wv = threadIdx.x >> 6;
    float* in = dien_top_lds;
    float* nxt = dien_top_lds + top.kmax * 16;           // (kmax: a multiple of 64)
    const int lastb = (U - 1) & 1;
    for (int i = threadIdx.x; i < H * 16; i += NT) in[i] = (&s1[lastb][0][0])[i];
    // k beyond a layer's K up to the next multiple of 64 meets zero weights in the twin: the inputs there must
    // be finite -- zeros
    for (int i = (H + 3 * D) * 16 + threadIdx.x; i < ((top.K[0] + 63) & ~63) * 16; i += NT) in[i] = 0.f;
    __syncthreads();
    for (int l = 0; l < top.n; ++l) {
      const int K = top.K[l], N = top.N[l], nch = (K + 63) >> 6;
      const bool fin = l + 1 == top.n;
      if (!fin)
        for (int i = N * 16 + threadIdx.x; i < ((N + 63) & ~63) * 16; i += NT) nxt[i] = 0.f;
      for (int t = wv; 16 * t < N; t += NWV) {
        // A operands from the layer's PACKED twin (mlp.hip pack_stream_kernel: per 128 units and 64 k a block of
        // 8192 floats, 1024 per 16 units, float4 q of lane (r, g) = W[unit r][64 c + 16 q + 4 j + g], j = 0..3 --
        // element j is the operand of MFMA step 16 c + 4 q + j): one coalesced 1-KB request per four steps.
        // (The first version read W [N, K] itself, a dword per lane and step: 16 cache lines per request, and
        // the launch took 100 us alone against 69 + 22 for the two it replaced.)
        const float* wp = top.Wp[l] + ((size_t)(t >> 3) * nch * 8192 + (t & 7) * 1024 + lane * 4);
        f32x4_ wq[4][4];
        float bv[4];
#pragma unroll
        for (int c = 0; c < 4; ++c)
          if (c < nch) {                                  // (uniform)
#pragma unroll
            for (int qq = 0; qq < 4; ++qq) wq[c][qq] = *reinterpret_cast<const f32x4_*>(wp + c * 8192 + qq * 256);
          }
#pragma unroll
        for (int qd = 0; qd < 4; ++qd) bv[qd] = top.b[l][min(16 * t + 4 * g + qd, N - 1)];
        f32x4_ acc = {0.f, 0.f, 0.f, 0.f};
        __builtin_amdgcn_sched_barrier(0);               // (all of the tile's requests before its first MFMA)
#pragma unroll
        for (int c = 0; c < 4; ++c)
          if (c < nch) {
#pragma unroll
            for (int qq = 0; qq < 4; ++qq) {
#pragma unroll
              for (int j = 0; j < 4; ++j)
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(wq[c][qq][j], in[(64 * c + 16 * qq + 4 * j + g) * 16 + r], acc, 0, 0, 0);
              __builtin_amdgcn_sched_barrier(0);         // (keeps the LDS operands next to their MFMAs)
            }
          }
#pragma unroll
        for (int qd = 0; qd < 4; ++qd) {
          const int unit = 16 * t + 4 * g + qd;
          if (unit < N) {
            const float v = act_apply(acc[qd] + bv[qd], top.act[l]);
            if (!fin) nxt[unit * 16 + r] = v;
            else if (live) {
              float* dst = top.out + (int64_t)(v0 + b) * top.ldo + unit;
              if (top.sc1) __hip_atomic_store(dst, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
              else *dst = v;
            }
          }
        }
      }
      __syncthreads();
      float* sw = in; in = nxt; nxt = sw;
    }
  }
  signal_done(done, gridDim.x, dien_top_lds);
}

}  // namespace

// Shapes the recurrent kernel is instantiated for.
bool dien_applicable(int32_t D, int32_t H) { return (D == 16 || D == 32 || D == 64) && (H == 8 || H == 16 || H == 32 || H == 64); }
int64_t dien_packed_floats(int32_t D, int32_t H) { return (int64_t)D * H + 3ll * H * H + 4ll * H; }

hipError_t launch_dien_pack(const float* const* w, float* packed, int32_t D, int32_t H, hipStream_t s) {
  const int64_t blocks = ((int64_t)(D > H ? D : H) * H + 255) / 256;
  hipLaunchKernelGGL(dien_pack_kernel, dim3((unsigned)(blocks < 1024 ? blocks : 1024)), dim3(256), 0, s, w, packed, D, H);
  return hipGetLastError();
}

// The top MLP rides in the recurrence's launch when its layers fit the in-kernel form: at most 4 of them, every
// input width a multiple of 4 (whole MFMA steps) and <= 256 (a tile's A operands live in 64 registers), the two
// activation buffers inside the default 64 KB of LDS next to the state buffers.
bool dien_top_fusable(int32_t n_layers, const int32_t* widths, int32_t H) {
  if (n_layers < 1 || n_layers > 4 || H % 16 != 0) return false;
  for (int l = 0; l < n_layers; ++l)
    if (widths[l] <= 0 || widths[l] > 256 || (widths[l] & 3) || widths[l + 1] <= 0) return false;
  return sizeof(float) * (2 * 16 * (size_t)dien_top_kmax(n_layers, widths) + 4 * 16 * (size_t)H) <= 60 * 1024;
}
// rows of one LDS activation buffer: the widest layer input, up to the end of its last 64-k chunk
int32_t dien_top_kmax(int32_t n_layers, const int32_t* widths) {
  int kmax = 0;
  for (int l = 0; l < n_layers; ++l) kmax = widths[l] > kmax ? widths[l] : kmax;
  return (kmax + 63) & ~63;
}

hipError_t launch_dien_rnn(const float* T, int64_t ldt, const QTable& q, int32_t Tn, int32_t D, int32_t H,
                           const float* packed, const float* const* w, int mfma, float* R, int64_t ldr,
                           hipStream_t s, const DienTop* top, const Done* done) {
  const int64_t n = q.cum[q.n_q];
  if (n <= 0) return hipSuccess;
  // shapes without an instance of their own (and "dien_mfma" 3, which the parity tests use): the any-shape form
  if (!dien_applicable(D, H) || mfma == 3)
    return top && top->n > 0 ? hipErrorInvalidValue : launch_dien_rnn_any(T, ldt, q, Tn, D, H, packed, R, ldr, s);
  if (top && top->n > 0 && !(mfma && H % 16 == 0)) return hipErrorInvalidValue;   // (the engine asks dien_top_fusable first)
  // (from here on D and H are values dien_applicable passed: every with_int below finds its instance)
  if (mfma && H % 16 == 0) {
    DienW W;
    for (int i = 0; i < 8; ++i) W.w[i] = w[i];
    DienTop tp;
    memset(&tp, 0, sizeof tp);
    if (top) tp = *top;
    Done dn;
    memset(&dn, 0, sizeof dn);
    if (done && tp.n > 0) dn = *done;
    const unsigned g16 = (unsigned)((n + 15) / 16);
    const size_t lds = tp.n > 0 ? sizeof(float) * 2 * 16 * (size_t)tp.kmax : 0;
    with_int<16, 32, 64>(D, [&](auto D_) { with_int<16, 32, 64>(H, [&](auto H_) { with_int<0, 1>(mfma == 2, [&](auto SPLIT) {
      launch_kb(dien_rnn_mfma_kernel<D_, H_, SPLIT>, dim3(g16), dim3(64 * (SPLIT ? 2 : 1) * (H_ / 16)), lds, s, nullptr,
                T, ldt, q, Tn, W, R, ldr, tp, dn);
    }); }); });
    return hipGetLastError();
  }
  const unsigned grid = (unsigned)((n + 3) / 4);
  with_int<16, 32, 64>(D, [&](auto D_) { with_int<8, 16, 32, 64>(H, [&](auto H_) {
    launch_kb(dien_rnn_kernel<D_, H_>, dim3(grid), dim3(256), 0, s, nullptr, T, ldt, q, Tn, packed, R, ldr);
  }); });
  return hipGetLastError();
}

}  // namespace drs
