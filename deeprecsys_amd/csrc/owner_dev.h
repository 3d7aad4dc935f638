// Device helper shared by the gather translation units (sls.hip, sls_wflat.hip, din.hip, dien.hip, din_any.hip): which query of a coalesced
// launch set owns valid-sample number `smp`.
#pragma once
#include <hip/hip_runtime.h>

#include "drs_internal.h"

namespace drs {
namespace {

// The select chain over queries 1 .. n_q - 1, wave-uniform: the kernel-argument arrays are never indexed dynamically.
// PICK runs for every query i in order, with `in`: the sample belongs to query i or a later one.
// (Macros, not functions: a callee is optimised on its own before it is inlined, which reorders the kernels' scalar
// arithmetic; expanded in place, every kernel compiles to the instructions of its hand-written chain.)
#define DRS_OWNER_CHAIN(q, smp, ...)                                                                                    \
  _Pragma("unroll") for (int i = 1; i < 8; ++i) {                                                                       \
    const bool in = i < (q).n_q && (smp) >= (q).cum[i];                                                                 \
    __VA_ARGS__                                                                                                         \
  }                                                                                                                     \
  if ((q).n_q > 8) { /* (launch sets of 9 .. 16 queries only: smaller ones never touch the upper half of the arrays) */ \
    _Pragma("unroll") for (int i = 8; i < DRS_MAX_COALESCE; ++i) {                                                      \
      const bool in = i < (q).n_q && (smp) >= (q).cum[i];                                                               \
      __VA_ARGS__                                                                                                       \
    }                                                                                                                   \
  }

// Sample smp of SlsArgs a: declares (under the names given) its number b in its query, its output row vrow, its
// query's fixed bag length ulen (-1: ragged bags, through off), indices idx and offsets off.  (Separate variables, in
// this order: the compiler's SSA form then orders them as in the kernels' hand-written chains, and so do the listings.)
#define DRS_OWNER_OF(a, smp, B_, VROW_, ULEN_, IDX_, OFF_)                                                              \
  [[maybe_unused]] int B_ = (smp), VROW_ = (a).q.vstart[0] + (smp), ULEN_ = (a).uniform_len[0];                         \
  [[maybe_unused]] const int32_t* IDX_ = (a).idx[0];                                                                    \
  [[maybe_unused]] const int32_t* OFF_ = (a).off[0];                                                                    \
  DRS_OWNER_PICK(a, smp, B_, VROW_, ULEN_, IDX_, OFF_)
// the selects alone, onto lvalues that already hold query 0's values
#define DRS_OWNER_PICK(a, smp, B_, VROW_, ULEN_, IDX_, OFF_)                                                            \
  DRS_OWNER_CHAIN((a).q, smp, B_ = in ? (smp) - (a).q.cum[i] : B_;                                                      \
                  VROW_ = in ? (a).q.vstart[i] + (smp) - (a).q.cum[i] : VROW_;                                          \
                  ULEN_ = in ? (a).uniform_len[i] : ULEN_;                                                              \
                  IDX_ = in ? (a).idx[i] : IDX_;                                                                        \
                  OFF_ = in ? (a).off[i] : OFF_;)
// the same as a value (din.hip's fused kernels keep one per sample of a workgroup)
struct Owner {
  int b, vrow, ulen;
  const int32_t* idx;
  const int32_t* off;
};
__device__ __forceinline__ Owner owner_of(const SlsArgs& a, int smp) {
  Owner o = {smp, a.q.vstart[0] + smp, a.uniform_len[0], a.idx[0], a.off[0]};
  DRS_OWNER_PICK(a, smp, o.b, o.vrow, o.ulen, o.idx, o.off)
  return o;
}

// Sample smp of QTable q: declares (under the names given) its number b in its query, the query's size bs and its first
// virtual row vstart
#define DRS_QOWNER_OF(q, smp, B_, BS_, VSTART_)                                                                         \
  [[maybe_unused]] int B_ = (smp), BS_ = (q).bs[0], VSTART_ = (q).vstart[0];                                            \
  DRS_OWNER_CHAIN(q, smp, B_ = in ? (smp) - (q).cum[i] : B_;                                                            \
                  BS_ = in ? (q).bs[i] : BS_;                                                                           \
                  VSTART_ = in ? (q).vstart[i] : VSTART_;)

}  // namespace
}  // namespace drs
