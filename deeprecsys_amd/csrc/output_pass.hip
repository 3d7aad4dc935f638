// libdrs_hip.so: the output pass on the device (include/drs_device_outputs.h), the mirror of input_pass.hip.  ONE launch per
// launch set, behind the set's last kernel: every query's scores go from the slot's [Mv, n_out] buffer, where the query
// starts at its virtual row, to the caller's own device array at the caller's row stride.  The arguments travel by value in
// the kernarg (OutPassArgs: no table in memory, no extra copy); output_plan.h says which lane moves which element.
//
// A set whose arrays were wrong (the slot's device error word is non-zero: input_pass.hip, the gather) was computed from
// clamped rows: every element of every query then receives the quiet NaN kOutPassNaN instead, so a consumer ordered on a
// stream never reads plausible scores nobody has signed off.  The pass moves sum(bs) * n_out floats -- 64 KB for n_out 1,
// 2 MB for MT-WnD's sets -- with one coalesced dword per lane and round: it is bound by its launch, not by bandwidth.
#include "drs_internal.h"
#include "output_plan.h"

namespace drs {

static_assert(kOutPassQueries == DRS_MAX_COALESCE, "OutPassArgs holds one entry per query of a launch set");

namespace {

__global__ __launch_bounds__(kOutPassThreads) void output_pass_kernel(const OutPassArgs a) {
  const int block = (int)blockIdx.x, tid = (int)threadIdx.x;
  const int qi = out_owner(a, block);
  const uint32_t* __restrict__ src = reinterpret_cast<const uint32_t*>(a.src);
  uint32_t* __restrict__ dst = reinterpret_cast<uint32_t*>(a.q[qi].dst);
  const bool failed = *a.err != 0;         // (one word, the same for every lane of every workgroup of the set)
  uint32_t v[kOutPassPerLane];
#pragma unroll
  for (int k = 0; k < kOutPassPerLane; ++k) {
    const int64_t e = out_element(a, qi, block, k, tid);
    v[k] = e >= 0 ? src[out_src_index(a, qi, e)] : 0u;
  }
#pragma unroll
  for (int k = 0; k < kOutPassPerLane; ++k) {
    const int64_t e = out_element(a, qi, block, k, tid);
    if (e >= 0) dst[out_dst_index(a, qi, e)] = failed ? kOutPassNaN : v[k];
  }
}

}  // namespace

hipError_t launch_output_pass(const OutPassArgs& a, int64_t grid, hipStream_t stream) {
  if (grid <= 0) return hipSuccess;
  hipLaunchKernelGGL(output_pass_kernel, dim3((unsigned)grid), dim3(kOutPassThreads), 0, stream, a);
  return hipGetLastError();
}

}  // namespace drs
