// Host helpers shared by the translation units that pick a kernel instance at run time (sls.hip, sls_wflat.hip, din.hip, dien.hip).
#pragma once
#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>

#include <cassert>
#include <type_traits>

namespace drs {
namespace {

// stop: optional event recorded BY the kernel dispatch itself (its completion signal) -- no
// separate marker packet between this launch and the next one on the stream
template <typename K, typename... X>
void launch_kb(K kernel, dim3 grid, dim3 block, size_t lds, hipStream_t s, hipEvent_t stop, const X&... x) {
  if (stop) hipExtLaunchKernelGGL(kernel, grid, block, lds, s, nullptr, stop, 0, x...);
  else hipLaunchKernelGGL(kernel, grid, block, lds, s, x...);
}
template <typename K, typename... X>
void launch_k(K kernel, dim3 grid, hipStream_t s, hipEvent_t stop, const X&... x) {
  launch_kb(kernel, grid, dim3(64), 0, s, stop, x...);
}

// f(std::integral_constant<int, V>) for the V of the list equal to v: one instance parameter of a launch, from its
// run-time value.  The callers only ask for instantiated values: one that is not is a bug of theirs, caught here
template <int V, int... Vs, class F>
void with_int(int v, F&& f) {
  if constexpr (sizeof...(Vs) == 0) {
    assert(v == V && "no kernel instance for this value of a launch parameter");
    f(std::integral_constant<int, V>{});
  } else if (v == V) f(std::integral_constant<int, V>{});
  else with_int<Vs...>(v, f);
}

}  // namespace
}  // namespace drs
