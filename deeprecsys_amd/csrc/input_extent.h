// The bytes the device input pass reads from one per-query array (include/drs_device_inputs.h): T rows of `count` elements,
// `stride` elements apart, `elem` bytes each -- (T - 1) * stride + count elements, or nothing when count == 0.  Plain C++
// with no dependency, so that a host program can include it on its own (tests/test_device_inputs_cpu.py does).
#pragma once
#include <stdint.h>

namespace drs {

// false: a negative argument, or an extent beyond 2^60 bytes -- a wild row stride must not wrap into a small extent that
// passes the allocation check (every comparison is made by division, nothing here can overflow)
inline bool input_extent_bytes(int64_t T, int64_t stride, int64_t count, int64_t elem, uint64_t* bytes) {
  *bytes = 0;
  if (T < 1 || stride < 0 || count < 0 || elem < 1) return false;
  if (count == 0) return true;
  const int64_t lim = ((int64_t)1 << 60) / elem;      // elements
  if (count > lim) return false;
  if (T > 1 && stride > (lim - count) / (T - 1)) return false;
  *bytes = (uint64_t)((T - 1) * stride + count) * (uint64_t)elem;
  return true;
}

// does [p, p + bytes) end inside the allocation [base, base + size)?  (p inside it; by subtraction, no sum that could wrap)
inline bool extent_inside(uint64_t p, uint64_t bytes, uint64_t base, uint64_t size) {
  return p >= base && p - base <= size && bytes <= size - (p - base);
}

}  // namespace drs
