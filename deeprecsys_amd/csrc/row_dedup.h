// Duplicate ids of a device row update (include/drs_device_rows.h; the kernels are device_rows.hip): which occurrence of an id
// is written.  The last one wins, so the passes keep, per id, the LARGEST position that names it, in an open-addressing table
// of 64-bit slots: one pass inserts every (id, position), the next asks for each position whether the table's entry for its
// id holds that very position.  The slot encoding, the capacity rule, the hash and the two probe loops are here, written over
// an atomics policy: the kernels hand in HIP's global-memory atomics, a host program plain loads and stores
// (tests/test_device_rows_cpu.py walks the same text under the address and undefined-behaviour sanitizers).  Plain C++ with
// no dependency, so that a host program can include it on its own.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define DRS_DEDUP_HD __host__ __device__
#else
#define DRS_DEDUP_HD
#endif

namespace drs {

// A slot holds (id << 32) | position: the id in the high bits, so that the unsigned maximum of two slots of ONE id is the
// one with the larger position and a slot never changes its id once it is claimed.  Legal ids are table rows, below 2^31
// (drs_create keeps a table's rows below that); legal positions are below 2^32.  The empty marker is all ones: its id
// field, 2^32 - 1, is no legal id, and (id 0, position 0) -- the slot 0 -- is an entry like any other.
constexpr uint64_t kDedupEmpty = ~(uint64_t)0;
constexpr int64_t kDedupMaxId = ((int64_t)1 << 31) - 1;
constexpr int64_t kDedupMaxPos = ((int64_t)1 << 32) - 1;
DRS_DEDUP_HD inline uint64_t dedup_slot(int64_t id, int64_t pos) { return ((uint64_t)id << 32) | (uint64_t)pos; }
DRS_DEDUP_HD inline int64_t dedup_id(uint64_t slot) { return (int64_t)(slot >> 32); }
DRS_DEDUP_HD inline int64_t dedup_pos(uint64_t slot) { return (int64_t)(slot & 0xffffffffu); }

// slots of the table n positions are inserted into: the power of two >= 2 n (never more than half full)
inline uint64_t dedup_capacity(int64_t n) {
  uint64_t cap = 2;
  while (cap < 2 * (uint64_t)(n > 0 ? n : 0)) cap <<= 1;
  return cap;
}

// an id's home bucket: the 64-bit finalizer of MurmurHash3 -- consecutive rows spread over the table
DRS_DEDUP_HD inline uint64_t dedup_hash(int64_t id) {
  uint64_t z = (uint64_t)id;
  z = (z ^ (z >> 33)) * 0xff51afd7ed558ccdull;
  z = (z ^ (z >> 33)) * 0xc4ceb9fe1a85ec53ull;
  return z ^ (z >> 33);
}

// The atomics policy `A`:
//   uint64_t load(const uint64_t* p)                      the slot's value
//   uint64_t cas(uint64_t* p, uint64_t expect, uint64_t v) stores v where *p == expect; returns what *p held
//   void     max(uint64_t* p, uint64_t v)                 *p = max(*p, v), unsigned
struct DedupHostAtomics {
  uint64_t load(const uint64_t* p) const { return *p; }
  uint64_t cas(uint64_t* p, uint64_t expect, uint64_t v) const {
    const uint64_t old = *p;
    if (old == expect) *p = v;
    return old;
  }
  void max(uint64_t* p, uint64_t v) const { if (v > *p) *p = v; }
};

// (id, pos) into the table of `cap` slots (a power of two): an empty slot on the id's probe chain is claimed, a slot that
// holds the id is raised to the larger position.  The chain is linear, wraps at the table's end and is walked at most `cap`
// steps: false says that every slot holds another id -- a full table, which the capacity rule excludes; the caller reports
// it instead of looping.
template <class A>
DRS_DEDUP_HD inline bool dedup_insert(uint64_t* slots, uint64_t cap, int64_t id, int64_t pos, const A& at) {
  const uint64_t v = dedup_slot(id, pos), mask = cap - 1;
  uint64_t h = dedup_hash(id) & mask;
  for (uint64_t k = 0; k < cap; ++k, h = (h + 1) & mask) {
    uint64_t cur = at.load(slots + h);
    if (cur == kDedupEmpty) {
      cur = at.cas(slots + h, kDedupEmpty, v);
      if (cur == kDedupEmpty) return true;
    }
    if (dedup_id(cur) == id) {
      at.max(slots + h, v);
      return true;
    }
  }
  return false;
}

// the position the table holds for `id` once every insert is done, or -1: the id was never inserted (an empty slot ends its
// chain, or -- a full table -- `cap` steps do)
template <class A>
DRS_DEDUP_HD inline int64_t dedup_lookup(const uint64_t* slots, uint64_t cap, int64_t id, const A& at) {
  const uint64_t mask = cap - 1;
  uint64_t h = dedup_hash(id) & mask;
  for (uint64_t k = 0; k < cap; ++k, h = (h + 1) & mask) {
    const uint64_t cur = at.load(slots + h);
    if (cur == kDedupEmpty) return -1;
    if (dedup_id(cur) == id) return dedup_pos(cur);
  }
  return -1;
}

// position r is written iff the table's entry for its id holds r: the last occurrence of every id, and every position
// where the ids are distinct
template <class A>
DRS_DEDUP_HD inline bool dedup_wins(const uint64_t* slots, uint64_t cap, int64_t id, int64_t r, const A& at) {
  return dedup_lookup(slots, cap, id, at) == r;
}

}  // namespace drs
