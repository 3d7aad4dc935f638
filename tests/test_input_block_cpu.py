"""csrc/input_block.h on its own, in a host program: the [dense | idx | off] block layout every per-call input path reads, the
host pass that fills a block (int64 -> int32 + the ENFORCEs) and the host-to-device copies of what was used of it.  The
program is built with the host sanitizers (a block is malloc'ed at exactly the layout's size, so one byte past it is seen)
and once without them; a last test pins that no .hip file restates the layout's arithmetic."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "deeprecsys_amd", "csrc")

BLOCK_MAIN = r"""
#include "input_block.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
using namespace drs::eng;
static int fails = 0;
#define CHECK(c) do { if (!(c)) { if (++fails < 40) printf("line %d: %s\n", __LINE__, #c); } } while (0)

// ---- the layout ----
static void layouts() {
  const int64_t P[4][4] = {{1, 0, 1, 1}, {64, 13, 3, 256}, {256, 16, 8, 20480}, {4096, 0, 26, 4096 * 32}};
  for (auto& p : P) {
    const int64_t mb = p[0], md = p[1], T = p[2], cap = p[3];
    const BlockLayout L(mb, md, T, cap);
    CHECK(L.dense_bytes == (size_t)(4 * mb * (md > 0 ? md : 1)));      // m_den 0 still reserves one float per row
    CHECK(L.idx_bytes == (size_t)(4 * T * cap));
    CHECK(L.off_bytes == (size_t)(4 * T * (mb + 1)));
    // dense, idx, off in this order, back to back: disjoint
    CHECK(L.dense_bytes > 0 && L.idx_at() == L.dense_bytes && L.off_at() == L.idx_at() + L.idx_bytes);
    CHECK(L.idx_at() % 4 == 0 && L.off_at() % 4 == 0 && L.bytes % 4 == 0);
    CHECK(L.bytes == L.dense_bytes + L.idx_bytes + L.off_bytes && L.off_at() + L.off_bytes == L.bytes);
    CHECK(L.padded % 256 == 0 && L.padded >= L.bytes && L.padded - L.bytes < 256);
    CHECK(L.off_stride() == (size_t)(mb + 1) && L.idx_elems() == (size_t)(T * cap) && L.off_elems() == (size_t)(T * (mb + 1)));
    CHECK(L.h_off_at(0, 0) == 0 && L.h_off_at(T - 1, mb) == L.off_elems() - 1 && L.h_off_at(1, 2) == (size_t)(mb + 1 + 2));
    for (int64_t n = 0; n <= cap; ++n) {
      const size_t u = L.used_prefix(n);
      if (u > L.off_at() || u < L.idx_at() || u != L.dense_bytes + 4 * (size_t)((T - 1) * cap + n)) { CHECK(!"used_prefix"); break; }
    }
    CHECK(L.used_prefix(cap) == L.off_at());
    char* base = reinterpret_cast<char*>(4096);
    const BlockView v = view_block(L, base);
    CHECK((char*)v.dense == base && (char*)v.idx == base + L.idx_at() && (char*)v.off == base + L.off_at());
  }
}

// ---- the host pass ----
static const int64_t ROWS[3] = {1000, 37, (int64_t)1 << 31};
struct Table { std::vector<int64_t> ids; std::vector<int32_t> lens; int64_t n_idx; };
static Table table_of(int t, int bs, const std::vector<int32_t>& lens) {
  Table tb;
  tb.lens = lens;
  tb.lens.resize((size_t)(bs > 0 ? bs : 1), 0);          // (never a null data())
  tb.n_idx = 0;
  for (int b = 0; b < bs; ++b) tb.n_idx += lens[(size_t)b];
  tb.ids.resize((size_t)tb.n_idx + 1);
  for (int64_t j = 0; j < tb.n_idx; ++j) tb.ids[(size_t)j] = (j * 7919 + t * 13 + (ROWS[t] - 1) * (j % 5 == 0)) % ROWS[t];
  return tb;
}
// a query of T = 3 tables into a block malloc'ed at exactly L.bytes, against the scalar loops
static void good_query(const BlockLayout& L, int bs, const std::vector<int32_t> lens[3]) {
  char* block = static_cast<char*>(malloc(L.bytes));
  memset(block, 0x5a, L.bytes);
  const BlockView v = view_block(L, block);
  for (int t = 0; t < 3; ++t) {
    const Table tb = table_of(t, bs, lens[t]);
    int32_t* idx32 = v.idx + (size_t)t * L.cap;
    int32_t* off = v.off + L.h_off_at(t, 0);
    ConvRes r;
    convert_table(L, ROWS[t], bs, tb.ids.data(), tb.n_idx, tb.lens.data(), idx32, off, r);
    CHECK(r.code == DRS_OK && r.n_idx == tb.n_idx && r.total == tb.n_idx);
    for (int64_t j = 0; j < tb.n_idx; ++j) CHECK(idx32[j] == (int32_t)tb.ids[(size_t)j]);
    for (int64_t j = tb.n_idx; j < L.cap; ++j) CHECK(idx32[j] == 0x5a5a5a5a);       // nothing past the last index
    int32_t acc = 0;
    bool same = true;
    CHECK(off[0] == 0);
    for (int b = 0; b < L.max_batch; ++b) {
      if (b < bs) { acc += tb.lens[(size_t)b]; same = same && tb.lens[(size_t)b] == tb.lens[0]; }
      CHECK(off[b + 1] == acc);
    }
    CHECK(r.same == same);
  }
  for (size_t k = 0; k < L.dense_bytes; ++k) CHECK(block[k] == 0x5a);               // the dense rows are not the pass's
  free(block);
}
static void good_queries() {
  const BlockLayout L(16, 5, 3, 16 * 13);
  const int mb = 16;
  std::vector<int32_t> uni[3], rag[3], none[3], zero[3], edge[3];
  for (int t = 0; t < 3; ++t) {
    uni[t].assign(mb, 13);                                                           // full and uniform: n_idx == cap
    for (int b = 0; b < 11; ++b) rag[t].push_back((b * 5 + t * 3) % 14);             // ragged, 11 of 16 samples
    zero[t].assign(7, 0);                                                            // samples, but n_idx == 0
    edge[t].assign(mb, 0);
    edge[t][(size_t)t] = 16 * 13;                                                    // n_idx == cap in one bag
  }
  good_query(L, mb, uni);
  good_query(L, 11, rag);
  good_query(L, 0, none);
  good_query(L, 7, zero);
  good_query(L, mb, edge);
  std::vector<int32_t> mixed[3] = {uni[0], rag[1], zero[2]};                         // uniform in one table, not in the next
  mixed[1].resize(mb, 1);
  mixed[2].resize(mb, 0);
  good_query(L, mb, mixed);
}
// the destination at every 4-byte misalignment of a 32-byte line: head and tail of the AVX2 form; the base form beside it
static void misaligned() {
  const int sizes[] = {0, 1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 100};
  for (int k = 0; k < 8; ++k)
    for (int n : sizes) {
      std::vector<int64_t> src((size_t)n + 1);
      for (int j = 0; j < n; ++j) src[(size_t)j] = (j * 31 + k) % 1000;
      for (int bad = -1; bad < 3; ++bad) {
        const int at = bad < 0 ? -1 : bad == 0 ? 0 : bad == 1 ? n / 2 : n - 1;
        if (bad >= 0 && n == 0) continue;
        std::vector<int64_t> s = src;
        if (at >= 0) s[(size_t)at] = bad == 1 ? -1 : 1000;
        if (at > 0 && bad == 2) s[0] = 999;                                          // the largest good index stays good
        for (int form = 0; form < 2; ++form) {
          void* p = nullptr;
          if (posix_memalign(&p, 32, (size_t)(k + n) * 4 > 0 ? (size_t)(k + n) * 4 : 4) != 0) { CHECK(!"posix_memalign"); return; }
          int32_t* d = static_cast<int32_t*>(p) + k;                                 // ends exactly at the allocation's end
          const int64_t got = form ? narrow_checked_base(s.data(), n, 1000, d) : narrow_checked(s.data(), n, 1000, d);
          CHECK(got == at);
          for (int j = 0; j < n; ++j) CHECK(d[j] == (int32_t)s[(size_t)j]);
          free(p);
        }
      }
    }
  int32_t d[16];
  std::vector<int64_t> s(16, 0);
  CHECK(narrow_checked(s.data(), 16, 0, d) == 0 && narrow_checked_base(s.data(), 16, 0, d) == 0);   // a table of no rows
  s[9] = (int64_t)1 << 32;                                                           // would narrow to 0: refused at full width
  CHECK(narrow_checked(s.data(), 16, 1000, d) == 9 && narrow_checked_base(s.data(), 16, 1000, d) == 9);
}
// bad inputs: the code and the position a sequential pass reports
static void bad_queries() {
  const BlockLayout L(16, 5, 3, 16 * 13);
  char* block = static_cast<char*>(malloc(L.bytes));
  const BlockView v = view_block(L, block);
  std::vector<int32_t> lens(16, 13);
  auto run = [&](int t, int bs, const int64_t* ids, int64_t n_idx, const int32_t* ln) {
    ConvRes r;
    convert_table(L, ROWS[t], bs, ids, n_idx, ln, v.idx + (size_t)t * L.cap, v.off + L.h_off_at(t, 0), r);
    return r;
  };
  Table tb = table_of(0, 16, lens);
  ConvRes r;
  std::vector<int32_t> ln = lens;
  ln[2] = -1;
  r = run(1, 16, tb.ids.data(), tb.n_idx, ln.data());
  CHECK(r.code == DRS_ERR_LENGTHS_SUM && r.bag == 2 && r.pos == -1);
  ln = lens; ln[15] = 12;                                                            // a sum short by one
  r = run(0, 16, tb.ids.data(), tb.n_idx, ln.data());
  CHECK(r.code == DRS_ERR_LENGTHS_SUM && r.pos == 0 && r.total == tb.n_idx - 1 && r.n_idx == tb.n_idx);
  ln = lens; ln[15] = 14;                                                            // ... long by one
  r = run(0, 16, tb.ids.data(), tb.n_idx, ln.data());
  CHECK(r.code == DRS_ERR_LENGTHS_SUM && r.pos == 0 && r.total == tb.n_idx + 1 && r.n_idx == tb.n_idx);
  ln = lens; ln[3] = 14;                                                             // ... long from bag 3 on: never past cap
  r = run(0, 16, tb.ids.data(), tb.n_idx, ln.data());
  CHECK(r.code == DRS_ERR_LENGTHS_SUM && r.pos == 0 && r.total > tb.n_idx);
  std::vector<int64_t> ids = tb.ids;
  ids[5] = ROWS[0];                                                                  // an index equal to rows
  r = run(0, 16, ids.data(), tb.n_idx, lens.data());
  CHECK(r.code == DRS_ERR_INDEX_RANGE && r.pos == 5 && r.val == ROWS[0]);
  ids = tb.ids; ids[17] = -1;
  r = run(0, 16, ids.data(), tb.n_idx, lens.data());
  CHECK(r.code == DRS_ERR_INDEX_RANGE && r.pos == 17 && r.val == -1);
  ids = tb.ids; ids[200] = (int64_t)1 << 31;                                         // table 2 has 2^31 rows: 2^31 - 1 passes, 2^31 not
  r = run(2, 16, ids.data(), tb.n_idx, lens.data());
  CHECK(r.code == DRS_ERR_INDEX_RANGE && r.pos == 200);
  ids[200] = ((int64_t)1 << 31) - 1;
  r = run(2, 16, ids.data(), tb.n_idx, lens.data());
  CHECK(r.code == DRS_OK);
  // two bad tables: the lower one reports
  ConvRes res[3];
  std::vector<int64_t> b1 = tb.ids, b2 = tb.ids;
  for (auto& x : b1) x %= ROWS[1];
  b1[9] = -1; b2[3] = ROWS[2];
  res[0] = run(0, 16, tb.ids.data(), tb.n_idx, lens.data());
  res[1] = run(1, 16, b1.data(), tb.n_idx, lens.data());
  res[2] = run(2, 16, b2.data(), tb.n_idx, lens.data());
  CHECK(res[0].code == DRS_OK && res[2].code == DRS_ERR_INDEX_RANGE && res[2].pos == 3);
  int first = -1;                                                                    // (seal_query's scan: the lowest table)
  for (int t = 2; t >= 0; --t) if (res[t].code != DRS_OK) first = t;
  CHECK(first == 1 && res[1].code == DRS_ERR_INDEX_RANGE && res[1].pos == 9 && res[1].val == -1);
  // null arrays, and one index more than the block holds: refused before anything is written
  memset(block, 0x5a, L.bytes);
  r = run(0, 16, nullptr, tb.n_idx, lens.data());
  CHECK(r.code == DRS_ERR_BAD_ARG && r.pos == -1);
  r = run(0, 16, tb.ids.data(), tb.n_idx, nullptr);
  CHECK(r.code == DRS_ERR_BAD_ARG && r.pos == -2);
  std::vector<int64_t> big((size_t)L.cap + 1, 1);
  ln = lens; ln[15] = 14;
  r = run(2, 16, big.data(), L.cap + 1, ln.data());
  CHECK(r.code == DRS_ERR_BAD_ARG && r.pos == -3 && r.n_idx == L.cap + 1);
  r = run(1, 16, big.data(), -1, ln.data());
  CHECK(r.code == DRS_ERR_BAD_ARG && r.pos == -3);
  for (size_t k = 0; k < L.bytes; ++k) if (block[k] != 0x5a) { CHECK(!"a refused table wrote into the block"); break; }
  r = run(0, 0, nullptr, 0, lens.data());                                            // no indices: a null index array is fine
  CHECK(r.code == DRS_OK && r.same);
  free(block);
}

// ---- the copies ----
static bool inside(const BlockCopy* c, int n_c, size_t at, size_t bytes) {
  for (int k = 0; k < n_c; ++k)
    if (c[k].at <= at && at + bytes <= c[k].at + c[k].bytes) return true;
  return bytes == 0;
}
static void plan_properties(const BlockLayout& L) {
  const int ns[] = {1, 2, 16};
  for (int n : ns)
    for (int fill = 0; fill < 3; ++fill)
      for (int offs = 0; offs < 3; ++offs)
        for (int merge = 0; merge < 2; ++merge) {
          size_t used[16];
          bool need[16];
          for (int i = 0; i < n; ++i) {
            const bool full = fill == 0 || (fill == 2 && i % 2 == 0);                // all full | all at one index | mixed
            used[i] = L.used_prefix(full ? L.cap : 1);
            need[i] = offs == 1 || (offs == 2 && i == n / 2);                        // none | all | one
          }
          BlockCopy c[32];
          const size_t step = L.padded;
          const int n_c = plan_block_copies(L, step, n, used, need, merge != 0, c);
          CHECK(n_c >= 1 && n_c <= 2 * n);
          for (int k = 0; k < n_c; ++k) {
            CHECK(c[k].bytes > 0 && c[k].at + c[k].bytes <= (size_t)n * step);       // inside the n blocks
            if (k) CHECK(c[k - 1].at + c[k - 1].bytes <= c[k].at);                   // in order, no overlap
          }
          for (int i = 0; i < n; ++i) {
            CHECK(inside(c, n_c, (size_t)i * step, used[i]));                        // every used byte
            if (need[i]) CHECK(inside(c, n_c, (size_t)i * step + L.off_at(), L.off_bytes));
          }
          // today's rule, restated: mostly full -> one copy, else a block at a time
          size_t sum = 0;
          bool any = false;
          for (int i = 0; i < n; ++i) { sum += used[i]; any = any || need[i]; }
          if (merge && 2 * sum >= (size_t)n * step) {
            CHECK(n_c == 1 && c[0].at == 0 && c[0].bytes == (any ? (size_t)n * step : (size_t)(n - 1) * step + used[n - 1]));
          } else {
            int k = 0;
            for (int i = 0; i < n; ++i) {
              CHECK(k < n_c && c[k].at == (size_t)i * step && c[k].bytes == used[i]);
              ++k;
              if (need[i]) { CHECK(k < n_c && c[k].at == (size_t)i * step + L.off_at() && c[k].bytes == L.off_bytes); ++k; }
            }
            CHECK(k == n_c);
          }
        }
}
static bool is_list(const BlockCopy* c, int n_c, std::vector<size_t> want) {
  if ((size_t)n_c * 2 != want.size()) return false;
  for (int k = 0; k < n_c; ++k)
    if (c[k].at != want[(size_t)2 * k] || c[k].bytes != want[(size_t)2 * k + 1]) return false;
  return true;
}
static void plan_lists() {
  // (64, 0, 1, 256): dense 256 | idx 1024 | off 260 = 1540 bytes, 1792 from block to block; a full prefix is 1280 bytes,
  // the prefix of one index 260 -- the lists the set form's three branches and the one-query form issued before
  const BlockLayout S(64, 0, 1, 256);
  CHECK(S.bytes == 1540 && S.padded == 1792 && S.off_at() == 1280 && S.used_prefix(256) == 1280 && S.used_prefix(1) == 260);
  BlockCopy c[32];
  size_t full[3] = {1280, 1280, 1280}, one[3] = {260, 260, 260};
  bool none[3] = {false, false, false}, mid[3] = {false, true, false};
  CHECK(is_list(c, plan_block_copies(S, 1792, 2, full, mid, true, c), {0, 3584}));                        // n blocks whole
  CHECK(is_list(c, plan_block_copies(S, 1792, 2, full, none, true, c), {0, 1792 + 1280}));                // ... to the last prefix
  CHECK(is_list(c, plan_block_copies(S, 1792, 3, one, mid, true, c), {0, 260, 1792, 260, 1792 + 1280, 260, 3584, 260}));
  CHECK(is_list(c, plan_block_copies(S, 1792, 3, one, none, true, c), {0, 260, 1792, 260, 3584, 260}));
  CHECK(is_list(c, plan_block_copies(S, 0, 1, full, mid + 1, false, c), {0, 1280, 1280, 260}));           // a query alone
  CHECK(is_list(c, plan_block_copies(S, 0, 1, full, none, false, c), {0, 1280}));
  CHECK(is_list(c, plan_block_copies(S, 0, 1, one, mid + 1, false, c), {0, 260, 1280, 260}));
  // (64, 13, 3, 256): 7180 bytes, 7424 apart; with three tables even one index per table is a prefix of 5380 bytes --
  // more than half a block, so the set goes whole
  const BlockLayout B(64, 13, 3, 256);
  CHECK(B.bytes == 7180 && B.padded == 7424 && B.used_prefix(1) == 5380);
  size_t b1[2] = {5380, 5380};
  bool all[2] = {true, true};
  CHECK(is_list(c, plan_block_copies(B, 7424, 2, b1, all, true, c), {0, 14848}));
  CHECK(is_list(c, plan_block_copies(B, 7424, 2, b1, none, true, c), {0, 7424 + 5380}));
}

int main() {
  layouts();
  good_queries();
  misaligned();
  bad_queries();
  plan_properties(BlockLayout(64, 13, 3, 256));
  plan_properties(BlockLayout(64, 0, 1, 256));
  plan_properties(BlockLayout(1, 0, 1, 1));
  plan_lists();
  printf("%d failures (avx2 %d)\n", fails, (int)!!__builtin_cpu_supports("avx2"));
  return fails != 0;
}
"""


@pytest.fixture(scope="module")
def block_main(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a C++ compiler builds the host program"
    d = tmp_path_factory.mktemp("input_block")
    src = d / "block_main.cpp"
    src.write_text(BLOCK_MAIN)

    def build(name, *flags):
        exe = d / name
        r = subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-g", "-I", CSRC] + list(flags) + [str(src), "-o", str(exe)],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        return str(exe)
    return build


def test_the_block_layout_the_host_pass_and_the_copies_under_the_host_sanitizers(block_main):
    """the header alone with -fsanitize=address,undefined, run directly: the four layouts, every table of the good and the
    bad queries into blocks of exactly the layout's size, destinations at every misalignment, and the copy lists"""
    # (the sanitizers' runtimes linked statically: the program then starts whatever else the loader brings in first)
    exe = block_main("block_main_san", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                     "-static-libasan", "-static-libubsan")
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "0 failures" in r.stdout, r.stdout + r.stderr


def test_the_same_program_without_the_sanitizers(block_main):
    """... and optimised, with the allocator's own alignment: the streaming-store form where the host has AVX2"""
    exe = block_main("block_main_o3", "-O3")
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "0 failures" in r.stdout, r.stdout + r.stderr


# the one place outside input_block.h that may spell the prefix sums' stride out: the device input pass gets max_batch as a
# kernel argument and computes the stride on the device (file, line, the line's text)
ALLOWED = [("input_pass.hip", 84, "int32_t* off = q.off + (int64_t)t * (a.max_batch + 1);")]
FORMULAS = [re.compile(r"max_batch\s*\+\s*1"),                                          # the stride of off / h_off
            re.compile(r"(?<![A-Za-z0-9_])T\s*\*\s*(?:\(\s*\w+\s*\)\s*)?(?:\w+(?:->|\.))*cap\b"),   # T * e->cap: the size of idx
            re.compile(r"max_batch\s*\*\s*\(\s*(?:\w+(?:->|\.))*m_den\s*>\s*0")]         # max_batch * (m_den > 0 ? m_den : 1)


def test_no_hip_file_restates_the_layout():
    found = []
    names = sorted(n for n in os.listdir(CSRC) if n.endswith(".hip"))
    assert "engine_inputs.hip" in names and "input_pass.hip" in names
    for name in names:
        for no, line in enumerate(open(os.path.join(CSRC, name)).read().split("\n"), 1):
            if any(f.search(line) for f in FORMULAS):
                found.append((name, no, line.strip()))
    assert found == ALLOWED, found
    # ... and the files that lay blocks out or index them read the engine's one layout
    for name in ("engine_create.hip", "engine_inputs.hip", "engine_device_inputs.hip", "engine_dispatch.hip", "engine_options.hip"):
        assert "e->blk" in open(os.path.join(CSRC, name)).read(), name
    hdr = open(os.path.join(CSRC, "input_block.h")).read()
    assert "hip" not in re.sub(r"//.*", "", hdr).lower()                                # plain C++: no HIP include, no HIP call
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "input_block.h" in mk
