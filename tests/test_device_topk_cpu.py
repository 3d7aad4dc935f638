"""CPU side of the top-k launch sets (include/drs_device_topk.h): the symbols and the header, the frozen symbol lists, the
ordering rule and the tiled selection (deeprecsys_amd/csrc/topk_plan.h) walked by a host program against std::sort, the
extent arithmetic of the refusals, the wrapper's argument checks, and the documents."""
import os
import re
import shutil
import subprocess

import pytest

from deeprecsys_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["drs_topk_rows", "drs_run_queues_device_topk_multi_async"]
C = N.C


def test_the_library_exports_both_symbols():
    L = N.lib()
    assert [n for n, _, _ in N.DEVICE_TOPK_SYMBOLS] == NAMES
    for name, res, args in N.DEVICE_TOPK_SYMBOLS:
        fn = getattr(L, name)
        assert fn.restype is res and fn.argtypes == args, name
    rows, multi = [a for _, _, a in N.DEVICE_TOPK_SYMBOLS]
    # h, d_scores, rows, n_out, row_stride, col, k, d_idx, d_top, stream
    assert rows == [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    # the eleven arguments of the device-input call; d_weights, wgt_row_stride, wgt_dtype; k, col, d_top_idx, d_top_scores,
    # stream, ordered
    assert multi[:11] == N.DEVICE_INPUT_SYMBOLS[0][2]
    assert multi[11:14] == N.DEVICE_WEIGHT_SYMBOLS[0][2][11:14] == [C.POINTER(C.c_void_p), N._i64p, N._i32p]
    assert multi[14:] == [N._i32p, C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_void_p, C.c_int32]
    assert N.TOPK_MAX == 1024


def test_the_header_declares_both_calls_and_the_abi_version_stays():
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "a C compiler preprocesses the header"
    text = subprocess.run([cc, "-E", "-dD", os.path.join(ROOT, "include", "drs.h")], capture_output=True, text=True, check=True).stdout
    flat = re.sub(r"\s+", " ", text)
    w, p = r"\s*\w+\s*", r"\s*\*\s*"
    rows = (r"int32_t drs_topk_rows\s*\(\s*drs_handle" + w + r", const float" + p + r"\w+\s*, int64_t" + w + r", int32_t" + w +
            r", int64_t" + w + r", int32_t" + w + r", int32_t" + w + r", int32_t" + p + r"\w+\s*, float" + p + r"\w+\s*, void" + p +
            r"\w+\s*\)\s*;")
    multi = (r"int32_t drs_run_queues_device_topk_multi_async\s*\(\s*drs_handle" + w + r", int32_t" + w + r", int32_t" + w +
             r", const int32_t" + p + r"\w+\s*, const float" + p + r"const" + p + r"\w+\s*, const int64_t" + p + r"const" + p +
             r"\w+\s*, const int64_t" + p + r"\w+\s*, const int64_t" + p + r"\w+\s*, const int32_t" + p + r"const" + p +
             r"\w+\s*, const int64_t" + p + r"\w+\s*, const int32_t" + p + r"\w+\s*, const void" + p + r"const" + p +
             r"\w+\s*, const int64_t" + p + r"\w+\s*, const int32_t" + p + r"\w+\s*, const int32_t" + p + r"\w+\s*, int32_t" + w +
             r", int32_t" + p + r"const" + p + r"\w+\s*, float" + p + r"const" + p + r"\w+\s*, void" + p + r"\w+\s*, int32_t" + w +
             r"\)\s*;")
    assert re.search(rows, flat), "drs_topk_rows"
    assert re.search(multi, flat), "drs_run_queues_device_topk_multi_async"
    assert re.search(r"#define DRS_TOPK_MAX 1024\b", flat) and re.search(r"#define DRS_ABI_VERSION 5\b", flat)
    hdr = open(os.path.join(ROOT, "include", "drs.h")).read()
    assert "#define DRS_ABI_VERSION 5" in hdr and '#include "drs_device_topk.h"' in hdr
    assert hdr.index('#include "drs_device_rows.h"') < hdr.index('#include "drs_device_topk.h"') < hdr.rindex("#ifdef __cplusplus")
    assert not any(re.search(r"\b%s\s*\(" % n, hdr) for n in NAMES)          # declared in drs_device_topk.h alone
    sat = open(os.path.join(ROOT, "include", "drs_device_topk.h")).read()
    for word in ("Order", "Ordering", "Completion", "Lifetime", "Written", "NaN", "0x7fc00000", "0xffffffff", "LOWER row", "-1",
                 "ordered == 0", "ordered == 1", "null stream", "drs_wait", "hipMemGetAddressRange", "DRS_ERR_BAD_ARG", "overlap",
                 "topk_pass[", "All six models"):
        assert word in sat, word


def test_every_older_symbol_list_is_unchanged(cpu_abi):
    names = [n for n, _, _ in N.SYMBOLS]
    assert len(names) == 40 and len(set(names)) == 40
    assert not set(names) & set(NAMES)
    older = {"WEIGHT_SYMBOLS": ["drs_stage_batch_weights", "drs_sls_weighted"],
             "FP8_SYMBOLS": ["drs_table_fp8_exponent"],
             "ROW_SYMBOLS": ["drs_update_rows", "drs_get_rows"],
             "DEVICE_INPUT_SYMBOLS": ["drs_run_queues_device_multi_async", "drs_run_queues_device_async"],
             "DEVICE_OUTPUT_SYMBOLS": ["drs_run_queues_device_io_multi_async", "drs_run_queues_device_io_async"],
             "DEVICE_WEIGHT_SYMBOLS": ["drs_run_queues_device_weighted_multi_async"],
             "DEVICE_ROW_SYMBOLS": ["drs_update_rows_device", "drs_get_rows_device"]}
    for attr, want in older.items():
        assert [n for n, _, _ in getattr(N, attr)] == want, attr
    assert len(N.DEVICE_OUTPUT_SYMBOLS[0][2]) == 15 and len(N.DEVICE_WEIGHT_SYMBOLS[0][2]) == 18
    assert N.lib().drs_abi_version() == 5
    # the CPU restatement binds the frozen list (the fixture has just done so) and knows nothing of the new names
    assert cpu_abi.drs_abi_version() == 5
    for name in NAMES:
        assert not hasattr(cpu_abi, name)


# ------------------------------------------------------------------------------------------------
# the order and the tiled selection: topk_plan.h alone in a host program
PLAN_MAIN = r"""
#include "topk_plan.h"
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <functional>
#include <vector>
using namespace drs;
static int fails = 0;
static int g_case = -1;
#define CHECK(c) do { if (!(c)) { if (fails < 20) printf("line %d (case %d): %s\n", __LINE__, g_case, #c); ++fails; } } while (0)

static void order() {
  // the sortable word, pattern by pattern
  CHECK(topk_sortable(0x00000000u) == 0x80000000u);            // +0.0
  CHECK(topk_sortable(0x80000000u) == 0x7fffffffu);            // -0.0: just below +0.0
  CHECK(topk_sortable(0x7f800000u) == 0xff800000u);            // +inf
  CHECK(topk_sortable(0xff800000u) == 0x007fffffu);            // -inf: the smallest word a score has
  CHECK(topk_sortable(0x00000001u) == 0x80000001u);            // the smallest denormal, and its negative
  CHECK(topk_sortable(0x80000001u) == 0x7ffffffeu);
  CHECK(topk_sortable(0x007fffffu) == 0x807fffffu);            // the largest denormal
  CHECK(topk_sortable(0x807fffffu) == 0x7f800000u);
  CHECK(topk_sortable(0x3f800000u) == 0xbf800000u);            // 1.0 and -1.0
  CHECK(topk_sortable(0xbf800000u) == 0x407fffffu);
  CHECK(topk_sortable(0x7f7fffffu) == 0xff7fffffu);            // FLT_MAX, just below +inf
  // every NaN, either sign, quiet or signalling, any payload: the one word above +inf
  const uint32_t nans[] = {0x7fc00000u, 0xffc00000u, 0x7f800001u, 0xff800001u, 0x7fffffffu, 0xffffffffu, 0x7fc12345u, 0xffa54321u};
  for (uint32_t b : nans) CHECK(topk_sortable(b) == 0xffffffffu);
  // the chain the header states: NaN > +inf > FLT_MAX > 1 > denormal > +0 > -0 > -denormal > -1 > -inf
  const uint32_t chain[] = {0xffc00000u, 0x7f800000u, 0x7f7fffffu, 0x3f800000u, 0x00000001u, 0x00000000u, 0x80000000u, 0x80000001u,
                            0xbf800000u, 0xff800000u};
  for (size_t i = 0; i + 1 < sizeof chain / sizeof *chain; ++i) CHECK(topk_sortable(chain[i]) > topk_sortable(chain[i + 1]));
  // the key: the word above the row's complement; the lower row ranks first among equal scores; 0 is never a key
  CHECK(topk_key(0x3f800000u, 0) == 0xbf800000ffffffffull);
  CHECK(topk_key(0x3f800000u, 5) == 0xbf800000fffffffaull && topk_key_row(topk_key(0x3f800000u, 5)) == 5);
  CHECK(topk_key(0x3f800000u, 4) > topk_key(0x3f800000u, 5));
  CHECK(topk_key(0x7fc00000u, 9) > topk_key(0xffc00001u, 10) && topk_key(0x7fc00000u, 9) > topk_key(0x7f800000u, 0));
  CHECK(topk_key(0xff800000u, 0x7fffffff) == 0x007fffff80000000ull);      // the smallest key there is
  CHECK(topk_key(0xff800000u, 0x7fffffff) > 0 && topk_key_row(0x007fffff80000000ull) == 0x7fffffffu);
  // the steps
  CHECK(topk_steps(1) == 1 && topk_steps(1024) == 1 && topk_steps(1025) == 2 && topk_steps(2048) == 2 && topk_steps(2049) == 3);
  CHECK(topk_tile_rows(1, 0) == 1 && topk_tile_rows(1024, 0) == 1024 && topk_tile_rows(1025, 0) == 1024 && topk_tile_rows(1025, 1) == 1);
  CHECK(topk_tile_rows(3000, 2) == 952);
  const uint64_t four[4] = {9, 7, 5, 0};
  CHECK(topk_rank(four, 4, 9) == 0 && topk_rank(four, 4, 7) == 1 && topk_rank(four, 4, 5) == 2 && topk_rank(four, 2, 5) == 2);
  // the range of k and the extents
  CHECK(topk_k_in_range(0, 0) && topk_k_in_range(0, 5) && topk_k_in_range(5, 5) && !topk_k_in_range(6, 5) && !topk_k_in_range(-1, 5));
  CHECK(topk_k_in_range(1024, 1024) && topk_k_in_range(1024, 5000) && !topk_k_in_range(1025, 5000));
  uint64_t tb = 1, ib = 1;
  CHECK(topk_extent_bytes(10, 3, &tb, &ib) && tb == 120 && ib == 40);
  CHECK(topk_extent_bytes(0, 3, &tb, &ib) && tb == 0 && ib == 0);
  CHECK(topk_extent_bytes(1024, 1, &tb, &ib) && tb == 4096 && ib == 4096);
  CHECK(!topk_extent_bytes(-1, 3, &tb, &ib) && !topk_extent_bytes(4, 0, &tb, &ib));
  CHECK(topk_source_bytes(600, 8, 3, &tb) && tb == (599 * 8 + 3) * 4);
  CHECK(topk_source_bytes(1, -5, 3, &tb) && tb == 12);                   // one row: the stride is not read
  CHECK(!topk_source_bytes(2, 2, 3, &tb) && !topk_source_bytes(2, (int64_t)1 << 62, 1, &tb));
  CHECK(sizeof(TopKArgs) <= 1024);                                       // travels by value in the kernarg
}

static uint32_t rng_state = 12345u;
static uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state; }

// pattern 0: random bits (NaNs, infinities, denormals and ties by chance), 1: all scores equal, 2: strictly ascending (every
// tile replaces the whole carry), 3: few distinct values (long runs of ties across tiles)
static void select(int pattern, int bs, int k, int stride) {
  std::vector<uint32_t> bits((size_t)bs * stride, 0xdeadbeefu);
  for (int r = 0; r < bs; ++r) {
    uint32_t b;
    if (pattern == 0) b = rnd();
    else if (pattern == 1) b = 0x3f000000u;
    else if (pattern == 2) { float f = (float)r - 1500.0f; memcpy(&b, &f, 4); }
    else { float f = (float)(rnd() % 3) - 1.0f; memcpy(&b, &f, 4); }
    bits[(size_t)r * stride] = b;
  }
  std::vector<uint64_t> want((size_t)bs), got((size_t)k);
  for (int r = 0; r < bs; ++r) want[(size_t)r] = topk_key(bits[(size_t)r * stride], r);
  std::sort(want.begin(), want.end(), std::greater<uint64_t>());
  for (int r = 0; r + 1 < bs; ++r) CHECK(want[(size_t)r] > want[(size_t)r + 1]);      // the keys of a query are distinct
  topk_select_host(bits.data(), stride, bs, k, got.data());
  for (int i = 0; i < k; ++i) CHECK(got[(size_t)i] == want[(size_t)i]);
  for (int i = 0; i < k; ++i) CHECK(topk_key_row(got[(size_t)i]) < (uint32_t)bs);
  if (pattern == 1) for (int i = 0; i < k; ++i) CHECK(topk_key_row(got[(size_t)i]) == (uint32_t)i);              // ties: by the lower row
  if (pattern == 2) for (int i = 0; i < k; ++i) CHECK(topk_key_row(got[(size_t)i]) == (uint32_t)(bs - 1 - i));   // the last rows first
}

int main() {
  order();
  int pattern, bs, k, stride;
  g_case = 0;
  while (scanf("%d %d %d %d", &pattern, &bs, &k, &stride) == 4) {
    if (bs < 1 || k < 1 || k > bs || k > DRS_TOPK_MAX || stride < 1) { printf("case %d: bad\n", g_case); return 2; }
    select(pattern, bs, k, stride);
    ++g_case;
  }
  printf("%d cases, %d failures\n", g_case, fails);
  return fails != 0;
}
"""

BS = [1, 2, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 3000]


def select_cases():
    cases = []
    for pattern in (0, 1, 2, 3):
        for bs in BS:
            for k in sorted(set(min(k, bs) for k in (1, 2, 10, 64, min(bs, 1024)))):
                cases.append((pattern, bs, k, 3 if bs in (257, 1025) else 1))
    return cases


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]],
                         ids=["plain", "sanitized"])
def test_the_order_and_the_tiled_selection_against_std_sort(tmp_path, flags):
    """csrc/topk_plan.h on its own, in a host program with its own main -- built plain, and under the address and
    undefined-behaviour sanitizers -- and run directly: the functions the kernel calls, and the selection step by step"""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a C++ compiler builds the host program"
    src = tmp_path / "topk_main.cpp"
    src.write_text(PLAN_MAIN)
    exe = tmp_path / "topk_main"
    subprocess.run([cxx, "-std=c++17"] + flags + ["-Wall", "-Werror", "-I", os.path.join(ROOT, "deeprecsys_amd", "csrc"), str(src),
                                                  "-o", str(exe)], check=True, capture_output=True, text=True)
    cases = select_cases()
    assert {c[1] for c in cases} == set(BS) and any(c[2] == 1024 for c in cases) and any(c[1] == 3000 and c[2] == 1024 for c in cases)
    text = "".join("%d %d %d %d\n" % c for c in cases)
    r = subprocess.run([str(exe)], input=text, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("%d cases, 0 failures" % len(cases)), r.stdout


def test_the_kernel_and_the_entry_points_use_the_plan():
    def read(name):
        return open(os.path.join(ROOT, "deeprecsys_amd", "csrc", name)).read()
    plan = read("topk_plan.h")
    for word in ("kTopKThreads = 256", "kTopKTile = 1024", "DRS_TOPK_MAX 1024", "DRS_OUT_HD inline uint32_t topk_sortable",
                 "DRS_OUT_HD inline uint64_t topk_key", "struct TopKArgs", "topk_select_host(", "NOT the fast path"):
        assert word in plan, word
    assert "hip" not in plan.replace("topk_pass.hip", "").replace("__HIPCC__", "").lower()      # no HIP dependency
    kernel = read("topk_pass.hip")
    for word in ("topk_key(", "topk_key_row(", "topk_steps(", "topk_tile_rows(", "kOutPassNaN", "kTopKQueries == DRS_MAX_COALESCE",
                 "__launch_bounds__(kTopKThreads)", "ulonglong2"):
        assert word in kernel, word
    assert "asm" not in kernel
    eng_src = read("engine_device_topk.hip")
    for word in ("check_device_set(", "enqueue_device_set(", "device_range_fault(", "extents_overlap(", "topk_k_in_range(",
                 "hipEventRecord(s.ev_out", "hipStreamWaitEvent(caller", "s.out_pass = true", "topk_pass[%d x %d]"):
        assert word in eng_src, word
    for name in os.listdir(os.path.join(ROOT, "deeprecsys_amd", "csrc")):
        if name.endswith(".hip"):
            assert len(read(name).splitlines()) < 1500, name


# ------------------------------------------------------------------------------------------------
# the wrapper's own checks
def test_device_top_refuses_what_the_tensors_show_without_touching_the_engine():
    import torch
    from deeprecsys_amd import dlrm_s_hip as M

    def refused(pair, word, k=4, n_out=2):
        with pytest.raises(ValueError) as err:
            M.device_top(pair, k, n_out, 0, 3)
        assert "out 3" in str(err.value) and word in str(err.value), (word, str(err.value))
    idx, sc = torch.zeros(4, dtype=torch.int32), torch.zeros((4, 2))
    refused((idx.to(torch.int64), sc), "idx must be torch.int32")              # wrong dtype
    refused((idx, sc.to(torch.float64)), "scores must be torch.float32")
    refused((torch.zeros(5, dtype=torch.int32), sc), "idx must be [4]")        # wrong shape
    refused((idx, torch.zeros((4, 3))), "scores must be [4, 2]")
    refused((idx, torch.zeros(8)), "scores must be [4, 2]")
    refused((torch.zeros(8, dtype=torch.int32)[::2], sc), "idx must be contiguous")
    refused((idx, torch.zeros((4, 4))[:, :2]), "scores must be contiguous")    # a column block: the rows go out contiguous
    refused((idx.numpy(), sc), "idx must be a torch tensor")
    refused((idx, None), "scores must be a torch tensor")
    refused(idx, "pair")
    refused((idx, sc, sc), "pair")
    refused((idx, sc), "idx lives on cpu")                                     # CPU tensors: everything else about them is right

    net = object.__new__(M._HipNet)

    class NoEngine(object):
        T, m_den, device, n_out = 3, 8, 0, 2

        def __getattr__(self, name):
            raise AssertionError("the engine was touched: " + name)
    net.engine = NoEngine()
    ids, lengths, fc = torch.zeros((3, 8), dtype=torch.int64), torch.full((3, 4), 2, dtype=torch.int32), torch.zeros((4, 8))
    req = [(ids, lengths, fc, 4)]
    for kw, word in ((dict(k=-1), "k:"), (dict(k=1025), "k:"), (dict(k=2, col=2), "col:"), (dict(k=2, col=-1), "col:"),
                     (dict(k=2, out=[(idx, sc), (idx, sc)]), "output pairs"), (dict(k=2), "ids lives on cpu")):
        with pytest.raises(ValueError) as err:
            net.run_queued_device_topk_multi(req, **kw)
        assert word in str(err.value), (kw, str(err.value))
    for cls in M.WRAPPERS.values():
        assert callable(getattr(cls, "run_queues_device_topk_multi")) and callable(getattr(cls, "finish_device"))
    assert len(M.WRAPPERS) == 6
    assert callable(N.Engine.run_queues_device_topk_multi_async) and callable(N.Engine.topk_rows)
    e = object.__new__(N.Engine)                   # the binding's own count check comes before the library
    with pytest.raises(ValueError):
        e.run_queues_device_topk_multi_async([(1, 0, 0, 1, 1, 0, 1, -1)], [1, 1], 0, [(0, 0)])
    with pytest.raises(ValueError):
        e.run_queues_device_topk_multi_async([(1, 0, 0, 1, 1, 0, 1, -1)], [1], 0, [])
    e._h = None


def test_the_documents_and_the_makefile_name_the_new_files_and_calls():
    def read(*p):
        return open(os.path.join(ROOT, *p)).read()
    integ = read("INTEGRATION.md")
    for word in ("drs_run_queues_device_topk_multi_async", "run_queues_device_topk_multi", "drs_device_topk.h", "torch.topk(outs[0][:, 0], 10)"):
        assert word in integ, word
    assert "run_queues_device_topk_multi" in read("README.md") and "drs_device_topk.h" in read("README.md")
    design = read("DESIGN.md")
    for word in ("drs_run_queues_device_topk_multi_async", "topk_pass.hip", "topk_plan.h", "ascending", "host-output form"):
        assert word in design, word
    mk = read("deeprecsys_amd", "csrc", "Makefile")
    for word in ("topk_pass.hip", "engine_device_topk.hip", "topk_plan.h", "drs_device_topk.h"):
        assert word in mk, word
    assert os.path.exists(os.path.join(ROOT, "tools", "device_topk_cost.py"))
    assert "topk_pass[" in read("profiles", "r30_device_topk.md")
