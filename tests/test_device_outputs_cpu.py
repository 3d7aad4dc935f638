"""CPU side of the device-output launch sets (include/drs_device_outputs.h): the symbols and the header, the frozen symbol
list, the output pass's planner and owner lookup (deeprecsys_amd/csrc/output_plan.h) walked by a host program over every set of
the catalogue of tests/device_inputs_ref.py, the extent and overlap arithmetic of the refusals at their edges, a numpy
restatement of the pass, the wrapper's argument checks, and the documents."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from deeprecsys_amd import _native as N
from tests import device_inputs_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["drs_run_queues_device_io_multi_async", "drs_run_queues_device_io_async"]
NAN_BITS = 0x7FC00000


def test_the_library_exports_both_symbols():
    L = N.lib()
    assert [n for n, _, _ in N.DEVICE_OUTPUT_SYMBOLS] == NAMES
    for name, res, args in N.DEVICE_OUTPUT_SYMBOLS:
        fn = getattr(L, name)
        assert fn.restype is res and fn.argtypes == args, name
    multi, one = [a for _, _, a in N.DEVICE_OUTPUT_SYMBOLS]
    # the first eleven (ten) arguments are the device-input call's; then d_out, out_row_stride, stream, ordered
    assert multi[:11] == N.DEVICE_INPUT_SYMBOLS[0][2] and one[:10] == N.DEVICE_INPUT_SYMBOLS[1][2]
    assert multi[11:] == [N.C.POINTER(N.C.c_void_p), N._i64p, N.C.c_void_p, N.C.c_int32]
    assert one[10:] == [N.C.c_void_p, N.C.c_int64, N.C.c_void_p, N.C.c_int32]


def test_the_header_declares_both_calls_and_the_abi_version_stays():
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "a C compiler preprocesses the header"
    text = subprocess.run([cc, "-E", os.path.join(ROOT, "include", "drs.h")], capture_output=True, text=True, check=True).stdout
    flat = re.sub(r"\s+", " ", text)
    w, p = r"\s*\w+\s*", r"\s*\*\s*"
    multi = (r"int32_t drs_run_queues_device_io_multi_async\s*\(\s*drs_handle" + w + r", int32_t" + w + r", int32_t" + w +
             r", const int32_t" + p + r"\w+\s*, const float" + p + r"const" + p + r"\w+\s*, const int64_t" + p + r"const" + p +
             r"\w+\s*, const int64_t" + p + r"\w+\s*, const int64_t" + p + r"\w+\s*, const int32_t" + p + r"const" + p +
             r"\w+\s*, const int64_t" + p + r"\w+\s*, const int32_t" + p + r"\w+\s*, float" + p + r"const" + p +
             r"\w+\s*, const int64_t" + p + r"\w+\s*, void" + p + r"\w+\s*, int32_t" + w + r"\)\s*;")
    one = (r"int32_t drs_run_queues_device_io_async\s*\(\s*drs_handle" + w + r", int32_t" + w + r", int32_t" + w + r", const float" + p +
           r"\w+\s*, const int64_t" + p + r"\w+\s*, int64_t" + w + r", int64_t" + w + r", const int32_t" + p + r"\w+\s*, int64_t" + w +
           r", int32_t" + w + r", float" + p + r"\w+\s*, int64_t" + w + r", void" + p + r"\w+\s*, int32_t" + w + r"\)\s*;")
    assert re.search(multi, flat), "drs_run_queues_device_io_multi_async"
    assert re.search(one, flat), "drs_run_queues_device_io_async"
    hdr = open(os.path.join(ROOT, "include", "drs.h")).read()
    assert "#define DRS_ABI_VERSION 5" in hdr and '#include "drs_device_outputs.h"' in hdr
    assert hdr.index('#include "drs_device_inputs.h"') < hdr.index('#include "drs_device_outputs.h"') < hdr.rindex("#ifdef __cplusplus")
    assert not any(n in hdr for n in NAMES)                    # declared in drs_device_outputs.h alone
    sat = open(os.path.join(ROOT, "include", "drs_device_outputs.h")).read()
    for word in ("Ordering", "Lifetime", "Written", "NaN", "0x7fc00000", "overlap", "Overlap", "responsibility", "ordered == 0",
                 "ordered == 1", "null stream", "drs_wait", "hipMemGetAddressRange", "DRS_ERR_BAD_ARG"):
        assert word in sat, word


def test_the_frozen_symbol_list_is_unchanged(cpu_abi):
    names = [n for n, _, _ in N.SYMBOLS]
    assert len(names) == 40 and len(set(names)) == 40
    assert not set(names) & set(NAMES)
    assert N.lib().drs_abi_version() == 5
    # the CPU restatement binds the frozen list (the fixture has just done so) and knows nothing of the new names
    assert cpu_abi.drs_abi_version() == 5
    for name in NAMES:
        assert not hasattr(cpu_abi, name)


# ------------------------------------------------------------------------------------------------
# the planner and the owner lookup, the extents and the overlap predicate: output_plan.h alone in a host program
PLAN_MAIN = r"""
#include "output_plan.h"
#include <stdio.h>
#include <string.h>
#include <vector>
using namespace drs;
static int fails = 0;
#define CHECK(c) do { if (!(c)) { if (fails < 20) printf("line %d (case %d): %s\n", __LINE__, g_case, #c); ++fails; } } while (0)
static int g_case = -1;

// one set, laid out as the engine lays it out (64-row virtual blocks per query, empty queries take none and no entry)
static void walk(int n_out, int extra, int n, const int* bs) {
  OutPassArgs a;
  memset(&a, 0, sizeof a);
  a.n_out = n_out;
  int64_t v = 0, total = 0;
  int nonempty = 0;
  for (int i = 0; i < n; ++i) {
    if (bs[i] == 0) continue;
    OutQuery& q = a.q[a.n_q++];
    q.dst = nullptr; q.stride = bs[i] > 1 ? n_out + extra : 0; q.vstart = (int32_t)v; q.bs = bs[i];
    v += (bs[i] + 63) / 64 * 64;
    total += (int64_t)bs[i] * n_out;
    ++nonempty;
  }
  const int64_t grid = plan_output_pass(a);
  CHECK(a.n_q == nonempty);                                  // an empty query has no entry: it owns nothing
  int64_t want_grid = 0;
  for (int i = 0; i < a.n_q; ++i) {
    CHECK(a.blk0[i] == want_grid);
    want_grid += ((int64_t)a.q[i].bs * n_out + kOutPassChunk - 1) / kOutPassChunk;
  }
  CHECK(grid == want_grid && a.blk0[a.n_q] == grid);
  CHECK((total == 0) == (grid == 0));
  // every (block, round, lane): what it owns
  std::vector<std::vector<int>> dst_hits(a.n_q);
  for (int i = 0; i < a.n_q; ++i) dst_hits[i].assign((size_t)((a.q[i].bs - 1) * a.q[i].stride + n_out), 0);
  std::vector<int> src_hits((size_t)(v * n_out), 0);
  int64_t owned = 0;
  for (int b = 0; b < grid; ++b) {
    const int qi = out_owner(a, b);
    CHECK(qi >= 0 && qi < a.n_q && b >= a.blk0[qi] && b < a.blk0[qi + 1]);
    for (int k = 0; k < kOutPassPerLane; ++k)
      for (int t = 0; t < kOutPassThreads; ++t) {
        const int64_t e = out_element(a, qi, b, k, t);
        if (e < 0) continue;
        ++owned;
        CHECK(e < (int64_t)a.q[qi].bs * n_out);
        const int64_t si = out_src_index(a, qi, e), di = out_dst_index(a, qi, e);
        const int64_t r = e / n_out, c = e % n_out;
        CHECK(si == (a.q[qi].vstart + r) * n_out + c && si >= 0 && si < (int64_t)src_hits.size());
        CHECK(di == r * a.q[qi].stride + c && di >= 0 && di < (int64_t)dst_hits[qi].size());
        if (si >= 0 && si < (int64_t)src_hits.size()) ++src_hits[(size_t)si];
        if (di >= 0 && di < (int64_t)dst_hits[qi].size()) ++dst_hits[qi][(size_t)di];
      }
  }
  CHECK(owned == total);                                     // nothing outside is owned ...
  for (int i = 0; i < a.n_q; ++i)                            // ... every element exactly once, the gap columns never
    for (size_t d = 0; d < dst_hits[i].size(); ++d) {
      const int64_t stride = a.q[i].bs > 1 ? a.q[i].stride : n_out;
      const bool inside = (int64_t)(d % (size_t)stride) < n_out;
      CHECK(dst_hits[i][d] == (inside ? 1 : 0));
    }
  for (int i = 0; i < a.n_q; ++i)                            // the source: the query's own rows once, the padding rows never
    for (int64_t r = 0; r < (a.q[i].bs + 63) / 64 * 64; ++r)
      for (int c = 0; c < n_out; ++c)
        CHECK(src_hits[(size_t)((a.q[i].vstart + r) * n_out + c)] == (r < a.q[i].bs ? 1 : 0));
}

static void edges() {
  uint64_t b = 1;
  // (bs - 1) * stride + n_out floats
  CHECK(output_extent_bytes(600, 1, 1, &b) && b == 2400);
  CHECK(output_extent_bytes(600, 8, 3, &b) && b == (599 * 8 + 3) * 4);
  CHECK(output_extent_bytes(0, -5, 3, &b) && b == 0);                    // an empty query: nothing is written
  CHECK(output_extent_bytes(1, -5, 3, &b) && b == 12);                   // one row: the stride is not read
  CHECK(output_extent_bytes(1, (int64_t)1 << 62, 3, &b) && b == 12);
  CHECK(output_extent_bytes(2, 3, 3, &b) && b == 24);                    // stride == n_out: the rows touch
  CHECK(!output_extent_bytes(2, 2, 3, &b) && b == 0);                    // stride n_out - 1: the rows overlap
  CHECK(!output_extent_bytes(2, 0, 3, &b));
  CHECK(!output_extent_bytes(2, -3, 3, &b));
  CHECK(!output_extent_bytes(-1, 3, 3, &b));
  CHECK(!output_extent_bytes(2, 3, 0, &b));
  // a stride that would wrap a 64-bit byte count is refused by the arithmetic: 2^62 floats * 4 bytes
  CHECK(!output_extent_bytes(2, (int64_t)1 << 62, 1, &b) && b == 0);
  CHECK(!output_extent_bytes(600, (int64_t)1 << 62, 3, &b));
  CHECK(!output_extent_bytes(3, INT64_MAX, 1, &b));
  // the limit itself: 2^60 bytes pass, one float more does not
  CHECK(output_extent_bytes(2, ((int64_t)1 << 58) - 4, 4, &b) && b == (uint64_t)1 << 60);
  CHECK(!output_extent_bytes(2, ((int64_t)1 << 58) - 3, 4, &b));
  // overlap: touching ranges are legal, one shared byte is not
  CHECK(!extents_overlap(1000, 100, 1100, 100));
  CHECK(!extents_overlap(1100, 100, 1000, 100));
  CHECK(extents_overlap(1000, 101, 1100, 100));
  CHECK(extents_overlap(1100, 100, 1000, 101));
  CHECK(extents_overlap(1000, 100, 1000, 100));                          // the same array twice
  CHECK(extents_overlap(1000, 100, 1040, 8) && extents_overlap(1040, 8, 1000, 100));   // one inside the other
  CHECK(extents_overlap(1000, 100, 1099, 1) && !extents_overlap(1000, 100, 1100, 1));
  CHECK(!extents_overlap(1000, 0, 1000, 100) && !extents_overlap(1000, 100, 1050, 0));  // an empty output shares nothing
  CHECK(!extents_overlap(0, 0, 0, 0));
  CHECK(!extents_overlap(UINT64_MAX - 99, 100, 0, 100));                 // p + bytes would wrap: no sum is formed
  CHECK(extents_overlap(UINT64_MAX - 99, 100, UINT64_MAX - 10, 4));
}

int main() {
  edges();
  int n_out, extra, n, bs[64];
  g_case = 0;
  while (scanf("%d %d %d", &n_out, &extra, &n) == 3) {
    if (n < 0 || n > kOutPassQueries) { printf("case %d: n=%d\n", g_case, n); return 2; }
    for (int i = 0; i < n; ++i) if (scanf("%d", &bs[i]) != 1) return 2;
    walk(n_out, extra, n, bs);
    ++g_case;
  }
  printf("%d cases, %d failures\n", g_case, fails);
  return fails != 0;
}
"""


def plan_cases():
    cases = []
    for qs in R.GOOD.values():
        for n_out in (1, 3):
            for extra in (0, 5):
                cases.append((n_out, extra, [q.bs for q in qs]))
    # the largest set the base engine takes, and the same rows at MT-WnD's width: the grid arithmetic
    for n_out in (1, 3, 1000):
        cases.append((n_out, 0, [600] * 16))
    cases.append((3, 5, [0, 0, 0]))
    cases.append((1, 0, [1]))
    return cases


def test_every_output_element_is_owned_by_exactly_one_lane_and_the_refusal_arithmetic(tmp_path):
    """csrc/output_plan.h on its own, in a host program under the address and undefined-behaviour sanitizers: the functions
    the kernel calls, walked over every (block, round, lane) of every set of the catalogue"""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a C++ compiler builds the host program"
    src = tmp_path / "plan_main.cpp"
    src.write_text(PLAN_MAIN)
    exe = tmp_path / "plan_main"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Werror",
                    "-I", os.path.join(ROOT, "deeprecsys_amd", "csrc"), str(src), "-o", str(exe)],
                   check=True, capture_output=True, text=True)
    cases = plan_cases()
    assert any(0 in bs for _, _, bs in cases) and any(len(bs) == 16 for _, _, bs in cases)
    text = "".join("%d %d %d %s\n" % (n_out, extra, len(bs), " ".join(map(str, bs))) for n_out, extra, bs in cases)
    r = subprocess.run([str(exe)], input=text, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("%d cases, 0 failures" % len(cases)), r.stdout
    # the entry point uses them: the output extent check lives in the new file, the pointer check is the inputs'
    eng_src = open(os.path.join(ROOT, "deeprecsys_amd", "csrc", "engine_device_outputs.hip")).read()
    for word in ("output_extent_bytes(", "extents_overlap(", "device_range_fault(", "plan_output_pass(", "hipEventRecord(s.ev_out",
                 "hipStreamWaitEvent(caller"):
        assert word in eng_src, word
    kernel = open(os.path.join(ROOT, "deeprecsys_amd", "csrc", "output_pass.hip")).read()
    for word in ("out_owner(", "out_element(", "out_src_index(", "out_dst_index(", "kOutPassNaN"):
        assert word in kernel, word
    assert "asm" not in kernel
    for name in os.listdir(os.path.join(ROOT, "deeprecsys_amd", "csrc")):
        if name.endswith(".hip"):
            assert len(open(os.path.join(ROOT, "deeprecsys_amd", "csrc", name)).read().splitlines()) < 1500, name


# ------------------------------------------------------------------------------------------------
# the pass restated with numpy
def output_pass(buf, n_out, bss, outs, strides, err_word):
    """The device output pass on one set, restated: buf is the slot's [Mv, n_out] buffer (query i at virtual row vstart_i,
    64-row blocks per non-empty query), outs[i] a flat float32 array that receives query i's rows `strides[i]` floats apart.
    A non-zero error word: the quiet NaN 0x7fc00000 in place of every score."""
    v = 0
    for bs, out, stride in zip(bss, outs, strides):
        if bs == 0:
            continue
        rows = buf[v:v + bs].view(np.uint32)
        if err_word:
            rows = np.full((bs, n_out), NAN_BITS, np.uint32)
        for r in range(bs):
            out.view(np.uint32)[r * stride:r * stride + n_out] = rows[r]
        v += (bs + 63) // 64 * 64
    return v


@pytest.mark.parametrize("name", list(R.GOOD))
def test_the_restatement_packs_every_good_set_by_its_virtual_rows(name):
    qs = R.GOOD[name]
    bss = [q.bs for q in qs]
    for n_out, extra in ((1, 0), (3, 0), (3, 5)):
        Mv = sum((b + 63) // 64 * 64 for b in bss)
        rng = np.random.RandomState(7)
        buf = rng.uniform(-1, 1, (Mv, n_out)).astype(np.float32)
        stride = n_out + extra
        sentinel = np.float32(-77.0)
        outs = [np.full(max((b - 1) * stride + n_out, 0) if b else 4, sentinel, np.float32) for b in bss]
        assert output_pass(buf, n_out, bss, outs, [stride] * len(bss), 0) == Mv
        # pinned against slicing by hand
        v = 0
        for b, out in zip(bss, outs):
            if b == 0:
                assert (out == sentinel).all()
                continue
            padded = np.full((b, stride), sentinel, np.float32)
            padded.reshape(-1)[:out.size] = out
            assert np.array_equal(padded[:, :n_out].view(np.uint32), buf[v:v + b].view(np.uint32))
            gaps = np.ones(out.size, bool)
            for r in range(b):
                gaps[r * stride:r * stride + n_out] = False
            assert (out[gaps] == sentinel).all() and gaps.sum() == (b - 1) * extra
            v += (b + 63) // 64 * 64
        # an error word: every element of every query the quiet NaN, the gaps and the empty queries untouched
        outs = [np.full(max((b - 1) * stride + n_out, 0) if b else 4, sentinel, np.float32) for b in bss]
        output_pass(buf, n_out, bss, outs, [stride] * len(bss), 4)
        for b, out in zip(bss, outs):
            if b == 0:
                assert (out == sentinel).all()
                continue
            written = np.zeros(out.size, bool)
            for r in range(b):
                written[r * stride:r * stride + n_out] = True
            assert (out.view(np.uint32)[written] == NAN_BITS).all() and np.isnan(out[written]).all()
            assert (out[~written] == sentinel).all()


# ------------------------------------------------------------------------------------------------
# the wrapper's own checks
def test_device_out_refuses_what_the_tensor_shows_without_touching_the_engine():
    import torch
    from deeprecsys_amd import dlrm_s_hip as M

    def refused(t, word, bs=4, n_out=2):
        with pytest.raises(ValueError) as err:
            M.device_out(t, bs, n_out, 0, 3)
        assert "out 3" in str(err.value) and word in str(err.value), (word, str(err.value))
    good = torch.zeros((4, 2))
    refused(good.to(torch.float64), "float32")                         # wrong dtype
    refused(good.to(torch.int32), "float32")
    refused(torch.zeros((5, 2)), "[4, 2]")                             # wrong shape: rows, columns, rank
    refused(torch.zeros((4, 3)), "[4, 2]")
    refused(torch.zeros(8), "[4, 2]")
    refused(torch.zeros((4, 4))[:, ::2], "contiguous")                 # last dimension not contiguous
    refused(torch.zeros((2, 4)).t(), "contiguous")
    refused(good.numpy(), "torch tensor")                              # not a tensor
    refused(None, "torch tensor")
    refused(good, "cuda:0")                                            # a CPU tensor: everything else about it is right
    refused(torch.zeros((4, 6))[:, 2:4], "cuda:0")                     # a column block is fine as a layout; this one lives on the CPU

    class Backwards(torch.Tensor):                                     # torch itself builds no negative stride: a tensor that reports one
        def stride(self, dim=None):
            return (-2, 1) if dim is None else (-2, 1)[dim]
    refused(good.as_subclass(Backwards), "negative row stride")

    # a net without an engine: the checks come before anything touches it
    net = object.__new__(M._HipNet)

    class NoEngine(object):
        T, m_den, device, n_out = 3, 8, 0, 2

        def __getattr__(self, name):
            raise AssertionError("the engine was touched: " + name)
    net.engine = NoEngine()
    ids, lengths, fc = torch.zeros((3, 8), dtype=torch.int64), torch.full((3, 4), 2, dtype=torch.int32), torch.zeros((4, 8))
    with pytest.raises(ValueError):
        net.run_queued_device_io_multi([(ids, lengths, fc, 4)])                      # CPU request tensors
    with pytest.raises(ValueError):
        net.run_queued_device_io_multi([(ids, lengths, fc, 4)], out=[good, good])    # one output per request
    for cls in M.WRAPPERS.values():
        assert callable(getattr(cls, "run_queues_device_io_multi")) and callable(getattr(cls, "finish_device"))
    assert len(M.WRAPPERS) == 6
    assert callable(N.Engine.run_queues_device_io_multi_async)


def test_the_documents_and_the_makefile_name_the_new_files_and_calls():
    def read(*p):
        return open(os.path.join(ROOT, *p)).read()
    integ = read("INTEGRATION.md")
    for word in ("drs_run_queues_device_io_multi_async", "run_queues_device_io_multi", "finish_device", "drs_device_outputs.h"):
        assert word in integ, word
    assert "run_queues_device_io_multi" in read("README.md") and "drs_device_outputs.h" in read("README.md")
    design = read("DESIGN.md")
    for word in ("drs_run_queues_device_io_multi_async", "output_pass.hip", "output_plan.h", "ev_out", "0x7fc00000", "hipGraph"):
        assert word in design, word
    mk = read("deeprecsys_amd", "csrc", "Makefile")
    for word in ("output_pass.hip", "engine_device_outputs.hip", "output_plan.h", "drs_device_outputs.h"):
        assert word in mk, word
    assert os.path.exists(os.path.join(ROOT, "tools", "device_outputs_cost.py"))
    assert "output_pass[" in read("profiles", "r27_device_outputs.md")
