"""CPU side of per-sample weights on the device-array path (include/drs_device_weights.h): the symbol and the header, the
frozen symbol lists, the wrapper's `device_weights` check, and the weight planner (deeprecsys_amd/csrc/weight_plan.h) walked by
a stand-alone host program, with and without the address and undefined-behaviour sanitizers: chunk counts at the chunk's
edges, head and tail peels at every misalignment of a 16-byte line, and the workgroup numbering of a mixed 16-query set."""
import os
import re
import shutil
import subprocess

import pytest

from deeprecsys_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "drs_run_queues_device_weighted_multi_async"


def test_the_library_exports_the_symbol():
    L = N.lib()
    assert [n for n, _, _ in N.DEVICE_WEIGHT_SYMBOLS] == [NAME]
    name, res, args = N.DEVICE_WEIGHT_SYMBOLS[0]
    fn = getattr(L, name)
    assert fn.restype is res and fn.argtypes == args
    # the device-input call's eleven arguments, then d_weights, wgt_row_stride, wgt_dtype, then the output call's last four
    assert args[:11] == N.DEVICE_INPUT_SYMBOLS[0][2]
    assert args[11:14] == [N.C.POINTER(N.C.c_void_p), N._i64p, N._i32p]
    assert args[14:] == N.DEVICE_OUTPUT_SYMBOLS[0][2][11:] and len(args) == 18
    assert (N.WEIGHT_FP32, N.WEIGHT_FP16, N.WEIGHT_BF16) == (N.TABLE_FP32, N.TABLE_FP16, N.TABLE_BF16) == (0, 1, 2)


def test_the_header_declares_the_call_and_the_abi_version_stays():
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "a C compiler preprocesses the header"
    text = subprocess.run([cc, "-E", os.path.join(ROOT, "include", "drs.h")], capture_output=True, text=True, check=True).stdout
    flat = re.sub(r"\s+", " ", text)
    w, p = r"\s*\w+\s*", r"\s*\*\s*"
    proto = (r"int32_t " + NAME + r"\s*\(\s*drs_handle" + w + r", int32_t" + w + r", int32_t" + w +
             r", const int32_t" + p + r"\w+\s*, const float" + p + r"const" + p + r"\w+\s*, const int64_t" + p + r"const" + p +
             r"\w+\s*, const int64_t" + p + r"\w+\s*, const int64_t" + p + r"\w+\s*, const int32_t" + p + r"const" + p +
             r"\w+\s*, const int64_t" + p + r"\w+\s*, const int32_t" + p + r"\w+\s*, const void" + p + r"const" + p +
             r"\w+\s*, const int64_t" + p + r"\w+\s*, const int32_t" + p + r"\w+\s*, float" + p + r"const" + p +
             r"\w+\s*, const int64_t" + p + r"\w+\s*, void" + p + r"\w+\s*, int32_t" + w + r"\)\s*;")
    assert re.search(proto, flat), NAME
    hdr = open(os.path.join(ROOT, "include", "drs.h")).read()
    assert "#define DRS_ABI_VERSION 5" in hdr and '#include "drs_device_weights.h"' in hdr
    assert hdr.index('#include "drs_device_outputs.h"') < hdr.index('#include "drs_device_weights.h"') < hdr.rindex("#ifdef __cplusplus")
    assert NAME not in hdr                                      # declared in drs_device_weights.h alone
    sat = open(os.path.join(ROOT, "include", "drs_device_weights.h")).read()
    for word in ("Widening", "Summation", "Unweighted", "Non-finite", "DRS_ERR_UNSUPPORTED", "DRS_ERR_BAD_ARG", "DRS_ERR_OOM",
                 "sls_pool", "sls_weighted_flat", "wgt_row_stride", "ELEMENTS", "ordered == 0", "ordered == 1", "drs_wait"):
        assert word in sat, word
    # the sentences that said weights do not travel on the device path are gone
    assert "do not travel" not in open(os.path.join(ROOT, "include", "drs_device_inputs.h")).read()
    assert "drs_device_weights.h" in open(os.path.join(ROOT, "include", "drs_weights.h")).read()


def test_no_older_symbol_list_changed(cpu_abi):
    assert N.lib().drs_abi_version() == 5 and cpu_abi.drs_abi_version() == 5
    names = [n for n, _, _ in N.SYMBOLS]
    assert len(names) == 40 and len(set(names)) == 40 and NAME not in names
    assert [n for n, _, _ in N.WEIGHT_SYMBOLS] == ["drs_stage_batch_weights", "drs_sls_weighted"]
    assert [n for n, _, _ in N.FP8_SYMBOLS] == ["drs_table_fp8_exponent"]
    assert [n for n, _, _ in N.ROW_SYMBOLS] == ["drs_update_rows", "drs_get_rows"]
    assert [n for n, _, _ in N.DEVICE_INPUT_SYMBOLS] == ["drs_run_queues_device_multi_async", "drs_run_queues_device_async"]
    assert [n for n, _, _ in N.DEVICE_OUTPUT_SYMBOLS] == ["drs_run_queues_device_io_multi_async", "drs_run_queues_device_io_async"]
    assert len(N.DEVICE_INPUT_SYMBOLS[0][2]) == 11 and len(N.DEVICE_OUTPUT_SYMBOLS[0][2]) == 15
    # the CPU restatement binds the frozen list (the fixture has just done so) and knows nothing of the new name
    assert not hasattr(cpu_abi, NAME)


# ------------------------------------------------------------------------------------------------
# the wrapper's own check
def test_device_weights_takes_three_dtypes_and_slices_and_refuses_what_the_tensor_shows():
    import torch
    from deeprecsys_amd import dlrm_s_hip as M

    class OnGpu(torch.Tensor):                                         # a CPU tensor that reports the engine's GPU: the checks read
        @property                                                      # what the tensor shows and touch no device
        def device(self):
            return torch.device("cuda", 0)

    def gpu(t):
        return t.as_subclass(OnGpu)
    assert M.device_weights(None, 3, 8, 0) is None
    for dtype, code, size in ((torch.float32, 0, 4), (torch.float16, 1, 2), (torch.bfloat16, 2, 2)):
        t = torch.zeros((3, 8), dtype=dtype)
        assert M.device_weights(gpu(t), 3, 8, 0) == (t.data_ptr(), 8, code)
        wide = torch.zeros((3, 21), dtype=dtype)
        for c0 in range(8):                                            # a column slice: the pointer moves by elements, the row stride stays
            assert M.device_weights(gpu(wide[:, c0:c0 + 8]), 3, 8, 0) == (wide.data_ptr() + c0 * size, 21, code)
        assert M.device_weights(gpu(torch.zeros((6, 8), dtype=dtype)[::2]), 3, 8, 0)[1] == 16     # a row-strided slice
        assert M.device_weights(gpu(torch.zeros((1, 8), dtype=dtype)), 1, 8, 0)[1] == 8           # one table: the stride is the width

    def refused(t, word, T=3, n=8):
        with pytest.raises(ValueError) as err:
            M.device_weights(t, T, n, 0, 5)
        assert "request 5" in str(err.value) and "weights" in str(err.value) and word in str(err.value), (word, str(err.value))
    good = torch.zeros((3, 8))
    refused(gpu(good.to(torch.float64)), "float32")                    # wrong dtype
    refused(gpu(good.to(torch.int32)), "bfloat16")
    refused(good, "cuda:0")                                            # wrong device: a CPU tensor, everything else right
    refused(gpu(torch.zeros((2, 8))), "[3, 8]")                        # wrong shape: tables, indices, rank
    refused(gpu(torch.zeros((3, 9))), "[3, 8]")
    refused(gpu(torch.zeros(24)), "[3, 8]")
    refused(gpu(torch.zeros((3, 16))[:, ::2]), "contiguous")           # last dimension not contiguous
    refused(gpu(torch.zeros((8, 3)).t()), "contiguous")
    refused(good.numpy(), "torch tensor")                              # not a tensor

    class Backwards(OnGpu):
        def stride(self, dim=None):
            return (-8, 1) if dim is None else (-8, 1)[dim]
    refused(good.as_subclass(Backwards), "negative row stride")

    # a request's sixth element reaches the check before anything touches the engine; device_request still takes 4 or 5
    net = object.__new__(M._HipNet)

    class NoEngine(object):
        T, m_den, device, n_out = 3, 8, 0, 2

        def __getattr__(self, name):
            raise AssertionError("the engine was touched: " + name)
    net.engine = NoEngine()
    ids, lengths, fc = gpu(torch.zeros((3, 8), dtype=torch.int64)), gpu(torch.full((3, 4), 2, dtype=torch.int32)), gpu(torch.zeros((4, 8)))
    with pytest.raises(ValueError) as err:
        net._device_queries([(ids, lengths, fc, 4, 2, gpu(torch.zeros((3, 7))))])
    assert "weights must be [3, 8]" in str(err.value)
    with pytest.raises(ValueError) as err:
        net._device_queries([(ids, lengths, fc, 4, 2, None, None)])
    assert "fixed_len[, weights]" in str(err.value)
    with pytest.raises(ValueError):
        M.device_request((ids, lengths, fc, 4, 2, None), 3, 8, 0)
    for cls in M.WRAPPERS.values():
        assert callable(getattr(cls, "run_queues_device_multi")) and callable(getattr(cls, "run_queues_device_io_multi"))


# ------------------------------------------------------------------------------------------------
# the planner: weight_plan.h alone in a host program
PLAN_MAIN = r"""
#include "weight_plan.h"
#include <stdio.h>
#include <string.h>
#include <vector>
using namespace drs;
static int fails = 0;
#define CHECK(c) do { if (!(c)) { if (fails < 20) printf("line %d: %s\n", __LINE__, #c); ++fails; } } while (0)

// a row of n elements of `elem` bytes at byte offset `mis` of a 16-byte line: every element is moved exactly once -- the head
// and the tail one by one, the vectors in between by the chunk that owns them, each vector whole and 16-byte aligned
static void walk_row(int elem, int mis, int64_t n) {
  const int per = 16 / elem;
  const uint64_t addr = 0x10000 + (uint64_t)mis;
  const WgtPeel p = wgt_peel(addr, elem, n);
  CHECK(p.head >= 0 && p.head < per && p.tail >= 0 && p.tail < per && p.nvec >= 0);
  CHECK((int64_t)p.head + p.nvec * per + p.tail == (n > 0 ? n : 0));
  if (n > 0) {
    const int to_line = ((16 - mis) % 16) / elem;
    CHECK(p.head == (to_line < n ? to_line : (int)n));
    if (p.nvec > 0 || p.tail > 0) CHECK((addr + (uint64_t)p.head * elem) % 16 == 0);
  }
  std::vector<int> hits((size_t)(n > 0 ? n : 0), 0);
  for (int j = 0; j < p.head; ++j) ++hits[(size_t)j];
  for (int j = 0; j < p.tail; ++j) ++hits[(size_t)(n - p.tail + j)];
  const int32_t nb = wgt_chunks(n);
  CHECK(nb == (n > 0 ? (n + kInPassWgt - 1) / kInPassWgt : 0));
  int64_t last = 0;
  for (int c = 0; c < nb; ++c) {
    const int64_t v0 = wgt_vec0(c, elem), v1 = wgt_vec0(c + 1, elem);
    CHECK(v0 == last && v1 - v0 == kInPassWgt / per);
    last = v1;
    for (int64_t v = v0; v < v1 && v < p.nvec; ++v)
      for (int j = 0; j < per; ++j) {
        const int64_t e = p.head + v * per + j;
        CHECK(e >= 0 && e < n);
        if (e >= 0 && e < n) ++hits[(size_t)e];
      }
  }
  CHECK(nb == 0 || last >= p.nvec);                          // the chunks reach every vector, whatever the head
  for (size_t e = 0; e < hits.size(); ++e) CHECK(hits[e] == 1);
}

int main() {
  static_assert(kInPassWgt % (256 * 8) == 0, "whole 16-byte loads per lane for 2- and 4-byte elements");
  // chunk counts at the edges
  CHECK(wgt_chunks(-3) == 0 && wgt_chunks(0) == 0 && wgt_chunks(1) == 1 && wgt_chunks(kInPassWgt - 1) == 1);
  CHECK(wgt_chunks(kInPassWgt) == 1 && wgt_chunks(kInPassWgt + 1) == 2 && wgt_chunks(2 * (int64_t)kInPassWgt + 1) == 3);
  CHECK(wgt_chunks((int64_t)1 << 31) == (int32_t)(((int64_t)1 << 31) / kInPassWgt));
  // every element misalignment of a 16-byte line, both element sizes, counts around the peels and around the chunk
  const int64_t counts[] = {0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 33, kInPassWgt - 1, kInPassWgt, kInPassWgt + 1, kInPassWgt + 9,
                            2 * kInPassWgt - 1, 2 * kInPassWgt + 8};
  int rows = 0;
  for (int elem = 2; elem <= 4; elem += 2)
    for (int mis = 0; mis < 16; mis += elem)
      for (int64_t n : counts) { walk_row(elem, mis, n); ++rows; }
  // the peels themselves, spelt out: 4-byte elements 4, 8, 12 bytes into a line; 2-byte elements 2 and 14 bytes in
  WgtPeel p = wgt_peel(0x1004, 4, 10);  CHECK(p.head == 3 && p.nvec == 1 && p.tail == 3);
  p = wgt_peel(0x1008, 4, 10);          CHECK(p.head == 2 && p.nvec == 2 && p.tail == 0);
  p = wgt_peel(0x100c, 4, 2);           CHECK(p.head == 1 && p.nvec == 0 && p.tail == 1);
  p = wgt_peel(0x1000, 4, 3);           CHECK(p.head == 0 && p.nvec == 0 && p.tail == 3);
  p = wgt_peel(0x1002, 2, 5);           CHECK(p.head == 5 && p.nvec == 0 && p.tail == 0);    // the row ends before the line does
  p = wgt_peel(0x1002, 2, 24);          CHECK(p.head == 7 && p.nvec == 2 && p.tail == 1);
  p = wgt_peel(0x100e, 2, 24);          CHECK(p.head == 1 && p.nvec == 2 && p.tail == 7);
  p = wgt_peel(0x1004, 4, 0);           CHECK(p.head == 0 && p.nvec == 0 && p.tail == 0);

  // the extent the pointer check takes: (T - 1) * stride + n elements; an empty query reads nothing; 2^60 bytes is the limit
  uint64_t b = 1;
  CHECK(weight_extent_bytes(3, 21, 8, 4, &b) && b == (2 * 21 + 8) * 4);
  CHECK(weight_extent_bytes(3, 21, 8, 2, &b) && b == (2 * 21 + 8) * 2);
  CHECK(weight_extent_bytes(3, 0, 8, 2, &b) && b == 16);                 // stride 0: one row read three times
  CHECK(weight_extent_bytes(3, 1 << 20, 0, 4, &b) && b == 0);
  CHECK(!weight_extent_bytes(3, -1, 8, 4, &b) && b == 0);
  CHECK(!weight_extent_bytes(3, 21, 8, 8, &b) && !weight_extent_bytes(3, 21, 8, 1, &b));
  CHECK(!weight_extent_bytes(2, (int64_t)1 << 62, 8, 4, &b) && !weight_extent_bytes(3, INT64_MAX, 1, 2, &b));
  CHECK(weight_extent_bytes(2, ((int64_t)1 << 59) - 4, 4, 2, &b) && b == (uint64_t)1 << 60);
  CHECK(!weight_extent_bytes(2, ((int64_t)1 << 59) - 3, 4, 2, &b));

  // a 16-query set in which every second query is unweighted (nb_wgt 0) or empty (no index, no dense row: its lengths
  // items alone): T 3, the numbers of an unweighted set up to each query's dense items, the weights behind them
  const int T = 3;
  int32_t nb_idx[16], nb_dense[16], nb_wgt[16], wg0[kInPassWgtQueries + 1], plain[17];
  int64_t want = 0, want_plain = 0;
  for (int i = 0; i < 16; ++i) {
    const int64_t n_idx = (i % 4 == 3) ? 0 : 100 + 3000 * i;
    nb_idx[i] = (int32_t)((n_idx + 2047) / 2048);
    nb_dense[i] = n_idx ? 1 + i % 2 : 0;
    nb_wgt[i] = (i % 2 == 0) ? wgt_chunks(n_idx) : 0;
    plain[i] = (int32_t)want_plain;
    want_plain += T * (1 + nb_idx[i]) + nb_dense[i];
  }
  const int64_t grid = plan_weighted_grid(16, T, nb_idx, nb_dense, nb_wgt, wg0);
  int64_t shift = 0;
  for (int i = 0; i < 16; ++i) {
    CHECK(wg0[i] == want && wg0[i] == plain[i] + shift);       // the unweighted numbering, moved by the weight items in front
    want += T * (1 + nb_idx[i]) + nb_dense[i] + T * nb_wgt[i];
    shift += T * nb_wgt[i];
    if (i % 2) CHECK(nb_wgt[i] == 0);
  }
  CHECK(grid == want && wg0[16] == grid && grid == want_plain + shift && shift > 0);
  // the owner lookup the kernel makes, and the kind of every workgroup of every query
  for (int64_t wg = 0; wg < grid; ++wg) {
    int qi = 0;
    for (int i = 1; i < 16; ++i) qi = wg >= wg0[i] ? i : qi;
    CHECK(wg >= wg0[qi] && wg < wg0[qi + 1]);
    const int64_t r = wg - wg0[qi] - T - (int64_t)T * nb_idx[qi] - nb_dense[qi];
    if (r >= 0) CHECK(nb_wgt[qi] > 0 && r < (int64_t)T * nb_wgt[qi]);
  }
  // fewer queries: the entries behind them hold the grid; no weights at all: the unweighted grid; too many blocks: -1
  int32_t zero[16] = {0};
  CHECK(plan_weighted_grid(5, T, nb_idx, nb_dense, zero, wg0) == plain[5] && wg0[5] == plain[5] && wg0[16] == plain[5]);
  CHECK(plan_weighted_grid(0, T, nb_idx, nb_dense, nb_wgt, wg0) == 0 && wg0[0] == 0);
  int32_t huge[16];
  for (int i = 0; i < 16; ++i) huge[i] = INT32_MAX / 8;
  CHECK(plan_weighted_grid(16, T, huge, nb_dense, huge, wg0) == -1);
  printf("%d rows, %d failures\n", rows, fails);
  return fails != 0;
}
"""


@pytest.mark.parametrize("sanitize", [True, False])
def test_the_weight_planner_in_a_host_program(tmp_path, sanitize):
    """csrc/weight_plan.h on its own: the functions the kernel and the host side call"""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a C++ compiler builds the host program"
    src = tmp_path / "weight_plan_main.cpp"
    src.write_text(PLAN_MAIN)
    exe = tmp_path / "weight_plan_main"
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-O1", "-g"] if sanitize else ["-O2"]
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror"] + flags +
                   ["-I", os.path.join(ROOT, "deeprecsys_amd", "csrc"), str(src), "-o", str(exe)], check=True, capture_output=True, text=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert re.search(r"^\d+ rows, 0 failures$", r.stdout.strip().splitlines()[-1]), r.stdout
    # the header has no HIP include, and the kernel and the host side use its functions
    plan = open(os.path.join(ROOT, "deeprecsys_amd", "csrc", "weight_plan.h")).read()
    assert "hip/" not in plan and "#include <stdint.h>" in plan
    kernel = open(os.path.join(ROOT, "deeprecsys_amd", "csrc", "input_pass.hip")).read()
    for word in ("wgt_peel(", "wgt_vec0(", "wgt_chunks(", "plan_weighted_grid(", "input_pass_weighted_kernel", "_Float16"):
        assert word in kernel, word
    host = open(os.path.join(ROOT, "deeprecsys_amd", "csrc", "engine_device_inputs.hip")).read()
    for word in ("plan_input_pass_weighted(", "launch_input_pass_weighted(", "device_range_fault(e, w,", "b.weighted = w != nullptr"):
        assert word in host, word
    assert "b.weighted = false" in open(os.path.join(ROOT, "deeprecsys_amd", "csrc", "engine_inputs.hip")).read()


def test_the_documents_and_the_makefile_name_the_new_files_and_the_call():
    def read(*p):
        return open(os.path.join(ROOT, *p)).read()
    assert NAME in read("README.md") and "drs_device_weights.h" in read("README.md")
    design = read("DESIGN.md")
    for word in (NAME, "weight_plan.h", "input_pass_weighted_kernel", "kInPassWgt"):
        assert word in design, word
    mk = read("deeprecsys_amd", "csrc", "Makefile")
    assert "weight_plan.h" in mk and "drs_device_weights.h" in mk
    assert os.path.exists(os.path.join(ROOT, "tools", "device_weights_cost.py"))
    assert "input_pass_kernel" in read("profiles", "r28_device_weights.md")
