"""CPU side of the device-input launch sets (include/drs_device_inputs.h): the symbols and the header, the frozen symbol list,
the catalogue of tests/device_inputs_ref.py pinned against the host path of the CPU restatement of the ABI (code that predates
the device path), the numpy restatement of the input pass, the wrapper's argument checks, and the documents."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from deeprecsys_amd import _native as N
from tests import device_inputs_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["drs_run_queues_device_multi_async", "drs_run_queues_device_async"]


def test_the_library_exports_both_symbols():
    """the built library, loaded as the binding loads it (no GPU needed to dlopen it): lib() binds DEVICE_INPUT_SYMBOLS and
    raises when one is missing"""
    L = N.lib()
    assert [n for n, _, _ in N.DEVICE_INPUT_SYMBOLS] == NAMES
    for name, res, args in N.DEVICE_INPUT_SYMBOLS:
        fn = getattr(L, name)
        assert fn.restype is res and fn.argtypes == args, name


def test_the_header_declares_both_calls_and_the_abi_version_stays():
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "a C compiler preprocesses the header"
    text = subprocess.run([cc, "-E", os.path.join(ROOT, "include", "drs.h")], capture_output=True, text=True, check=True).stdout
    flat = re.sub(r"\s+", " ", text)
    w, p = r"\s*\w+\s*", r"\s*\*\s*"
    multi = (r"int32_t drs_run_queues_device_multi_async\s*\(\s*drs_handle" + w + r", int32_t" + w + r", int32_t" + w +
             r", const int32_t" + p + r"\w+\s*, const float" + p + r"const" + p + r"\w+\s*, const int64_t" + p + r"const" + p +
             r"\w+\s*, const int64_t" + p + r"\w+\s*, const int64_t" + p + r"\w+\s*, const int32_t" + p + r"const" + p +
             r"\w+\s*, const int64_t" + p + r"\w+\s*, const int32_t" + p + r"\w+\s*\)\s*;")
    one = (r"int32_t drs_run_queues_device_async\s*\(\s*drs_handle" + w + r", int32_t" + w + r", int32_t" + w + r", const float" + p +
           r"\w+\s*, const int64_t" + p + r"\w+\s*, int64_t" + w + r", int64_t" + w + r", const int32_t" + p + r"\w+\s*, int64_t" + w +
           r", int32_t" + w + r"\)\s*;")
    assert re.search(multi, flat), "drs_run_queues_device_multi_async"
    assert re.search(one, flat), "drs_run_queues_device_async"
    hdr = open(os.path.join(ROOT, "include", "drs.h")).read()
    assert "#define DRS_ABI_VERSION 5" in hdr and '#include "drs_device_inputs.h"' in hdr
    assert not any(n in hdr for n in NAMES)                    # declared in drs_device_inputs.h alone
    sat = open(os.path.join(ROOT, "include", "drs_device_inputs.h")).read()
    for word in ("Ordering", "Lifetime", "Read-only", "hipMemoryTypeDevice", "hipMemGetAddressRange", "DRS_ERR_LENGTHS_SUM",
                 "position"):
        assert word in sat, word


def test_the_frozen_symbol_list_is_unchanged(cpu_abi):
    names = [n for n, _, _ in N.SYMBOLS]
    assert len(names) == 40 and len(set(names)) == 40
    assert not set(names) & set(NAMES)
    # the CPU restatement binds the frozen list (the fixture has just done so) and knows nothing of the new names
    assert cpu_abi.drs_abi_version() == 5
    for name in NAMES:
        assert not hasattr(cpu_abi, name)


def test_the_catalogue_covers_the_edges_the_pass_has():
    singles = [qs[0] for name, qs in R.GOOD.items() if name.startswith("ragged_")]
    assert {q.bs for q in singles} == {1, 63, 64, 65, 255, 256, 257, 600}
    assert {q.ids.shape[1] for q in singles} >= {0, 1, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, R.CAP}
    assert any(q.bs >= 3 and (q.lengths[:, 0] == 0).all() and (q.lengths[:, -1] == 0).all() and (q.lengths[:, 1:-1] == 0).any()
               for q in singles)
    assert {q.fixed_len for qs in R.GOOD.values() for q in qs} >= {-1, 1, 2, 8}
    assert sorted({len(qs) for qs in R.GOOD.values()}) == [1, 2, 3, 4, 16]
    assert [q.bs for q in R.GOOD["empty_first_and_middle"]] == [0, 65, 0, 64]
    for qs in R.GOOD.values():
        for q in qs:
            assert q.ids.shape == (R.T, q.ids.shape[1]) and q.lengths.shape == (R.T, q.bs) and q.ids.shape[1] <= R.CAP
            assert q.fixed_len == -1 or q.fixed_len == R.host_uniform(q)
    # mixed promises: one ragged query against fixed lengths that merely differ
    assert [R.host_uniform(q) for q in R.GOOD["promises_8_8_ragged"]] == [8, 8, -1]
    assert [q.fixed_len for q in R.GOOD["promises_8_8_2"]] == [8, 8, 2]
    assert not R.same_forms(R.GOOD["unpromised_bs65_L1"]) and R.same_forms(R.GOOD["fixed_bs65_L1"])


@pytest.mark.parametrize("name", list(R.GOOD))
def test_the_restatement_equals_the_host_rules_on_every_good_set(name):
    """convert_table's rules, stated with numpy's own operations: the indices cast to int32, offsets = [0, cumsum(lengths)],
    the tail up to max_batch holding the total"""
    for q in R.GOOD[name]:
        idx32, off, code = R.input_pass(q.ids, q.lengths, R.ROWS, q.fixed_len)
        assert code == N.OK
        assert np.array_equal(idx32, q.ids.astype(np.int32)) and idx32.dtype == np.int32
        want = np.empty((R.T, R.MAX_BATCH + 1), np.int64)
        want[:, 0] = 0
        want[:, 1:q.bs + 1] = np.cumsum(q.lengths.astype(np.int64), axis=1)
        want[:, q.bs + 1:] = q.ids.shape[1]
        assert np.array_equal(off, want)
        assert np.all(off[:, q.bs] == q.ids.shape[1])


@pytest.mark.parametrize("name", list(R.BAD))
def test_what_the_pass_stores_for_a_bad_set_is_safe_to_gather_from(name):
    qs, code, _ = R.BAD[name]
    codes = []
    for q in qs:
        idx32, off, c = R.input_pass(q.ids, q.lengths, R.ROWS, q.fixed_len)
        codes.append(c)
        n = q.ids.shape[1]
        assert all(((idx32[t] >= 0) & (idx32[t] < R.ROWS[t])).all() for t in range(R.T))
        assert (np.diff(off.astype(np.int64), axis=1) >= 0).all() and off.min() >= 0 and off.max() <= n
    assert sorted(set(codes) - {N.OK}) == [code]          # exactly one kind of error in the set


@pytest.mark.parametrize("name", list(R.BAD))
def test_the_host_path_of_the_cpu_abi_gives_every_bad_set_its_code(cpu_abi, name):
    """pins the catalogue against code that predates the device path"""
    qs, _, host_code = R.BAD[name]
    eng = R.make_engine()
    try:
        if host_code == N.OK:
            eng.run_queues_multi_async(R.host_args(qs), slot=0)
            assert eng.wait(0, sum(q.bs for q in qs)).shape == (sum(q.bs for q in qs), 1)
        else:
            with pytest.raises(N.DrsError) as err:
                eng.run_queues_multi_async(R.host_args(qs), slot=0)
            assert err.value.code == host_code
    finally:
        eng.close()


def test_the_wrapper_refuses_what_the_tensors_show_without_touching_the_engine():
    import torch
    from deeprecsys_amd import dlrm_s_hip as M
    ids, lengths, fc = torch.zeros((3, 8), dtype=torch.int64), torch.full((3, 4), 2, dtype=torch.int32), torch.zeros((4, 8))

    def refused(req, word):
        with pytest.raises(ValueError) as err:
            M.device_request(req, 3, 8, 0)
        assert word in str(err.value), (word, str(err.value))
    refused((ids.to(torch.int32), lengths, fc, 4), "ids")                          # wrong dtype
    refused((ids, lengths.to(torch.int64), fc, 4), "lengths")
    refused((ids, lengths, fc.to(torch.float64), 4), "fc")
    refused((torch.zeros((3, 16), dtype=torch.int64)[:, ::2], lengths, fc, 4), "ids")     # last dimension not contiguous
    refused((ids, torch.zeros((4, 3), dtype=torch.int32).t(), fc, 4), "lengths")
    refused((ids, lengths, torch.zeros((4, 16))[:, :8], 4), "fc")                   # rows of fc not contiguous
    refused((ids[:2], lengths, fc, 4), "ids")                                       # T rows
    refused((ids, lengths, fc, 5), "lengths")                                       # bs columns
    refused((ids.numpy(), lengths, fc, 4), "ids")                                   # not a tensor
    refused((ids, lengths, fc, 4), "ids")                                           # a CPU tensor: the first argument checked
    refused((ids, lengths, fc), "request 0")
    # a net without an engine: the checks come before anything touches it
    net = object.__new__(M._HipNet)

    class NoEngine(object):
        T, m_den, device = 3, 8, 0

        def __getattr__(self, name):
            raise AssertionError("the engine was touched: " + name)
    net.engine = NoEngine()
    with pytest.raises(ValueError):
        net.run_queued_device_multi([(ids, lengths, fc, 4)])
    for cls in (M.DLRM_Wrapper, M.DIN_Wrapper, M.NCF_Wrapper):
        assert callable(getattr(cls, "run_queues_device_multi"))


EXTENT_MAIN = r"""
#include "input_extent.h"
#include <stdio.h>
using drs::input_extent_bytes;
using drs::extent_inside;
static int fails = 0;
#define CHECK(c) do { if (!(c)) { printf("line %d: %s\n", __LINE__, #c); ++fails; } } while (0)
int main() {
  uint64_t b = 1;
  // (T - 1) * stride + count elements
  CHECK(input_extent_bytes(3, 1000, 260, 8, &b) && b == (2 * 1000 + 260) * 8);
  CHECK(input_extent_bytes(3, 65, 65, 4, &b) && b == (2 * 65 + 65) * 4);
  CHECK(input_extent_bytes(1, 0, 520, 4, &b) && b == 2080);
  CHECK(input_extent_bytes(1, 123456, 7, 8, &b) && b == 56);            // one row: the stride does not count
  CHECK(input_extent_bytes(8, 0, 5, 8, &b) && b == 40);                 // stride 0: every row the same
  CHECK(input_extent_bytes(3, 1000, 0, 8, &b) && b == 0);               // nothing is read
  // negative arguments
  CHECK(!input_extent_bytes(3, -1, 5, 8, &b) && b == 0);
  CHECK(!input_extent_bytes(3, 5, -1, 8, &b));
  CHECK(!input_extent_bytes(0, 5, 5, 8, &b));
  // strides that would wrap a 64-bit byte count: 2 * 2^62 * 8, 4 * 2^62, 2^61 * 4 * 2 ...
  CHECK(!input_extent_bytes(3, (int64_t)1 << 62, 260, 8, &b) && b == 0);
  CHECK(!input_extent_bytes(5, (int64_t)1 << 62, 1, 8, &b));
  CHECK(!input_extent_bytes(3, (int64_t)1 << 61, 65, 4, &b));
  CHECK(!input_extent_bytes(2, INT64_MAX, 1, 8, &b));
  CHECK(!input_extent_bytes(1, 0, INT64_MAX, 4, &b));
  // the limit itself: 2^60 bytes pass, one element more does not
  CHECK(input_extent_bytes(2, ((int64_t)1 << 57) - 4, 4, 8, &b) && b == (uint64_t)1 << 60);
  CHECK(!input_extent_bytes(2, ((int64_t)1 << 57) - 3, 4, 8, &b));
  // inside an allocation [1000, 1000 + 4096)
  CHECK(extent_inside(1000, 4096, 1000, 4096));
  CHECK(!extent_inside(1000, 4097, 1000, 4096));
  CHECK(extent_inside(1000 + 4088, 8, 1000, 4096));
  CHECK(!extent_inside(1000 + 4089, 8, 1000, 4096));
  CHECK(extent_inside(1000 + 4096, 0, 1000, 4096));
  CHECK(!extent_inside(999, 1, 1000, 4096));
  CHECK(!extent_inside(1000 + 4097, 0, 1000, 4096));
  CHECK(!extent_inside(2000, UINT64_MAX - 100, 1000, 4096));           // p + bytes would wrap
  CHECK(extent_inside(UINT64_MAX - 4095, 4095, UINT64_MAX - 4095, 4095));
  printf("%d failures\n", fails);
  return fails != 0;
}
"""


def test_the_extent_arithmetic_of_the_pointer_check(tmp_path):
    """csrc/input_extent.h on its own, in a host program: the extents the pass reads, the refusals of negative and wrapping
    strides, and the comparison against an allocation -- the part of the pointer check no GPU test may show by overrunning"""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a C++ compiler builds the host program"
    src = tmp_path / "extent_main.cpp"
    src.write_text(EXTENT_MAIN)
    exe = tmp_path / "extent_main"
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "deeprecsys_amd", "csrc"), str(src), "-o", str(exe)],
                   check=True, capture_output=True, text=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout
    eng_src = open(os.path.join(ROOT, "deeprecsys_amd", "csrc", "engine_device_inputs.hip")).read()
    assert eng_src.count("input_extent_bytes(") == 3 and "extent_inside(" in eng_src       # the entry point uses it for all three arrays


def test_the_documents_name_the_calls():
    def read(*p):
        return open(os.path.join(ROOT, *p)).read()
    assert "drs_run_queues_device_multi_async" in read("INTEGRATION.md") and "run_queues_device_multi" in read("INTEGRATION.md")
    assert "run_queues_device_multi" in read("README.md") and "drs_device_inputs.h" in read("README.md")
    design = read("DESIGN.md")
    for word in ("drs_run_queues_device_multi_async", "input_pass.hip", "kErrLengths"):
        assert word in design, word
    mk = read("deeprecsys_amd", "csrc", "Makefile")
    assert "input_pass.hip" in mk and "engine_device_inputs.hip" in mk and "drs_device_inputs.h" in mk
