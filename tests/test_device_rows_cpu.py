"""CPU side of the device row updates (include/drs_device_rows.h): the de-duplication table of csrc/row_dedup.h walked by a host
program under the address and undefined-behaviour sanitizers against tests/row_update_ref.py's last-wins answer, the symbols
and the header, the frozen symbol lists, the wrapper's argument rules, and the documents."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from deeprecsys_amd import _native as N
from tests import row_update_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["drs_update_rows_device", "drs_get_rows_device"]
MAX_ID, MAX_POS = (1 << 31) - 1, (1 << 32) - 1
M64 = (1 << 64) - 1


# ------------------------------------------------------------------------------------------------
# row_dedup.h alone in a host program
DEDUP_MAIN = r"""
#include "row_dedup.h"
#include <stdio.h>
#include <vector>
using namespace drs;
static int fails = 0;
#define CHECK(c) do { if (!(c)) { printf("line %d: %s\n", __LINE__, #c); ++fails; } } while (0)

int main() {
  // the encoding and the capacity rule
  CHECK(dedup_slot(0, 0) == 0 && dedup_slot(0, 0) != kDedupEmpty);
  CHECK(dedup_slot(kDedupMaxId, kDedupMaxPos) == 0x7fffffffffffffffull && dedup_slot(kDedupMaxId, kDedupMaxPos) != kDedupEmpty);
  CHECK(dedup_id(dedup_slot(kDedupMaxId, kDedupMaxPos)) == kDedupMaxId && dedup_pos(dedup_slot(kDedupMaxId, kDedupMaxPos)) == kDedupMaxPos);
  CHECK(dedup_id(dedup_slot(5, 0)) == 5 && dedup_pos(dedup_slot(5, 0)) == 0 && dedup_pos(dedup_slot(0, 9)) == 9);
  CHECK(dedup_id(kDedupEmpty) > kDedupMaxId);                          // the empty marker's id field is no legal id
  CHECK(dedup_slot(7, 3) > dedup_slot(7, 2) && dedup_slot(7, 0) > dedup_slot(6, kDedupMaxPos));   // the maximum keeps the id
  CHECK(dedup_capacity(0) == 2 && dedup_capacity(1) == 2 && dedup_capacity(2) == 4 && dedup_capacity(3) == 8 && dedup_capacity(4) == 8);
  CHECK(dedup_capacity(5) == 16 && dedup_capacity(257) == 1024 && dedup_capacity((int64_t)1 << 24) == (uint64_t)1 << 25);

  long long cap_in, n;
  int k = 0;
  while (scanf("%lld %lld", &cap_in, &n) == 2) {
    std::vector<long long> id((size_t)n), pos((size_t)n);
    for (long long i = 0; i < n; ++i)
      if (scanf("%lld %lld", &id[(size_t)i], &pos[(size_t)i]) != 2) return 2;
    const uint64_t cap = cap_in > 0 ? (uint64_t)cap_in : dedup_capacity(n);
    CHECK((cap & (cap - 1)) == 0);
    std::vector<uint64_t> slots((size_t)cap, kDedupEmpty);
    const DedupHostAtomics at;
    long long full_at = -1;
    for (long long i = 0; i < n && full_at < 0; ++i)
      if (!dedup_insert(slots.data(), cap, id[(size_t)i], pos[(size_t)i], at)) full_at = i;
    long long used = 0;
    for (uint64_t s : slots) used += s != kDedupEmpty;
    printf("case %d cap %llu full %lld used %lld home", k, (unsigned long long)cap, full_at, used);
    for (long long i = 0; i < n; ++i) printf(" %llu", (unsigned long long)(dedup_hash(id[(size_t)i]) & (cap - 1)));
    printf(" wins");
    for (long long i = 0; i < n; ++i) printf(" %d", (int)dedup_wins(slots.data(), cap, id[(size_t)i], pos[(size_t)i], at));
    printf("\n");
    ++k;
  }
  printf("%d cases, %d failures\n", k, fails);
  return fails != 0;
}
"""


def dedup_hash(i):
    """row_dedup.h's dedup_hash, restated (the host program prints every id's home bucket: the two are held together)"""
    z = i & M64
    z = ((z ^ (z >> 33)) * 0xff51afd7ed558ccd) & M64
    z = ((z ^ (z >> 33)) * 0xc4ceb9fe1a85ec53) & M64
    return z ^ (z >> 33)


def colliding_ids(cap, bucket, count):
    """the first `count` ids whose home bucket in a table of `cap` slots is `bucket`, by brute force"""
    out, i = [], 0
    while len(out) < count:
        if dedup_hash(i) & (cap - 1) == bucket:
            out.append(i)
        i += 1
    return out


def expected_wins(ids, pos):
    """R.resolve's last-wins answer: the entries in the order of their positions, each id's last one kept"""
    order = np.argsort(np.asarray(pos, dtype=np.uint64), kind="stable")
    entry = np.arange(len(ids), dtype=np.float32)[order].reshape(-1, 1)          # (which entry a row of V came from)
    _, kept = R.resolve(np.asarray(ids, np.int64)[order], entry)
    wins = np.zeros(len(ids), int)
    wins[kept[:, 0].astype(int)] = 1
    return wins.tolist()


def dedup_cases():
    """name -> (cap or 0: the capacity rule, ids, positions)"""
    rng = np.random.RandomState(3)
    seq = lambda n: list(range(n))
    cases = {
        "one": (0, [41], [0]),
        "distinct": (0, rng.permutation(1000)[:300].tolist(), seq(300)),
        "one_id_257_times": (0, [12345] * 257, seq(257)),
        "id0_at_position0": (0, [0, 9, 0, 3], seq(4)),
        "id0_alone": (0, [0], [0]),
        "largest_id_and_position": (0, [MAX_ID, 0, MAX_ID, MAX_ID - 1], [7, 0, MAX_POS, MAX_POS - 1]),
        "repeats": (0, rng.randint(0, 40, size=200).tolist(), seq(200)),
    }
    # 12 ids that share the LAST bucket of a 32-slot table, some of them twice: the probe chain wraps past the table's end
    col = colliding_ids(32, 31, 12)
    cases["one_home_bucket_wraps"] = (32, col + col[::3], seq(16))
    # exactly n entries at capacity 2 n
    cases["half_full"] = (0, rng.permutation(100000)[:128].tolist(), seq(128))
    return cases


def run_dedup(tmp_path, cases):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a C++ compiler builds the host program"
    src, exe = tmp_path / "dedup_main.cpp", tmp_path / "dedup_main"
    src.write_text(DEDUP_MAIN)
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Werror",
                    "-I", os.path.join(ROOT, "deeprecsys_amd", "csrc"), str(src), "-o", str(exe)], check=True, capture_output=True, text=True)
    text = "".join("%d %d %s\n" % (cap, len(ids), " ".join("%d %d" % p for p in zip(ids, pos))) for cap, ids, pos in cases)
    r = subprocess.run([str(exe)], input=text, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == "%d cases, 0 failures" % len(cases), r.stdout
    out = []
    for line in lines[:-1]:
        m = re.match(r"case \d+ cap (\d+) full (-?\d+) used (\d+) home((?: \d+)*) wins((?: \d+)*)$", line)
        assert m, line
        out.append((int(m.group(1)), int(m.group(2)), int(m.group(3)), [int(x) for x in m.group(4).split()], [int(x) for x in m.group(5).split()]))
    return out


def test_the_table_keeps_every_ids_last_position(tmp_path):
    """csrc/row_dedup.h on its own, in a host program under the sanitizers: the insert and lookup loops the kernels run, with
    plain loads and stores for atomics.  The winners are R.resolve's for every list."""
    cases = dedup_cases()
    got = run_dedup(tmp_path, list(cases.values()))
    for (name, (cap_in, ids, pos)), (cap, full_at, used, home, wins) in zip(cases.items(), got):
        assert full_at == -1, name
        assert cap == (cap_in or 1 << (2 * len(ids) - 1).bit_length()), name          # the power of two >= 2 n
        assert cap_in or cap >= 2 * len(ids), name
        assert used == len(set(ids)), name
        assert home == [dedup_hash(i) & (cap - 1) for i in ids], name
        assert wins == expected_wins(ids, pos), name
    by = dict(zip(cases, got))
    assert by["distinct"][4] == [1] * 300                                  # every id distinct: every position wins
    assert by["one_id_257_times"][4] == [0] * 256 + [1]
    assert by["id0_at_position0"][4] == [0, 1, 1, 1] and by["id0_alone"][4] == [1]
    assert by["largest_id_and_position"][4] == [0, 1, 1, 1]
    assert set(by["one_home_bucket_wraps"][3]) == {31} and by["one_home_bucket_wraps"][2] == 12
    assert by["half_full"][0] == 256 and by["half_full"][2] == 128          # n entries at capacity 2 n


def test_a_full_table_ends_the_probe_with_an_error(tmp_path):
    """8 slots, 8 distinct ids fill them; the ninth id finds no slot: insert reports it after 8 steps instead of looping, and
    its lookup ends likewise.  An id that is in the table is still raised."""
    ids = [100, 101, 102, 103, 104, 105, 106, 107]
    (cap, full_at, used, _, wins), = run_dedup(tmp_path, [(8, ids + [104, 999, 100], list(range(11)))])
    assert (cap, full_at, used) == (8, 9, 8)
    # 104's second entry (position 8) went in before the table refused 999; nothing after the refusal was inserted
    assert wins == [1, 1, 1, 1, 0, 1, 1, 1, 1, 0, 0]
    # the capacity rule never lets the kernels get there
    src = open(os.path.join(ROOT, "deeprecsys_amd", "csrc", "row_dedup.h")).read()
    assert "k < cap" in src and "while (true)" not in src and "for (;;)" not in src


# ------------------------------------------------------------------------------------------------
# symbols and headers
def test_the_library_exports_both_symbols():
    L = N.lib()
    assert [n for n, _, _ in N.DEVICE_ROW_SYMBOLS] == NAMES
    for name, res, args in N.DEVICE_ROW_SYMBOLS:
        fn = getattr(L, name)
        assert fn.restype is res and fn.argtypes == args, name
    upd, get = [a for _, _, a in N.DEVICE_ROW_SYMBOLS]
    V, I32, I64 = N.C.c_void_p, N.C.c_int32, N.C.c_int64
    assert upd == [V, I32, I64, V, V, I64, I32, V, I32]
    assert get == [V, I32, I64, V, V, I64, V, I32]
    assert N.DEVICE_ROWS_MAX == 1 << 24


def test_the_header_declares_both_calls_and_the_abi_version_stays():
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "a C compiler preprocesses the header"
    text = subprocess.run([cc, "-E", os.path.join(ROOT, "include", "drs.h")], capture_output=True, text=True, check=True).stdout
    flat = re.sub(r"\s+", " ", text)
    w, p = r"\s*\w+\s*", r"\s*\*\s*"
    upd = (r"int32_t drs_update_rows_device\s*\(\s*drs_handle" + w + r", int32_t" + w + r", int64_t" + w + r", const int64_t" + p + r"\w+\s*, const void" + p +
           r"\w+\s*, int64_t" + w + r", int32_t" + w + r", void" + p + r"\w+\s*, int32_t" + w + r"\)\s*;")
    get = (r"int32_t drs_get_rows_device\s*\(\s*drs_handle" + w + r", int32_t" + w + r", int64_t" + w + r", const int64_t" + p + r"\w+\s*, float" + p +
           r"\w+\s*, int64_t" + w + r", void" + p + r"\w+\s*, int32_t" + w + r"\)\s*;")
    assert re.search(upd, flat), "drs_update_rows_device"
    assert re.search(get, flat), "drs_get_rows_device"
    hdr = open(os.path.join(ROOT, "include", "drs.h")).read()
    assert "#define DRS_ABI_VERSION 5" in hdr and '#include "drs_device_rows.h"' in hdr
    assert hdr.index('#include "drs_rows.h"') < hdr.index('#include "drs_device_rows.h"') < hdr.rindex("#ifdef __cplusplus")
    assert not any(re.search(r"\b%s\s*\(" % n, hdr) for n in NAMES)          # declared in drs_device_rows.h alone
    sat = open(os.path.join(ROOT, "include", "drs_device_rows.h")).read()
    for word in ("Ordering", "ordered == 0", "ordered == 1", "null stream", "LAST", "DRS_DEVICE_ROWS_MAX", "DRS_ERR_INDEX_RANGE", "DRS_ERR_BAD_ARG",
                 "hipMemGetAddressRange", "changes nothing", "drs_sync", "val_row_stride"):
        assert word in sat, word
    assert re.search(r"#define DRS_DEVICE_ROWS_MAX \(\(int64_t\)1 << 24\)", sat)


def test_the_frozen_symbol_lists_are_unchanged(cpu_abi):
    names = [n for n, _, _ in N.SYMBOLS]
    assert len(names) == 40 and len(set(names)) == 40
    assert [n for n, _, _ in N.ROW_SYMBOLS] == ["drs_update_rows", "drs_get_rows"]
    assert not (set(names) | {n for n, _, _ in N.ROW_SYMBOLS}) & set(NAMES)
    assert N.lib().drs_abi_version() == 5
    # the CPU restatement binds the frozen list (the fixture has just done so) and knows nothing of the new names
    assert cpu_abi.drs_abi_version() == 5
    for name in NAMES:
        assert not hasattr(cpu_abi, name)


# ------------------------------------------------------------------------------------------------
# the wrapper's own checks
def test_the_wrapper_refuses_what_the_tensors_show_without_touching_the_engine():
    import torch
    from deeprecsys_amd import dlrm_s_hip as M

    def refused(fn, word, *a, **kw):
        with pytest.raises(ValueError) as err:
            fn(*a, **kw)
        assert word in str(err.value), (word, str(err.value))

    ids = torch.zeros(4, dtype=torch.int64)
    refused(M.device_row_ids, "torch tensor", np.zeros(4, np.int64), 0)
    refused(M.device_row_ids, "int64", ids.to(torch.int32), 0)
    refused(M.device_row_ids, "[n]", ids.reshape(2, 2), 0)
    refused(M.device_row_ids, "contiguous", torch.zeros(8, dtype=torch.int64)[::2], 0)
    refused(M.device_row_ids, "cuda:0", ids, 0)                          # a CPU tensor: everything else about it is right

    D = 8
    good = torch.zeros((4, D))
    refused(M.device_row_values, "torch tensor", good.numpy(), 4, D, 0)
    refused(M.device_row_values, "float32", good.to(torch.float64), 4, D, 0)
    refused(M.device_row_values, "float32", good.to(torch.int32), 4, D, 0)
    refused(M.device_row_values, "[4, 8]", torch.zeros((5, D)), 4, D, 0)
    refused(M.device_row_values, "[4, 8]", torch.zeros((4, D + 1)), 4, D, 0)
    refused(M.device_row_values, "[4, 8]", torch.zeros(4 * D), 4, D, 0)
    refused(M.device_row_values, "contiguous", torch.zeros((4, 2 * D))[:, ::2], 4, D, 0)
    refused(M.device_row_values, "contiguous", torch.zeros((D, 4)).t(), 4, D, 0)
    refused(M.device_row_values, "row stride", torch.zeros((1, D)).expand(4, D), 4, D, 0)      # stride 0: the rows overlap
    for dt in (torch.float32, torch.float16, torch.bfloat16):                                    # the three types get as far as the device
        refused(M.device_row_values, "cuda:0", good.to(dt), 4, D, 0)
    refused(M.device_row_values, "cuda:0", torch.zeros((4, 3 * D))[:, D:2 * D], 4, D, 0)       # a column block is a fine layout
    # the read-back's output: float32 only
    refused(M.device_row_values, "out: must be torch.float32", good.to(torch.float16), 4, D, 0, name="out", dtypes=(torch.float32,))
    assert not M.on_device(ids, 0) and not M.on_device(np.zeros(4, np.int64), 0) and not M.on_device([1, 2], 0)

    # numpy arguments take the host route unchanged; the device-only arguments are refused there
    calls = []

    class Host(object):
        device, D = 0, 8

        def update_rows(self, t, i, v):
            calls.append(("update_rows", t))

        def get_rows(self, t, i):
            calls.append(("get_rows", t))
            return "rows"

        def __getattr__(self, name):
            raise AssertionError("the engine was touched: " + name)
    net = object.__new__(M._HipNet)
    net.engine = Host()
    net.update_embedding_rows(1, np.zeros(4, np.int64), np.zeros((4, D), np.float32))
    assert net.embedding_rows(2, [3]) == "rows" and calls == [("update_rows", 1), ("get_rows", 2)]
    refused(net.update_embedding_rows, "stream", 1, np.zeros(4, np.int64), np.zeros((4, D), np.float32), stream=0)
    refused(net.embedding_rows, "out", 1, np.zeros(4, np.int64), out=good)
    assert calls == [("update_rows", 1), ("get_rows", 2)]
    for cls in M.WRAPPERS.values():
        assert callable(getattr(cls.net_cls, "update_embedding_rows")) and callable(getattr(cls.net_cls, "embedding_rows"))
    assert len(M.WRAPPERS) == 6
    assert callable(N.Engine.update_rows_device) and callable(N.Engine.get_rows_device)


def test_the_documents_and_the_makefile_name_the_new_files_and_calls():
    def read(*p):
        return open(os.path.join(ROOT, *p)).read()
    integ = read("INTEGRATION.md")
    for word in ("drs_update_rows_device", "drs_get_rows_device", "drs_device_rows.h"):
        assert word in integ, word
    assert "drs_update_rows_device" in read("README.md") and "r29_device_rows.md" in read("README.md")
    design = read("DESIGN.md")
    for word in ("drs_update_rows_device", "device_rows.hip", "row_dedup.h", "place_rows_kernel", "neither drains nor waits"):
        assert word in design, word
    mk = read("deeprecsys_amd", "csrc", "Makefile")
    for word in ("device_rows.hip", "row_dedup.h", "drs_device_rows.h"):
        assert word in mk, word
    kernel = read("deeprecsys_amd", "csrc", "device_rows.hip")
    for word in ("dedup_insert(", "dedup_lookup(", "launch_convert_rows(", "device_range_fault(", "i8_row_offset(", "hipStreamWaitEvent("):
        assert word in kernel, word
    assert "asm" not in kernel
    assert os.path.exists(os.path.join(ROOT, "tools", "device_rows_cost.py"))
    assert "bench.py" in read("profiles", "r29_device_rows.md")
