"""Compile check of csrc/table_convert.hip, the translation unit that fills and converts embedding tables: its kernel set
is one template per destination, generic over the source reader, and nothing of it is left in the gather's sls.hip."""
import functools
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wall", "-Wno-unused-function", "-Wno-inline-asm"]
needs_hipcc = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")

READERS = {"Elems": "SrcElems", "Fill": "SrcFill", "I8": "SrcI8", "I4": "SrcI4", "F8": "SrcF8"}
# destination kernel -> the readers it is instantiated for (None: not a template)
EXPECTED = {
    "write_elems_kernel": ["Elems", "I8", "I4", "F8"],           # fp32 / fp16 / bf16 elements (the fill: flat, below)
    "quantize_rows_kernel": ["Elems", "Fill", "I4", "F8"],       # int8 rowwise rows
    "pack4_rows_kernel": ["Elems", "Fill", "I8", "F8"],          # int4 rowwise rows
    "to_fp8_rows_kernel": ["Elems", "Fill"],                     # fp8 e4m3 codes
    "absmax_rows_kernel": ["Elems"],                             # an fp8 table's scale
    "relayout_rows_kernel": [None],                              # rowwise rows, plain <-> line-packed
    "fill_uniform_kernel": [None],                               # the flat fp32 / fp16 / bf16 fill
    "convert_table_kernel": [None],                              # the flat fp32 / fp16 / bf16 arena pass
}


@functools.lru_cache(maxsize=None)
def listing(name):
    """The device listing of csrc/<name>, compiled once per session with the Makefile's flags (--offload-device-only -S)."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    out = os.path.join(tempfile.mkdtemp(prefix="drs_isa_"), name.replace(".hip", ".s"))
    r = subprocess.run([hipcc] + FLAGS + ["--offload-device-only", "-S", "-o", out, os.path.join(ROOT, "deeprecsys_amd", "csrc", name)],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    asm = open(out).read()
    shutil.rmtree(os.path.dirname(out))
    return asm


def instance(symbol):
    """(kernel, reader) of a mangled drs:: kernel symbol: _ZN3drs<n><kernel>[INS_<m><reader>E...]"""
    m = re.match(r"_ZN3drs(\d+)", symbol)
    rest = symbol[m.end():]
    kernel, rest = rest[:int(m.group(1))], rest[int(m.group(1)):]
    m = re.match(r"INS_(\d+)", rest)
    return kernel, rest[m.end():m.end() + int(m.group(1))] if m else None


@needs_hipcc
def test_one_kernel_per_destination_and_none_uses_scratch():
    asm = listing("table_convert.hip")
    found = []
    for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", asm, re.S):
        found.append(instance(m.group(1)))
        assert int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", m.group(2)).group(1)) == 0, m.group(1)
    want = {(k, READERS[r] if r else None) for k, rs in EXPECTED.items() for r in rs}
    assert len(found) == len(set(found)) and set(found) == want, sorted(set(found) ^ want, key=str)
    assert set(re.findall(r"\.vgpr_spill_count:\s+(\d+)", asm)) == {"0"}


@needs_hipcc
def test_the_gather_translation_unit_holds_no_table_writing_kernel():
    names = re.findall(r"\.amdhsa_kernel (\S+)", listing("sls.hip"))
    assert names
    stray = [n for n in names if re.search(r"quantize|pack4|relayout|fp8_rows|absmax|fill_uniform|convert_table|write_elems|probe_", n)]
    assert not stray, stray
