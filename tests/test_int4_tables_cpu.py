"""CPU side of 4-bit rowwise embedding tables (engine option "table_dtype" 9): the --accel_table_dtype flag, the order in
which the host code sets the option, the documented quantization and pooling formulas against torch's
embedding_bag_4bit_prepack / embedding_bag_4bit_rowwise_offsets, and the ISA of the int4 kernels (hipcc cross-compiles
here)."""
import os
import re
import shutil

import numpy as np
import pytest

from deeprecsys_amd import _native as N
from deeprecsys_amd import dlrm_s_hip
from deeprecsys_amd.utils.utils import cli
from tests import helpers as H
from tests.test_table_convert_cpu import listing

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_flag_maps_int4_rowwise_to_9_and_still_refuses_int4():
    assert N.TABLE_INT4_ROWWISE == 9
    assert cli(["--accel_table_dtype", "int4_rowwise"]).accel_table_dtype == "int4_rowwise"
    args = cli([])
    args.accel_table_dtype = "int4_rowwise"
    assert dlrm_s_hip._table_dtype(args) == N.TABLE_INT4_ROWWISE
    with pytest.raises(SystemExit):
        cli(["--accel_table_dtype", "int4"])
    args.accel_table_dtype = "int4"
    with pytest.raises(ValueError):
        dlrm_s_hip._table_dtype(args)


class _Recorder(object):
    """Stand-in for N.Engine: records every call made on it, in order."""
    log = []

    def __init__(self, *a, **kw):
        self.num_slots = int(kw.get("num_slots", 1))
        _Recorder.log.append(("create", self.num_slots))

    def set_option(self, key, value, user=True):
        _Recorder.log.append(("set_option", key, value))

    def get_option(self, key):
        return self.num_slots if key == "preferred_slots" else 0

    def __getattr__(self, name):
        def call(*a, **kw):
            _Recorder.log.append((name,) + tuple(x for x in a if isinstance(x, (int, str))))
        return call


@pytest.mark.parametrize("init", ["numpy", "device"])
def test_int4_table_dtype_is_set_before_any_table_write(monkeypatch, init):
    meta, _ = H.load_fixture("dlrm_dot_small")
    args = H.args_from(meta["args"], accel_table_dtype="int4_rowwise", accel_table_init=init)
    np.random.seed(args.numpy_rand_seed)
    net = H.NET_CLS[args.model_type](args)
    monkeypatch.setattr(dlrm_s_hip.N, "Engine", _Recorder)
    _Recorder.log = []
    net._create_engine()
    log = _Recorder.log
    dtype_calls = [i for i, c in enumerate(log) if c[:2] == ("set_option", "table_dtype")]
    writes = [i for i, c in enumerate(log) if c[0] in ("set_table", "fill_table_uniform")]
    creates = [i for i, c in enumerate(log) if c[0] == "create"]
    assert len(writes) == len(net.ln_emb) and dtype_calls
    assert dtype_calls == [c + 1 for c in creates]
    assert all(log[i][2] == N.TABLE_INT4_ROWWISE for i in dtype_calls)
    assert max(dtype_calls) < min(writes)


def quantize_rows4(W):
    """docs/OPTIONS.md's 4-bit quantization, restated in numpy fp32 (no contraction; np.rint rounds half to even): per
    row [D / 2 code bytes | fp16 scale | fp16 bias] as embedding_bag_4bit_prepack lays it out (the engine pads the codes
    to a multiple of 4 bytes)."""
    W = np.ascontiguousarray(W, np.float32)
    bias_h = W.min(axis=1, keepdims=True).astype(np.float16)
    bias = bias_h.astype(np.float32)
    with np.errstate(over="ignore"):
        scale_h = ((W.max(axis=1, keepdims=True) - bias).astype(np.float32) / np.float32(15.0)).astype(np.float16)
    scale_h[scale_h == 0] = 1
    with np.errstate(divide="ignore", over="ignore"):
        inv = (np.float32(1.0) / scale_h.astype(np.float32)).astype(np.float32)
    scale_h[np.isinf(inv)] = 1
    inv[np.isinf(inv)] = 1
    q = np.clip(np.rint(((W - bias).astype(np.float32) * inv).astype(np.float32)), 0, 15).astype(np.uint8)
    codes = (q[:, 0::2] | (q[:, 1::2] << 4)).astype(np.uint8)
    return np.concatenate([codes, scale_h.view(np.uint8).reshape(-1, 2), bias_h.view(np.uint8).reshape(-1, 2)], axis=1)


def special_rows(W):
    W[1] = 0.75                                         # a constant row: scale 0 -> 1
    W[2, :] = np.abs(W[2, :]) + 0.5
    W[2, 0] = -0.0                                      # a row whose minimum is -0
    W[3] *= 1e-6
    W[4] = np.round(W[4] * 4) / 4                       # many ties after scaling
    return W


@pytest.mark.parametrize("D", [2, 4, 6, 10, 16, 64, 128, 256])
def test_quantization_formula_matches_embedding_bag_4bit_prepack(D):
    torch = pytest.importorskip("torch")
    rng = np.random.RandomState(D)
    W = special_rows(rng.uniform(-2, 3, (300, D)).astype(np.float32))
    ref = torch.ops.quantized.embedding_bag_4bit_prepack(torch.from_numpy(W)).numpy()
    assert ref.shape == (300, D // 2 + 4)
    assert np.array_equal(quantize_rows4(W), ref)


def pool4(P, D, idx, lens):
    """The engine's sequential order on packed rows: acc = fmaf(scale, q, acc + bias) per row, in fp32.  (The fma is
    formed in float64: scale * q is exact there, and its sum with the 24-bit acc + bias is rounded once more to fp32.)"""
    codes = P[:, :D // 2]
    q = np.empty((P.shape[0], D), np.float64)
    q[:, 0::2] = codes & 15
    q[:, 1::2] = codes >> 4
    s = P[:, D // 2:D // 2 + 2].copy().view(np.float16).astype(np.float64)
    b = P[:, D // 2 + 2:D // 2 + 4].copy().view(np.float16).astype(np.float32)
    out = np.zeros((len(lens), D), np.float32)
    j = 0
    for k, n in enumerate(lens):
        acc = np.zeros(D, np.float32)
        for r in idx[j:j + n]:
            acc = (s[r] * q[r] + (acc + b[r]).astype(np.float32).astype(np.float64)).astype(np.float32)
        out[k] = acc
        j += n
    return out


@pytest.mark.parametrize("D", [2, 6, 16, 64])
def test_fma_pooling_matches_embedding_bag_4bit_rowwise_offsets(D):
    torch = pytest.importorskip("torch")
    rng = np.random.RandomState(100 + D)
    W = special_rows(rng.uniform(-2, 3, (300, D)).astype(np.float32))
    P = torch.ops.quantized.embedding_bag_4bit_prepack(torch.from_numpy(W))
    lens = rng.randint(0, 8, size=40).astype(np.int64)
    lens[[0, 7, 39]] = 0                                 # empty bags
    idx = rng.randint(0, 300, size=int(lens.sum())).astype(np.int64)
    idx[:5] = np.arange(5)
    offsets = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    ref = torch.ops.quantized.embedding_bag_4bit_rowwise_offsets(
        P, torch.from_numpy(idx), torch.from_numpy(offsets), mode=0, include_last_offset=False).numpy()
    got = pool4(P.numpy(), D, idx, lens)
    assert np.array_equal(got.view(np.uint32), ref.astype(np.float32).view(np.uint32))


def test_options_doc_names_the_value():
    doc = open(os.path.join(ROOT, "docs", "OPTIONS.md")).read()
    assert "DRS_TABLE_INT4_ROWWISE" in doc and "int4_rowwise" in doc
    assert re.search(r"`table_dtype`[^\n]*\b9\b", doc)
    hdr = open(os.path.join(ROOT, "include", "drs.h")).read()
    assert "DRS_TABLE_INT4_ROWWISE = 9" in hdr and "#define DRS_ABI_VERSION 5" in hdr


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_int4_kernels_exist_and_do_not_spill():
    """sls.hip compiled with the Makefile's flags: an int4 instance of each of the five gather families exists; every one
    of them uses no scratch, and nothing spills a VGPR.  The RMC1 form reads its 20 rows per lane with non-temporal 2-byte
    loads of the codes, each beside a non-temporal dword load of the row's fp16 scale and bias.  (The kernels that write
    int4 tables -- quantize, write out, int4 -> int8: table_convert.hip, tests/test_table_convert_cpu.py.)"""
    asm = listing("sls.hip")
    found = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", asm, re.S):
        name, body = m.group(1), m.group(2)
        kind = re.search(r"(sls_kernel|sls_one_kernel|sls_flat_kernel|sls_flatc_kernel|sls_any_kernel)", name)
        if not kind or "2I4E" not in name:
            continue
        found[kind.group(1)] = found.get(kind.group(1), 0) + 1
        assert int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body).group(1)) == 0, name
    for kind in ("sls_kernel", "sls_one_kernel", "sls_flat_kernel", "sls_flatc_kernel", "sls_any_kernel"):
        assert found.get(kind, 0) > 0, (kind, found)
    assert set(re.findall(r"\.vgpr_spill_count:\s+(\d+)", asm)) == {"0"}
    body = re.search(r"^(_ZN3drs12_GLOBAL__N_116sls_flatc_kernelILi16ELi20ELb1ENS0_2I4EEEvNS_7SlsArgsEi):(.*?)^\.Lfunc_end",
                     asm, re.S | re.M).group(2)
    assert len(re.findall(r"global_load_ushort .* nt", body)) == 20
    assert len(re.findall(r"global_load_dword .* nt", body)) == 20
    assert "global_load_dwordx4" not in body and not re.search(r"global_load_dwordx\d .* nt", body)
