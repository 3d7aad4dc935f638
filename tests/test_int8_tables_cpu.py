"""CPU side of 8-bit rowwise embedding tables (engine option "table_dtype" 8): the --accel_table_dtype flag, the order in
which the host code sets the option, the documented quantization formula against torch's embedding_bag_byte_prepack, and
the ISA of the int8 gather kernels (hipcc cross-compiles here)."""
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


def test_flag_maps_int8_rowwise_to_8_and_still_refuses_int8():
    assert N.TABLE_INT8_ROWWISE == 8
    assert cli(["--accel_table_dtype", "int8_rowwise"]).accel_table_dtype == "int8_rowwise"
    args = cli([])
    args.accel_table_dtype = "int8_rowwise"
    assert dlrm_s_hip._table_dtype(args) == N.TABLE_INT8_ROWWISE
    with pytest.raises(SystemExit):
        cli(["--accel_table_dtype", "int8"])
    args.accel_table_dtype = "int8"
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
def test_int8_table_dtype_is_set_before_any_table_write(monkeypatch, init):
    meta, _ = H.load_fixture("dlrm_dot_small")
    args = H.args_from(meta["args"], accel_table_dtype="int8_rowwise", accel_table_init=init)
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
    assert all(log[i][2] == N.TABLE_INT8_ROWWISE for i in dtype_calls)
    assert max(dtype_calls) < min(writes)


def quantize_rows(W):
    """docs/OPTIONS.md's quantization, restated in numpy fp32 (no contraction; np.rint rounds half to even): per row
    [codes | scale | bias] as embedding_bag_byte_prepack lays it out (D + 8 bytes; the engine pads the codes to a
    multiple of 8 bytes)."""
    W = np.ascontiguousarray(W, np.float32)
    mn = W.min(axis=1, keepdims=True)
    mx = W.max(axis=1, keepdims=True)
    rng = (mx - mn).astype(np.float32)
    scale = (rng / np.float32(255.0)).astype(np.float32)
    inv = (np.float32(255.0) / (rng + np.float32(1e-8))).astype(np.float32)
    q = np.rint(((W - mn).astype(np.float32) * inv).astype(np.float32)).astype(np.uint8)
    return np.concatenate([q, scale.view(np.uint8).reshape(-1, 4), mn.view(np.uint8).reshape(-1, 4)], axis=1)


@pytest.mark.parametrize("D", [1, 3, 4, 10, 16, 64, 128, 256])
def test_quantization_formula_matches_embedding_bag_byte_prepack(D):
    torch = pytest.importorskip("torch")
    rng = np.random.RandomState(D)
    W = rng.uniform(-2, 3, (300, D)).astype(np.float32)
    W[1] = 0.75                                         # a constant row: scale 0
    W[2, :] = np.abs(W[2, :]) + 0.5
    W[2, 0] = -0.0                                      # a row whose minimum is -0
    W[3] *= 1e-6
    W[4] = np.round(W[4] * 4) / 4                       # many ties after scaling
    ref = torch.ops.quantized.embedding_bag_byte_prepack(torch.from_numpy(W)).numpy()
    assert ref.shape == (300, D + 8)
    assert np.array_equal(quantize_rows(W), ref)


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_int8_gather_kernels_exist_and_do_not_spill():
    """sls.hip compiled with the Makefile's flags: every int8 instantiation of the five gather families exists, uses no
    scratch and spills no VGPR; the RMC1 form reads its 20 rows per lane with non-temporal dword loads of the codes, each
    beside a non-temporal 8-byte load of the row's scale and bias, all issued before the first sum, and converts the codes
    with v_cvt_f32_ubyte0..3.  (The kernels that write int8 tables: table_convert.hip, tests/test_table_convert_cpu.py.)"""
    asm = listing("sls.hip")
    found = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", asm, re.S):
        name, body = m.group(1), m.group(2)
        kind = re.search(r"(sls_kernel|sls_one_kernel|sls_flat_kernel|sls_flatc_kernel|sls_any_kernel)", name)
        if not kind or "2I8E" not in name:
            continue
        found[kind.group(1)] = found.get(kind.group(1), 0) + 1
        assert int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body).group(1)) == 0, name
    for kind in ("sls_kernel", "sls_one_kernel", "sls_flat_kernel", "sls_flatc_kernel", "sls_any_kernel"):
        assert found.get(kind, 0) > 0, (kind, found)
    assert set(re.findall(r"\.vgpr_spill_count:\s+(\d+)", asm)) == {"0"}
    body = re.search(r"^(_ZN3drs12_GLOBAL__N_116sls_flatc_kernelILi16ELi20ELb1ENS0_2I8EEEvNS_7SlsArgsEi):(.*?)^\.Lfunc_end",
                     asm, re.S | re.M).group(2)
    assert len(re.findall(r"global_load_dword .* nt", body)) == 20
    assert len(re.findall(r"global_load_dwordx2 .* nt", body)) == 20
    assert "global_load_dwordx4" not in body
    assert all("v_cvt_f32_ubyte%d" % k in body for k in range(4))
    # every row load of the wave is in flight before the first sum: between the first and the last row load there is no
    # vmcnt(0) drain and no fma (the 40 loads are one HBM round trip)
    lines = [ln.strip() for ln in body.splitlines()]
    rows = [i for i, ln in enumerate(lines) if ln.startswith("global_load") and ln.endswith(" nt")]
    assert len(rows) == 40
    between = lines[rows[0]:rows[-1]]
    assert not any(re.match(r"s_waitcnt vmcnt\(0\)", ln) for ln in between), "vmcnt(0) before the last row load"
    assert not any("fma" in ln.split(" ")[0] for ln in between), "a sum before the last row load"
