"""CPU side of half-precision embedding tables (engine option "table_dtype"): the --accel_table_dtype flag, the order
in which the host code sets the option, and the ISA of the half gather kernels (hipcc cross-compiles here)."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from deeprecsys_amd import _native as N
from deeprecsys_amd import dlrm_s_hip
from deeprecsys_amd.utils.utils import cli
from tests import helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_flag_defaults_to_fp32_and_rejects_other_words():
    assert cli([]).accel_table_dtype == "fp32"
    for w in ("fp16", "bf16", "fp32"):
        assert cli(["--accel_table_dtype", w]).accel_table_dtype == w
    with pytest.raises(SystemExit):
        cli(["--accel_table_dtype", "fp8"])
    assert (N.TABLE_FP32, N.TABLE_FP16, N.TABLE_BF16) == (0, 1, 2)
    args = cli([])
    args.accel_table_dtype = "int8"               # (a JSON config can set anything: refused at engine build)
    with pytest.raises(ValueError):
        dlrm_s_hip._table_dtype(args)


class _Recorder(object):
    """Stand-in for N.Engine: records every call made on it, in order."""
    log = []

    def __init__(self, *a, **kw):
        self.num_slots = int(kw.get("num_slots", 1))
        self.pref = None
        _Recorder.log.append(("create", self.num_slots))

    def set_option(self, key, value, user=True):
        _Recorder.log.append(("set_option", key, value))
        if key == "table_dtype" and value != N.TABLE_FP32:
            self.pref = 6                        # the class may change with the element size: re-created below

    def get_option(self, key):
        if key == "preferred_slots":
            return self.pref if self.pref is not None else self.num_slots
        return 0

    def __getattr__(self, name):
        def call(*a, **kw):
            _Recorder.log.append((name,) + tuple(x for x in a if isinstance(x, (int, str))))
        return call


@pytest.mark.parametrize("dtype,init", [("fp16", "numpy"), ("bf16", "device"), ("fp32", "numpy"), ("fp32", "device")])
def test_table_dtype_is_set_before_any_table_write_and_never_for_fp32(monkeypatch, dtype, init):
    meta, _ = H.load_fixture("dlrm_dot_small")
    args = H.args_from(meta["args"], accel_table_dtype=dtype, accel_table_init=init)
    np.random.seed(args.numpy_rand_seed)
    net = H.NET_CLS[args.model_type](args)
    monkeypatch.setattr(dlrm_s_hip.N, "Engine", _Recorder)
    _Recorder.log = []
    net._create_engine()
    log = _Recorder.log
    dtype_calls = [i for i, c in enumerate(log) if c[:2] == ("set_option", "table_dtype")]
    writes = [i for i, c in enumerate(log) if c[0] in ("set_table", "fill_table_uniform")]
    creates = [i for i, c in enumerate(log) if c[0] == "create"]
    assert len(writes) == len(net.ln_emb)
    if dtype == "fp32":
        assert dtype_calls == [] and len(creates) == 1
        return
    # every engine made gets the option right after it is created, before the preferred_slots comparison that may
    # re-create it and before the tables are written
    assert len(creates) == 2 and dtype_calls == [c + 1 for c in creates]
    assert all(log[i][2] == dlrm_s_hip._TABLE_DTYPES[dtype] for i in dtype_calls)
    assert max(dtype_calls) < min(writes)


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_half_gather_kernels_do_not_spill(tmp_path):
    """sls.hip compiled with the Makefile's flags: every half instantiation of the gather kernels (sls_kernel,
    sls_one_kernel, sls_flat_kernel, sls_flatc_kernel, sls_any_kernel) uses no scratch and spills no VGPR, and reads its
    rows with 8-byte loads (4 elements per lane, like the fp32 forms' 16 bytes)."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src = os.path.join(ROOT, "deeprecsys_amd", "csrc")
    out = str(tmp_path / "sls.s")
    flags = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wall", "-Wno-unused-function", "-Wno-inline-asm"]
    r = subprocess.run([hipcc] + flags + ["--offload-device-only", "-S", "-o", out, os.path.join(src, "sls.hip")],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    asm = open(out).read()
    found = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", asm, re.S):
        name, body = m.group(1), m.group(2)
        kind = re.search(r"(sls_kernel|sls_one_kernel|sls_flat_kernel|sls_flatc_kernel|sls_any_kernel)", name)
        policy = "bf16" if "4BF16E" in name else "f16" if "3F16E" in name else None
        if not kind or not policy:
            continue
        found.setdefault((kind.group(1), policy), 0)
        found[(kind.group(1), policy)] += 1
        assert int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body).group(1)) == 0, name
    for kind in ("sls_kernel", "sls_one_kernel", "sls_flat_kernel", "sls_flatc_kernel", "sls_any_kernel"):
        for policy in ("f16", "bf16"):
            assert found.get((kind, policy), 0) > 0, (kind, policy, found)
    # the metadata of every kernel of the file: no VGPR spills anywhere
    assert set(re.findall(r"\.vgpr_spill_count:\s+(\d+)", asm)) == {"0"}
    # the RMC1 gather's half form: its 20 row loads per lane are 8-byte loads
    body = re.search(r"^(_ZN3drs12_GLOBAL__N_116sls_flatc_kernelILi16ELi20ELb1ENS0_3F16EEEvNS_7SlsArgsEi):(.*?)^\.Lfunc_end",
                     asm, re.S | re.M).group(2)
    assert len(re.findall(r"global_load_dwordx2 .* nt", body)) == 20
    assert "global_load_dwordx4" not in body
