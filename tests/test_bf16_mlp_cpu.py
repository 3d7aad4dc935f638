"""CPU side of the bf16 FC layers (engine option "mlp_dtype"): the ISA of gemm_bf16_kernel (hipcc cross-compiles here), the
--accel_mlp_dtype flag and when the host code sets the option, and the header's function set."""
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
CSRC = os.path.join(ROOT, "deeprecsys_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_gemm_bf16_kernel_isa(tmp_path):
    """Every gemm_bf16_kernel instance: no scratch, no spills, and ONE MFMA shape -- v_mfma_f32_16x16x32_bf16 -- so that an
    output's bits cannot depend on which instance served it; the fp32 -> bf16 rounding is the NaN-safe plain cast."""
    out = str(tmp_path / "gemm_bf16.s")
    r = subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wno-unused-function", "-Wno-inline-asm",
                        "--offload-device-only", "-S", "-o", out, os.path.join(CSRC, "gemm_bf16.hip")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    text = open(out).read()
    # code of each kernel: from its label to the end of the function
    bodies = dict((m.group(1), m.group(2)) for m in re.finditer(r"^(_ZN\w*gemm_bf16_kernel\w*):[^\n]*\n(.*?)\n\.Lfunc_end", text, re.S | re.M))
    assert len(bodies) == 6, sorted(bodies)                    # three tile shapes x (16-byte | 4-byte input loads)
    for name, body in bodies.items():
        shapes = set(re.findall(r"\bv_(?:s?mfma\w*)", body))
        assert shapes == {"v_mfma_f32_16x16x32_bf16"}, (name, shapes)
        assert "v_cvt_pk_bf16_f32" in body, name
        assert not re.search(r"\bscratch_|\bbuffer_(?:load|store)", body), name
    # the kernels' metadata
    seen = {}
    for m in re.finditer(r"- \.agpr_count:.*?\.wavefront_size:\s+\d+", text, re.S):
        blk = m.group(0)
        nm = re.search(r"\.name:\s+(\S+)", blk).group(1)
        if "gemm_bf16_kernel" in nm:
            seen[nm] = blk
    assert len(seen) == 6, sorted(seen)
    for nm, blk in seen.items():
        assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1)) == 0, nm
        assert int(re.search(r"\.vgpr_spill_count:\s+(\d+)", blk).group(1)) == 0, nm
        assert int(re.search(r"\.sgpr_spill_count:\s+(\d+)", blk).group(1)) == 0, nm


def test_flag_defaults_to_fp32_and_rejects_other_words():
    assert cli([]).accel_mlp_dtype == "fp32"
    for w in ("fp32", "bf16"):
        assert cli(["--accel_mlp_dtype", w]).accel_mlp_dtype == w
    with pytest.raises(SystemExit):
        cli(["--accel_mlp_dtype", "bogus"])
    with pytest.raises(SystemExit):
        cli(["--accel_mlp_dtype", "fp16"])                      # (unbounded dense features overflow it: not offered)
    assert (N.MLP_FP32, N.MLP_BF16) == (0, 2) and N.MLP_BF16 == N.TABLE_BF16
    args = cli([])
    args.accel_mlp_dtype = "half"                               # (a JSON config can set anything: refused at engine build)
    with pytest.raises(ValueError):
        dlrm_s_hip._mlp_dtype(args)


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


@pytest.mark.parametrize("word", ["bf16", "fp32"])
def test_mlp_dtype_is_set_before_any_layer_and_never_for_fp32(monkeypatch, word):
    meta, _ = H.load_fixture("dlrm_dot_small")
    args = H.args_from(meta["args"], accel_mlp_dtype=word)
    np.random.seed(args.numpy_rand_seed)
    net = H.NET_CLS[args.model_type](args)
    monkeypatch.setattr(dlrm_s_hip.N, "Engine", _Recorder)
    _Recorder.log = []
    net._create_engine()
    log = _Recorder.log
    calls = [i for i, c in enumerate(log) if c[:2] == ("set_option", "mlp_dtype")]
    layers = [i for i, c in enumerate(log) if c[0] == "set_fc"]
    assert layers
    if word == "fp32":
        assert calls == []
        return
    assert len(calls) == 1 and log[calls[0]][2] == N.MLP_BF16 and calls[0] < min(layers)


def test_fp32_sets_nothing_on_the_cpu_abi(cpu_abi):
    """The CPU ABI the host tests run on does not know the key: the default flag must never reach it."""
    meta, _ = H.load_fixture("dlrm_dot_small")
    args = H.args_from(meta["args"], accel_mlp_dtype="fp32")
    net, lX, lS_l, lS_i, lT = H.materialize(args)
    calls = []
    real = N.Engine.set_option

    def spy(self, key, value, user=True):
        calls.append(key)
        return real(self, key, value, user)
    N.Engine.set_option = spy
    try:
        net.create(lX[0], lS_l[0], lS_i[0], lT[0])
        try:
            assert "mlp_dtype" not in calls and "mlp_dtype" not in net.engine.user_options
            net.stage_batches(lX, lS_l, lS_i)
            assert net.run_staged(0, len(lS_l[0][0])).shape[0] == len(lS_l[0][0])
        finally:
            net.engine.close()
    finally:
        N.Engine.set_option = real


def test_header_declares_the_constants_and_no_new_function():
    text = open(os.path.join(ROOT, "include", "drs.h")).read()
    assert re.search(r"DRS_MLP_FP32\s*=\s*0\b", text) and re.search(r"DRS_MLP_BF16\s*=\s*2\b", text)
    declared = set(re.findall(r"\b(drs_\w+)\s*\(", text))
    bound = set(name for name, _, _ in N.SYMBOLS)
    assert declared == bound, declared ^ bound                    # (the binding lists what the header declared before this option)
    assert '"mlp_dtype"' in text
