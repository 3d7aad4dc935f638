"""CPU side of NCF's one-launch form under "mlp_dtype" 2 (engine option "mlp_bf16_fuse"): the documents name NCF next to the
key, and an NCF net's engine build sets the option behind mlp_dtype, before the first layer, and only when asked to."""
import os
import re

import numpy as np
import pytest

from deeprecsys_amd import _native as N
from deeprecsys_amd import dlrm_s_hip
from tests import helpers as H
from tests.test_bf16_mlp_cpu import _Recorder

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_options_document_and_header_name_ncf_next_to_the_key():
    doc = open(os.path.join(ROOT, "docs", "OPTIONS.md")).read()
    row = [l for l in doc.split("\n") if l.startswith("| `mlp_bf16_fuse` |")]
    assert len(row) == 1
    assert "NCF" in row[0] and "DLRM" in row[0] and "fused_bf16_kernel<sum>" in row[0]
    header = open(os.path.join(ROOT, "include", "drs.h")).read()
    line = [l for l in header.split("\n") if '"mlp_bf16_fuse"' in l]
    assert len(line) == 1 and "NCF" in line[0] and "DLRM" in line[0], line
    assert re.search(r'"mlp_bf16_fuse" 0\|1\b', line[0])


def _ncf_engine_calls(monkeypatch, **flags):
    meta, _ = H.load_fixture("ncf_mini")
    args = H.args_from(meta["args"], **flags)
    assert args.model_type == "ncf"
    np.random.seed(args.numpy_rand_seed)
    net = H.NET_CLS[args.model_type](args)
    assert net.kind == N.MODEL_NCF
    monkeypatch.setattr(dlrm_s_hip.N, "Engine", _Recorder)
    _Recorder.log = []
    net._create_engine()
    return list(_Recorder.log)


def test_ncf_engine_build_sets_mlp_dtype_then_the_option_before_the_first_layer(monkeypatch):
    log = _ncf_engine_calls(monkeypatch, accel_mlp_dtype="bf16", accel_mlp_bf16_fuse=1)
    fuse = [i for i, c in enumerate(log) if c[:2] == ("set_option", "mlp_bf16_fuse")]
    dtype = [i for i, c in enumerate(log) if c[:2] == ("set_option", "mlp_dtype")]
    layers = [i for i, c in enumerate(log) if c[0] == "set_fc"]
    assert layers and len(fuse) == 1 and len(dtype) == 1
    assert log[dtype[0]] == ("set_option", "mlp_dtype", N.MLP_BF16) and log[fuse[0]] == ("set_option", "mlp_bf16_fuse", 1)
    assert dtype[0] < fuse[0] < min(layers)


@pytest.mark.parametrize("flags", [{}, {"accel_mlp_dtype": "bf16"}, {"accel_mlp_bf16_fuse": 0},
                                   {"accel_mlp_dtype": "bf16", "accel_mlp_bf16_fuse": 0}])
def test_without_the_flag_an_ncf_engine_is_never_given_the_key(monkeypatch, flags):
    log = _ncf_engine_calls(monkeypatch, **flags)
    assert [c for c in log if c[0] == "set_fc"]
    assert [c for c in log if c[:2] == ("set_option", "mlp_bf16_fuse")] == []
