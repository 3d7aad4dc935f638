"""CPU side of the fused bf16 launch (engine option "mlp_bf16_fuse"): the --accel_mlp_bf16_fuse flag and when the host code
sets the option, the documents that name the key, and the header's unchanged function set."""
import os
import re

import numpy as np
import pytest

from deeprecsys_amd import _native as N
from deeprecsys_amd import dlrm_s_hip
from deeprecsys_amd.utils.utils import cli
from tests import helpers as H
from tests.test_bf16_mlp_cpu import _Recorder

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_flag_defaults_to_off_and_takes_0_or_1():
    assert cli([]).accel_mlp_bf16_fuse == 0
    for v in (0, 1):
        assert cli(["--accel_mlp_bf16_fuse", str(v)]).accel_mlp_bf16_fuse == v
    with pytest.raises(SystemExit):
        cli(["--accel_mlp_bf16_fuse", "2"])
    args = cli([])
    args.accel_mlp_bf16_fuse = 3                                 # (a JSON config can set anything: refused at engine build)
    with pytest.raises(ValueError):
        dlrm_s_hip._mlp_bf16_fuse(args)


def _engine_calls(monkeypatch, **flags):
    meta, _ = H.load_fixture("dlrm_dot_small")
    args = H.args_from(meta["args"], **flags)
    np.random.seed(args.numpy_rand_seed)
    net = H.NET_CLS[args.model_type](args)
    monkeypatch.setattr(dlrm_s_hip.N, "Engine", _Recorder)
    _Recorder.log = []
    net._create_engine()
    return list(_Recorder.log)


def test_with_the_flag_the_option_follows_mlp_dtype_and_precedes_the_layers(monkeypatch):
    log = _engine_calls(monkeypatch, accel_mlp_dtype="bf16", accel_mlp_bf16_fuse=1)
    fuse = [i for i, c in enumerate(log) if c[:2] == ("set_option", "mlp_bf16_fuse")]
    dtype = [i for i, c in enumerate(log) if c[:2] == ("set_option", "mlp_dtype")]
    layers = [i for i, c in enumerate(log) if c[0] == "set_fc"]
    assert layers and len(fuse) == 1 and len(dtype) == 1
    assert log[fuse[0]] == ("set_option", "mlp_bf16_fuse", 1) and log[dtype[0]] == ("set_option", "mlp_dtype", N.MLP_BF16)
    assert dtype[0] < fuse[0] < min(layers)


@pytest.mark.parametrize("flags", [{}, {"accel_mlp_dtype": "bf16"}, {"accel_mlp_bf16_fuse": 0}])
def test_without_the_flag_the_key_is_never_set(monkeypatch, flags):
    """The CPU restatement of the ABI does not know the key: only a user who asked for it may reach it."""
    log = _engine_calls(monkeypatch, **flags)
    assert [c for c in log if c[0] == "set_fc"]
    assert [c for c in log if c[:2] == ("set_option", "mlp_bf16_fuse")] == []


def test_default_flags_set_nothing_on_the_cpu_abi(cpu_abi):
    meta, _ = H.load_fixture("dlrm_dot_small")
    net, lX, lS_l, lS_i, lT = H.materialize(H.args_from(meta["args"]))
    net.create(lX[0], lS_l[0], lS_i[0], lT[0])
    try:
        assert "mlp_bf16_fuse" not in net.engine.user_options
    finally:
        net.engine.close()


def test_header_and_options_document_name_the_key_and_the_function_set_is_unchanged():
    header = open(os.path.join(ROOT, "include", "drs.h")).read()
    assert '"mlp_bf16_fuse"' in header
    assert "`mlp_bf16_fuse`" in open(os.path.join(ROOT, "docs", "OPTIONS.md")).read()
    declared = set(re.findall(r"\b(drs_\w+)\s*\(", header))
    assert declared == set(name for name, _, _ in N.SYMBOLS), declared ^ set(name for name, _, _ in N.SYMBOLS)
    assert re.search(r"DRS_ABI_VERSION\s+5\b", header)
    # the product key count in the header's comment is the option table's
    table = open(os.path.join(ROOT, "deeprecsys_amd", "csrc", "engine_options.hip")).read()
    body = table[table.index("const OptDesc kOptions[] = {"):table.index("#undef OPT\n")]
    body = re.sub(r"#ifdef DRS_LAB\n.*?#else\n", "", body, flags=re.S)      # (the product's side of each #ifdef)
    keys = re.findall(r'^\s*(?:OPT|OPT_RO)\("(\w+)"|^\s*\{"(\w+)"', body, re.M)
    assert "mlp_bf16_fuse" in [a or b for a, b in keys]
