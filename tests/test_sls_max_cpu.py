"""CPU side of max pooling (engine option "sls_max", --accel_sls_max): the flag, when the host code sets the option, and
the documents that name the key."""
import os

import pytest

from deeprecsys_amd import _native as N
from deeprecsys_amd import dlrm_s_hip
from deeprecsys_amd.utils.utils import FLAG_CHOICES, cli
from tests.test_sls_pool_cpu import ROOT, _engine_calls


def test_flag_defaults_to_0_and_takes_0_or_1():
    assert cli([]).accel_sls_max == 0 and FLAG_CHOICES["accel_sls_max"] == (0, 1) and N.POOL_MAX == 1
    assert cli(["--accel_sls_max", "1"]).accel_sls_max == 1
    for bad in ("2", "max", "-1"):
        with pytest.raises(SystemExit):
            cli(["--accel_sls_max", bad])
    args = cli([])
    assert dlrm_s_hip._sls_max(args) == 0
    args.accel_sls_max = 2                                       # (a JSON config can set anything: refused at engine build)
    with pytest.raises(ValueError):
        dlrm_s_hip._sls_max(args)
    del args.accel_sls_max                                       # (a namespace from before the flag)
    assert dlrm_s_hip._sls_max(args) == 0


@pytest.mark.parametrize("flags", [{}, {"accel_table_dtype": "int8_rowwise", "accel_table_int8_lines": 1}, {"accel_mlp_dtype": "bf16"}])
def test_max_adds_one_call_before_the_table_writes_and_the_default_adds_none(monkeypatch, flags):
    base = _engine_calls(monkeypatch, **flags)
    assert [c for c in base if c[:2] == ("set_option", "sls_max")] == []
    assert _engine_calls(monkeypatch, accel_sls_max=0, **flags) == base
    with_flag = _engine_calls(monkeypatch, accel_sls_max=1, **flags)
    creates = [c for c in with_flag if c[0] == "create"]
    calls = [i for i, c in enumerate(with_flag) if c[:2] == ("set_option", "sls_max")]
    assert [with_flag[i] for i in calls] == [("set_option", "sls_max", 1)] * len(creates) and creates
    assert [c for c in with_flag if c[:2] != ("set_option", "sls_max")] == base
    assert max(calls) < min(i for i, c in enumerate(with_flag) if c[0] in ("set_table", "fill_table_uniform", "set_fc"))


def test_documents_name_the_key():
    assert "`sls_max`" in open(os.path.join(ROOT, "docs", "OPTIONS.md")).read()
    assert '"sls_max" 0|1' in open(os.path.join(ROOT, "include", "drs.h")).read()
    assert "--accel_sls_max" in open(os.path.join(ROOT, "README.md")).read()
