"""CPU side of DIN's narrow tables (engine option "din_table_dtype"): the --accel_din_table_dtype flag, when the host code
sets the option, and its refusal on every other model."""
import numpy as np
import pytest

from deeprecsys_amd import _native as N
from deeprecsys_amd import dlrm_s_hip
from deeprecsys_amd.utils.utils import FLAG_CHOICES, cli
from tests import helpers as H
from tests.test_half_tables_cpu import _Recorder

WORDS = {"fp32": N.TABLE_FP32, "fp16": N.TABLE_FP16, "bf16": N.TABLE_BF16, "fp8_e4m3": N.TABLE_FP8_E4M3}


def test_flag_takes_the_four_words_and_no_rowwise_type():
    assert cli([]).accel_din_table_dtype == "fp32" and FLAG_CHOICES["accel_din_table_dtype"] == tuple(WORDS)
    for w, v in WORDS.items():
        assert dlrm_s_hip._din_table_dtype(cli(["--accel_din_table_dtype", w]), N.MODEL_DIN) == v
    for bad in ("int8_rowwise", "int4_rowwise", "fp8"):
        with pytest.raises(SystemExit):
            cli(["--accel_din_table_dtype", bad])
    args = cli([])
    args.accel_din_table_dtype = "int8_rowwise"      # (a JSON config can set anything: refused at engine build)
    with pytest.raises(ValueError):
        dlrm_s_hip._din_table_dtype(args, N.MODEL_DIN)


@pytest.mark.parametrize("word", sorted(WORDS))
def test_din_sets_the_option_before_any_table_write_and_never_for_fp32(monkeypatch, word):
    meta, _ = H.load_fixture("din_mini")
    args = H.args_from(meta["args"], accel_din_table_dtype=word)
    np.random.seed(args.numpy_rand_seed)
    net = H.NET_CLS[args.model_type](args)
    monkeypatch.setattr(dlrm_s_hip.N, "Engine", _Recorder)
    _Recorder.log = log = []
    net._create_engine()
    calls = [i for i, c in enumerate(log) if c[:2] == ("set_option", "din_table_dtype")]
    writes = [i for i, c in enumerate(log) if c[0] in ("set_table", "fill_table_uniform")]
    creates = [i for i, c in enumerate(log) if c[0] == "create"]
    assert len(writes) == len(net.ln_emb) and creates and [c for c in log if c[:2] == ("set_option", "table_dtype")] == []
    # right after every engine is created, before anything else is set or written; an fp32 engine is never told
    assert calls == ([] if word == "fp32" else [c + 1 for c in creates]) and all(log[i][2] == WORDS[word] for i in calls)
    assert not calls or max(calls) < min(writes)


@pytest.mark.parametrize("case", ["dlrm_dot_small", "dien_mini"])
def test_another_model_refuses_the_flag_at_construction(case):
    meta, _ = H.load_fixture(case)
    np.random.seed(0)
    H.NET_CLS[meta["args"]["model_type"]](H.args_from(meta["args"], accel_din_table_dtype="fp32"))
    with pytest.raises(ValueError, match="accel_din_table_dtype"):
        H.NET_CLS[meta["args"]["model_type"]](H.args_from(meta["args"], accel_din_table_dtype="fp16"))
