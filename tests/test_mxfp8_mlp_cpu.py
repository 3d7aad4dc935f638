"""CPU side of the MXFP8 FC layers (engine option "mlp_mxfp8"): the --accel_mlp_dtype mxfp8 word and when the host code sets
the option -- once, before the first layer, with no "mlp_dtype" and no "mlp_int8" beside it, and never for fp32."""
import numpy as np
import pytest

from deeprecsys_amd import dlrm_s_hip
from deeprecsys_amd.utils.utils import FLAG_CHOICES, cli
from tests import helpers as H
from tests.test_int8_mlp_cpu import _Recorder


@pytest.mark.parametrize("word", ["mxfp8", "fp32"])
def test_mlp_mxfp8_is_set_once_before_any_layer_and_never_for_fp32(monkeypatch, word):
    assert "mxfp8" in FLAG_CHOICES["accel_mlp_dtype"] and cli(["--accel_mlp_dtype", word]).accel_mlp_dtype == word
    meta, _ = H.load_fixture("dlrm_dot_small")
    args = H.args_from(meta["args"], accel_mlp_dtype=word)
    np.random.seed(args.numpy_rand_seed)
    net = H.NET_CLS[args.model_type](args)
    monkeypatch.setattr(dlrm_s_hip.N, "Engine", _Recorder)
    _Recorder.log = log = []
    net._create_engine()
    keys = [c[1] for c in log if c[0] == "set_option"]
    assert "mlp_dtype" not in keys and "mlp_int8" not in keys and keys.count("mlp_mxfp8") == (word == "mxfp8")
    if word == "mxfp8":
        assert log.index(("set_option", "mlp_mxfp8", 1)) < min(i for i, c in enumerate(log) if c[0] == "set_fc")
