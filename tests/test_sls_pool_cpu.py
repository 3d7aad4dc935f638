"""CPU side of mean pooling (engine option "sls_pool", --accel_sls_pool): the flag and when the host code sets the
option, the documents, and the checker the GPU tests (tests/test_sls_pool.py) compare against -- a bag's mean is its
sequential fp32 sum divided by (float)len, one correctly rounded division per element, which is what torch's CPU
embedding_bag(mode="mean") computes, bit for bit; an empty bag is +0.0."""
import os

import numpy as np
import pytest

from deeprecsys_amd import _native as N
from deeprecsys_amd import dlrm_s_hip
from deeprecsys_amd.utils.utils import FLAG_CHOICES, cli
from oracle import oracle as orc
from tests import helpers as H
from tests.test_bf16_mlp_cpu import _Recorder

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the checker ------------------------------------------------------------------------------------------------------
def mean_of(sums, lens):
    """[bags, D] fp32 sums -> the means: numpy float32 / float32 (IEEE, correctly rounded); empty bags keep their +0.0"""
    sums = np.asarray(sums, dtype=np.float32)
    d = np.maximum(np.asarray(lens), 1).astype(np.float32)[:, None]
    out = sums / d
    assert out.dtype == np.float32
    return out


def torch_mean(W, idx, lens):
    """torch's CPU embedding_bag(mode="mean") of one table: [bags, D] fp32"""
    import torch
    import torch.nn.functional as F
    lens = np.asarray(lens, dtype=np.int64)
    off = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    out = F.embedding_bag(torch.from_numpy(np.ascontiguousarray(idx, dtype=np.int64)), torch.from_numpy(np.ascontiguousarray(W, dtype=np.float32)),
                          torch.from_numpy(off), mode="mean")
    return out.numpy()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("D", [4, 10, 64])
def test_torch_cpu_mean_is_the_sequential_sum_divided_by_the_length(D):
    """What the GPU tests compare against.  Passes without the feature: it pins the checker, not the engine."""
    rng = np.random.RandomState(D)
    rows = 997
    W = rng.uniform(-1, 1, (rows, D)).astype(np.float32)
    lens = np.array([0, 1, 2, 3, 7, 20, 80, 0, 80, 20, 7, 3, 2, 1, 0] * 3, dtype=np.int32)
    idx = rng.randint(0, rows, size=int(lens.sum())).astype(np.int64)
    want = mean_of(orc.sls(W, idx, lens), lens)
    got = torch_mean(W, idx, lens)
    assert same_bits(got, want)
    empty = lens == 0
    assert empty.sum() == 9 and same_bits(want[empty], np.zeros((9, D), np.float32))      # +0.0, not -0.0, not NaN
    # ... and it is a division: multiplying by the rounded reciprocal gives other bits somewhere
    recip = orc.sls(W, idx, lens) * (np.float32(1) / np.maximum(lens, 1).astype(np.float32))[:, None]
    assert not same_bits(recip, want)


# ---- flag -------------------------------------------------------------------------------------------------------------
def test_flag_defaults_to_sum_and_takes_sum_or_mean():
    assert cli([]).accel_sls_pool == "sum"
    for w in ("sum", "mean"):
        assert cli(["--accel_sls_pool", w]).accel_sls_pool == w
    assert FLAG_CHOICES["accel_sls_pool"] == ("sum", "mean")
    for bad in ("max", "1", "Mean"):
        with pytest.raises(SystemExit):
            cli(["--accel_sls_pool", bad])


def test_helper_maps_the_words_and_refuses_anything_else():
    assert (N.POOL_SUM, N.POOL_MEAN) == (0, 1)
    args = cli([])
    assert dlrm_s_hip._sls_pool(args) == N.POOL_SUM
    args.accel_sls_pool = "mean"
    assert dlrm_s_hip._sls_pool(args) == N.POOL_MEAN
    for bad in ("max", "avg", 1, "MEAN"):
        args.accel_sls_pool = bad                                # (a JSON config can set anything: refused at engine build)
        with pytest.raises(ValueError):
            dlrm_s_hip._sls_pool(args)
    del args.accel_sls_pool                                      # (a namespace from before the flag)
    assert dlrm_s_hip._sls_pool(args) == N.POOL_SUM


def _engine_calls(monkeypatch, **flags):
    meta, _ = H.load_fixture("dlrm_dot_small")
    args = H.args_from(meta["args"], **flags)
    np.random.seed(args.numpy_rand_seed)
    net = H.NET_CLS[args.model_type](args)
    monkeypatch.setattr(dlrm_s_hip.N, "Engine", _Recorder)
    _Recorder.log = []
    net._create_engine()
    return list(_Recorder.log)


@pytest.mark.parametrize("flags", [{}, {"accel_table_dtype": "int8_rowwise", "accel_table_int8_lines": 1}, {"accel_table_dtype": "fp16"},
                                   {"accel_mlp_dtype": "bf16", "accel_mlp_bf16_fuse": 1}])
def test_mean_adds_one_call_and_sum_adds_none(monkeypatch, flags):
    """The CPU restatement of the ABI does not know the key: only a user who asked for mean may reach it."""
    base = _engine_calls(monkeypatch, **flags)
    assert [c for c in base if c[0] == "set_fc"]
    assert [c for c in base if c[:2] == ("set_option", "sls_pool")] == []
    assert _engine_calls(monkeypatch, accel_sls_pool="sum", **flags) == base
    with_flag = _engine_calls(monkeypatch, accel_sls_pool="mean", **flags)
    creates = [c for c in with_flag if c[0] == "create"]
    pool = [c for c in with_flag if c[:2] == ("set_option", "sls_pool")]
    assert pool == [("set_option", "sls_pool", 1)] * len(creates) and creates
    assert [c for c in with_flag if c[:2] != ("set_option", "sls_pool")] == base
    writes = [i for i, c in enumerate(with_flag) if c[0] in ("set_table", "fill_table_uniform", "set_fc")]
    assert max(i for i, c in enumerate(with_flag) if c[:2] == ("set_option", "sls_pool")) < min(writes)


def test_default_flags_set_nothing_on_the_cpu_abi(cpu_abi):
    meta, _ = H.load_fixture("dlrm_dot_small")
    net, lX, lS_l, lS_i, lT = H.materialize(H.args_from(meta["args"]))
    net.create(lX[0], lS_l[0], lS_i[0], lT[0])
    try:
        assert "sls_pool" not in net.engine.user_options
    finally:
        net.engine.close()


# ---- documents --------------------------------------------------------------------------------------------------------
def test_documents_name_the_key():
    assert "`sls_pool`" in open(os.path.join(ROOT, "docs", "OPTIONS.md")).read()
    assert '"sls_pool" 0|1' in open(os.path.join(ROOT, "include", "drs.h")).read()
    assert "--accel_sls_pool" in open(os.path.join(ROOT, "README.md")).read()
