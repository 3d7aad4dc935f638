"""Mean pooling on the GPU (-m gpu): engine option "sls_pool" 1, --accel_sls_pool mean.

The contract (docs/OPTIONS.md): every bag's pooled vector is the fp32 sum the same gather form computes under "sls_pool" 0,
divided by (float)len -- one correctly rounded fp32 division per element, an empty bag stays +0.0.  Three checkers:
  * a sum engine holding the same tables: pooled columns / bag lengths in numpy fp32, bit for bit, under every gather form
    and stored type;
  * torch's CPU embedding_bag(mode="mean") for the sequential order on fp32 tables (tests/test_sls_pool_cpu.py pins that
    it is the sequential sum / len);
  * whole models with a fixed bag length of 4: the oracle on tables / 4 (scaling by a power of two commutes with fp32
    addition away from underflow).
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from deeprecsys_amd import _native as N
from oracle import oracle as orc
from tests import helpers as H
from tests.test_half_tables import SETTINGS, _load, upcast
from tests.test_sls_pool_cpu import mean_of, same_bits, torch_mean

pytestmark = pytest.mark.gpu

# stored types: name -> (table_dtype, table_int8_lines)
TYPES = {"fp32": (N.TABLE_FP32, 0), "fp16": (N.TABLE_FP16, 0), "bf16": (N.TABLE_BF16, 0),
         "int8": (N.TABLE_INT8_ROWWISE, 0), "int8_lines": (N.TABLE_INT8_ROWWISE, 1)}


def _engine(rows, D, L, B, kind, pool, slots=2, staged=2):
    T = len(rows)
    eng = N.Engine(N.MODEL_DLRM, rows, D, [8, D], [D * (T + 1), 4, 1], N.INTERACT_CAT, sigmoid_top=2,
                   max_batch=B, max_lookups=L, num_staged_batches=staged, num_slots=slots)
    dtype, lines = TYPES[kind]
    if lines:
        eng.set_option("table_int8_lines", 1)
    if dtype != N.TABLE_FP32:
        eng.set_option("table_dtype", dtype)
    if pool:
        eng.set_option("sls_pool", pool)
    return eng


def _divisors(lens_b, bs, D):
    """[bs, T * D]: the bag length under every pooled column"""
    return np.concatenate([np.repeat(np.asarray(l[:bs])[:, None], D, axis=1) for l in lens_b], axis=1)


def _mean_rows(R_sum, lens_b, bs, D):
    T = len(lens_b)
    return np.concatenate([mean_of(R_sum[:, D + t * D:D + (t + 1) * D], lens_b[t][:bs]) for t in range(T)], axis=1)


# ------------------------------------------------------------------------------------------------------------------------
# 1. every form, every stored type
@pytest.mark.parametrize("kind", sorted(TYPES))
@pytest.mark.parametrize("D", [8, 10, 16, 32, 64, 128])
@pytest.mark.parametrize("L", [1, 2, 20, 80, "ragged"])
def test_mean_is_the_same_forms_sum_divided_by_the_bag_length(kind, D, L):
    """Sequential / split ring walk, one-lookup copy, flat and flat-coalesced, the any-width form (D = 10), the line-packed
    int8 layout (D = 32): the mean engine's pooled columns are the sum engine's divided by the bag lengths, bit for bit,
    for single queries and coalesced sets of 12 and 16; empty bags are +0.0; the bottom-MLP columns are the same."""
    rng = np.random.RandomState(D * 7 + (0 if L == "ragged" else L))
    T, B = 3, 48
    Lmax = 30 if L == "ragged" else L
    rows = [1501 + 13 * t for t in range(T)]
    tables = [rng.uniform(-1, 1, (r, D)).astype(np.float32) for r in rows]
    idx, lens = [], []
    for b in range(2):
        if L == "ragged":
            ln = [rng.randint(0, Lmax + 1, size=B).astype(np.int32) for _ in range(T)]
            for t in range(T):
                ln[t][:3] = 0                                          # empty bags
        else:
            ln = [np.full(B, L, np.int32) for _ in range(T)]
        ix = [rng.randint(0, rows[t], size=int(ln[t].sum())).astype(np.int64) for t in range(T)]
        for t in range(T):
            if ix[t].size:
                ix[t][0], ix[t][-1] = 0, rows[t] - 1
        idx.append(ix)
        lens.append(ln)
    dense = [rng.rand(B, 8).astype(np.float32) for _ in range(2)]
    mean = _engine(rows, D, Lmax, B, kind, 1)
    ssum = _engine(rows, D, Lmax, B, kind, 0)
    try:
        assert mean.get_option("sls_pool") == 1 and ssum.get_option("sls_pool") == 0
        for eng in (mean, ssum):
            _load(eng, 11, tables, D, T)
            for b in range(2):
                eng.stage_batch(b, dense[b], idx[b], lens[b])
        torch_ref = {}

        def torch_rows(b, bs):
            if (b, bs) not in torch_ref:
                torch_ref[(b, bs)] = np.concatenate(
                    [torch_mean(tables[t], idx[b][t][:int(lens[b][t][:bs].sum())], lens[b][t][:bs]) for t in range(T)], axis=1)
            return torch_ref[(b, bs)]

        def check(Rm, Rs, b, bs, exact, where):
            assert same_bits(Rm[:, :D], Rs[:, :D]), where                         # the bottom MLP's columns
            assert same_bits(Rm[:, D:], _mean_rows(Rs, lens[b], bs, D)), where
            empty = _divisors(lens[b], bs, D) == 0
            assert not np.any(Rm[:, D:].view(np.uint32)[empty]), where           # +0.0: no 0 / 0, no -0.0
            if exact and kind == "fp32":
                assert same_bits(Rm[:, D:], torch_rows(b, bs)), where

        jobs12 = [((k % 2), (B, 1, 17, 0)[k % 4]) for k in range(12)]
        jobs16 = [((k + 1) % 2, (5, B, 33, 1)[k % 4]) for k in range(16)]
        for exact, flat, one in SETTINGS:
            for eng in (mean, ssum):
                eng.set_option("sls_exact", exact)
                eng.set_option("sls_flat", flat)
                eng.set_option("sls_one", one)
            for b in range(2):
                for bs in (B, 1, 29):
                    mean.forward(b, bs)
                    ssum.forward(b, bs)
                    check(mean.fetch_interaction(bs), ssum.fetch_interaction(bs), b, bs, exact, (exact, flat, one, b, bs))
            for jobs in (jobs12, jobs16):
                for eng in (mean, ssum):
                    eng.forward_multi_async(1, [b for b, _ in jobs], [n for _, n in jobs])
                    eng.wait(1, sum(n for _, n in jobs))
                vrows = sum((n + 63) // 64 * 64 for _, n in jobs)
                Rm, Rs = mean.fetch_interaction(vrows, slot=1), ssum.fetch_interaction(vrows, slot=1)
                v = 0
                for b, n in jobs:                                                # (pad rows between queries: not compared)
                    if n:
                        check(Rm[v:v + n], Rs[v:v + n], b, n, exact, (exact, flat, one, len(jobs), b, n))
                    v += (n + 63) // 64 * 64
    finally:
        mean.close()
        ssum.close()


# ------------------------------------------------------------------------------------------------------------------------
# 2. a division, not a reciprocal; subnormal means
def test_the_kernel_divides_and_keeps_subnormal_means():
    D, rows = 16, 4096
    rng = np.random.RandomState(77)
    W = rng.uniform(-1, 1, (rows, D)).astype(np.float32)
    W[rows - 1] = np.float32(1e-38)                                              # 80 of these: the mean 1e-38 is subnormal
    lens = np.array([3, 7, 11, 80] * 4 + [80], dtype=np.int32)
    B = lens.size
    idx = rng.randint(0, rows - 1, size=int(lens.sum())).astype(np.int64)
    idx[-80:] = rows - 1
    sums = orc.sls(W, idx, lens)
    want = mean_of(sums, lens)
    # the case cannot go blind: in every bag the quotient and the product with the rounded reciprocal differ somewhere
    recip = sums * (np.float32(1) / lens.astype(np.float32))[:, None]
    differs = (recip.view(np.uint32) != want.view(np.uint32)).any(axis=1)
    assert differs[:-1].all(), differs
    tiny = np.float32(np.finfo(np.float32).tiny)
    assert np.all(want[-1] > 0) and np.all(want[-1] < tiny) and np.all(sums[-1] >= tiny)
    eng = N.Engine(N.MODEL_DLRM, [rows], D, [8, D], [2 * D, 1], N.INTERACT_CAT, sigmoid_top=1,
                   max_batch=B, max_lookups=80, num_staged_batches=1, num_slots=1)
    try:
        eng.set_table(0, W)
        eng.set_fc(N.MLP_BOT, 0, np.zeros((D, 8), np.float32), np.zeros(D, np.float32))
        eng.set_fc(N.MLP_TOP, 0, np.zeros((1, 2 * D), np.float32), np.zeros(1, np.float32))
        eng.stage_batch(0, np.zeros((B, 8), np.float32), [idx], [lens])
        eng.set_option("sls_exact", 1)
        eng.forward(0, B)
        assert same_bits(eng.fetch_interaction(B)[:, D:], sums)
        eng.set_option("sls_pool", 1)
        eng.forward(0, B)
        got = eng.fetch_interaction(B)[:, D:]
        assert same_bits(got, want), np.argwhere(got.view(np.uint32) != want.view(np.uint32))[:8]
        assert same_bits(got, torch_mean(W, idx, lens))
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------------------------------
# 3. whole models
def _model_case(case, **flags):
    meta, z = H.load_fixture(case)
    dlrm = meta["args"].get("model_type", "dlrm") == "dlrm"
    if dlrm:
        flags.update(num_indices_per_lookup=4, num_indices_per_lookup_fixed=True)
    args = H.args_from(meta["args"], accel_sls_pool="mean", **flags)
    net, lX, lS_l, lS_i, lT = H.materialize(args)
    net.create(lX[0], lS_l[0], lS_i[0], lT[0])
    try:
        eng = net.engine
        assert eng.get_option("sls_pool") == 1
        assert all(np.all(l == (4 if dlrm else 1)) for per in lS_l for l in per)
        emb = net.emb_w
        up = [upcast(W, "fp16") for W in emb] if flags.get("accel_table_dtype") == "fp16" else emb
        net.emb_w = [W / np.float32(4) for W in up] if dlrm else up              # the mean of 4 rows of W: the sum of 4 rows of W / 4
        om = H.oracle_model(net)
        net.emb_w = emb
        no_dense = args.model_type in H.NO_DENSE
        net.stage_batches(None if no_dense else lX, lS_l, lS_i)
        n = len(lS_l[0][0])
        eng.set_option("sls_exact", 1)
        for bid in range(len(lS_l)):
            for bs in sorted({n, 1, max(1, n // 2)}):
                got = net.run_staged(bid, bs)
                R = eng.fetch_interaction(bs)
                exp, R_exp = om.forward(None if no_dense else lX[bid], lS_i[bid], lS_l[bid], bs=bs, want_R=True)
                assert same_bits(R, R_exp), (case, bid, bs)
                assert H.close(got, exp, rtol=1e-6, atol=1e-7), (case, np.abs(got - exp).max())
    finally:
        net.engine.close()


@pytest.mark.parametrize("case", ["dlrm_rm1_mini", "dlrm_dot_small", "dlrm_cat_small", "ncf_mini", "wnd_mini", "mtwnd_mini"])
def test_models_with_mean_pooling_match_the_oracle_on_scaled_tables(case):
    _model_case(case)


def test_rm1_mini_with_mean_pooling_and_fp16_tables():
    _model_case("dlrm_rm1_mini", accel_table_dtype="fp16")


# ------------------------------------------------------------------------------------------------------------------------
# 4. option behaviour
def _small(kind="fp32", pool=0, D=32, L=20, T=4, B=32, rows=3000, seed=4):
    rng = np.random.RandomState(seed)
    tables = [rng.uniform(-1, 1, (rows, D)).astype(np.float32) for _ in range(T)]
    ix = [rng.randint(0, rows, size=B * L).astype(np.int64) for _ in range(T)]
    ln = [np.full(B, L, np.int32) for _ in range(T)]
    eng = _engine([rows] * T, D, L, B, kind, pool, slots=1, staged=1)
    return eng, tables, rng.rand(B, 8).astype(np.float32), ix, ln


def test_option_reads_back_and_bad_values_change_nothing():
    D, T, B = 32, 4, 32
    eng, tables, X, ix, ln = _small()
    try:
        _load(eng, 3, tables, D, T)
        eng.stage_batch(0, X, ix, ln)
        nbytes = eng.gather_bytes(0, B)
        assert eng.get_option("sls_pool") == 0
        eng.forward(0, B)
        R0 = eng.fetch_interaction(B).copy()
        eng.set_option("sls_pool", N.POOL_MEAN)
        assert eng.get_option("sls_pool") == 1 and eng.gather_bytes(0, B) == nbytes
        for bad in (2, -1, 7):
            with pytest.raises(N.DrsError) as e:
                eng.set_option("sls_pool", bad)
            assert e.value.code == N.ERR_BAD_ARG and eng.get_option("sls_pool") == 1
        eng.forward(0, B)
        R1 = eng.fetch_interaction(B).copy()
        assert same_bits(R1[:, D:], _mean_rows(R0, ln, B, D)) and not same_bits(R1, R0)
        eng.set_option("sls_pool", N.POOL_SUM)                                   # 1 then 0: the sum engine's bits again
        assert eng.get_option("sls_pool") == 0
        eng.forward(0, B)
        assert same_bits(eng.fetch_interaction(B), R0)
    finally:
        eng.close()


def test_either_order_with_the_table_options_gives_the_same_bits():
    D, T, B, L, rows = 32, 4, 32, 20, 3000
    first, tables, X, ix, ln = _small("int8_lines", 1)                           # table_int8_lines, table_dtype, sls_pool, set_table
    last = N.Engine(N.MODEL_DLRM, [rows] * T, D, [8, D], [D * (T + 1), 4, 1], N.INTERACT_CAT, sigmoid_top=2,
                    max_batch=B, max_lookups=L, num_staged_batches=1, num_slots=1)
    try:
        last.set_option("sls_pool", 1)                                           # sls_pool, set_table, table_dtype, table_int8_lines
        _load(first, 3, tables, D, T)
        _load(last, 3, tables, D, T)
        last.set_option("table_dtype", N.TABLE_INT8_ROWWISE)
        last.set_option("table_int8_lines", 1)
        assert last.get_option("sls_pool") == 1 and first.get_option("table_bytes") == last.get_option("table_bytes")
        outs = []
        for eng in (first, last):
            eng.stage_batch(0, X, ix, ln)
            outs.append(eng.forward(0, B).copy())
            outs.append(eng.fetch_interaction(B).copy())
        assert same_bits(outs[0], outs[2]) and same_bits(outs[1], outs[3])
    finally:
        first.close()
        last.close()


def test_dispatch_log_carries_the_mean_token_only_under_mean():
    D, T, B = 64, 4, 64
    eng, tables, X, ix, ln = _small(D=D, L=80, B=B, rows=5000)
    try:
        eng.set_option("dispatch_log", 1)
        _load(eng, 1, tables, D, T)
        eng.stage_batch(0, X, ix, ln)
        eng.forward(0, B)
        d = " ".join(eng.last_dispatch())
        assert "sls_flatc_kernel<16,20,nt>" in d and "mean" not in d, d
        eng.set_option("sls_pool", 1)
        eng.forward(0, B)
        assert "sls_flatc_kernel<16,20,nt,mean>" in " ".join(eng.last_dispatch()), eng.last_dispatch()
        eng.set_option("sls_exact", 1)
        eng.forward(0, B)
        assert "sls_kernel<16,sequential,mean>" in " ".join(eng.last_dispatch()), eng.last_dispatch()
        eng.set_option("table_dtype", N.TABLE_FP16)
        eng.forward(0, B)
        assert "sls_kernel<16,sequential,f16,mean>" in " ".join(eng.last_dispatch()), eng.last_dispatch()
        eng.set_option("sls_pool", 0)
        eng.forward(0, B)
        d = " ".join(eng.last_dispatch())
        assert "sls_kernel<16,sequential,f16>" in d and "mean" not in d, d
    finally:
        eng.close()


@pytest.mark.parametrize("case", ["din_mini", "dien_mini"])
def test_din_and_dien_refuse_mean_and_keep_serving_the_same_bits(case):
    meta, z = H.load_fixture(case)
    net, lX, lS_l, lS_i, lT = H.materialize(H.args_from(meta["args"]))
    net.create(lX[0], lS_l[0], lS_i[0], lT[0])
    try:
        eng = net.engine
        net.stage_batches(None, lS_l, lS_i)
        n = len(lS_l[0][0])
        before = net.run_staged(0, n).copy()
        R0 = eng.fetch_interaction(n).copy()
        with pytest.raises(N.DrsError) as e:
            eng.set_option("sls_pool", 1)
        assert e.value.code == N.ERR_UNSUPPORTED and "sls_pool" in str(e.value)
        with pytest.raises(N.DrsError) as e:
            eng.set_option("sls_pool", 2)
        assert e.value.code == N.ERR_BAD_ARG
        assert eng.get_option("sls_pool") == 0
        eng.set_option("sls_pool", 0)                                            # (what it is: nothing to do)
        assert same_bits(net.run_staged(0, n), before) and same_bits(eng.fetch_interaction(n), R0)
    finally:
        net.engine.close()


# ------------------------------------------------------------------------------------------------------------------------
# 5. the stand-alone operator follows the handle
@pytest.mark.parametrize("D", [10, 64])
def test_drs_sls_follows_the_handle(D):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    rng = np.random.RandomState(D)
    rows, bags, L = 5003, 257, 40
    W = rng.uniform(-1, 1, (rows, D)).astype(np.float32)
    lengths = rng.randint(0, L + 1, size=bags).astype(np.int32)
    lengths[5] = 0
    idx = rng.randint(0, rows, size=int(lengths.sum())).astype(np.int32)
    sums = orc.sls(W, idx, lengths)
    eng = N.Engine(N.MODEL_DLRM, [16, 16], 8, [4, 8], [24, 4, 1], N.INTERACT_CAT, sigmoid_top=2,
                   max_batch=4, max_lookups=2, num_staged_batches=1, num_slots=1)
    try:
        dW, di, dl = (torch.from_numpy(a).cuda() for a in (W, idx, lengths))
        out = torch.full((bags, D), float("nan"), device="cuda")
        for pool, want in ((1, mean_of(sums, lengths)), (0, sums)):
            eng.set_option("sls_pool", pool)
            out.fill_(float("nan"))
            torch.cuda.synchronize()   # inputs/outputs were produced on torch's stream, the op runs on the engine's
            eng.sls(dW.data_ptr(), rows, D, di.data_ptr(), dl.data_ptr(), bags, idx.size, out.data_ptr(), exact_order=True)
            assert same_bits(out.cpu().numpy(), want), (D, pool)
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------------------------------
# 6. the stand-alone entry
def test_stand_alone_entry_with_mean_pooling(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = dict(arch_mlp_bot="16-8", arch_mlp_top="64-16-1", arch_embedding_size="-".join(["3000"] * 6),
               arch_sparse_feature_size=8, num_indices_per_lookup_fixed=True, num_indices_per_lookup=20,
               arch_interaction_op="dot", model_type="dlrm", model_name="mini")
    path = str(tmp_path / "mini.json")
    json.dump(cfg, open(path, "w"))
    r = subprocess.run([sys.executable, "-m", "deeprecsys_amd.dlrm_s_hip", "--inference_only", "--use_accel",
                        "--config_file", path, "--nepochs", "3", "--num_batches", "2", "--mini_batch_size", "64",
                        "--max_mini_batch_size", "64", "--accel_sls_pool", "mean"],
                       cwd=root, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.count("***") == 6, r.stdout[-2000:]
