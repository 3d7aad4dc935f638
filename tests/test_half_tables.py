"""Half-precision embedding tables on the GPU (-m gpu): engine option "table_dtype" 1 (fp16) / 2 (bf16).

The checker is the oracle run on the UPCAST tables -- W rounded to the table's element type and widened back to fp32
(numpy's float16, torch's bfloat16: both round to nearest even).  Every half gather form widens a row piece to fp32
before it sums, in the order of its fp32 twin: the sequential form is bit-identical to the oracle on the upcast tables,
and every form is bit-identical to an fp32 engine loaded with the upcast tables, under every option setting.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from deeprecsys_amd import _native as N
from oracle import oracle as orc
from tests import helpers as H

pytestmark = pytest.mark.gpu

DTYPES = {"fp16": N.TABLE_FP16, "bf16": N.TABLE_BF16}


def upcast(W, dtype):
    """W as a table of element type `dtype` holds it, widened back to fp32."""
    W = np.ascontiguousarray(W, dtype=np.float32)
    if dtype in ("fp16", N.TABLE_FP16):
        with np.errstate(over="ignore"):              # (overflow to +-inf is the rounding asked for)
            return W.astype(np.float16).astype(np.float32)
    import torch
    return torch.from_numpy(W).to(torch.bfloat16).to(torch.float32).numpy()


def _engine(rows, D, L, B, dtype, slots=2, staged=2):
    T = len(rows)
    eng = N.Engine(N.MODEL_DLRM, rows, D, [8, D], [D * (T + 1), 4, 1], N.INTERACT_CAT, sigmoid_top=2,
                   max_batch=B, max_lookups=L, num_staged_batches=staged, num_slots=slots)
    if dtype != N.TABLE_FP32:
        eng.set_option("table_dtype", dtype)
    return eng


def _load(eng, rng_seed, tables, D, T):
    rng = np.random.RandomState(rng_seed)
    for t in range(T):
        eng.set_table(t, tables[t])
    eng.set_fc(N.MLP_BOT, 0, rng.randn(D, 8).astype(np.float32), rng.randn(D).astype(np.float32))
    eng.set_fc(N.MLP_TOP, 0, rng.randn(4, D * (T + 1)).astype(np.float32) * 0.05, np.zeros(4, np.float32))
    eng.set_fc(N.MLP_TOP, 1, rng.randn(1, 4).astype(np.float32), np.zeros(1, np.float32))


# option settings every case runs under: (sls_exact, sls_flat, sls_one)
SETTINGS = [(1, 1, 1), (1, 1, 16), (1, 1, 64), (1, 1, 0), (0, 1, 1), (0, 0, 1), (0, 2, 1)]


@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("D", [4, 8, 10, 12, 16, 32, 64, 128, 256])
@pytest.mark.parametrize("L", [1, 20, 80, "ragged"])
def test_half_gather_matches_oracle_on_upcast_tables(dtype, D, L):
    """Every gather form a half engine reaches (sequential / split ring walk, one-lookup copy, flat and flat-coalesced,
    the any-width form for D = 10) against the oracle on the upcast tables: sequential order bitwise, wave-split within
    the fp32 split tolerance; and bitwise against an fp32 engine holding the upcast tables, for single queries and
    coalesced sets of 12 and 16."""
    rng = np.random.RandomState(D * 7 + (0 if L == "ragged" else L))
    T, B = 3, 48
    Lmax = 30 if L == "ragged" else L
    rows = [1501 + 13 * t for t in range(T)]
    tables = [rng.uniform(-1, 1, (r, D)).astype(np.float32) for r in rows]
    up = [upcast(W, dtype) for W in tables]
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
    half = _engine(rows, D, Lmax, B, DTYPES[dtype], slots=2)
    ref = _engine(rows, D, Lmax, B, N.TABLE_FP32, slots=2)
    try:
        assert half.get_option("table_dtype") == DTYPES[dtype] and ref.get_option("table_dtype") == 0
        _load(half, 11, tables, D, T)
        _load(ref, 11, up, D, T)
        for eng in (half, ref):
            for b in range(2):
                eng.stage_batch(b, dense[b], idx[b], lens[b])

        def pooled(b, bs):
            out = []
            for t in range(T):
                n = int(lens[b][t][:bs].sum())
                out.append(orc.sls(up[t], idx[b][t][:n], lens[b][t][:bs]))
            return np.concatenate(out, axis=1)
        jobs12 = [((k % 2), (B, 1, 17, 0)[k % 4]) for k in range(12)]
        jobs16 = [((k + 1) % 2, (5, B, 33, 1)[k % 4]) for k in range(16)]
        for exact, flat, one in SETTINGS:
            for eng in (half, ref):
                eng.set_option("sls_exact", exact)
                eng.set_option("sls_flat", flat)
                eng.set_option("sls_one", one)
            for b in range(2):
                for bs in (B, 1, 29):
                    got = half.forward(b, bs)
                    R = half.fetch_interaction(bs)
                    assert np.array_equal(got, ref.forward(b, bs)), (exact, flat, one, b, bs)
                    assert np.array_equal(R, ref.fetch_interaction(bs)), (exact, flat, one, b, bs)
                    if exact:
                        assert np.array_equal(R[:, D:], pooled(b, bs)), (exact, flat, one, b, bs)
                    else:
                        assert H.close(R[:, D:], pooled(b, bs), rtol=1e-5, atol_scale=2e-6), (flat, one, b, bs)
            for jobs in (jobs12, jobs16):
                outs = []
                for eng in (half, ref):
                    eng.forward_multi_async(1, [b for b, _ in jobs], [n for _, n in jobs])
                    outs.append(eng.wait(1, sum(n for _, n in jobs)))
                vrows = sum((n + 63) // 64 * 64 for _, n in jobs)
                Rh, Rr = half.fetch_interaction(vrows, slot=1), ref.fetch_interaction(vrows, slot=1)
                assert np.array_equal(outs[0], outs[1]) and np.array_equal(Rh, Rr), (exact, flat, one, len(jobs))
                v = 0
                for b, n in jobs:
                    if exact:
                        assert np.array_equal(Rh[v:v + n, D:], pooled(b, n)), (one, len(jobs), b, n)
                    else:
                        assert H.close(Rh[v:v + n, D:], pooled(b, n), rtol=1e-5, atol_scale=2e-6), (flat, len(jobs), b, n)
                    v += (n + 63) // 64 * 64
    finally:
        half.close()
        ref.close()


@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_rounding_edge_cases_through_one_lookup_bags(dtype):
    """Round to nearest even at ties, the largest finite value, overflow to infinity, subnormals, -0.0, +-inf and NaN:
    one-lookup bags copy each stored row out (0.0 + row), which equals the oracle on the upcast table -- bitwise where
    the value is not a NaN, and a NaN stays a NaN."""
    D, B = 16, 64
    vals = np.array([1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -11),
                     65504.0, 65519.0, 65520.0, -65520.0, 3.4e38, 1e-8, 3e-8, 1e-6, -1e-6, 6.1e-5, 1e-40,
                     -0.0, 0.0, np.inf, -np.inf, np.nan, -np.nan, 0.1, 1.0 / 3.0], dtype=np.float32)
    rows = (vals.size + D - 1) // D * 4
    W = np.zeros((rows, D), np.float32)
    W.reshape(-1)[:vals.size] = vals
    W.reshape(-1)[rows * D - vals.size:] = vals[::-1]
    up = upcast(W, dtype)
    eng = N.Engine(N.MODEL_DLRM, [rows], D, [8, D], [2 * D, 1], N.INTERACT_CAT, sigmoid_top=1,
                   max_batch=B, max_lookups=1, num_staged_batches=1, num_slots=1)
    try:
        eng.set_option("table_dtype", DTYPES[dtype])
        eng.set_table(0, W)
        eng.set_fc(N.MLP_BOT, 0, np.zeros((D, 8), np.float32), np.zeros(D, np.float32))
        eng.set_fc(N.MLP_TOP, 0, np.zeros((1, 2 * D), np.float32), np.zeros(1, np.float32))
        ix = (np.arange(B) % rows).astype(np.int64)
        eng.stage_batch(0, np.zeros((B, 8), np.float32), [ix], [np.ones(B, np.int32)])
        exp = orc.sls(up, ix, np.ones(B, np.int32))
        for one in (1, 0):                     # the copy form and the lane-group-per-bag sequential form
            eng.set_option("sls_exact", 1)
            eng.set_option("sls_one", one)
            eng.forward(0, B)
            got = eng.fetch_interaction(B)[:, D:]
            nan = np.isnan(exp)
            assert np.array_equal(np.isnan(got), nan), one
            assert np.array_equal(got[~nan].view(np.uint32), exp[~nan].view(np.uint32)), one
        # what the rounding must have produced (the upcast itself): fp16 overflow and its ties, kept subnormals
        if dtype == "fp16":
            assert np.isinf(up.reshape(-1)[7]) and up.reshape(-1)[6] == 65504.0 and up.reshape(-1)[12] != 0.0
            assert up.reshape(-1)[0] == 1.0 and up.reshape(-1)[1] == 1 + 2.0 ** -9
        else:
            assert up.reshape(-1)[2] == 1.0 and up.reshape(-1)[3] == 1 + 2.0 ** -6 and up.reshape(-1)[15] != 0.0
    finally:
        eng.close()


def _pooled_engine_state(eng, B, D):
    eng.set_option("sls_exact", 1)
    eng.forward(0, B)
    return eng.fetch_interaction(B)[:, D:].copy()


def test_every_table_writing_path():
    """set_table before / after the conversion, the device fill, 1 -> 0 -> placements, table_bytes."""
    rng = np.random.RandomState(3)
    rows, D, T, L, B = [2000, 1700], 64, 2, 20, 64
    tables = [rng.uniform(-1, 1, (r, D)).astype(np.float32) for r in rows]
    ix = [rng.randint(0, rows[t], size=B * L).astype(np.int64) for t in range(T)]
    ln = [np.full(B, L, np.int32) for _ in range(T)]
    X = rng.rand(B, 8).astype(np.float32)
    up = [upcast(W, "fp16") for W in tables]
    exp = np.concatenate([orc.sls(up[t], ix[t], ln[t]) for t in range(T)], axis=1)
    a = _engine(rows, D, L, B, N.TABLE_FP32, slots=1, staged=1)
    b = _engine(rows, D, L, B, N.TABLE_FP16, slots=1, staged=1)
    try:
        fp32_bytes = a.get_option("table_bytes")
        _load(a, 5, tables, D, T)            # set_table, then table_dtype 1: the device rounds the arena
        a.set_option("table_dtype", N.TABLE_FP16)
        _load(b, 5, tables, D, T)            # table_dtype 1, then set_table: rounded chunk by chunk on the device
        assert a.get_option("table_bytes") * 2 == fp32_bytes == b.get_option("table_bytes") * 2
        for e in (a, b):
            e.stage_batch(0, X, ix, ln)
        Ra, Rb = _pooled_engine_state(a, B, D), _pooled_engine_state(b, B, D)
        assert np.array_equal(Ra, exp) and np.array_equal(Rb, exp)
        # 1 -> 0: an fp32 arena holding the upcast values; then placement candidates of it
        a.set_option("table_dtype", N.TABLE_FP32)
        assert a.get_option("table_bytes") == fp32_bytes and a.get_option("table_placements") == 1
        assert np.array_equal(_pooled_engine_state(a, B, D), exp)
        a.set_option("table_placement", -1)
        assert a.get_option("table_placements") == 2 and np.array_equal(_pooled_engine_state(a, B, D), exp)
        a.set_option("table_placement", -2)
        assert a.get_option("table_placements") == 1 and np.array_equal(_pooled_engine_state(a, B, D), exp)
        # half placements: candidates are copies of the half arena, and the conversion frees them all
        b.set_option("table_placement", -1)
        assert b.get_option("table_placements") == 2 and np.array_equal(_pooled_engine_state(b, B, D), exp)
        b.set_option("table_dtype", N.TABLE_BF16)
        assert b.get_option("table_placements") == 1 and b.get_option("table_bytes") * 2 == fp32_bytes
        assert np.array_equal(_pooled_engine_state(b, B, D),
                              np.concatenate([orc.sls(upcast(up[t], "bf16"), ix[t], ln[t]) for t in range(T)], axis=1))
        # the device fill: fill_table_uniform's fp32 value, rounded
        for dt in ("fp16", "bf16"):
            b.set_option("table_dtype", DTYPES[dt])
            fills = []
            for t in range(T):
                b.fill_table_uniform(t, -0.25, 0.5, 77)
                fills.append(upcast(orc.fill_table_uniform(rows[t], D, t, -0.25, 0.5, 77, nthreads=0), dt))
            assert np.array_equal(_pooled_engine_state(b, B, D),
                                  np.concatenate([orc.sls(fills[t], ix[t], ln[t]) for t in range(T)], axis=1)), dt
        # values outside 0..2 are refused and change nothing
        with pytest.raises(N.DrsError) as e:
            b.set_option("table_dtype", 3)
        assert e.value.code == N.ERR_BAD_ARG and b.get_option("table_dtype") == N.TABLE_BF16
    finally:
        a.close()
        b.close()


def test_byte_accounting_and_launch_forms_follow_the_element_size():
    """drs_gather_bytes counts D * 2 bytes per gathered row of a half table, and the by-model defaults are those
    drs_create derives for the element size."""
    rows, D, T, L, B = [3000] * 4, 64, 4, 80, 32
    e = _engine(rows, D, L, B, N.TABLE_FP32, slots=3, staged=1)
    try:
        rng = np.random.RandomState(1)
        ix = [rng.randint(0, 3000, size=B * L).astype(np.int64) for _ in range(T)]
        e.stage_batch(0, rng.rand(B, 8).astype(np.float32), ix, [np.full(B, L, np.int32) for _ in range(T)])
        assert e.gather_bytes(0, B) == B * T * (L * D * 4 + L * 4 + 4 + D * 4)
        e.set_option("table_dtype", N.TABLE_FP16)
        assert e.gather_bytes(0, B) == B * T * (L * D * 2 + L * 4 + 4 + D * 4)
        for key in ("mlp_streams", "mlp_rows32", "mlp_stream_2cu", "preferred_slots", "preferred_coalesce", "gather_bound"):
            e.get_option(key)
    finally:
        e.close()


@pytest.mark.parametrize("case", [c for c in H.MODEL_CASES if not c.startswith(("din", "dien"))])
def test_models_with_fp16_tables_match_oracle_on_upcast_tables(case):
    meta, z = H.load_fixture(case)
    args = H.args_from(meta["args"], accel_table_dtype="fp16")
    net, lX, lS_l, lS_i, lT = H.materialize(args)
    net.create(lX[0], lS_l[0], lS_i[0], lT[0])
    try:
        assert net.engine.get_option("table_dtype") == N.TABLE_FP16
        emb = net.emb_w
        net.emb_w = [upcast(W, "fp16") for W in emb]
        om = H.oracle_model(net)
        net.emb_w = emb
        no_dense = args.model_type in H.NO_DENSE
        net.stage_batches(None if no_dense else lX, lS_l, lS_i)
        n = len(lS_l[0][0])
        net.engine.set_option("sls_exact", 1)
        for bid in range(len(lS_l)):
            for bs in sorted({n, 1, max(1, n // 2)}):
                got = net.run_staged(bid, bs)
                R = net.engine.fetch_interaction(bs)
                exp, R_exp = om.forward(None if no_dense else lX[bid], lS_i[bid], lS_l[bid], bs=bs, want_R=True)
                assert np.array_equal(R, R_exp), (case, bid, bs)
                assert H.close(got, exp, rtol=1e-6, atol=1e-7), (case, np.abs(got - exp).max())
    finally:
        net.engine.close()


def test_rmc1_shape_with_fp16_tables_in_pipelined_sets_of_12():
    """The bench's RMC1 shape (8 x 1M x 64, L 80, 256 samples) with fp16 tables filled on the device, served as bench.py
    serves it: the default flat-coalesced gather, sets of 12 queries, 3 sets in flight -- every query against the oracle
    on the upcast tables."""
    from deeprecsys_amd.data_generator.dlrm_data import generate_fast_input_data
    rows, D, T, L, B, seed = 1_000_000, 64, 8, 80, 256, 99
    args = H.args_from({}, arch_sparse_feature_size=D, arch_embedding_size="-".join([str(rows)] * T),
                       arch_mlp_bot="128-64-64", arch_mlp_top="256-64-1", arch_interaction_op="cat",
                       num_indices_per_lookup=L, num_batches=2, max_mini_batch_size=B, mini_batch_size=B,
                       numpy_rand_seed=seed, accel_table_init="device", model_type="dlrm", accel_slots=3,
                       accel_table_dtype="fp16")
    np.random.seed(seed)
    net = H.M.DLRM_Net(args)
    _, lX, lS_l, lS_i = generate_fast_input_data(2, B, 128, [rows] * T, L, seed)
    net.create(lX[0], lS_l[0], lS_i[0], None)
    try:
        eng = net.engine
        net.stage_batches(lX, lS_l, lS_i)
        lo, hi = -float(np.sqrt(1 / rows)), float(np.sqrt(1 / rows))
        net.emb_w = [upcast(orc.fill_table_uniform(rows, D, t, lo, hi, seed, nthreads=0), "fp16") for t in range(T)]
        om = H.oracle_model(net)
        # (half the gathered bytes: the engine's own estimate now puts RMC1 "in between" -- its MLP launch outlasts the
        # gather -- and it asks for 16-query sets on two MLP streams; the sets below stay the bench's 12)
        assert eng.get_option("table_dtype") == N.TABLE_FP16 and eng.get_option("preferred_coalesce") in (12, 16)
        assert eng.get_option("sls_exact") == 0 and eng.get_option("shared_stream") == 2
        ref = {}
        sets = [[((s + k) % 2, 256 if (s + k) % 5 else 165) for k in range(12)] for s in range(3)]
        for rnd in range(2):
            for s in range(3):
                eng.forward_multi_async(s, [b for b, _ in sets[s]], [n for _, n in sets[s]])
            outs = [eng.wait(s, sum(n for _, n in sets[s])) for s in range(3)]
        assert any(",f16>" in d for d in eng.last_dispatch()), eng.last_dispatch()
        for s in range(3):
            Rv = eng.fetch_interaction(256 * 12, slot=s)
            o = v = 0
            for k, (bid, n) in enumerate(sets[s]):
                if (bid, n) not in ref:
                    ref[(bid, n)] = om.forward(lX[bid], lS_i[bid], lS_l[bid], bs=n, want_R=True, nthreads=0)
                exp, R_exp = ref[(bid, n)]
                assert H.close(Rv[v:v + n], R_exp, rtol=1e-5, atol_scale=2e-6), (s, k)
                assert H.close(outs[s][o:o + n], exp, rtol=H.RTOL_OUT, atol=1e-7), (s, k)
                o += n
                v += (n + 63) // 64 * 64
    finally:
        net.engine.close()


@pytest.mark.parametrize("case", ["din_mini", "dien_mini"])
def test_din_and_dien_refuse_half_tables_and_keep_serving_fp32(case):
    meta, z = H.load_fixture(case)
    args = H.args_from(meta["args"])
    net, lX, lS_l, lS_i, lT = H.materialize(args)
    om = H.oracle_model(net)
    net.create(lX[0], lS_l[0], lS_i[0], lT[0])
    try:
        eng = net.engine
        net.stage_batches(None, lS_l, lS_i)
        n = len(lS_l[0][0])
        eng.set_option("sls_exact", 1)
        before = net.run_staged(0, n).copy()
        R0 = eng.fetch_interaction(n).copy()
        for v in (N.TABLE_FP16, N.TABLE_BF16):
            with pytest.raises(N.DrsError) as e:
                eng.set_option("table_dtype", v)
            assert e.value.code == N.ERR_UNSUPPORTED
        with pytest.raises(N.DrsError) as e:
            eng.set_option("table_dtype", 3)
        assert e.value.code == N.ERR_BAD_ARG
        eng.set_option("table_dtype", N.TABLE_FP32)          # (what it is: nothing to do)
        assert eng.get_option("table_dtype") == N.TABLE_FP32
        assert np.array_equal(net.run_staged(0, n), before) and np.array_equal(eng.fetch_interaction(n), R0)
        _, R_exp = om.forward(None, lS_i[0], lS_l[0], bs=n, want_R=True)
        if case == "din_mini":
            assert np.array_equal(R0, R_exp)
    finally:
        net.engine.close()


def test_dispatch_log_carries_the_dtype_token():
    rows, D, T, L, B = [5000] * 4, 64, 4, 80, 64
    rng = np.random.RandomState(2)
    tables = [rng.uniform(-1, 1, (r, D)).astype(np.float32) for r in rows]
    ix = [rng.randint(0, rows[t], size=B * L).astype(np.int64) for t in range(T)]
    ln = [np.full(B, L, np.int32) for _ in range(T)]
    e = _engine(rows, D, L, B, N.TABLE_FP32, slots=1, staged=1)
    try:
        e.set_option("dispatch_log", 1)
        _load(e, 1, tables, D, T)
        e.stage_batch(0, rng.rand(B, 8).astype(np.float32), ix, ln)
        e.forward(0, B)
        d32 = " ".join(e.last_dispatch())
        assert "sls_flatc_kernel<16,20,nt>" in d32 and "f16" not in d32
        for name, dt in (("f16", N.TABLE_FP16), ("bf16", N.TABLE_BF16)):
            e.set_option("table_dtype", dt)
            e.forward(0, B)
            d = " ".join(e.last_dispatch())
            assert "sls_flatc_kernel<16,20,nt,%s>" % name in d, d
            e.set_option("sls_exact", 1)
            e.forward(0, B)
            assert "sls_kernel<16,sequential,%s>" % name in " ".join(e.last_dispatch())
            e.set_option("sls_exact", 0)
    finally:
        e.close()


def test_stand_alone_entry_and_queue_harness_with_fp16_tables(tmp_path):
    """`python -m deeprecsys_amd.dlrm_s_hip --accel_table_dtype fp16` prints its `***` lines, and a short
    `DeepRecSys.py --queue --model_accel` run serves its queries from fp16 tables."""
    import json
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = dict(arch_mlp_bot="16-8", arch_mlp_top="64-16-1", arch_embedding_size="-".join(["3000"] * 6),
               arch_sparse_feature_size=8, num_indices_per_lookup_fixed=True, num_indices_per_lookup=20,
               arch_interaction_op="dot", model_type="dlrm", model_name="mini")
    path = str(tmp_path / "mini.json")
    json.dump(cfg, open(path, "w"))
    r = subprocess.run([sys.executable, "-m", "deeprecsys_amd.dlrm_s_hip", "--inference_only", "--use_accel",
                        "--config_file", path, "--nepochs", "3", "--num_batches", "2", "--mini_batch_size", "64",
                        "--max_mini_batch_size", "64", "--accel_table_dtype", "fp16"],
                       cwd=root, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.count("***") == 6, r.stdout[-2000:]
    r = subprocess.run([sys.executable, "-m", "deeprecsys_amd.DeepRecSys", "--queue", "--model_accel",
                        "--inference_engines", "0", "--config_file", path, "--num_batches", "4", "--nepochs", "1",
                        "--avg_arrival_rate", "1", "--max_mini_batch_size", "64", "--avg_mini_batch_size", "32",
                        "--accel_table_dtype", "fp16", "--accel_table_placements", "1",
                        "--log_file", str(tmp_path / "log" / "out.log")],
                       cwd=root, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert len(open(str(tmp_path / "log" / "out.log")).read().strip().splitlines()) == 4
