"""Per-sample weights on the GPU (-m gpu): drs_stage_batch_weights, drs_sls_weighted, --accel_sls_weights.

The checker is tests/test_sls_weights_cpu.py's `weighted_ref` (and its rowwise twin): per bag the sequential chain
acc = fma(w, x, acc), which that file pins to torch's CPU operators bit for bit.  Under "sls_exact" 1 the engine's pooled
columns equal it bit for bit for every stored type (half types: on the upcast table; rowwise types: on torch's codes);
under "sls_exact" 0 they are held to the split order's tolerance of tests/test_gpu_parity.py.  Weights of 1.0 (or NULL)
give the unweighted engine's bits, and an unweighted query keeps its sequential bits inside a weighted launch set.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from deeprecsys_amd import _native as N
from deeprecsys_amd import dlrm_s_hip
from oracle import oracle as orc
from tests import helpers as H
from tests.test_half_tables import _load, upcast
from tests.test_sls_weights_cpu import codes4, codes8, same_bits, weighted_ref, weighted_ref_rowwise

pytestmark = pytest.mark.gpu

# stored types: name -> (table_dtype, the line-packing option to set first or None)
TYPES = {"fp32": (N.TABLE_FP32, None), "fp16": (N.TABLE_FP16, None), "bf16": (N.TABLE_BF16, None),
         "int8": (N.TABLE_INT8_ROWWISE, None), "int8_lines": (N.TABLE_INT8_ROWWISE, "table_int8_lines"),
         "int4": (N.TABLE_INT4_ROWWISE, None), "int4_lines": (N.TABLE_INT4_ROWWISE, "table_int4_lines")}
# ... and the types _engine builds besides: the weighted cases of fp8 tables are tests/test_fp8_tables.py's
ENGINE_TYPES = dict(TYPES, fp8=(N.TABLE_FP8_E4M3, None))
T, B = 3, 48
ROWS = [1501 + 13 * t for t in range(T)]


def _engine(rows, D, L, B_, kind, slots=2, staged=3):
    n = len(rows)
    eng = N.Engine(N.MODEL_DLRM, rows, D, [8, D], [D * (n + 1), 4, 1], N.INTERACT_CAT, sigmoid_top=2,
                   max_batch=B_, max_lookups=L, num_staged_batches=staged, num_slots=slots)
    dtype, lines = ENGINE_TYPES[kind]
    if lines:
        eng.set_option(lines, 1)
    if dtype != N.TABLE_FP32:
        eng.set_option("table_dtype", dtype)
    return eng


def _stored(kind, W):
    """what the engine's table of this type holds, in the form the reference takes: an fp32 table, or (codes, scale, bias)"""
    if kind == "fp32":
        return np.ascontiguousarray(W, np.float32)
    if kind in ("fp16", "bf16"):
        return upcast(W, kind)
    return (codes8(W) if kind.startswith("int8") else codes4(W))[1:]


def _ref(stored, idx, lens, w):
    if isinstance(stored, tuple):
        return weighted_ref_rowwise(stored[0], stored[1], stored[2], idx, lens, w)
    return weighted_ref(stored, idx, lens, w)


def _inputs(rng, L):
    """three input sets: [0] and [1] fresh, [2] the indices of [0] again (staged without weights)"""
    idx, lens = [], []
    for _ in range(2):
        if L == "ragged":
            ln = [rng.randint(0, 41, size=B).astype(np.int32) for _ in range(T)]
            for t in range(T):
                ln[t][[0, 7, B - 1]] = 0                                       # three empty bags per table
        else:
            ln = [np.full(B, L, np.int32) for _ in range(T)]
        ix = [rng.randint(0, ROWS[t], size=int(ln[t].sum())).astype(np.int64) for t in range(T)]
        for t in range(T):
            if ix[t].size:
                ix[t][0], ix[t][-1] = 0, ROWS[t] - 1
        idx.append(ix)
        lens.append(ln)
    idx.append(idx[0])
    lens.append(lens[0])
    return idx, lens


JOBS12 = [((0, 1, 2)[k % 3], (B, 1, 29, 0)[k % 4]) for k in range(12)]
JOBS16 = [((1, 2, 0)[k % 3], (5, B, 33, 1)[k % 4]) for k in range(16)]


def _run_set(eng, jobs):
    eng.forward_multi_async(1, [b for b, _ in jobs], [n for _, n in jobs])
    eng.wait(1, sum(n for _, n in jobs))
    vrows = sum((n + 63) // 64 * 64 for _, n in jobs)
    R = eng.fetch_interaction(vrows, slot=1)
    out, v = [], 0
    for b, n in jobs:                                                          # (pad rows between queries: not compared)
        out.append(R[v:v + n].copy())
        v += (n + 63) // 64 * 64
    return out


# ------------------------------------------------------------------------------------------------------------------------
# 1. every stored type, width and bag shape: sequential bits, split tolerance, weights of ones, mixed sets
@pytest.mark.parametrize("kind", sorted(TYPES))
@pytest.mark.parametrize("D", [8, 10, 16, 32, 64, 128, 256])
@pytest.mark.parametrize("L", [1, 2, 20, 130, "ragged"])
def test_weighted_gather_against_the_sequential_fma_chain(kind, D, L):
    """L 130 crosses the 128-index LDS chunk, D 10 takes sls_any_kernel, D 256 takes G 64.  Three engines on the same
    tables: `we` (batch 0 weighted, batch 1 weighted with table 1 left NULL, batch 2 unweighted), `on` (batch 0 weights of
    1.0, batch 1 NULL for every table, batch 2 unweighted) and `un` (nothing weighted)."""
    rng = np.random.RandomState(D * 11 + (7 if L == "ragged" else L))
    Lmax = 40 if L == "ragged" else L
    tables = [rng.uniform(-1, 1, (r, D)).astype(np.float32) for r in ROWS]
    stored = [_stored(kind, W) for W in tables]
    idx, lens = _inputs(rng, L)
    dense = [rng.rand(B, 8).astype(np.float32) for _ in range(2)]
    dense.append(dense[0])
    wts = [[rng.uniform(0, 1, size=idx[b][t].size).astype(np.float32) for t in range(T)] for b in range(2)]
    wts[1][1] = None
    ones = [np.ones(i.size, np.float32) for i in idx[0]]

    def eff(b, t):                                                             # the weights batch b's table t is pooled with
        return np.ones(idx[b][t].size, np.float32) if b == 2 or wts[b][t] is None else wts[b][t]

    ref = [np.concatenate([_ref(stored[t], idx[b][t], lens[b][t], eff(b, t)) for t in range(T)], axis=1) for b in range(3)]
    empty = [np.concatenate([np.repeat((lens[b][t] == 0)[:, None], D, axis=1) for t in range(T)], axis=1) for b in range(3)]
    we, on, un = (_engine(ROWS, D, Lmax, B, kind) for _ in range(3))
    try:
        for eng in (we, on, un):
            _load(eng, 11, tables, D, T)
        for b in range(3):
            we.stage_batch(b, dense[b], idx[b], lens[b], weights=wts[b] if b < 2 else None)
            on.stage_batch(b, dense[b], idx[b], lens[b], weights=(ones, [None] * T, None)[b])
            un.stage_batch(b, dense[b], idx[b], lens[b])
        assert (we.get_option("sls_weighted"), on.get_option("sls_weighted"), un.get_option("sls_weighted")) == (2, 2, 0)
        for eng in (we, on, un):
            eng.set_option("sls_exact", 1)
        alone = {}
        for b in range(3):
            for bs in (B, 1, 29):
                where = (kind, D, L, b, bs)
                we.forward(b, bs)
                Rw = we.fetch_interaction(bs)
                on.forward(b, bs)
                Ro = on.fetch_interaction(bs)
                un.forward(b, bs)
                Ru = un.fetch_interaction(bs)
                alone[(b, bs)] = Ru.copy()
                assert same_bits(Rw[:, D:], ref[b][:bs]), where                 # the fma chain, bit for bit
                assert not np.any(Rw[:, D:].view(np.uint32)[empty[b][:bs]]), where   # empty bags: +0.0
                assert same_bits(Rw[:, :D], Ru[:, :D]), where                   # the bottom MLP's columns
                assert same_bits(Ro, Ru), where                                 # weights of 1.0 / NULL: the unweighted bits
        for jobs in (JOBS12, JOBS16):
            got_w, got_o, got_u = _run_set(we, jobs), _run_set(on, jobs), _run_set(un, jobs)
            assert "w>" in " ".join(we.last_dispatch(1)) and "w>" not in " ".join(un.last_dispatch(1))
            for (b, n), Rw, Ro, Ru in zip(jobs, got_w, got_o, got_u):
                if not n:
                    continue
                where = (kind, D, L, len(jobs), b, n)
                assert same_bits(Rw[:, D:], ref[b][:n]), where
                assert same_bits(Rw[:, :D], Ru[:, :D]) and same_bits(Ro, Ru), where
                if b == 2 and (b, n) in alone:                                 # the unweighted query of a mixed set: its bits served alone
                    assert same_bits(Rw, alone[(b, n)]), where
        # split order: the tolerance tests/test_gpu_parity.py holds the unweighted split order to (n eps sum |w x| has the
        # unweighted bound's form; weights in [0, 1))
        we.set_option("sls_exact", 0)
        worst = 0.0
        for b in range(3):
            for bs in (B, 1, 29):
                we.forward(b, bs)
                Rw = we.fetch_interaction(bs)[:, D:]
                worst = max(worst, float(np.abs(Rw.astype(np.float64) - ref[b][:bs]).max()))
                assert H.close(Rw, ref[b][:bs], rtol=1e-5, atol_scale=2e-6), (kind, D, L, b, bs, worst)
        for jobs in (JOBS12, JOBS16):
            for (b, n), Rw in zip(jobs, _run_set(we, jobs)):
                if n:
                    assert H.close(Rw[:, D:], ref[b][:n], rtol=1e-5, atol_scale=2e-6), (kind, D, L, len(jobs), b, n)
        print("split order, worst |got - ref| = %.3g (%s, D %d, L %s)" % (worst, kind, D, L))
    finally:
        for eng in (we, on, un):
            eng.close()


# ------------------------------------------------------------------------------------------------------------------------
# 2. the dispatch log
def _fixed(D, L, rows=5000, n_tables=4, B_=64, seed=4):
    rng = np.random.RandomState(seed)
    tables = [rng.uniform(-1, 1, (rows, D)).astype(np.float32) for _ in range(n_tables)]
    ix = [rng.randint(0, rows, size=B_ * L).astype(np.int64) for _ in range(n_tables)]
    ln = [np.full(B_, L, np.int32) for _ in range(n_tables)]
    wt = [rng.uniform(0, 1, size=B_ * L).astype(np.float32) for _ in range(n_tables)]
    eng = _engine([rows] * n_tables, D, L, B_, "fp32", slots=1, staged=2)
    _load(eng, 1, tables, D, n_tables)
    return eng, tables, rng.rand(B_, 8).astype(np.float32), ix, ln, wt


def _log(eng):
    return " ".join(eng.last_dispatch())


@pytest.mark.parametrize("L,flat,ring", [(20, "sls_flatc_kernel<16,5,nt>", "sls_kernel<16,sequential,w>"),
                                         (40, "sls_flatc_kernel<16,10,nt>", "sls_kernel<16,split,nt,w>")])
def test_dispatch_log_carries_w_on_weighted_launches_only(L, flat, ring):
    """A fixed-L set at D 64: the flat-coalesced form without weights, the ring walk with them -- split (non-temporal)
    beyond the short-bag bound 2048 / D = 32, sequential up to it (plan_sls's unchanged rule: L 20 is a short bag at D 64,
    so the split line of a weighted launch shows at L 40) -- and the first line again once the batch is staged anew."""
    D, Bq = 64, 64
    eng, tables, X, ix, ln, wt = _fixed(D, L)
    try:
        eng.stage_batch(0, X, ix, ln)
        eng.forward(0, Bq)
        first = _log(eng)
        assert flat in first and ",w>" not in first and "<w>" not in first, first
        eng.stage_batch_weights(0, wt)
        eng.forward(0, Bq)
        assert ring in _log(eng) and "flat" not in _log(eng), _log(eng)
        eng.set_option("sls_exact", 1)
        eng.forward(0, Bq)
        assert "sls_kernel<16,sequential,w>" in _log(eng), _log(eng)
        eng.set_option("table_dtype", N.TABLE_FP16)
        eng.forward(0, Bq)
        assert "sls_kernel<16,sequential,f16,w>" in _log(eng), _log(eng)
        eng.set_option("table_dtype", N.TABLE_FP32)
        eng.set_option("sls_exact", 0)
        eng.stage_batch(0, X, ix, ln)                                          # staged again: unweighted again
        eng.forward(0, Bq)
        assert _log(eng) == first
    finally:
        eng.close()


def test_one_lookup_bags_and_odd_widths_take_the_weighted_ring_and_any_forms():
    eng, tables, X, ix, ln, wt = _fixed(64, 1)
    try:
        eng.stage_batch(0, X, ix, ln)
        eng.forward(0, 64)
        assert "sls_one_kernel<16," in _log(eng), _log(eng)
        eng.stage_batch_weights(0, wt)
        eng.forward(0, 64)
        assert "sls_kernel<16,sequential,w>" in _log(eng) and "sls_one_kernel" not in _log(eng), _log(eng)
    finally:
        eng.close()
    eng, tables, X, ix, ln, wt = _fixed(10, 5)
    try:
        eng.stage_batch(0, X, ix, ln)
        eng.forward(0, 64)
        assert "sls_any_kernel[" in _log(eng), _log(eng)
        eng.stage_batch_weights(0, wt)
        eng.forward(0, 64)
        assert "sls_any_kernel<w>[" in _log(eng), _log(eng)
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------------------------------
# 3. errors and counters
def test_errors_and_counters():
    D, L, Bq, n_tables = 32, 20, 64, 4
    eng, tables, X, ix, ln, wt = _fixed(D, L)
    try:
        eng.stage_batch(0, X, ix, ln)
        eng.stage_batch(1, X, ix, ln)
        assert eng.get_option("sls_weighted") == 0
        plain = eng.gather_bytes(0, Bq)
        half = eng.gather_bytes(0, Bq // 2)
        eng.set_option("sls_exact", 1)
        eng.forward(0, Bq)
        R0 = eng.fetch_interaction(Bq).copy()
        # a count that is not the staged one: refused, nothing changes
        short = list(wt)
        short[2] = wt[2][:-1]
        with pytest.raises(N.DrsError) as e:
            eng.stage_batch_weights(0, short)
        assert e.value.code == N.ERR_LENGTHS_SUM
        assert eng.get_option("sls_weighted") == 0 and eng.gather_bytes(0, Bq) == plain
        eng.forward(0, Bq)
        assert same_bits(eng.fetch_interaction(Bq), R0)
        with pytest.raises(N.DrsError) as e:
            eng.stage_batch_weights(7, wt)
        assert e.value.code == N.ERR_BAD_ARG
        # weights: 4 more bytes per looked-up row, and the read-only option counts the batches
        eng.stage_batch_weights(0, wt)
        assert eng.get_option("sls_weighted") == 1
        assert eng.gather_bytes(0, Bq) == plain + 4 * n_tables * Bq * L
        assert eng.gather_bytes(0, Bq // 2) == half + 4 * n_tables * (Bq // 2) * L
        assert eng.gather_bytes(1, Bq) == plain
        eng.stage_batch_weights(1, [None] * n_tables)
        assert eng.get_option("sls_weighted") == 2 and eng.gather_bytes(1, Bq) == plain + 4 * n_tables * Bq * L
        with pytest.raises(N.DrsError) as e:
            eng.set_option("sls_weighted", 1)                                  # read only
        assert e.value.code == N.ERR_BAD_ARG
        # the profiling byte count follows
        eng.set_profiling(1)
        eng.reset_kernel_time()
        eng.forward(0, Bq)
        assert eng.kernel_bytes(N.KERNEL_SLS_CLOCK) == plain + 4 * n_tables * Bq * L
        eng.set_profiling(0)
        # mean pooling and weights refuse each other, in either order
        with pytest.raises(N.DrsError) as e:
            eng.set_option("sls_pool", 1)
        assert e.value.code == N.ERR_UNSUPPORTED and eng.get_option("sls_pool") == 0
        eng.stage_batch(0, X, ix, ln)
        eng.stage_batch(1, X, ix, ln)
        assert eng.get_option("sls_weighted") == 0 and eng.gather_bytes(0, Bq) == plain
        eng.set_option("sls_pool", 1)
        with pytest.raises(N.DrsError) as e:
            eng.stage_batch_weights(0, wt)
        assert e.value.code == N.ERR_UNSUPPORTED and eng.get_option("sls_weighted") == 0
        eng.set_option("sls_pool", 0)
        eng.forward(0, Bq)
        assert same_bits(eng.fetch_interaction(Bq), R0)
    finally:
        eng.close()


@pytest.mark.parametrize("case", ["din_mini", "dien_mini"])
def test_din_and_dien_refuse_weights_and_keep_serving_the_same_bits(case):
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
            eng.stage_batch_weights(0, [np.ones(len(i), np.float32) for i in lS_i[0]])
        assert e.value.code == N.ERR_UNSUPPORTED and eng.get_option("sls_weighted") == 0
        with pytest.raises(N.DrsError) as e:
            eng.stage_batch_weights(0, [None] * len(lS_i[0]))
        assert e.value.code == N.ERR_UNSUPPORTED
        assert same_bits(net.run_staged(0, n), before) and same_bits(eng.fetch_interaction(n), R0)
    finally:
        net.engine.close()


# ------------------------------------------------------------------------------------------------------------------------
# 4. an out-of-range index: Caffe2's ENFORCE, not a fault
def test_out_of_range_index_in_a_weighted_bag_is_refused_and_contributes_nothing():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    D, L, Bq = 32, 20, 64
    eng, tables, X, ix, ln, wt = _fixed(D, L)
    try:
        # the staged path: the host's range check refuses the batch; the weighted batch staged before keeps its bits
        eng.set_option("sls_exact", 1)
        eng.stage_batch(0, X, ix, ln, weights=wt)
        eng.forward(0, Bq)
        R0 = eng.fetch_interaction(Bq).copy()
        bad = [i.copy() for i in ix]
        bad[1][5] = 5000
        with pytest.raises(N.DrsError) as e:
            eng.stage_batch(0, X, bad, ln, weights=wt)
        assert e.value.code == N.ERR_INDEX_RANGE and eng.get_option("sls_weighted") == 1
        eng.forward(0, Bq)
        assert same_bits(eng.fetch_interaction(Bq), R0)
        # the operator (device pointers, no host check): the kernel's own range check flags the index, reads row 0 in its
        # place and gives the row the weight 0
        for Dw in (32, 10):
            rng = np.random.RandomState(Dw)
            rows, bags = 777, 33
            W = rng.uniform(-1, 1, (rows, Dw)).astype(np.float32)
            lengths = rng.randint(1, 9, size=bags).astype(np.int32)
            idx = rng.randint(0, rows, size=int(lengths.sum())).astype(np.int32)
            w = rng.uniform(-2, 2, size=idx.size).astype(np.float32)
            hit = int(lengths[:4].sum()) + 1
            idx[hit] = rows                                                    # one past the table
            idx[hit + 3] = -1
            w0 = w.copy()
            w0[[hit, hit + 3]] = 0
            want = weighted_ref(W, np.where((idx < 0) | (idx >= rows), 0, idx), lengths, w0)
            dW, di, dl, dw = (torch.from_numpy(a).cuda() for a in (W, idx, lengths, w))
            out = torch.full((bags, Dw), float("nan"), device="cuda")
            torch.cuda.synchronize()
            with pytest.raises(N.DrsError) as e:
                eng.sls(dW.data_ptr(), rows, Dw, di.data_ptr(), dl.data_ptr(), bags, idx.size, out.data_ptr(), exact_order=True,
                        wgt_ptr=dw.data_ptr())
            assert e.value.code == N.ERR_INDEX_RANGE
            assert same_bits(out.cpu().numpy(), want), Dw
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------------------------------
# 5. the stand-alone operator
@pytest.mark.parametrize("D", [10, 64])
def test_drs_sls_weighted_is_the_fma_chain(D):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    rng = np.random.RandomState(D)
    rows, bags, L = 5003, 257, 40
    W = rng.uniform(-1, 1, (rows, D)).astype(np.float32)
    lengths = rng.randint(0, L + 1, size=bags).astype(np.int32)
    lengths[5] = 0
    idx = rng.randint(0, rows, size=int(lengths.sum())).astype(np.int32)
    w = rng.uniform(-2, 2, size=idx.size).astype(np.float32)
    want = weighted_ref(W, idx, lengths, w)
    eng = N.Engine(N.MODEL_DLRM, [16, 16], 8, [4, 8], [24, 4, 1], N.INTERACT_CAT, sigmoid_top=2,
                   max_batch=4, max_lookups=2, num_staged_batches=1, num_slots=1)
    try:
        dW, di, dl, dw = (torch.from_numpy(a).cuda() for a in (W, idx, lengths, w))
        out = torch.full((bags, D), float("nan"), device="cuda")
        torch.cuda.synchronize()   # inputs/outputs were produced on torch's stream, the op runs on the engine's
        eng.sls(dW.data_ptr(), rows, D, di.data_ptr(), dl.data_ptr(), bags, idx.size, out.data_ptr(), exact_order=True,
                wgt_ptr=dw.data_ptr())
        assert same_bits(out.cpu().numpy(), want), D
        out.fill_(float("nan"))
        torch.cuda.synchronize()
        eng.sls(dW.data_ptr(), rows, D, di.data_ptr(), dl.data_ptr(), bags, idx.size, out.data_ptr(), exact_order=False,
                wgt_ptr=dw.data_ptr())
        assert H.close(out.cpu().numpy(), want, rtol=1e-5, atol_scale=2e-6), D
        out.fill_(float("nan"))
        torch.cuda.synchronize()
        eng.sls(dW.data_ptr(), rows, D, di.data_ptr(), dl.data_ptr(), bags, idx.size, out.data_ptr(), exact_order=True)
        assert same_bits(out.cpu().numpy(), orc.sls(W, idx, lengths)), D        # (the unweighted operator is what it was)
        eng.set_option("sls_pool", 1)
        with pytest.raises(N.DrsError) as e:
            eng.sls(dW.data_ptr(), rows, D, di.data_ptr(), dl.data_ptr(), bags, idx.size, out.data_ptr(), exact_order=True,
                    wgt_ptr=dw.data_ptr())
        assert e.value.code == N.ERR_UNSUPPORTED
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------------------------------
# 6. a whole model
def test_rm1_mini_with_uniform_weights():
    """--accel_sls_weights uniform: the pooled columns of R equal weighted_ref, and the outputs equal the oracle's FC
    layers (orc.fc takes R directly) run over that R -- the chain is first held to the oracle's own forward without weights."""
    meta, z = H.load_fixture("dlrm_rm1_mini")
    args = H.args_from(meta["args"], accel_sls_weights="uniform")
    net, lX, lS_l, lS_i, lT = H.materialize(args)
    lS_w = dlrm_s_hip.sls_weights(args, lS_i)
    net.create(lX[0], lS_l[0], lS_i[0], lT[0])
    try:
        eng = net.engine
        om = H.oracle_model(net)
        D = net.m_spa
        n_top = len(net.top_w)

        def top(R):
            x = R
            for i, (Wt, bt) in enumerate(net.top_w):
                x = orc.fc(x, Wt, bt, orc.ACT_SIGMOID if i + 1 == om.sigmoid_top else orc.ACT_RELU)   # (sigmoid_top counts layers from 1)
            return x

        assert 1 <= om.sigmoid_top <= n_top
        eng.set_option("sls_exact", 1)
        n = len(lS_l[0][0])
        net.stage_batches(lX, lS_l, lS_i)
        exp, R_exp = om.forward(lX[0], lS_i[0], lS_l[0], bs=n, want_R=True)
        assert same_bits(top(R_exp), exp)                                      # the chain of orc.fc calls is the oracle's top MLP
        plain = net.run_staged(0, n).copy()
        assert same_bits(eng.fetch_interaction(n), R_exp)
        net.stage_batches(lX, lS_l, lS_i, lS_w)
        assert eng.get_option("sls_weighted") == len(lS_l)
        for bid in range(len(lS_l)):
            for bs in sorted({n, 1, max(1, n // 2)}):
                got = net.run_staged(bid, bs)
                R = eng.fetch_interaction(bs)
                _, R_un = om.forward(lX[bid], lS_i[bid], lS_l[bid], bs=bs, want_R=True)
                want = np.concatenate([weighted_ref(net.emb_w[t], lS_i[bid][t], lS_l[bid][t][:bs], lS_w[bid][t])
                                       for t in range(len(net.emb_w))], axis=1)
                assert same_bits(R[:, :D], R_un[:, :D]) and same_bits(R[:, D:], want), (bid, bs)
                assert not same_bits(R, R_un)
                assert H.close(got, top(R), rtol=1e-6, atol=1e-7), (bid, bs, np.abs(got - top(R)).max())
        assert not same_bits(net.run_staged(0, n), plain)
    finally:
        net.engine.close()


# ------------------------------------------------------------------------------------------------------------------------
# 7. the stand-alone entry
def test_stand_alone_entry_with_uniform_weights(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = dict(arch_mlp_bot="16-8", arch_mlp_top="64-16-1", arch_embedding_size="-".join(["3000"] * 6),
               arch_sparse_feature_size=8, num_indices_per_lookup_fixed=True, num_indices_per_lookup=20,
               arch_interaction_op="dot", model_type="dlrm", model_name="mini")
    path = str(tmp_path / "mini.json")
    json.dump(cfg, open(path, "w"))
    r = subprocess.run([sys.executable, "-m", "deeprecsys_amd.dlrm_s_hip", "--inference_only", "--use_accel",
                        "--config_file", path, "--nepochs", "3", "--num_batches", "2", "--mini_batch_size", "64",
                        "--max_mini_batch_size", "64", "--accel_sls_weights", "uniform"],
                       cwd=root, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.count("***") == 6, r.stdout[-2000:]
