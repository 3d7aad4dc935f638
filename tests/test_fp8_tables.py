"""fp8 e4m3 embedding tables on the GPU (-m gpu): engine option "table_dtype" 4.

The checker is `fp8_decoded` (tests/test_fp8_tables_cpu.py): torch's float8_e4m3fn codes of W * 2**k under the per-table
scale rule, widened back and multiplied by 2**-k.  The kernels sum the decoded codes and multiply a bag's finished sum
by 2**-k; a power of two commutes with every fp32 add, fma and division here, so every fp8 gather form serves the bits
of its fp32 twin on the decoded tables: each case compares an fp8 engine with an fp32 engine loaded with them, bit for
bit, and the sequential order with the oracle.
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
from tests.test_fp8_tables_cpu import fp8_decoded, fp8_exponent
from tests.test_half_tables import SETTINGS, _engine, _load, upcast

pytestmark = pytest.mark.gpu

FP8 = N.TABLE_FP8_E4M3
FACTORS = (1.0, 1e-3, 37.0)            # per-table magnitudes: three different scale exponents


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _tables(rng, rows, D):
    return [(rng.uniform(-1, 1, (r, D)) * FACTORS[t % 3]).astype(np.float32) for t, r in enumerate(rows)]


def _pooled(eng, B, D, b=0):
    eng.forward(b, B)
    return eng.fetch_interaction(B)[:, D:].copy()


# ---- 1. every form against the fp32 twin --------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [4, 8, 10, 12, 16, 32, 64, 128, 256])
@pytest.mark.parametrize("L", [1, 20, 80, "ragged"])
def test_fp8_gather_serves_the_bits_of_the_fp32_twin_on_decoded_tables(D, L):
    rng = np.random.RandomState(D * 7 + (0 if L == "ragged" else L))
    T, B = 3, 48
    Lmax = 30 if L == "ragged" else L
    rows = [1501 + 13 * t for t in range(T)]
    tables = _tables(rng, rows, D)
    dec, ks = zip(*[fp8_decoded(W) for W in tables])
    assert len(set(ks)) == 3
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
    f8 = _engine(rows, D, Lmax, B, FP8, slots=2)
    ref = _engine(rows, D, Lmax, B, N.TABLE_FP32, slots=2)
    try:
        assert f8.get_option("table_dtype") == 4 and ref.get_option("table_dtype") == 0
        _load(f8, 11, tables, D, T)
        _load(ref, 11, dec, D, T)
        assert [f8.table_fp8_exponent(t) for t in range(T)] == list(ks)
        with pytest.raises(N.DrsError) as e:
            ref.table_fp8_exponent(0)
        assert e.value.code == N.ERR_UNSUPPORTED
        for eng in (f8, ref):
            for b in range(2):
                eng.stage_batch(b, dense[b], idx[b], lens[b])

        def pooled(b, bs):
            out = []
            for t in range(T):
                n = int(lens[b][t][:bs].sum())
                out.append(orc.sls(dec[t], idx[b][t][:n], lens[b][t][:bs]))
            return np.concatenate(out, axis=1)
        jobs12 = [((k % 2), (B, 1, 17, 0)[k % 4]) for k in range(12)]
        jobs16 = [((k + 1) % 2, (5, B, 33, 1)[k % 4]) for k in range(16)]
        for exact, flat, one in SETTINGS:
            for eng in (f8, ref):
                eng.set_option("sls_exact", exact)
                eng.set_option("sls_flat", flat)
                eng.set_option("sls_one", one)
            for b in range(2):
                for bs in (B, 1, 29):
                    got = f8.forward(b, bs)
                    R = f8.fetch_interaction(bs)
                    assert np.array_equal(_bits(got), _bits(ref.forward(b, bs))), (exact, flat, one, b, bs)
                    assert np.array_equal(_bits(R), _bits(ref.fetch_interaction(bs))), (exact, flat, one, b, bs)
                    if exact:
                        assert np.array_equal(_bits(R[:, D:]), _bits(pooled(b, bs))), (exact, flat, one, b, bs)
                    else:
                        assert H.close(R[:, D:], pooled(b, bs), rtol=1e-5, atol_scale=2e-6), (flat, one, b, bs)
            for jobs in (jobs12, jobs16):
                outs = []
                for eng in (f8, ref):
                    eng.forward_multi_async(1, [b for b, _ in jobs], [n for _, n in jobs])
                    outs.append(eng.wait(1, sum(n for _, n in jobs)))
                vrows = sum((n + 63) // 64 * 64 for _, n in jobs)
                R8, Rr = f8.fetch_interaction(vrows, slot=1), ref.fetch_interaction(vrows, slot=1)
                assert np.array_equal(_bits(outs[0]), _bits(outs[1])), (exact, flat, one, len(jobs))
                v = 0
                for b, n in jobs:                      # (the rows between two queries of a set belong to nobody)
                    assert np.array_equal(_bits(R8[v:v + n]), _bits(Rr[v:v + n])), (exact, flat, one, len(jobs), b, n)
                    if exact:
                        assert np.array_equal(_bits(R8[v:v + n, D:]), _bits(pooled(b, n))), (one, len(jobs), b, n)
                    else:
                        assert H.close(R8[v:v + n, D:], pooled(b, n), rtol=1e-5, atol_scale=2e-6), (flat, len(jobs), b, n)
                    v += (n + 63) // 64 * 64
    finally:
        f8.close()
        ref.close()


# ---- 2. the quantizer's edge cases --------------------------------------------------------------------------------------
def test_quantizer_edge_cases_through_one_lookup_bags():
    """Ties to even, the subnormal codes and what rounds to zero below them, -0.0, +-inf, NaN, and every |code| from 0 to
    0x7E as its exact value: a one-lookup bag copies each stored row out as 0.0f + row (the kernels' one-row sum, the
    oracle's too), which equals 0.0f + the decoded table bit for bit where that is not a NaN; a NaN stays a NaN.  The
    largest element is 448.0, so k = 0; the second table holds the same values times 2**-20, so k = 20."""
    import torch
    D, B = 16, 64
    below = np.nextafter(np.float32(2.0 ** -10), np.float32(0))
    special = [17.0, 19.0, -17.0, 2.0 ** -9, 2.0 ** -10, 1.5 * 2.0 ** -10, below, -below, -0.0, 0.0, np.inf, -np.inf, np.nan,
               3 * 2.0 ** -10, 2.5 * 2.0 ** -9, 3.5 * 2.0 ** -9, 0.1, -1.0 / 3.0, 447.0, 431.9]
    codes = torch.arange(0x7F, dtype=torch.int32).to(torch.uint8).view(torch.float8_e4m3fn).to(torch.float32).numpy()
    assert codes[0x7E] == 448.0 and codes.size == 127
    vals = np.concatenate([np.array(special, np.float32), codes, -codes[1:40]])
    rows = (vals.size + D - 1) // D
    W0 = np.zeros((rows, D), np.float32)
    W0.reshape(-1)[:vals.size] = vals
    W1 = W0 * np.float32(2.0 ** -20)
    dec0, k0 = fp8_decoded(W0)
    dec1, k1 = fp8_decoded(W1)
    assert (k0, k1) == (0, 20)
    # what the rounding must have produced (the checker itself)
    d = dec0.reshape(-1)
    assert (d[0], d[1], d[2], d[3], d[4], d[5], d[6]) == (16.0, 20.0, -16.0, 2.0 ** -9, 0.0, 2.0 ** -9, 0.0)
    assert np.isnan(d[10:13]).all() and d[13] == 2.0 ** -8 and d[14] == 2.0 ** -8 and d[15] == 2.0 ** -7
    assert np.array_equal(d[len(special):len(special) + 127], codes)
    assert np.array_equal(_bits(dec1[~np.isnan(dec1)]), _bits(dec0[~np.isnan(dec0)] * np.float32(2.0 ** -20)))
    eng = N.Engine(N.MODEL_DLRM, [rows, rows], D, [8, D], [3 * D, 1], N.INTERACT_CAT, sigmoid_top=1,
                   max_batch=B, max_lookups=1, num_staged_batches=1, num_slots=1)
    try:
        eng.set_option("table_dtype", FP8)
        eng.set_table(0, W0)
        eng.set_table(1, W1)
        assert (eng.table_fp8_exponent(0), eng.table_fp8_exponent(1)) == (0, 20)
        eng.set_fc(N.MLP_BOT, 0, np.zeros((D, 8), np.float32), np.zeros(D, np.float32))
        eng.set_fc(N.MLP_TOP, 0, np.zeros((1, 3 * D), np.float32), np.zeros(1, np.float32))
        ix = (np.arange(B) % rows).astype(np.int64)
        ones = np.ones(B, np.int32)
        eng.stage_batch(0, np.zeros((B, 8), np.float32), [ix, ix], [ones, ones])
        exp = np.concatenate([orc.sls(dec0, ix, ones), orc.sls(dec1, ix, ones)], axis=1)
        assert np.array_equal(_bits(exp[:, :D][~np.isnan(exp[:, :D])]), _bits((np.float32(0) + dec0[ix])[~np.isnan(dec0[ix])]))
        nan = np.isnan(exp)
        for one in (1, 0):                     # the copy form and the lane-group-per-bag sequential form
            eng.set_option("sls_exact", 1)
            eng.set_option("sls_one", one)
            got = _pooled(eng, B, D)
            assert np.array_equal(np.isnan(got), nan), one
            assert np.array_equal(_bits(got[~nan]), _bits(exp[~nan])), one
        # the same table arriving through the arena conversion: the device quantizer again, and the device absmax
        conv = N.Engine(N.MODEL_DLRM, [rows, rows], D, [8, D], [3 * D, 1], N.INTERACT_CAT, sigmoid_top=1,
                        max_batch=B, max_lookups=1, num_staged_batches=1, num_slots=1)
        try:
            conv.set_table(0, W0)
            conv.set_table(1, W1)
            conv.set_option("table_dtype", FP8)
            assert (conv.table_fp8_exponent(0), conv.table_fp8_exponent(1)) == (0, 20)
            conv.set_fc(N.MLP_BOT, 0, np.zeros((D, 8), np.float32), np.zeros(D, np.float32))
            conv.set_fc(N.MLP_TOP, 0, np.zeros((1, 3 * D), np.float32), np.zeros(1, np.float32))
            conv.stage_batch(0, np.zeros((B, 8), np.float32), [ix, ix], [ones, ones])
            conv.set_option("sls_exact", 1)
            got = _pooled(conv, B, D)
            assert np.array_equal(np.isnan(got), nan) and np.array_equal(_bits(got[~nan]), _bits(exp[~nan]))
        finally:
            conv.close()
    finally:
        eng.close()


# ---- 3. weights and mean ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [32, 64])
def test_weighted_and_mean_bags_serve_the_bits_of_the_fp32_twin(D):
    rng = np.random.RandomState(40 + D)
    T, B, L = 3, 48, 20
    rows = [1501 + 13 * t for t in range(T)]
    tables = _tables(rng, rows, D)
    dec = [fp8_decoded(W)[0] for W in tables]
    ix = [rng.randint(0, rows[t], size=B * L).astype(np.int64) for t in range(T)]
    ln = [np.full(B, L, np.int32) for _ in range(T)]
    X = rng.rand(B, 8).astype(np.float32)
    wts = [rng.uniform(0.5, 2.0, size=B * L).astype(np.float32), None, rng.uniform(0.5, 2.0, size=B * L).astype(np.float32)]
    f8 = _engine(rows, D, L, B, FP8, slots=1, staged=1)
    ref = _engine(rows, D, L, B, N.TABLE_FP32, slots=1, staged=1)
    try:
        _load(f8, 11, tables, D, T)
        _load(ref, 11, dec, D, T)
        for eng in (f8, ref):
            eng.set_option("dispatch_log", 1)
            eng.stage_batch(0, X, ix, ln, weights=wts)
        for exact in (0, 1):
            for wflat in (0, 1):
                for eng in (f8, ref):
                    eng.set_option("sls_exact", exact)
                    eng.set_option("sls_weighted_flat", wflat)
                for bs in (B, 29):
                    a, b = f8.forward(0, bs), ref.forward(0, bs)
                    d8 = [t for t in f8.last_dispatch() if t.startswith("sls_")]
                    d32 = [t for t in ref.last_dispatch() if t.startswith("sls_")]
                    assert len(d8) == 1 and "f8,w>" in d8[0] and d8[0].replace("f8,w>", "w>") == d32[0], (d8, d32)
                    assert np.array_equal(_bits(a), _bits(b)), (exact, wflat, bs)
                    assert np.array_equal(_bits(f8.fetch_interaction(bs)), _bits(ref.fetch_interaction(bs))), (exact, wflat, bs)
        # weighted, sequential: torch's chain acc = fma(w, row, acc) on the decoded tables
        import torch
        for t in (0, 2):
            bag = torch.nn.functional.embedding_bag(torch.from_numpy(ix[t]), torch.from_numpy(dec[t]),
                                                    torch.arange(0, B * L, L), mode="sum",
                                                    per_sample_weights=torch.from_numpy(wts[t])).numpy()
            assert np.array_equal(_bits(f8.fetch_interaction(B)[:29, D + t * D:D + (t + 1) * D]), _bits(bag[:29])), t
        # mean pooling, on unweighted batches (staging again drops the weights)
        for eng in (f8, ref):
            eng.stage_batch(0, X, ix, ln)
            eng.set_option("sls_pool", 1)
        for exact, flat in ((0, 1), (0, 0), (0, 2), (1, 1)):
            for eng in (f8, ref):
                eng.set_option("sls_exact", exact)
                eng.set_option("sls_flat", flat)
            for bs in (B, 29):
                a, b = f8.forward(0, bs), ref.forward(0, bs)
                assert any("f8,mean>" in t for t in f8.last_dispatch()), f8.last_dispatch()
                assert np.array_equal(_bits(a), _bits(b)), (exact, flat, bs)
                R = f8.fetch_interaction(bs)
                assert np.array_equal(_bits(R), _bits(ref.fetch_interaction(bs))), (exact, flat, bs)
                if exact:
                    exp = np.concatenate([orc.sls(dec[t], ix[t][:bs * L], ln[t][:bs]) / np.float32(L) for t in range(T)], axis=1)
                    assert np.array_equal(_bits(R[:, D:]), _bits(exp))
    finally:
        f8.close()
        ref.close()


# ---- 4. conversions -----------------------------------------------------------------------------------------------------
def test_every_conversion_with_fp8_on_either_side():
    rng = np.random.RandomState(3)
    rows, D, T, L, B = [2000, 1700, 1300], 64, 3, 20, 64
    tables = _tables(rng, rows, D)
    dec, ks = zip(*[fp8_decoded(W) for W in tables])
    ix = [rng.randint(0, rows[t], size=B * L).astype(np.int64) for t in range(T)]
    ln = [np.full(B, L, np.int32) for _ in range(T)]
    X = rng.rand(B, 8).astype(np.float32)
    exp = np.concatenate([orc.sls(dec[t], ix[t], ln[t]) for t in range(T)], axis=1)

    def state(eng):
        eng.set_option("sls_exact", 1)
        return _pooled(eng, B, D)
    a = _engine(rows, D, L, B, N.TABLE_FP32, slots=1, staged=1)      # set_table, then table_dtype 4
    b = _engine(rows, D, L, B, FP8, slots=1, staged=1)               # table_dtype 4, then set_table
    h = _engine(rows, D, L, B, N.TABLE_FP16, slots=1, staged=1)      # fp16, then table_dtype 4
    q = _engine(rows, D, L, B, N.TABLE_FP32, slots=1, staged=1)      # the decoded tables, int8-quantized
    try:
        fp32_bytes = a.get_option("table_bytes")
        _load(a, 5, tables, D, T)
        a.set_option("table_dtype", FP8)
        _load(b, 5, tables, D, T)
        for e in (a, b):
            e.stage_batch(0, X, ix, ln)
            assert [e.table_fp8_exponent(t) for t in range(T)] == list(ks)
            assert sum(r * D for r in rows) <= e.get_option("table_bytes") <= sum((r * D + 255) // 256 * 256 for r in rows)
            assert e.gather_bytes(0, B) == B * T * (L * D + L * 4 + 4 + D * 4)
        assert np.array_equal(_bits(state(a)), _bits(exp)) and np.array_equal(_bits(state(b)), _bits(exp))
        # placement candidates are copies of the fp8 arena; the scales stay
        b.set_option("table_placement", -1)
        assert b.get_option("table_placements") == 2 and np.array_equal(_bits(state(b)), _bits(exp))
        # bad values are refused and change nothing
        for bad in (3, 10):
            with pytest.raises(N.DrsError) as e:
                b.set_option("table_dtype", bad)
            assert e.value.code == N.ERR_BAD_ARG and b.get_option("table_dtype") == 4
        # the line-packing options are only remembered
        b.set_option("table_int8_lines", 1)
        b.set_option("table_int4_lines", 1)
        assert b.get_option("table_dtype") == 4 and np.array_equal(_bits(state(b)), _bits(exp))
        b.set_option("table_int8_lines", 0)
        b.set_option("table_int4_lines", 0)
        # 4 -> 0: an fp32 arena of the decoded values
        a.set_option("table_dtype", N.TABLE_FP32)
        assert a.get_option("table_bytes") == fp32_bytes and np.array_equal(_bits(state(a)), _bits(exp))
        with pytest.raises(N.DrsError) as e:
            a.table_fp8_exponent(0)
        assert e.value.code == N.ERR_UNSUPPORTED
        # ... and 0 -> 4 again: the decoded values are fp8 values under the same scale
        a.set_option("table_dtype", FP8)
        assert [a.table_fp8_exponent(t) for t in range(T)] == list(ks) and np.array_equal(_bits(state(a)), _bits(exp))
        # 1 -> 4 quantizes the fp16-rounded tables
        _load(h, 5, tables, D, T)
        h.stage_batch(0, X, ix, ln)
        h.set_option("table_dtype", FP8)
        dech, kh = zip(*[fp8_decoded(upcast(W, "fp16")) for W in tables])
        assert [h.table_fp8_exponent(t) for t in range(T)] == list(kh)
        assert np.array_equal(_bits(state(h)), _bits(np.concatenate([orc.sls(dech[t], ix[t], ln[t]) for t in range(T)], axis=1)))
        # 4 -> 2: the decoded values, rounded to bf16
        h.set_option("table_dtype", N.TABLE_BF16)
        assert np.array_equal(_bits(state(h)),
                              _bits(np.concatenate([orc.sls(upcast(dech[t], "bf16"), ix[t], ln[t]) for t in range(T)], axis=1)))
        # 4 -> 8 and 4 -> 9: the decoded tables through that type's own quantizer
        _load(q, 5, dec, D, T)
        q.stage_batch(0, X, ix, ln)
        for dt in (N.TABLE_INT8_ROWWISE, N.TABLE_INT4_ROWWISE):
            q.set_option("table_dtype", N.TABLE_FP32)
            _load(q, 5, dec, D, T)
            q.set_option("table_dtype", dt)
            b.set_option("table_dtype", dt)
            assert b.get_option("table_dtype") == dt and b.get_option("table_placements") == 1
            for exact in (1, 0):
                for e in (b, q):
                    e.set_option("sls_exact", exact)
                assert np.array_equal(_bits(b.forward(0, B)), _bits(q.forward(0, B))), (dt, exact)
                assert np.array_equal(_bits(b.fetch_interaction(B)), _bits(q.fetch_interaction(B))), (dt, exact)
            # ... and back: a rowwise arena refuses 4 as it always has (ERR_BAD_ARG, nothing changes); by way of 0 it is
            # the quantization of each row's value
            before = _bits(state(b))
            with pytest.raises(N.DrsError) as e:
                b.set_option("table_dtype", FP8)
            assert e.value.code == N.ERR_BAD_ARG and b.get_option("table_dtype") == dt
            assert np.array_equal(_bits(state(b)), before), dt
            for eng in (b, q):
                eng.set_option("table_dtype", N.TABLE_FP32)
                eng.set_option("table_dtype", FP8)
            assert [b.table_fp8_exponent(t) for t in range(T)] == [q.table_fp8_exponent(t) for t in range(T)]
            assert np.array_equal(_bits(state(b)), _bits(state(q))), dt
            _load(b, 5, tables, D, T)
    finally:
        for e in (a, b, h, q):
            e.close()


def test_dispatch_log_carries_f8_and_the_form_fp16_takes():
    rows, D, T, L, B = [5000] * 4, 64, 4, 80, 64
    rng = np.random.RandomState(2)
    tables = [rng.uniform(-1, 1, (r, D)).astype(np.float32) for r in rows]
    ix = [rng.randint(0, rows[t], size=B * L).astype(np.int64) for t in range(T)]
    ln = [np.full(B, L, np.int32) for _ in range(T)]
    e = _engine(rows, D, L, B, N.TABLE_FP16, slots=1, staged=1)
    try:
        e.set_option("dispatch_log", 1)
        _load(e, 1, tables, D, T)
        e.stage_batch(0, rng.rand(B, 8).astype(np.float32), ix, ln)
        e.forward(0, B)
        assert "sls_flatc_kernel<16,20,nt,f16>" in " ".join(e.last_dispatch())
        e.set_option("table_dtype", FP8)
        e.forward(0, B)
        d = " ".join(e.last_dispatch())
        assert "sls_flatc_kernel<16,20,nt,f8>" in d, d
        e.set_option("sls_exact", 1)
        e.forward(0, B)
        assert "sls_kernel<16,sequential,f8>" in " ".join(e.last_dispatch())
        for key in ("mlp_streams", "mlp_rows32", "mlp_stream_2cu", "preferred_slots", "preferred_coalesce", "gather_bound"):
            e.get_option(key)
    finally:
        e.close()


# ---- 5. the device fill -------------------------------------------------------------------------------------------------
def test_fill_then_convert_equals_convert_then_fill():
    rows, D, T, L, B = [2000, 1700], 32, 2, 20, 64
    rng = np.random.RandomState(9)
    ix = [rng.randint(0, rows[t], size=B * L).astype(np.int64) for t in range(T)]
    ln = [np.full(B, L, np.int32) for _ in range(T)]
    X = rng.rand(B, 8).astype(np.float32)
    a = _engine(rows, D, L, B, N.TABLE_FP32, slots=1, staged=1)
    b = _engine(rows, D, L, B, FP8, slots=1, staged=1)
    try:
        assert fp8_exponent(0.05) == 13            # 0.05 * 2**13 = 409.6: away from a boundary, so the samples' absmax agrees
        fills = []
        for t in range(T):
            a.fill_table_uniform(t, -0.05, 0.05, 77)
            b.fill_table_uniform(t, -0.05, 0.05, 77)
            fills.append(fp8_decoded(orc.fill_table_uniform(rows[t], D, t, -0.05, 0.05, 77, nthreads=0)))
        a.set_option("table_dtype", FP8)
        rs = np.random.RandomState(5)
        for e in (a, b):
            e.set_fc(N.MLP_BOT, 0, rs.randn(D, 8).astype(np.float32), np.zeros(D, np.float32))
            e.set_fc(N.MLP_TOP, 0, np.zeros((4, D * (T + 1)), np.float32), np.zeros(4, np.float32))
            e.set_fc(N.MLP_TOP, 1, np.zeros((1, 4), np.float32), np.zeros(1, np.float32))
            e.stage_batch(0, X, ix, ln)
            e.set_option("sls_exact", 1)
            assert [e.table_fp8_exponent(t) for t in range(T)] == [13] * T == [k for _, k in fills]
        exp = np.concatenate([orc.sls(fills[t][0], ix[t], ln[t]) for t in range(T)], axis=1)
        Ra, Rb = _pooled(a, B, D), _pooled(b, B, D)
        assert np.array_equal(_bits(Ra), _bits(Rb)) and np.array_equal(_bits(Ra), _bits(exp))
    finally:
        a.close()
        b.close()


# ---- 6. whole models ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["dlrm_rm1_mini", "dlrm_dot_small", "wnd_mini", "ncf_mini", "mtwnd_mini"])
def test_models_with_fp8_tables_match_oracle_on_decoded_tables(case):
    meta, z = H.load_fixture(case)
    args = H.args_from(meta["args"], accel_table_dtype="fp8_e4m3")
    net, lX, lS_l, lS_i, lT = H.materialize(args)
    net.create(lX[0], lS_l[0], lS_i[0], lT[0])
    try:
        assert net.engine.get_option("table_dtype") == 4
        emb = net.emb_w
        decoded = [fp8_decoded(W) for W in emb]
        assert [net.engine.table_fp8_exponent(t) for t in range(len(emb))] == [k for _, k in decoded]
        net.emb_w = [d for d, _ in decoded]
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
                assert np.array_equal(_bits(R), _bits(R_exp)), (case, bid, bs)
                assert H.close(got, exp, rtol=1e-6, atol=1e-7), (case, np.abs(got - exp).max())
    finally:
        net.engine.close()


@pytest.mark.parametrize("case", ["din_mini", "dien_mini"])
def test_din_and_dien_refuse_fp8_tables_and_keep_serving_fp32(case):
    meta, z = H.load_fixture(case)
    args = H.args_from(meta["args"])
    net, lX, lS_l, lS_i, lT = H.materialize(args)
    net.create(lX[0], lS_l[0], lS_i[0], lT[0])
    try:
        eng = net.engine
        net.stage_batches(None, lS_l, lS_i)
        n = len(lS_l[0][0])
        eng.set_option("sls_exact", 1)
        before = net.run_staged(0, n).copy()
        R0 = eng.fetch_interaction(n).copy()
        with pytest.raises(N.DrsError) as e:
            eng.set_option("table_dtype", FP8)
        assert e.value.code == N.ERR_UNSUPPORTED and eng.get_option("table_dtype") == N.TABLE_FP32
        with pytest.raises(N.DrsError) as e:
            eng.table_fp8_exponent(0)
        assert e.value.code == N.ERR_UNSUPPORTED
        assert np.array_equal(_bits(net.run_staged(0, n)), _bits(before)) and np.array_equal(_bits(eng.fetch_interaction(n)), _bits(R0))
    finally:
        net.engine.close()


# ---- 7. the stand-alone entry -------------------------------------------------------------------------------------------
def test_stand_alone_entry_with_fp8_tables(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = dict(arch_mlp_bot="16-8", arch_mlp_top="64-16-1", arch_embedding_size="-".join(["3000"] * 6),
               arch_sparse_feature_size=8, num_indices_per_lookup_fixed=True, num_indices_per_lookup=20,
               arch_interaction_op="dot", model_type="dlrm", model_name="mini")
    path = str(tmp_path / "mini.json")
    json.dump(cfg, open(path, "w"))
    r = subprocess.run([sys.executable, "-m", "deeprecsys_amd.dlrm_s_hip", "--inference_only", "--use_accel",
                        "--config_file", path, "--nepochs", "3", "--num_batches", "2", "--mini_batch_size", "64",
                        "--max_mini_batch_size", "64", "--accel_table_dtype", "fp8_e4m3"],
                       cwd=root, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.count("***") == 6, r.stdout[-2000:]
