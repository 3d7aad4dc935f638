"""4-bit rowwise embedding tables on the GPU (-m gpu): engine option "table_dtype" 9.

The checker is torch's CPU implementation of the format: embedding_bag_4bit_prepack quantizes the fp32 rows, and
embedding_bag_4bit_rowwise_offsets pools them (acc = fmaf(scale, q, acc + bias) per row, in index order).  The sequential
gather (sls_exact 1) is bit-identical to it; every one-lookup form returns a row's value fmaf(scale, q, 0 + bias), which
is the one-row bag; the other forms apply the same per-row step in their own fp32 order and are checked against the int8
tables' bound (tests/test_int8_tables.py `terms`).
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

pytestmark = pytest.mark.gpu
I4 = N.TABLE_INT4_ROWWISE
I8 = N.TABLE_INT8_ROWWISE


def prepack(W):
    import torch
    return torch.ops.quantized.embedding_bag_4bit_prepack(torch.from_numpy(np.ascontiguousarray(W, np.float32)))


def pool(P, idx, lens):
    """embedding_bag_4bit_rowwise_offsets (sum) over bags of the given lengths: [len(lens), D] float32."""
    import torch
    lens = np.asarray(lens, np.int64)
    offsets = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    out = torch.ops.quantized.embedding_bag_4bit_rowwise_offsets(
        P, torch.from_numpy(np.asarray(idx, np.int64)[:int(lens.sum())].copy()), torch.from_numpy(offsets), mode=0,
        include_last_offset=False)
    return out.numpy().astype(np.float32)


def dequant(W):
    """Every row's value: its one-row bag, fmaf(scale, q, 0 + bias)."""
    rows = np.asarray(W).shape[0]
    return pool(prepack(W), np.arange(rows), np.ones(rows, np.int64))


def dequant8(W):
    """The same through torch's byte format: what a conversion 8 -> anything reads."""
    import torch
    rows = np.asarray(W).shape[0]
    P = torch.ops.quantized.embedding_bag_byte_prepack(torch.from_numpy(np.ascontiguousarray(W, np.float32)))
    out = torch.ops.quantized.embedding_bag_byte_rowwise_offsets(
        P, torch.arange(rows, dtype=torch.int64), torch.arange(rows, dtype=torch.int64), mode=0, include_last_offset=False)
    return out.numpy().astype(np.float32)


def terms(W):
    """|scale * q| + |bias| per element: the magnitude of what a row adds at each step of the fma form (the int8 tables'
    bound, for the reason given in tests/test_int8_tables.py)."""
    P = prepack(W).numpy()
    h = P.shape[1] - 4
    q = np.empty((P.shape[0], 2 * h), np.float64)
    q[:, 0::2] = P[:, :h] & 15
    q[:, 1::2] = P[:, :h] >> 4
    s = P[:, h:h + 2].copy().view(np.float16).astype(np.float64)
    b = P[:, h + 2:h + 4].copy().view(np.float16).astype(np.float64)
    return (np.abs(s * q) + np.abs(b)).astype(np.float32)


def upcast16(W):
    with np.errstate(over="ignore"):
        return np.ascontiguousarray(W, np.float32).astype(np.float16).astype(np.float32)


def _engine(rows, D, L, B, dtype, slots=2, staged=2):
    T = len(rows)
    eng = N.Engine(N.MODEL_DLRM, rows, D, [8, D], [D * (T + 1), 4, 1], N.INTERACT_CAT, sigmoid_top=2,
                   max_batch=B, max_lookups=L, num_staged_batches=staged, num_slots=slots)
    if dtype != N.TABLE_FP32:
        eng.set_option("table_dtype", dtype)
    return eng


def _fc(eng, D, T, seed=11):
    rng = np.random.RandomState(seed)
    eng.set_fc(N.MLP_BOT, 0, rng.randn(D, 8).astype(np.float32), rng.randn(D).astype(np.float32))
    eng.set_fc(N.MLP_TOP, 0, rng.randn(4, D * (T + 1)).astype(np.float32) * 0.05, np.zeros(4, np.float32))
    eng.set_fc(N.MLP_TOP, 1, rng.randn(1, 4).astype(np.float32), np.zeros(1, np.float32))


def _load(eng, tables, D):
    for t, W in enumerate(tables):
        eng.set_table(t, W)
    _fc(eng, D, len(tables))


# option settings every case runs under: (sls_exact, sls_flat, sls_one) -- test_int8_tables.py's
SETTINGS = [(1, 1, 1), (1, 1, 16), (1, 1, 64), (1, 1, 0), (0, 1, 1), (0, 0, 1), (0, 2, 1)]


def _special_rows(W):
    W[0] = 0.3125                                   # a constant row: scale 0 -> 1, every code 0
    W[1] = np.abs(W[1]) + 0.25
    W[1, W.shape[1] // 2] = -0.0                    # a row whose minimum is -0
    W[2] *= 1e-6                                    # a row whose fp16 scale is subnormal
    W[3] = np.round(W[3] * 4) / 4                   # a row full of rounding ties after scaling
    return W


def _stride(D):
    return (D // 2 + 3) // 4 * 4 + 4                # bytes between int4 rows


def _stride8(D):
    return (D + 7) // 8 * 8 + 8                     # ... between int8 rows


def _one_row_bags(eng, rows, D, B, ix_per_table):
    """pooled columns of L = 1 bags over the given rows of each table, under every sls_one setting (sls_exact 1)"""
    T = len(rows)
    eng.stage_batch(0, np.zeros((B, 8), np.float32), ix_per_table, [np.ones(B, np.int32)] * T)
    out = []
    eng.set_option("sls_exact", 1)
    for one in (1, 16, 64, 0):
        eng.set_option("sls_one", one)
        eng.forward(0, B)
        out.append(eng.fetch_interaction(B)[:, D:].copy())
    return out


def _same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


# ------------------------------------------------------------------------------------------------------------------------
# 1. the gather against torch
@pytest.mark.parametrize("D", [2, 6, 8, 12, 16, 32, 64, 128, 256])
@pytest.mark.parametrize("L", [1, 20, 80, "ragged"])
def test_int4_gather_against_torch(D, L):
    """sls_exact 1: the pooled columns are bit-identical to embedding_bag_4bit_rowwise_offsets.  Every other form (split
    ring walk, flat, flat-coalesced, one-lookup) is within 4 L 2^-24 of the sum of the magnitudes each row adds, gives
    the same bits run to run, and the same bits for a query served alone and inside coalesced sets of 12 and 16."""
    rng = np.random.RandomState(D * 7 + (0 if L == "ragged" else L))
    T, B = 3, 48
    Lmax = 30 if L == "ragged" else L
    rows = [1501 + 13 * t for t in range(T)]
    tables = [_special_rows(rng.uniform(-1, 1, (r, D)).astype(np.float32)) for r in rows]
    packed = [prepack(W) for W in tables]
    mags = [terms(W) for W in tables]
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
    eng = _engine(rows, D, Lmax, B, I4, slots=2)
    try:
        _load(eng, tables, D)
        for b in range(2):
            eng.stage_batch(b, dense[b], idx[b], lens[b])
        refs = {}

        def ref(b, bs):
            if (b, bs) not in refs:
                out, bound = [], []
                for t in range(T):
                    n = int(lens[b][t][:bs].sum())
                    out.append(pool(packed[t], idx[b][t][:n], lens[b][t][:bs]))
                    bound.append(orc.sls(mags[t], idx[b][t][:n], lens[b][t][:bs]) * (4.0 * max(Lmax, 1) * 2.0 ** -24))
                refs[(b, bs)] = (np.concatenate(out, axis=1), np.concatenate(bound, axis=1))
            return refs[(b, bs)]

        def check(got, b, bs, exact, what):
            exp, bound = ref(b, bs)
            if exact:
                assert _same(got, exp), what
            else:
                err = np.abs(got.astype(np.float64) - exp)
                assert np.all(err <= bound), (what, float((err - bound).max()))

        jobs12 = [((k % 2), (B, 1, 17, 0)[k % 4]) for k in range(12)]
        jobs16 = [((k + 1) % 2, (5, B, 33, 1)[k % 4]) for k in range(16)]
        for exact, flat, one in SETTINGS:
            eng.set_option("sls_exact", exact)
            eng.set_option("sls_flat", flat)
            eng.set_option("sls_one", one)
            alone = {}
            for b in range(2):
                for bs in sorted({B, 1, 29, 17, 5, 33, 0} - {0}):
                    eng.forward(b, bs)
                    R = eng.fetch_interaction(bs)[:, D:].copy()
                    eng.forward(b, bs)
                    assert np.array_equal(eng.fetch_interaction(bs)[:, D:], R), ("run to run", exact, flat, one, b, bs)
                    check(R, b, bs, exact, (exact, flat, one, b, bs))
                    alone[(b, bs)] = R
            for jobs in (jobs12, jobs16):
                eng.forward_multi_async(1, [b for b, _ in jobs], [n for _, n in jobs])
                eng.wait(1, sum(n for _, n in jobs))
                vrows = sum((n + 63) // 64 * 64 for _, n in jobs)
                Rc = eng.fetch_interaction(vrows, slot=1)
                v = 0
                for b, n in jobs:
                    if n:
                        assert np.array_equal(Rc[v:v + n, D:], alone[(b, n)]), (exact, flat, one, len(jobs), b, n)
                    v += (n + 63) // 64 * 64
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------------------------------
# 2. one-row bags pin the quantization on every writing path
@pytest.mark.parametrize("D", [12, 16, 64, 128])
def test_one_row_bags_pin_the_quantization_on_every_writing_path(D):
    """L = 1 bags over every row of small tables return fmaf(s, q, 0 + b) of embedding_bag_4bit_prepack's rows, bit for
    bit, whichever way the table was written: set_table after table_dtype 9, table_dtype 9 after set_table (0 -> 9),
    fp16 -> 9, int8 -> 9, and fill_table_uniform (orc.fill_table_uniform's values, quantized) -- which 9 -> 0 then
    holds as fp32."""
    rng = np.random.RandomState(D)
    rows, B = [300, 257], 320
    T = len(rows)
    tables = [_special_rows(rng.uniform(-1, 1, (r, D)).astype(np.float32)) for r in rows]
    ix = [(np.arange(B) % r).astype(np.int64) for r in rows]

    def expect(tabs):
        return np.concatenate([dequant(W)[ix[t]] for t, W in enumerate(tabs)], axis=1)

    a = _engine(rows, D, 1, B, I4, slots=1, staged=1)            # table_dtype 9, then set_table
    b = _engine(rows, D, 1, B, N.TABLE_FP32, slots=1, staged=1)  # set_table, then table_dtype 9
    c = _engine(rows, D, 1, B, N.TABLE_FP16, slots=1, staged=1)  # fp16 tables, then table_dtype 9
    d = _engine(rows, D, 1, B, I8, slots=1, staged=1)            # int8 tables, then table_dtype 9
    try:
        _load(a, tables, D)
        for eng in (b, c, d):
            _load(eng, tables, D)
            eng.set_option("table_dtype", I4)
        exp = expect(tables)
        for eng, e in ((a, exp), (b, exp), (c, expect([upcast16(W) for W in tables])),
                       (d, expect([dequant8(W) for W in tables]))):
            assert eng.get_option("table_dtype") == I4
            for k, got in enumerate(_one_row_bags(eng, rows, D, B, ix)):
                assert _same(got, e), k
        fills = []
        for t in range(T):
            a.fill_table_uniform(t, -0.25, 0.5, 77)
            fills.append(orc.fill_table_uniform(rows[t], D, t, -0.25, 0.5, 77, nthreads=0))
        e = expect(fills)
        for k, got in enumerate(_one_row_bags(a, rows, D, B, ix)):
            assert _same(got, e), k
        a.set_option("table_dtype", N.TABLE_FP32)                # 9 -> 0 holds each row's value
        for k, got in enumerate(_one_row_bags(a, rows, D, B, ix)):
            assert _same(got, e), k
    finally:
        for eng in (a, b, c, d):
            eng.close()


@pytest.mark.parametrize("D", [12, 32])
def test_line_packed_int8_rows_convert_to_int4(D):
    """8 -> 9 out of the line-packed int8 layout (table_int8_lines 1; D 12: five rows to a line, D 32: three): every
    int8 row's value, quantized as prepack quantizes it; and back, 9 -> 8, into the line-packed layout again."""
    rng = np.random.RandomState(40 + D)
    rows, B = [301, 130], 320
    tables = [_special_rows(rng.uniform(-1, 1, (r, D)).astype(np.float32)) for r in rows]
    ix = [(np.arange(B) % r).astype(np.int64) for r in rows]
    eng = _engine(rows, D, 1, B, N.TABLE_FP32, slots=1, staged=1)
    try:
        eng.set_option("table_int8_lines", 1)
        eng.set_option("table_dtype", I8)
        _load(eng, tables, D)
        lines_bytes = eng.get_option("table_bytes")
        assert lines_bytes == sum(((r + 128 // _stride8(D) - 1) // (128 // _stride8(D)) * 128 + 255) // 256 * 256 for r in rows)
        eng.set_option("table_dtype", I4)
        assert eng.get_option("table_bytes") == sum((r * _stride(D) + 255) // 256 * 256 for r in rows)
        v8 = [dequant8(W) for W in tables]
        e = np.concatenate([dequant(v8[t])[ix[t]] for t in range(len(rows))], axis=1)
        for k, got in enumerate(_one_row_bags(eng, rows, D, B, ix)):
            assert _same(got, e), k
        eng.set_option("table_dtype", I8)
        assert eng.get_option("table_bytes") == lines_bytes
        e = np.concatenate([dequant8(dequant(v8[t]))[ix[t]] for t in range(len(rows))], axis=1)
        for k, got in enumerate(_one_row_bags(eng, rows, D, B, ix)):
            assert _same(got, e), k
    finally:
        eng.close()


@pytest.mark.parametrize("D", [12, 32])
def test_line_packed_int4_rows_convert_to_line_packed_int8(D):
    """9 -> 8 with BOTH sides line-packed (table_int4_lines 1 and table_int8_lines 1; D 12: ten int4 rows and five int8
    rows to a line, D 32: six and three): every int4 row's value, quantized as byte prepack quantizes it.  Tables of 37
    and 5 rows: the last line of each is partly filled on either side."""
    rng = np.random.RandomState(60 + D)
    rows, B = [37, 5], 37
    tables = [_special_rows(rng.uniform(-1, 1, (r, D)).astype(np.float32)) for r in rows]
    ix = [(np.arange(B) % r).astype(np.int64) for r in rows]                  # every row of either table
    n4, n8 = 128 // _stride(D), 128 // _stride8(D)
    eng = _engine(rows, D, 1, B, N.TABLE_FP32, slots=1, staged=1)
    try:
        eng.set_option("table_int4_lines", 1)
        eng.set_option("table_int8_lines", 1)
        eng.set_option("table_dtype", I4)
        _load(eng, tables, D)
        assert eng.get_option("table_bytes") == sum(((r + n4 - 1) // n4 * 128 + 255) // 256 * 256 for r in rows)
        eng.set_option("table_dtype", I8)
        assert eng.get_option("table_bytes") == sum(((r + n8 - 1) // n8 * 128 + 255) // 256 * 256 for r in rows)
        e = np.concatenate([dequant8(dequant(W))[ix[t]] for t, W in enumerate(tables)], axis=1)
        for k, got in enumerate(_one_row_bags(eng, rows, D, B, ix)):
            assert _same(got, e), k
    finally:
        eng.close()


def test_rows_wider_than_a_wave_take_the_generic_form():
    """D 258 (even, no multiple of 4, above 256): sls_any_kernel<i4> walks the row in two passes of 64 x 4 columns;
    ragged bags with empty ones, bit-identical to embedding_bag_4bit_rowwise_offsets under either sls_exact."""
    D, T, B, Lmax = 258, 2, 16, 9
    rng = np.random.RandomState(258)
    rows = [300, 77]
    tables = [_special_rows(rng.uniform(-1, 1, (r, D)).astype(np.float32)) for r in rows]
    ln = [rng.randint(0, Lmax + 1, size=B).astype(np.int32) for _ in range(T)]
    for t in range(T):
        ln[t][:2] = 0
    ix = [rng.randint(0, rows[t], size=int(ln[t].sum())).astype(np.int64) for t in range(T)]
    for t in range(T):
        ix[t][0], ix[t][-1] = 0, rows[t] - 1
    exp = np.concatenate([pool(prepack(tables[t]), ix[t], ln[t]) for t in range(T)], axis=1)
    eng = _engine(rows, D, Lmax, B, I4, slots=1, staged=1)
    try:
        _load(eng, tables, D)
        eng.set_option("dispatch_log", 1)
        eng.stage_batch(0, rng.rand(B, 8).astype(np.float32), ix, ln)
        for exact in (1, 0):
            eng.set_option("sls_exact", exact)
            eng.forward(0, B)
            assert "sls_any_kernel<i4>" in " ".join(eng.last_dispatch()), eng.last_dispatch()
            assert _same(eng.fetch_interaction(B)[:, D:], exp), exact
    finally:
        eng.close()


def test_set_table_quantizes_whole_rows_across_staging_chunks():
    """A table of more than 16 M elements crosses the bus in several chunks of whole rows: the rows on both sides of
    every chunk boundary and the last rows come out as prepack quantizes them."""
    D, B = 16, 256
    rows = [(17 << 20) // D + 37, 90]
    rng = np.random.RandomState(5)
    tables = [rng.uniform(-1, 1, (r, D)).astype(np.float32) for r in rows]
    chunk = (16 << 20) // D
    picks = np.unique(np.concatenate([np.arange(0, 8), np.arange(chunk - 60, chunk + 60), np.arange(rows[0] - 68, rows[0])]))
    ix0 = np.resize(picks, B).astype(np.int64)
    ix = [ix0, (np.arange(B) % rows[1]).astype(np.int64)]
    eng = _engine(rows, D, 1, B, I4, slots=1, staged=1)
    try:
        _load(eng, tables, D)
        P0 = prepack(tables[0][picks])
        pos = {int(r): k for k, r in enumerate(picks)}
        e0 = pool(P0, [pos[int(r)] for r in ix0], np.ones(B, np.int64))
        e = np.concatenate([e0, dequant(tables[1])[ix[1]]], axis=1)
        for got in _one_row_bags(eng, rows, D, B, ix):
            assert _same(got, e)
        assert eng.get_option("table_bytes") == (rows[0] * 12 + 255) // 256 * 256 + (rows[1] * 12 + 255) // 256 * 256
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------------------------------
# 3. accounting and conversions
def test_accounting_conversions_placements_and_refusals():
    """gather_bytes counts D / 2 + 4 bytes per gathered row, table_bytes follows the layout, the dispatch log names the
    int4 launches, placement candidates copy the int4 arena, table_int8_lines changes nothing, 10 is refused, 9 -> 0
    gives an fp32 arena of the row values and 9 -> 8 torch's byte prepack of them."""
    rows, D, T, L, B = [3000, 2000, 1000, 700], 64, 4, 80, 32
    rng = np.random.RandomState(1)
    tables = [_special_rows(rng.uniform(-1, 1, (r, D)).astype(np.float32)) for r in rows]
    ix = [rng.randint(0, rows[t], size=B * L).astype(np.int64) for t in range(T)]
    ln = [np.full(B, L, np.int32) for _ in range(T)]
    X = rng.rand(B, 8).astype(np.float32)
    exp = np.concatenate([pool(prepack(tables[t]), ix[t], ln[t]) for t in range(T)], axis=1)
    nbytes = sum((r * _stride(D) + 255) // 256 * 256 for r in rows)
    e = _engine(rows, D, L, B, N.TABLE_FP32, slots=3, staged=1)
    f = _engine(rows, D, L, B, N.TABLE_FP32, slots=1, staged=1)
    try:
        _load(e, tables, D)
        e.set_option("dispatch_log", 1)
        e.stage_batch(0, X, ix, ln)
        assert e.gather_bytes(0, B) == B * T * (L * D * 4 + L * 4 + 4 + D * 4)
        e.set_option("table_dtype", I4)
        assert e.get_option("table_dtype") == I4
        assert e.gather_bytes(0, B) == B * T * (L * (D // 2 + 4) + L * 4 + 4 + D * 4)
        assert e.get_option("table_bytes") == nbytes
        for key in ("mlp_streams", "preferred_slots", "preferred_coalesce", "gather_bound"):
            e.get_option(key)
        e.forward(0, B)
        assert "sls_flatc_kernel<16,20,nt,i4>" in " ".join(e.last_dispatch()), e.last_dispatch()
        e.set_option("sls_exact", 1)
        e.forward(0, B)
        assert "sls_kernel<16,sequential,i4>" in " ".join(e.last_dispatch()), e.last_dispatch()
        R4 = e.fetch_interaction(B)[:, D:].copy()
        assert _same(R4, exp)
        # table_int8_lines 1 after table_dtype 9: remembered, the arena and the bits stay
        e.set_option("table_int8_lines", 1)
        assert e.get_option("table_int8_lines") == 1 and e.get_option("table_bytes") == nbytes
        e.forward(0, B)
        assert np.array_equal(e.fetch_interaction(B)[:, D:], R4)
        assert "i4>" in " ".join(e.last_dispatch()) and "i8l" not in " ".join(e.last_dispatch())
        # ... and before it: the same arena
        f.set_option("table_int8_lines", 1)
        f.set_option("table_dtype", I4)
        _load(f, tables, D)
        f.stage_batch(0, X, ix, ln)
        f.set_option("sls_exact", 1)
        f.forward(0, B)
        assert f.get_option("table_bytes") == nbytes and np.array_equal(f.fetch_interaction(B)[:, D:], R4)
        # placement candidates are copies of the int4 arena
        e.set_option("table_placement", -1)
        assert e.get_option("table_placements") == 2
        e.forward(0, B)
        assert np.array_equal(e.fetch_interaction(B)[:, D:], R4)
        # 10 is refused and changes nothing
        with pytest.raises(N.DrsError) as er:
            e.set_option("table_dtype", 10)
        assert er.value.code == N.ERR_BAD_ARG and e.get_option("table_dtype") == I4
        assert e.get_option("table_placements") == 2
        e.forward(0, B)
        assert np.array_equal(e.fetch_interaction(B)[:, D:], R4)
        # 9 -> 0: an fp32 arena holding each row's value; its one-row bags equal the int4 ones
        one = [(np.arange(B) * 7 % r).astype(np.int64) for r in rows]
        ones = [np.ones(B, np.int32)] * T
        e.stage_batch(0, X, one, ones)
        e.forward(0, B)
        R1 = e.fetch_interaction(B)[:, D:].copy()
        vals = [dequant(W) for W in tables]
        assert _same(R1, np.concatenate([vals[t][one[t]] for t in range(T)], axis=1))
        e.set_option("table_dtype", N.TABLE_FP32)
        assert e.get_option("table_placements") == 1 and e.get_option("table_bytes") == sum(
            (r * D + 63) // 64 * 64 * 4 for r in rows)
        e.forward(0, B)
        assert np.array_equal(e.fetch_interaction(B)[:, D:], R1)
        assert "i4" not in " ".join(e.last_dispatch())
        # 9 -> 8 (f; table_int8_lines 1 is remembered: the line-packed int8 arena): torch's byte prepack of the row values
        f.stage_batch(0, X, one, ones)
        f.set_option("table_dtype", I8)
        f.forward(0, B)
        assert _same(f.fetch_interaction(B)[:, D:], np.concatenate([dequant8(vals[t])[one[t]] for t in range(T)], axis=1))
        # ... and 9 -> 1 rounds each row's value to fp16 (nearest even)
        f.set_option("table_dtype", I4)
        f.set_option("table_dtype", N.TABLE_FP16)
        f.forward(0, B)
        again = [dequant(dequant8(vals[t])) for t in range(T)]
        assert _same(f.fetch_interaction(B)[:, D:], np.concatenate([upcast16(again[t])[one[t]] for t in range(T)], axis=1))
    finally:
        e.close()
        f.close()


def test_odd_width_is_unsupported_and_the_engine_keeps_serving_fp32():
    rows, D, T, L, B = [500, 300], 5, 2, 6, 16
    rng = np.random.RandomState(2)
    tables = [rng.uniform(-1, 1, (r, D)).astype(np.float32) for r in rows]
    ix = [rng.randint(0, rows[t], size=B * L).astype(np.int64) for t in range(T)]
    ln = [np.full(B, L, np.int32) for _ in range(T)]
    e = _engine(rows, D, L, B, N.TABLE_FP32, slots=1, staged=1)
    try:
        _load(e, tables, D)
        e.stage_batch(0, rng.rand(B, 8).astype(np.float32), ix, ln)
        e.forward(0, B)
        before = e.fetch_interaction(B).copy()
        assert _same(before[:, D:], np.concatenate([orc.sls(tables[t], ix[t], ln[t]) for t in range(T)], axis=1))
        nbytes = e.get_option("table_bytes")
        with pytest.raises(N.DrsError) as er:
            e.set_option("table_dtype", I4)
        assert er.value.code == N.ERR_UNSUPPORTED
        assert e.get_option("table_dtype") == N.TABLE_FP32 and e.get_option("table_bytes") == nbytes
        e.forward(0, B)
        assert np.array_equal(e.fetch_interaction(B), before)
    finally:
        e.close()


# ------------------------------------------------------------------------------------------------------------------------
# 4. DIN and DIEN
@pytest.mark.parametrize("case", ["din_mini", "dien_mini"])
def test_din_and_dien_refuse_int4_tables(case):
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
        with pytest.raises(N.DrsError) as e:
            eng.set_option("table_dtype", I4)
        assert e.value.code == N.ERR_UNSUPPORTED and eng.get_option("table_dtype") == N.TABLE_FP32
        assert np.array_equal(net.run_staged(0, n), before)
    finally:
        net.engine.close()


# ------------------------------------------------------------------------------------------------------------------------
# 5. whole models
@pytest.mark.parametrize("case", [c for c in H.MODEL_CASES if not c.startswith(("din", "dien"))])
def test_models_with_int4_tables(case):
    """Every fixture model but DIN / DIEN with --accel_table_dtype int4_rowwise: with sls_exact 1 the interaction tensor
    is the one of torch's pooled sums (the pooled columns themselves, or for the dot interaction the dot products of
    them), bit for bit; the outputs are within 1e-4 of the oracle model run on the dequantized tables."""
    meta, z = H.load_fixture(case)
    args = H.args_from(meta["args"], accel_table_dtype="int4_rowwise")
    net, lX, lS_l, lS_i, lT = H.materialize(args)
    net.create(lX[0], lS_l[0], lS_i[0], lT[0])
    try:
        assert net.engine.get_option("table_dtype") == I4
        emb = net.emb_w
        packed = [prepack(W) for W in emb]
        net.emb_w = [dequant(W) for W in emb]
        om = H.oracle_model(net)
        net.emb_w = emb
        no_dense = args.model_type in H.NO_DENSE
        net.stage_batches(None if no_dense else lX, lS_l, lS_i)
        n = len(lS_l[0][0])
        net.engine.set_option("sls_exact", 1)
        D = int(args.arch_sparse_feature_size)
        for bid in range(len(lS_l)):
            for bs in sorted({n, 1, max(1, n // 2)}):
                got = net.run_staged(bid, bs)
                R = net.engine.fetch_interaction(bs)
                exp, R_om = om.forward(None if no_dense else lX[bid], lS_i[bid], lS_l[bid], bs=bs, want_R=True)
                assert H.close(got, exp, rtol=1e-4, atol=1e-4), (case, np.abs(got - exp).max())
                if args.model_type == "dlrm":
                    pooled = []
                    for t in range(len(emb)):
                        ln = np.asarray(lS_l[bid][t][:bs], np.int64)
                        pooled.append(pool(packed[t], lS_i[bid][t], ln))
                    if net.arch_interaction_op == "dot":
                        Tt = np.stack([R_om[:, :D]] + pooled, axis=1)
                        R_exp = orc.interact_dot(Tt, itself=bool(net.arch_interaction_itself))
                    else:
                        R_exp = np.concatenate([R_om[:, :D]] + pooled, axis=1)
                else:
                    R_exp = R_om            # one lookup per bag: the pooled value is the row's value
                assert _same(R, R_exp), (case, bid, bs)
    finally:
        net.engine.close()


def test_rm1_mini_with_int4_tables_and_mean_pooling():
    """sls_pool 1 composes: the pooled columns are torch's int4 sums divided by the bag lengths (one correctly rounded
    fp32 division per element; an empty bag stays +0), bit for bit under sls_exact 1."""
    meta, z = H.load_fixture("dlrm_rm1_mini")
    args = H.args_from(meta["args"], accel_table_dtype="int4_rowwise", accel_sls_pool="mean")
    net, lX, lS_l, lS_i, lT = H.materialize(args)
    net.create(lX[0], lS_l[0], lS_i[0], lT[0])
    try:
        eng = net.engine
        assert eng.get_option("table_dtype") == I4 and eng.get_option("sls_pool") == 1
        assert net.arch_interaction_op == "cat"
        packed = [prepack(W) for W in net.emb_w]
        net.stage_batches(lX, lS_l, lS_i)
        n = len(lS_l[0][0])
        eng.set_option("sls_exact", 1)
        eng.set_option("dispatch_log", 1)
        D = int(args.arch_sparse_feature_size)
        for bid in range(len(lS_l)):
            net.run_staged(bid, n)
            R = eng.fetch_interaction(n)[:, D:]
            assert "i4,mean" in " ".join(eng.last_dispatch()), eng.last_dispatch()
            cols = []
            for t in range(len(packed)):
                ln = np.asarray(lS_l[bid][t][:n], np.int64)
                div = np.where(ln > 0, ln, 1).astype(np.float32)[:, None]
                cols.append((pool(packed[t], lS_i[bid][t], ln) / div).astype(np.float32))
            assert _same(R, np.concatenate(cols, axis=1)), bid
    finally:
        net.engine.close()


# ------------------------------------------------------------------------------------------------------------------------
# 6. the stand-alone entry and the queue harness
def test_stand_alone_entry_and_queue_harness_with_int4_tables(tmp_path):
    """`python -m deeprecsys_amd.dlrm_s_hip --accel_table_dtype int4_rowwise` prints its `***` lines, and a short
    `DeepRecSys.py --queue --model_accel` run serves its queries from int4 tables."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = dict(arch_mlp_bot="16-8", arch_mlp_top="64-16-1", arch_embedding_size="-".join(["3000"] * 6),
               arch_sparse_feature_size=8, num_indices_per_lookup_fixed=True, num_indices_per_lookup=20,
               arch_interaction_op="dot", model_type="dlrm", model_name="mini")
    path = str(tmp_path / "mini.json")
    json.dump(cfg, open(path, "w"))
    r = subprocess.run([sys.executable, "-m", "deeprecsys_amd.dlrm_s_hip", "--inference_only", "--use_accel",
                        "--config_file", path, "--nepochs", "3", "--num_batches", "2", "--mini_batch_size", "64",
                        "--max_mini_batch_size", "64", "--accel_table_dtype", "int4_rowwise"],
                       cwd=root, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.count("***") == 6, r.stdout[-2000:]
    r = subprocess.run([sys.executable, "-m", "deeprecsys_amd.DeepRecSys", "--queue", "--model_accel",
                        "--inference_engines", "0", "--config_file", path, "--num_batches", "4", "--nepochs", "1",
                        "--avg_arrival_rate", "1", "--max_mini_batch_size", "64", "--avg_mini_batch_size", "32",
                        "--accel_table_dtype", "int4_rowwise", "--accel_table_placements", "1",
                        "--log_file", str(tmp_path / "log" / "out.log")],
                       cwd=root, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert len(open(str(tmp_path / "log" / "out.log")).read().strip().splitlines()) == 4
