"""The line-packed int4 rowwise layout on the GPU (-m gpu): engine option "table_int4_lines" 1 on top of "table_dtype" 9.

The layout moves rows, never values: an engine with the option serves the bits of a plain int4 engine holding the same
tables, under every launch form, and with sls_exact 1 the bits of torch's embedding_bag_4bit_rowwise_offsets over
embedding_bag_4bit_prepack rows.
"""
import numpy as np
import pytest

from deeprecsys_amd import _native as N
from tests import helpers as H

pytestmark = pytest.mark.gpu
I4 = N.TABLE_INT4_ROWWISE
I8 = N.TABLE_INT8_ROWWISE
KEY = "table_int4_lines"

# option settings every case runs under: (sls_exact, sls_flat, sls_one) -- test_half_tables.py's
SETTINGS = [(1, 1, 1), (1, 1, 16), (1, 1, 64), (1, 1, 0), (0, 1, 1), (0, 0, 1), (0, 2, 1)]


# ---- the independent checker (test_int4_tables.py's idea, restated) ---------------------------------------------------
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


# ---- the layout rule (docs/OPTIONS.md) ---------------------------------------------------------------------------------
def row_bytes(D):
    return (D // 2 + 3) // 4 * 4 + 4


def rows_per_line(D):
    S = row_bytes(D)
    return 128 // S if S < 128 and 128 % S else 0


def table_bytes(rows, D, lines):
    S, n = row_bytes(D), rows_per_line(D) if lines else 0
    total = 0
    for r in rows:
        total += (((r + n - 1) // n * 128 if n else r * S) + 255) // 256 * 256
    return total


def _engine(rows, D, L, B, lines, dtype=I4, slots=2, staged=2, lines_first=True):
    T = len(rows)
    eng = N.Engine(N.MODEL_DLRM, rows, D, [8, D], [D * (T + 1), 4, 1], N.INTERACT_CAT, sigmoid_top=2,
                   max_batch=B, max_lookups=L, num_staged_batches=staged, num_slots=slots)
    if lines and lines_first:
        eng.set_option(KEY, 1)
    if dtype != N.TABLE_FP32:
        eng.set_option("table_dtype", dtype)
    if lines and not lines_first:
        eng.set_option(KEY, 1)
    eng.set_option("dispatch_log", 1)
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


def _special_rows(W):
    W[0] = 0.3125                                   # a constant row: scale 0 -> 1, every code 0
    W[1] = np.abs(W[1]) + 0.25
    W[1, W.shape[1] // 2] = -0.0                    # a row whose minimum is -0
    W[2] *= 1e-6                                    # a row whose fp16 scale is subnormal
    return W


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _pooled(eng, D, bs, slot=0):
    return eng.fetch_interaction(bs, slot=slot)[:, D:].copy()


def _log(eng, slot=0):
    return " ".join(eng.last_dispatch(slot))


def _planted(rows, n):
    """rows an index set must hold: the table's first and last row, every residue r % n, both sides of line boundaries"""
    n = max(n, 1)
    return sorted(set([0, rows - 1] + list(range(0, 2 * n + 1)) + [n - 1, n, 7 * n - 1, 7 * n, rows - 1 - n, rows - n, rows - 2]))


def _inputs(rng, rows, D, L, B, n_sets=2):
    """n_sets index sets: fixed bags of L rows or ragged ones with empty bags; the planted rows lead table t's indices"""
    T = len(rows)
    Lmax = 30 if L == "ragged" else L
    idx, lens = [], []
    for b in range(n_sets):
        if L == "ragged":
            ln = [rng.randint(0, Lmax + 1, size=B).astype(np.int32) for _ in range(T)]
            for t in range(T):
                ln[t][:3] = 0                                          # empty bags
                ln[t][3:5] = Lmax
        else:
            ln = [np.full(B, L, np.int32) for _ in range(T)]
        ix = [rng.randint(0, rows[t], size=int(ln[t].sum())).astype(np.int64) for t in range(T)]
        for t in range(T):
            plant = np.array(_planted(rows[t], rows_per_line(D)), np.int64)
            assert plant.size < ix[t].size
            ix[t][:plant.size] = plant
            ix[t][-1] = rows[t] - 1
        idx.append(ix)
        lens.append(ln)
    return idx, lens, Lmax


def _assert_coverage(idx, lens, rows, D, bs):
    """EVERY index set, in what its first bs samples gather, holds every residue r % n, the first and last row and both
    sides of a line boundary of every table"""
    n = max(rows_per_line(D), 1)
    for ix, ln in zip(idx, lens):
        for t, r in enumerate(rows):
            used = ix[t][:int(ln[t][:bs].sum())]
            assert set(used % n) == set(range(n)), (t, "residues")
            assert 0 in used and r - 1 in used, (t, "first and last row")
            if n > 1:
                assert n - 1 in used and n in used, (t, "both sides of a line boundary")
            assert used.max() < r


ROWS = [3001, 2003, 1001]          # 3001 = n k + 1 for every n of the rule; none is a multiple of 2, 3, 4, 5, 6 or 10


# ---- 1. bit identity with plain int4, under every launch form --------------------------------------------------------
@pytest.mark.parametrize("D", [12, 32, 40, 48, 64, 100, 128, 30])
@pytest.mark.parametrize("L", [1, 20, 80, "ragged"])
def test_lines_serve_the_bits_of_plain_int4_under_every_form(D, L):
    """Two engines on the same fp32 tables, plain int4 and line-packed: equal interaction tensors as uint32 for single
    queries of B, 1 and 17 samples and for a coalesced set of three, under every setting of SETTINGS (sequential / split
    ring walk, one-lookup copy, flat, flat-coalesced; D 30: the any-width form).  With sls_exact 1 the pooled columns
    are torch's as well."""
    rng = np.random.RandomState(D * 13 + (0 if L == "ragged" else L))
    B = 32
    rows = ROWS if D < 100 else ROWS[:2]
    T = len(rows)
    n = rows_per_line(D)
    assert n == {12: 10, 32: 6, 40: 5, 48: 4, 64: 3, 100: 2, 128: 1, 30: 6}[D]
    assert all(r % n for r in rows if n > 1) and rows[0] % n == (1 if n > 1 else 0), (D, n)
    tables = [_special_rows(rng.uniform(-1, 1, (r, D)).astype(np.float32)) for r in rows]
    idx, lens, Lmax = _inputs(rng, rows, D, L, B)
    _assert_coverage(idx, lens, rows, D, B)
    dense = [rng.rand(B, 8).astype(np.float32) for _ in range(2)]
    packed = [prepack(W) for W in tables]
    torch_sums = {(b, bs): np.concatenate([pool(packed[t], idx[b][t][:int(lens[b][t][:bs].sum())], lens[b][t][:bs])
                                           for t in range(T)], axis=1) for b in range(2) for bs in (B, 1, 17)}
    plain = _engine(rows, D, Lmax, B, 0)
    lines = _engine(rows, D, Lmax, B, 1)
    try:
        assert lines.get_option(KEY) == 1 and plain.get_option(KEY) == 0
        assert lines.get_option("table_dtype") == I4 and plain.get_option("table_dtype") == I4
        assert lines.get_option("table_bytes") == table_bytes(rows, D, 1)
        assert plain.get_option("table_bytes") == table_bytes(rows, D, 0)
        for eng in (plain, lines):
            _load(eng, tables, D)
            for b in range(2):
                eng.stage_batch(b, dense[b], idx[b], lens[b])
        jobs = [(0, B), (1, 17), (0, 1)]
        vrows = sum((m + 63) // 64 * 64 for _, m in jobs)
        for exact, flat, one in SETTINGS:
            for eng in (plain, lines):
                eng.set_option("sls_exact", exact)
                eng.set_option("sls_flat", flat)
                eng.set_option("sls_one", one)
            for b in range(2):
                for bs in (B, 1, 17):
                    plain.forward(b, bs)
                    lines.forward(b, bs)
                    want, got = plain.fetch_interaction(bs), lines.fetch_interaction(bs)
                    assert np.array_equal(_bits(got), _bits(want)), (exact, flat, one, b, bs)
                    if exact:
                        assert np.array_equal(_bits(got[:, D:]), _bits(torch_sums[(b, bs)])), (flat, one, b, bs)
                    log = _log(lines)
                    assert ",i4l>" in log or "<i4l>" in log, log
                    assert "i4l" not in _log(plain) and ("i4>" in _log(plain))
            for eng in (plain, lines):
                eng.forward_multi_async(1, [b for b, _ in jobs], [m for _, m in jobs])
                eng.wait(1, sum(m for _, m in jobs))
            want, got = plain.fetch_interaction(vrows, slot=1), lines.fetch_interaction(vrows, slot=1)
            v = 0
            for b, m in jobs:
                assert np.array_equal(_bits(got[v:v + m]), _bits(want[v:v + m])), (exact, flat, one, "set", b, m)
                v += (m + 63) // 64 * 64
    finally:
        plain.close()
        lines.close()


# ---- 2. against an independent checker ---------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [32, 64, 128])
def test_sequential_sums_are_torchs_bit_for_bit(D):
    """sls_exact 1, ragged bags: the pooled sums are embedding_bag_4bit_rowwise_offsets over embedding_bag_4bit_prepack
    rows, bit for bit."""
    rng = np.random.RandomState(D + 3)
    T, B = 3, 64
    rows = ROWS
    tables = [_special_rows(rng.uniform(-1, 1, (r, D)).astype(np.float32)) for r in rows]
    packed = [prepack(W) for W in tables]
    idx, lens, Lmax = _inputs(rng, rows, D, "ragged", B, n_sets=1)
    _assert_coverage(idx, lens, rows, D, B)
    eng = _engine(rows, D, Lmax, B, 1, staged=1)
    try:
        _load(eng, tables, D)
        eng.stage_batch(0, rng.rand(B, 8).astype(np.float32), idx[0], lens[0])
        eng.set_option("sls_exact", 1)
        for bs in (B, 17, 1):
            eng.forward(0, bs)
            exp = np.concatenate([pool(packed[t], idx[0][t][:int(lens[0][t][:bs].sum())], lens[0][t][:bs]) for t in range(T)], axis=1)
            assert np.array_equal(_bits(_pooled(eng, D, bs)), _bits(exp)), bs
            assert "sequential,i4l>" in _log(eng)
    finally:
        eng.close()


# ---- 3. index range ----------------------------------------------------------------------------------------------------
def test_the_unused_slots_of_the_last_line_are_out_of_range():
    """rows = 6 k + 1 at D 32: the last line holds one row and five unused slots.  The indices rows, rows + 1 (slots),
    6 (k + 1) - 1 (the last slot) and 6 (k + 1) are refused with DRS_ERR_INDEX_RANGE, staged or passed with the call,
    and the next valid query is served correctly."""
    D, L, B, k = 32, 4, 8, 350
    rows = [6 * k + 1]
    assert rows_per_line(D) == 6
    rng = np.random.RandomState(2)
    W = rng.uniform(-1, 1, (rows[0], D)).astype(np.float32)
    good = rng.randint(0, rows[0], size=B * L).astype(np.int64)
    good[:3] = [rows[0] - 1, rows[0] - 2, 0]
    ln = [np.full(B, L, np.int32)]
    X = rng.rand(B, 8).astype(np.float32)
    exp = pool(prepack(W), good, ln[0])
    eng = _engine(rows, D, L, B, 1, staged=1)
    try:
        _load(eng, [W], D)
        eng.set_option("sls_exact", 1)
        eng.stage_batch(0, X, [good], ln)
        eng.forward(0, B)
        assert np.array_equal(_bits(_pooled(eng, D, B)), _bits(exp))
        for bad_ix in (rows[0], rows[0] + 1, 6 * (k + 1) - 1, 6 * (k + 1)):
            bad = good.copy()
            bad[5] = bad_ix
            with pytest.raises(N.DrsError) as e:
                eng.stage_batch(0, X, [bad], ln)
            assert e.value.code == N.ERR_INDEX_RANGE, bad_ix
            with pytest.raises(N.DrsError) as e:
                eng.forward_inputs(X, [bad], ln, B)
            assert e.value.code == N.ERR_INDEX_RANGE, bad_ix
            # the batch staged before is untouched, and a valid query passed with the call is served
            eng.forward(0, B)
            assert np.array_equal(_bits(_pooled(eng, D, B)), _bits(exp)), bad_ix
            eng.forward_inputs(X, [good], ln, B)
            assert np.array_equal(_bits(_pooled(eng, D, B)), _bits(exp)), bad_ix
    finally:
        eng.close()


# ---- 4. option life cycle ----------------------------------------------------------------------------------------------
def test_option_life_cycle_on_one_engine():
    D, L, B, T = 64, 20, 32, 3
    rows = [3001, 2002, 1000]
    rng = np.random.RandomState(4)
    tables = [_special_rows(rng.uniform(-1, 1, (r, D)).astype(np.float32)) for r in rows]
    up16 = [W.astype(np.float16).astype(np.float32) for W in tables]
    ix = [rng.randint(0, rows[t], size=B * L).astype(np.int64) for t in range(T)]
    for t in range(T):
        ix[t][:8] = [0, 1, 2, 3, 4, 5, rows[t] - 1, rows[t] - 2]
    ln = [np.full(B, L, np.int32) for _ in range(T)]
    X = rng.rand(B, 8).astype(np.float32)
    fp32_bytes = sum((r * D + 63) // 64 * 64 * 4 for r in rows)

    def run(eng):
        eng.stage_batch(0, X, ix, ln)
        out = []
        for exact in (1, 0):
            eng.set_option("sls_exact", exact)
            eng.forward(0, B)
            out.append(_bits(_pooled(eng, D, B)))
        return np.stack(out)

    plain = _engine(rows, D, L, B, 0, slots=1, staged=1)
    a = _engine(rows, D, L, B, 1, slots=1, staged=1)                               # lines, then table_dtype 9
    b = _engine(rows, D, L, B, 1, slots=1, staged=1, lines_first=False)            # table_dtype 9, then lines
    c = _engine(rows, D, L, B, 0, dtype=N.TABLE_FP32, slots=1, staged=1)           # fp32 -> 9 with lines
    d = _engine(rows, D, L, B, 0, dtype=N.TABLE_FP16, slots=1, staged=1)           # fp16 -> 9 with lines
    p16 = _engine(rows, D, L, B, 0, slots=1, staged=1)
    try:
        for eng in (plain, a, b, c, d):
            _load(eng, tables, D)
        _load(p16, up16, D)
        want, want16 = run(plain), run(p16)
        assert np.array_equal(want[0], _bits(np.concatenate([pool(prepack(tables[t]), ix[t], ln[t]) for t in range(T)], axis=1)))
        gb = plain.gather_bytes(0, B)
        assert gb == B * T * (L * (D // 2 + 4) + L * 4 + 4 + D * 4)
        assert ",i4>" in _log(plain) and "i4l" not in _log(plain)
        c.set_option(KEY, 1)
        assert c.get_option("table_bytes") == fp32_bytes                           # (fp32: only remembered)
        c.set_option("table_dtype", I4)
        d.set_option("table_dtype", I4)
        d.set_option(KEY, 1)
        for eng, w in ((a, want), (b, want), (c, want), (d, want16)):
            assert eng.get_option(KEY) == 1 and eng.get_option("table_dtype") == I4
            assert eng.get_option("table_bytes") == table_bytes(rows, D, 1) == sum(((r + 2) // 3 * 128 + 255) // 256 * 256 for r in rows)
            assert np.array_equal(run(eng), w)
            assert eng.gather_bytes(0, B) == gb
            assert "i4l" in _log(eng)
        assert plain.get_option("table_bytes") == table_bytes(rows, D, 0) == sum((r * 36 + 255) // 256 * 256 for r in rows)
        # a value other than 0 and 1 is refused and changes nothing
        for bad in (2, -1):
            with pytest.raises(N.DrsError) as er:
                a.set_option(KEY, bad)
            assert er.value.code == N.ERR_BAD_ARG and a.get_option(KEY) == 1
        assert a.get_option("table_bytes") == table_bytes(rows, D, 1) and np.array_equal(run(a), want)
        # table_int8_lines keeps its independence: on an int4 arena it is only remembered
        a.set_option("table_int8_lines", 1)
        assert a.get_option("table_bytes") == table_bytes(rows, D, 1) and np.array_equal(run(a), want) and "i4l" in _log(a)
        a.set_option("table_int8_lines", 0)
        # placement candidates copy the arena bytes
        a.set_option("table_placement", -1)
        assert a.get_option("table_placements") == 2 and np.array_equal(run(a), want)
        # lines 1 -> 0: plain int4's arena and bits
        a.set_option(KEY, 0)
        assert a.get_option(KEY) == 0 and a.get_option("table_bytes") == table_bytes(rows, D, 0)
        assert a.get_option("table_placements") == 1
        assert np.array_equal(run(a), want) and "i4l" not in _log(a) and ",i4>" in _log(a)
        # ... and back
        a.set_option(KEY, 1)
        assert a.get_option("table_bytes") == table_bytes(rows, D, 1) and np.array_equal(run(a), want) and "i4l" in _log(a)
        # 9 with lines -> 0: an fp32 arena whose one-row bags are the rows' values
        one = [(np.arange(B) * 7 % r).astype(np.int64) for r in rows]
        for t in range(T):
            one[t][:3] = [rows[t] - 1, 0, rows[t] - 2]
        b.set_option("table_dtype", N.TABLE_FP32)
        assert b.get_option(KEY) == 1 and b.get_option("table_bytes") == fp32_bytes
        b.stage_batch(0, X, one, [np.ones(B, np.int32)] * T)
        b.set_option("sls_exact", 1)
        b.forward(0, B)
        exp = np.concatenate([dequant(tables[t])[one[t]] for t in range(T)], axis=1)
        assert np.array_equal(_bits(_pooled(b, D, B)), _bits(exp))
        assert "i4" not in _log(b)
        # 9 with lines <-> 8, without and with table_int8_lines: the same conversions from the plain int4 engine, bitwise
        for i8_lines in (0, 1):
            for eng in (plain, a):
                eng.set_option("table_int8_lines", i8_lines)
                eng.set_option("table_dtype", I8)
                assert eng.get_option("table_dtype") == I8
            assert a.get_option("table_bytes") == plain.get_option("table_bytes")
            got8, want8 = run(a), run(plain)
            assert np.array_equal(got8, want8)
            assert ("i8l" in _log(a)) == bool(i8_lines) and "i4" not in _log(a)
            for eng in (plain, a):
                eng.set_option("table_dtype", I4)
            assert a.get_option("table_bytes") == table_bytes(rows, D, 1) and plain.get_option("table_bytes") == table_bytes(rows, D, 0)
            assert np.array_equal(run(a), run(plain))
            assert "i4l" in _log(a) and ",i4>" in _log(plain)
        # ... and the layout moved under a line-packed int8 arena's feet: 8 with lines, then table_int4_lines 0, then 9
        a.set_option("table_dtype", I8)
        a.set_option(KEY, 0)
        a.set_option("table_dtype", I4)
        plain.set_option("table_dtype", I8)
        plain.set_option("table_dtype", I4)
        assert a.get_option("table_bytes") == table_bytes(rows, D, 0) and np.array_equal(run(a), run(plain))
    finally:
        for eng in (plain, a, b, c, d, p16):
            eng.close()


# ---- 5. plain layout kept ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [24, 56, 256])
def test_exact_fit_and_wide_rows_keep_the_plain_layout(D):
    """S = 16, 32 (a power of two: rows never cross a line) and S = 132 (> 128): the option is accepted, the arena is the
    plain one and the log says i4."""
    L, B = 20, 16
    rows = [1001, 700]
    assert rows_per_line(D) == 0
    rng = np.random.RandomState(D)
    tables = [rng.uniform(-1, 1, (r, D)).astype(np.float32) for r in rows]
    ix = [rng.randint(0, r, size=B * L).astype(np.int64) for r in rows]
    ln = [np.full(B, L, np.int32)] * 2
    X = rng.rand(B, 8).astype(np.float32)
    plain = _engine(rows, D, L, B, 0, slots=1, staged=1)
    lines = _engine(rows, D, L, B, 1, slots=1, staged=1)
    try:
        assert lines.get_option(KEY) == 1
        assert lines.get_option("table_bytes") == plain.get_option("table_bytes") == table_bytes(rows, D, 0)
        for eng in (plain, lines):
            _load(eng, tables, D)
            eng.stage_batch(0, X, ix, ln)
        for exact in (1, 0):
            for eng in (plain, lines):
                eng.set_option("sls_exact", exact)
                eng.forward(0, B)
            assert np.array_equal(_bits(lines.fetch_interaction(B)), _bits(plain.fetch_interaction(B)))
            log = _log(lines)
            assert ",i4>" in log and "i4l" not in log, log
        lines.set_option(KEY, 0)
        assert lines.get_option(KEY) == 0
    finally:
        plain.close()
        lines.close()


# ---- 6. every table-writing path ---------------------------------------------------------------------------------------
def test_every_table_writing_path_places_rows_like_the_conversion():
    """drs_set_table of a table longer than one staging pass (chunks of (16 << 20) / D rows: 262 144 at D 64, no multiple
    of 3, so later chunks start inside a line), drs_fill_table_uniform, and a table replaced after the conversion: each
    against the plain int4 engine, bitwise."""
    D, B = 64, 256
    chunk = (16 << 20) // D                                              # engine_create.hip drs_set_table
    assert chunk == 262144 and chunk % 3 != 0
    rows = [chunk + 70001, 3001]
    assert rows[1] % 3 == 1                                              # (a last line with two unused slots)
    rng = np.random.RandomState(8)
    tables = [rng.uniform(-1, 1, (r, D)).astype(np.float32) for r in rows]
    picks = np.unique(np.concatenate([np.arange(0, 10), np.arange(chunk - 40, chunk + 40), np.arange(rows[0] - 40, rows[0])]))
    ix = [np.resize(picks, B).astype(np.int64), (np.arange(B) * 11 % rows[1]).astype(np.int64)]
    ix[1][:4] = [0, rows[1] - 1, rows[1] - 2, 3]
    ones = [np.ones(B, np.int32)] * 2
    X = np.zeros((B, 8), np.float32)
    Lb = 8
    bag_ix = [np.resize(picks, B * Lb).astype(np.int64), rng.randint(0, rows[1], size=B * Lb).astype(np.int64)]
    bags = [np.full(B, Lb, np.int32)] * 2

    def read(eng):
        out = []
        eng.set_option("sls_exact", 1)
        eng.stage_batch(0, X, ix, ones)
        eng.forward(0, B)
        out.append(_bits(_pooled(eng, D, B)))
        eng.stage_batch(0, X, bag_ix, bags)
        for exact in (1, 0):
            eng.set_option("sls_exact", exact)
            eng.forward(0, B)
            out.append(_bits(_pooled(eng, D, B)))
        return out

    def same(x, y):
        return all(np.array_equal(p, q) for p, q in zip(x, y))

    plain = _engine(rows, D, Lb, B, 0, slots=1, staged=1)
    lines = _engine(rows, D, Lb, B, 1, slots=1, staged=1)
    late = _engine(rows, D, Lb, B, 0, dtype=N.TABLE_FP32, slots=1, staged=1)
    try:
        for eng in (plain, lines, late):
            _load(eng, tables, D)                                         # lines: staged chunk by chunk, quantized in place
        late.set_option(KEY, 1)
        late.set_option("table_dtype", I4)                                # late: converted as a whole
        want = read(plain)
        assert same(read(lines), want) and same(read(late), want)
        assert "i4l" in _log(lines) and "i4l" in _log(late) and "i4l" not in _log(plain)
        exp = np.concatenate([dequant(tables[0][picks])[np.searchsorted(picks, ix[0])], dequant(tables[1])[ix[1]]], axis=1)
        assert np.array_equal(want[0], _bits(exp))
        # a table replaced after the conversion
        W1 = rng.uniform(-2, 2, (rows[1], D)).astype(np.float32)
        for eng in (plain, lines, late):
            eng.set_table(1, W1)
        want = read(plain)
        assert same(read(lines), want) and same(read(late), want)
        assert np.array_equal(want[0][:, D:], _bits(dequant(W1)[ix[1]]))
        # the device-side fill, the same seed on both
        for eng in (plain, lines):
            for t in range(2):
                eng.fill_table_uniform(t, -0.25, 0.5, 77)
        assert same(read(lines), read(plain))
        assert lines.get_option("table_bytes") == table_bytes(rows, D, 1)
    finally:
        plain.close()
        lines.close()
        late.close()


# ---- 7. dispatch log ---------------------------------------------------------------------------------------------------
def test_dispatch_log_names_the_line_packed_forms():
    D, T, B = 32, 2, 32
    rows = [3001, 2003]
    rng = np.random.RandomState(6)
    tables = [rng.uniform(-1, 1, (r, D)).astype(np.float32) for r in rows]
    X = rng.rand(B, 8).astype(np.float32)
    eng = _engine(rows, D, 80, B, 1, slots=1, staged=2)
    any_w = _engine(rows, 30, 20, B, 1, slots=1, staged=1)
    try:
        _load(eng, tables, D)
        eng.stage_batch(0, X, [rng.randint(0, r, size=B * 80).astype(np.int64) for r in rows], [np.full(B, 80, np.int32)] * T)
        eng.stage_batch(1, X, [rng.randint(0, r, size=B).astype(np.int64) for r in rows], [np.ones(B, np.int32)] * T)
        nt = ",nt" if eng.get_option("sls_nt") else ""
        eng.forward(0, B)
        assert "sls_flatc_kernel<8,10%s,i4l>" % nt in _log(eng), eng.last_dispatch()
        eng.set_option("sls_flat", 2)
        eng.forward(0, B)
        assert "sls_flat_kernel<8,10,bpw1%s,i4l>" % nt in _log(eng), eng.last_dispatch()
        eng.set_option("sls_flat", 0)
        eng.forward(0, B)
        assert "sls_kernel<8,split%s,i4l>" % nt in _log(eng), eng.last_dispatch()
        eng.set_option("sls_flat", 1)
        eng.set_option("sls_exact", 1)
        eng.forward(0, B)
        assert "sls_kernel<8,sequential,i4l>" in _log(eng), eng.last_dispatch()
        eng.forward(1, B)
        assert "sls_one_kernel<8," in _log(eng) and ",i4l>" in _log(eng), eng.last_dispatch()
        eng.set_option("sls_pool", 1)
        eng.forward(0, B)
        assert "sls_kernel<8,sequential,i4l,mean>" in _log(eng), eng.last_dispatch()
        eng.set_option("sls_pool", 0)
        eng.set_option(KEY, 0)
        for b, exact in ((0, 0), (0, 1), (1, 1)):
            eng.set_option("sls_exact", exact)
            eng.forward(b, B)
            assert "i4l" not in _log(eng) and ",i4>" in _log(eng), eng.last_dispatch()
        # the any-width form
        _load(any_w, [W[:, :30].copy() for W in tables], 30)
        any_w.stage_batch(0, X, [rng.randint(0, r, size=B * 20).astype(np.int64) for r in rows], [np.full(B, 20, np.int32)] * T)
        any_w.forward(0, B)
        assert "sls_any_kernel<i4l>" in _log(any_w), any_w.last_dispatch()
        any_w.set_option("sls_pool", 1)
        any_w.forward(0, B)
        assert "sls_any_kernel<i4l,mean>" in _log(any_w), any_w.last_dispatch()
    finally:
        eng.close()
        any_w.close()


# ---- 8. model level ----------------------------------------------------------------------------------------------------
def _model_pair(case, **extra):
    """the fixture model built with plain int4 tables and with --accel_table_int4_lines 1: equal interaction tensors and
    outputs, bit for bit"""
    meta, z = H.load_fixture(case)
    nets = []
    try:
        for lines in (0, 1):
            args = H.args_from(meta["args"], accel_table_dtype="int4_rowwise", accel_table_int4_lines=lines, **extra)
            net, lX, lS_l, lS_i, lT = H.materialize(args)
            net.create(lX[0], lS_l[0], lS_i[0], lT[0])
            nets.append(net)
            assert net.engine.get_option("table_dtype") == I4 and net.engine.get_option(KEY) == lines
            assert (KEY in net.engine.user_options) == bool(lines)
            net.stage_batches(None if args.model_type in H.NO_DENSE else lX, lS_l, lS_i)
            net.engine.set_option("dispatch_log", 1)
        n = len(lS_l[0][0])
        lined = rows_per_line(int(nets[0].args.arch_sparse_feature_size)) > 0
        for exact in (1, 0):
            for net in nets:
                net.engine.set_option("sls_exact", exact)
            for bid in range(len(lS_l)):
                for bs in sorted({n, 1, max(1, n // 2)}):
                    out = [net.run_staged(bid, bs).copy() for net in nets]
                    R = [net.engine.fetch_interaction(bs) for net in nets]
                    assert np.array_equal(_bits(R[1]), _bits(R[0])), (case, exact, bid, bs)
                    assert np.array_equal(_bits(out[1]), _bits(out[0])), (case, exact, bid, bs)
                    assert ("i4l" in _log(nets[1].engine)) == lined and "i4l" not in _log(nets[0].engine)
        return nets[1].engine.last_dispatch()
    finally:
        for net in nets:
            net.engine.close()


@pytest.mark.parametrize("case", [c for c in H.MODEL_CASES if not c.startswith(("din", "dien"))])
def test_models_with_line_packed_int4_tables(case):
    _model_pair(case)


def test_rm1_mini_with_line_packed_int4_tables_and_mean_pooling():
    log = " ".join(_model_pair("dlrm_rm1_mini", accel_sls_pool="mean"))
    assert "i4l,mean" in log, log


# ---- 9. DIN and DIEN ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["din_mini", "dien_mini"])
def test_din_and_dien_accept_the_option_and_still_refuse_int4(case):
    meta, z = H.load_fixture(case)
    args = H.args_from(meta["args"], accel_table_int4_lines=1)
    net, lX, lS_l, lS_i, lT = H.materialize(args)
    ref, _, _, _, _ = H.materialize(H.args_from(meta["args"]))
    net.create(lX[0], lS_l[0], lS_i[0], lT[0])
    ref.create(lX[0], lS_l[0], lS_i[0], lT[0])
    try:
        eng = net.engine
        assert eng.get_option(KEY) == 1 and ref.engine.get_option(KEY) == 0
        n = len(lS_l[0][0])
        for m in (net, ref):
            m.stage_batches(None, lS_l, lS_i)
            m.engine.set_option("sls_exact", 1)
        before = ref.run_staged(0, n).copy()
        assert np.array_equal(_bits(net.run_staged(0, n)), _bits(before))
        with pytest.raises(N.DrsError) as e:
            eng.set_option("table_dtype", I4)
        assert e.value.code == N.ERR_UNSUPPORTED and eng.get_option("table_dtype") == N.TABLE_FP32
        eng.set_option(KEY, 0)
        assert eng.get_option(KEY) == 0
        eng.set_option(KEY, 1)
        assert eng.get_option(KEY) == 1
        assert np.array_equal(_bits(net.run_staged(0, n)), _bits(before))
    finally:
        net.engine.close()
        ref.engine.close()


# ---- 10. pipelined sets ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [32, 64])
def test_pipelined_sets_match_plain_int4(D):
    """Sets of 16 mixed-size queries, three sets in flight, every gather on the engine's one gather stream
    (shared_stream 2): every query of every set is bit-identical to plain int4's."""
    rng = np.random.RandomState(D + 80)
    B, L = 128, 20                     # (a set of more than 1 024 rows: smaller ones keep to their slot's own stream)
    rows = ROWS
    tables = [rng.uniform(-1, 1, (r, D)).astype(np.float32) for r in rows]
    idx, lens, Lmax = _inputs(rng, rows, D, L, B)
    _assert_coverage(idx, lens, rows, D, B)
    dense = [rng.rand(B, 8).astype(np.float32) for _ in range(2)]
    plain = _engine(rows, D, Lmax, B, 0, slots=3)
    lines = _engine(rows, D, Lmax, B, 1, slots=3)
    try:
        for eng in (plain, lines):
            eng.set_option("shared_stream", 2)
            _load(eng, tables, D)
            for b in range(2):
                eng.stage_batch(b, dense[b], idx[b], lens[b])
        sets = [[((k + s) % 2, (B, 65, 1, 17)[(k + s) % 4]) for k in range(16)] for s in range(3)]
        for exact in (0, 1):
            got = {}
            for eng in (plain, lines):
                eng.set_option("sls_exact", exact)
                for rnd in range(2):
                    for s, jobs in enumerate(sets):
                        eng.forward_multi_async(s, [b for b, _ in jobs], [m for _, m in jobs])
                    for s, jobs in enumerate(sets):
                        eng.wait(s, sum(m for _, m in jobs))
                got[eng] = [eng.fetch_interaction(sum((m + 63) // 64 * 64 for _, m in jobs), slot=s) for s, jobs in enumerate(sets)]
                assert ("i4l" in _log(eng, 2)) == (eng is lines)
                assert "set[16 queries" in _log(eng, 2) and "gather on stream_g" in _log(eng, 2), eng.last_dispatch(2)
            for s, jobs in enumerate(sets):
                v = 0
                for b, m in jobs:
                    assert np.array_equal(_bits(got[lines][s][v:v + m]), _bits(got[plain][s][v:v + m])), (exact, s, b, m)
                    v += (m + 63) // 64 * 64
    finally:
        plain.close()
        lines.close()
