"""The line-packed int8 rowwise layout on the GPU (-m gpu): engine option "table_int8_lines" 1 on top of "table_dtype" 8.

The layout moves rows, never values: an engine with the option serves the bits of a plain int8 engine holding the same
tables, under every launch form, and with sls_exact 1 the bits of torch's embedding_bag_byte_rowwise_offsets over
embedding_bag_byte_prepack rows.
"""
import numpy as np
import pytest

from deeprecsys_amd import _native as N
from tests import helpers as H

pytestmark = pytest.mark.gpu
I8 = N.TABLE_INT8_ROWWISE

# option settings every case runs under: (sls_exact, sls_flat, sls_one) -- test_half_tables.py's
SETTINGS = [(1, 1, 1), (1, 1, 16), (1, 1, 64), (1, 1, 0), (0, 1, 1), (0, 0, 1), (0, 2, 1)]


# ---- the independent checker (test_int8_tables.py's idea, restated) ---------------------------------------------------
def prepack(W):
    import torch
    return torch.ops.quantized.embedding_bag_byte_prepack(torch.from_numpy(np.ascontiguousarray(W, np.float32)))


def pool(P, idx, lens):
    """embedding_bag_byte_rowwise_offsets (sum) over bags of the given lengths: [len(lens), D] float32."""
    import torch
    lens = np.asarray(lens, np.int64)
    offsets = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    out = torch.ops.quantized.embedding_bag_byte_rowwise_offsets(
        P, torch.from_numpy(np.asarray(idx, np.int64)[:int(lens.sum())].copy()), torch.from_numpy(offsets), mode=0,
        include_last_offset=False)
    return out.numpy().astype(np.float32)


def dequant(W):
    """Every row's value: its one-row bag, fmaf(scale, q, 0 + bias)."""
    rows = np.asarray(W).shape[0]
    return pool(prepack(W), np.arange(rows), np.ones(rows, np.int64))


# ---- the layout rule (docs/OPTIONS.md) ---------------------------------------------------------------------------------
def row_bytes(D):
    return (D + 7) // 8 * 8 + 8


def rows_per_line(D):
    S = row_bytes(D)
    return 128 // S if S < 128 and 128 % S else 0


def table_bytes(rows, D, lines):
    S, n = row_bytes(D), rows_per_line(D) if lines else 0
    total = 0
    for r in rows:
        total += (((r + n - 1) // n * 128 if n else r * S) + 255) // 256 * 256
    return total


def _engine(rows, D, L, B, lines, dtype=I8, slots=2, staged=2, lines_first=True):
    T = len(rows)
    eng = N.Engine(N.MODEL_DLRM, rows, D, [8, D], [D * (T + 1), 4, 1], N.INTERACT_CAT, sigmoid_top=2,
                   max_batch=B, max_lookups=L, num_staged_batches=staged, num_slots=slots)
    if lines and lines_first:
        eng.set_option("table_int8_lines", 1)
    if dtype != N.TABLE_FP32:
        eng.set_option("table_dtype", dtype)
    if lines and not lines_first:
        eng.set_option("table_int8_lines", 1)
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
    W[0] = 0.3125                                   # a constant row: scale 0, exact
    W[1] = np.abs(W[1]) + 0.25
    W[1, W.shape[1] // 2] = -0.0                    # a row whose minimum is -0
    return W


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _pooled(eng, D, bs, slot=0):
    return eng.fetch_interaction(bs, slot=slot)[:, D:].copy()


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
                ln[t][3] = Lmax
        else:
            ln = [np.full(B, L, np.int32) for _ in range(T)]
        ix = [rng.randint(0, rows[t], size=int(ln[t].sum())).astype(np.int64) for t in range(T)]
        for t in range(T):
            plant = np.array(_planted(rows[t], rows_per_line(D)), np.int64)
            k = min(plant.size, ix[t].size)
            ix[t][:k] = plant[:k]
            ix[t][-1] = rows[t] - 1
        idx.append(ix)
        lens.append(ln)
    return idx, lens, Lmax


def _assert_coverage(idx, lens, rows, D, bs):
    """the indices the first bs samples gather hold every residue r % n, the first and last row and both sides of a line
    boundary of every table"""
    n = max(rows_per_line(D), 1)
    for t, r in enumerate(rows):
        used = np.concatenate([ix[t][:int(ln[t][:bs].sum())] for ix, ln in zip(idx, lens)])
        assert set(used % n) == set(range(n)), (t, "residues")
        assert 0 in used and r - 1 in used, (t, "first and last row")
        if n > 1:
            assert n - 1 in used and n in used, (t, "both sides of a line boundary")
        assert used.max() < r


# ---- 1. bit identity with plain int8, under every launch form --------------------------------------------------------
@pytest.mark.parametrize("D", [12, 16, 28, 32, 40, 48, 64, 100, 30])
@pytest.mark.parametrize("L", [1, 20, 80, "ragged"])
def test_lines_serve_the_bits_of_plain_int8_under_every_form(D, L):
    """Two engines on the same fp32 tables, plain int8 and line-packed: equal interaction tensors as uint32 for single
    queries of B, 1 and 17 samples and for a coalesced set of mixed sizes with an empty query, under every setting of
    SETTINGS (sequential / split ring walk, one-lookup copy, flat, flat-coalesced; D 30: the any-width form)."""
    rng = np.random.RandomState(D * 11 + (0 if L == "ragged" else L))
    T, B = 3, 64
    rows = [2051, 2053, 2057]                                          # no multiple of 2, 3 or 5
    n = rows_per_line(D)
    assert n > 0 and all(r % n for r in rows if n > 1) and all(r % k for r in rows for k in (2, 3, 5)), (D, n)
    tables = [_special_rows(rng.uniform(-1, 1, (r, D)).astype(np.float32)) for r in rows]
    idx, lens, Lmax = _inputs(rng, rows, D, L, B)
    # (a one-sample query sees one bag per table: the planted rows need the whole batch, or several bags)
    _assert_coverage(idx, lens, rows, D, B)
    dense = [rng.rand(B, 8).astype(np.float32) for _ in range(2)]
    plain = _engine(rows, D, Lmax, B, 0)
    lines = _engine(rows, D, Lmax, B, 1)
    try:
        assert lines.get_option("table_int8_lines") == 1 and plain.get_option("table_int8_lines") == 0
        assert lines.get_option("table_dtype") == I8 and plain.get_option("table_dtype") == I8
        assert lines.get_option("table_bytes") == table_bytes(rows, D, 1)
        assert plain.get_option("table_bytes") == table_bytes(rows, D, 0)
        for eng in (plain, lines):
            _load(eng, tables, D)
            for b in range(2):
                eng.stage_batch(b, dense[b], idx[b], lens[b])
        jobs = [(k % 2, (B, 1, 17, 0, 33)[k % 5]) for k in range(12)]
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
                    log = " ".join(lines.last_dispatch())
                    assert ",i8l>" in log or "<i8l>" in log, log
                    assert "i8l" not in " ".join(plain.last_dispatch())
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
@pytest.mark.parametrize("D", [16, 32, 64])
def test_sequential_sums_are_fbgemms_bit_for_bit(D):
    """sls_exact 1, ragged bags: the pooled sums are embedding_bag_byte_rowwise_offsets over embedding_bag_byte_prepack
    rows, bit for bit."""
    rng = np.random.RandomState(D + 3)
    T, B = 3, 64
    rows = [2051, 2053, 2057]
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
            assert "sequential,i8l>" in " ".join(eng.last_dispatch())
    finally:
        eng.close()


# ---- 3. index range ----------------------------------------------------------------------------------------------------
def test_the_unused_slots_of_the_last_line_are_out_of_range():
    """rows = 3 k + 1 at D 32: the last line holds one row and two unused slots.  The indices rows, rows + 1 (the slots)
    and 3 (k + 1) - 1 ... are refused with DRS_ERR_INDEX_RANGE, staged or passed with the call, and the next valid query
    is served correctly."""
    D, L, B, k = 32, 4, 8, 700
    rows = [3 * k + 1]
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
        assert 3 * (k + 1) - 1 == rows[0] + 1
        for bad_ix in (rows[0], rows[0] + 1, 3 * (k + 1) - 1, 3 * (k + 1)):
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
    D, L, B, T = 32, 20, 32, 3
    rows = [3001, 2002, 1000]
    rng = np.random.RandomState(4)
    tables = [_special_rows(rng.uniform(-1, 1, (r, D)).astype(np.float32)) for r in rows]
    up16 = [W.astype(np.float16).astype(np.float32) for W in tables]
    ix = [rng.randint(0, rows[t], size=B * L).astype(np.int64) for t in range(T)]
    for t in range(T):
        ix[t][:8] = [0, 1, 2, 3, 4, 5, rows[t] - 1, rows[t] - 2]
    ln = [np.full(B, L, np.int32) for _ in range(T)]
    X = rng.rand(B, 8).astype(np.float32)

    def run(eng):
        eng.stage_batch(0, X, ix, ln)
        out = []
        for exact in (1, 0):
            eng.set_option("sls_exact", exact)
            eng.forward(0, B)
            out.append(_bits(_pooled(eng, D, B)))
        return np.stack(out)

    plain = _engine(rows, D, L, B, 0, slots=1, staged=1)
    a = _engine(rows, D, L, B, 1, slots=1, staged=1)                               # lines, then table_dtype 8
    b = _engine(rows, D, L, B, 1, slots=1, staged=1, lines_first=False)            # table_dtype 8, then lines
    c = _engine(rows, D, L, B, 0, dtype=N.TABLE_FP32, slots=1, staged=1)           # fp32 -> 8 with lines
    d = _engine(rows, D, L, B, 0, dtype=N.TABLE_FP16, slots=1, staged=1)           # fp16 -> 8 with lines
    p16 = _engine(rows, D, L, B, 0, slots=1, staged=1)
    try:
        for eng in (plain, a, b, c, d):
            _load(eng, tables, D)
        _load(p16, up16, D)
        want, want16 = run(plain), run(p16)
        gb = plain.gather_bytes(0, B)
        assert gb == B * T * (L * (D + 8) + L * 4 + 4 + D * 4)
        c.set_option("table_int8_lines", 1)
        assert c.get_option("table_bytes") == sum((r * D + 63) // 64 * 64 * 4 for r in rows)   # (fp32: only remembered)
        c.set_option("table_dtype", I8)
        d.set_option("table_dtype", I8)
        d.set_option("table_int8_lines", 1)
        for eng, w in ((a, want), (b, want), (c, want), (d, want16)):
            assert eng.get_option("table_int8_lines") == 1 and eng.get_option("table_dtype") == I8
            assert eng.get_option("table_bytes") == table_bytes(rows, D, 1) == sum(((r + 2) // 3 * 128 + 255) // 256 * 256 for r in rows)
            assert np.array_equal(run(eng), w)
            assert eng.gather_bytes(0, B) == gb
            assert "i8l" in " ".join(eng.last_dispatch())
        assert plain.get_option("table_bytes") == table_bytes(rows, D, 0) == sum((r * 40 + 255) // 256 * 256 for r in rows)
        # a value other than 0 and 1 is refused and changes nothing
        for bad in (2, -1):
            with pytest.raises(N.DrsError) as er:
                a.set_option("table_int8_lines", bad)
            assert er.value.code == N.ERR_BAD_ARG and a.get_option("table_int8_lines") == 1
        assert a.get_option("table_bytes") == table_bytes(rows, D, 1) and np.array_equal(run(a), want)
        # placement candidates copy the arena bytes
        a.set_option("table_placement", -1)
        assert a.get_option("table_placements") == 2 and np.array_equal(run(a), want)
        # lines 1 -> 0: plain int8's arena and bits
        a.set_option("table_int8_lines", 0)
        assert a.get_option("table_int8_lines") == 0 and a.get_option("table_bytes") == table_bytes(rows, D, 0)
        assert a.get_option("table_placements") == 1
        assert np.array_equal(run(a), want) and "i8l" not in " ".join(a.last_dispatch())
        # ... and back
        a.set_option("table_int8_lines", 1)
        assert a.get_option("table_bytes") == table_bytes(rows, D, 1) and np.array_equal(run(a), want)
        # 8 with lines -> 0: an fp32 arena whose one-row bags are the dequantized rows
        one = [(np.arange(B) * 7 % r).astype(np.int64) for r in rows]
        for t in range(T):
            one[t][:3] = [rows[t] - 1, 0, rows[t] - 2]
        b.set_option("table_dtype", N.TABLE_FP32)
        assert b.get_option("table_int8_lines") == 1 and b.get_option("table_bytes") == sum((r * D + 63) // 64 * 64 * 4 for r in rows)
        b.stage_batch(0, X, one, [np.ones(B, np.int32)] * T)
        b.set_option("sls_exact", 1)
        b.forward(0, B)
        exp = np.concatenate([dequant(tables[t])[one[t]] for t in range(T)], axis=1)
        assert np.array_equal(_bits(_pooled(b, D, B)), _bits(exp))
        assert "i8" not in " ".join(b.last_dispatch())
    finally:
        for eng in (plain, a, b, c, d, p16):
            eng.close()


@pytest.mark.parametrize("D", [24, 56, 128])
def test_exact_fit_and_wide_rows_keep_the_plain_layout(D):
    """S = 32, 64 (a power of two: rows never cross a line) and S = 136 (> 128): the option is accepted, the arena is the
    plain one and the log says i8."""
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
        assert lines.get_option("table_int8_lines") == 1
        assert lines.get_option("table_bytes") == plain.get_option("table_bytes") == table_bytes(rows, D, 0)
        for eng in (plain, lines):
            _load(eng, tables, D)
            eng.stage_batch(0, X, ix, ln)
        for exact in (1, 0):
            for eng in (plain, lines):
                eng.set_option("sls_exact", exact)
                eng.forward(0, B)
            assert np.array_equal(_bits(lines.fetch_interaction(B)), _bits(plain.fetch_interaction(B)))
            log = " ".join(lines.last_dispatch())
            assert ",i8>" in log and "i8l" not in log, log
        lines.set_option("table_int8_lines", 0)
        assert lines.get_option("table_int8_lines") == 0
    finally:
        plain.close()
        lines.close()


# ---- 5. every table-writing path ---------------------------------------------------------------------------------------
def test_every_table_writing_path_places_rows_like_the_conversion():
    """drs_set_table of a table longer than one staging pass (chunks of (16 << 20) / D rows: 524 288 at D 32, no multiple
    of 3, so later chunks start inside a line), drs_fill_table_uniform, and a table replaced after the conversion: each
    against the plain int8 engine, bitwise."""
    D, B = 32, 256
    chunk = (16 << 20) // D                                              # engine_create.hip drs_set_table
    assert chunk % 3 != 0
    rows = [chunk + 70001, 3001]
    assert all(r % 3 for r in rows)
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
        late.set_option("table_int8_lines", 1)
        late.set_option("table_dtype", I8)                                # late: converted as a whole
        want = read(plain)
        assert same(read(lines), want) and same(read(late), want)
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


# ---- 6. dispatch log ---------------------------------------------------------------------------------------------------
def test_dispatch_log_names_the_line_packed_forms():
    D, T, B = 32, 2, 32
    rows = [3001, 2002]
    rng = np.random.RandomState(6)
    tables = [rng.uniform(-1, 1, (r, D)).astype(np.float32) for r in rows]
    X = rng.rand(B, 8).astype(np.float32)
    eng = _engine(rows, D, 80, B, 1, slots=1, staged=2)
    try:
        _load(eng, tables, D)
        eng.stage_batch(0, X, [rng.randint(0, r, size=B * 80).astype(np.int64) for r in rows], [np.full(B, 80, np.int32)] * T)
        eng.stage_batch(1, X, [rng.randint(0, r, size=B).astype(np.int64) for r in rows], [np.ones(B, np.int32)] * T)
        nt = ",nt" if eng.get_option("sls_nt") else ""
        eng.forward(0, B)
        assert "sls_flatc_kernel<8,10%s,i8l>" % nt in " ".join(eng.last_dispatch()), eng.last_dispatch()
        eng.set_option("sls_exact", 1)
        eng.forward(0, B)
        assert "sls_kernel<8,sequential,i8l>" in " ".join(eng.last_dispatch()), eng.last_dispatch()
        eng.forward(1, B)
        log = " ".join(eng.last_dispatch())
        assert "sls_one_kernel<8," in log and ",i8l>" in log, log
        eng.set_option("table_int8_lines", 0)
        for b, exact in ((0, 0), (0, 1), (1, 1)):
            eng.set_option("sls_exact", exact)
            eng.forward(b, B)
            log = " ".join(eng.last_dispatch())
            assert "i8l" not in log and ",i8>" in log, log
    finally:
        eng.close()


# ---- 7. model level ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in H.MODEL_CASES if not c.startswith(("din", "dien"))])
def test_models_with_line_packed_int8_tables(case):
    """Every fixture model but DIN / DIEN built with --accel_table_int8_lines 1 --accel_table_dtype int8_rowwise: the
    interaction tensor and the outputs are bit-identical to the same model built with plain int8."""
    meta, z = H.load_fixture(case)
    nets = []
    try:
        for lines in (0, 1):
            args = H.args_from(meta["args"], accel_table_dtype="int8_rowwise", accel_table_int8_lines=lines)
            net, lX, lS_l, lS_i, lT = H.materialize(args)
            net.create(lX[0], lS_l[0], lS_i[0], lT[0])
            nets.append(net)
            assert net.engine.get_option("table_dtype") == I8 and net.engine.get_option("table_int8_lines") == lines
            assert ("table_int8_lines" in net.engine.user_options) == bool(lines)
            net.stage_batches(None if args.model_type in H.NO_DENSE else lX, lS_l, lS_i)
        n = len(lS_l[0][0])
        for exact in (1, 0):
            for net in nets:
                net.engine.set_option("sls_exact", exact)
            for bid in range(len(lS_l)):
                for bs in sorted({n, 1, max(1, n // 2)}):
                    out = [net.run_staged(bid, bs).copy() for net in nets]
                    R = [net.engine.fetch_interaction(bs) for net in nets]
                    assert np.array_equal(_bits(R[1]), _bits(R[0])), (case, exact, bid, bs)
                    assert np.array_equal(_bits(out[1]), _bits(out[0])), (case, exact, bid, bs)
    finally:
        for net in nets:
            net.engine.close()


@pytest.mark.parametrize("case", ["din_mini", "dien_mini"])
def test_din_and_dien_accept_the_option_and_still_refuse_int8(case):
    meta, z = H.load_fixture(case)
    args = H.args_from(meta["args"], accel_table_int8_lines=1)
    net, lX, lS_l, lS_i, lT = H.materialize(args)
    ref, _, _, _, _ = H.materialize(H.args_from(meta["args"]))
    net.create(lX[0], lS_l[0], lS_i[0], lT[0])
    ref.create(lX[0], lS_l[0], lS_i[0], lT[0])
    try:
        eng = net.engine
        assert eng.get_option("table_int8_lines") == 1 and ref.engine.get_option("table_int8_lines") == 0
        n = len(lS_l[0][0])
        for m in (net, ref):
            m.stage_batches(None, lS_l, lS_i)
            m.engine.set_option("sls_exact", 1)
        before = ref.run_staged(0, n).copy()
        assert np.array_equal(_bits(net.run_staged(0, n)), _bits(before))
        with pytest.raises(N.DrsError) as e:
            eng.set_option("table_dtype", I8)
        assert e.value.code == N.ERR_UNSUPPORTED and eng.get_option("table_dtype") == N.TABLE_FP32
        eng.set_option("table_int8_lines", 0)
        assert eng.get_option("table_int8_lines") == 0
        eng.set_option("table_int8_lines", 1)
        assert eng.get_option("table_int8_lines") == 1
        assert np.array_equal(_bits(net.run_staged(0, n)), _bits(before))
    finally:
        net.engine.close()
        ref.engine.close()


# ---- 8. pipelined sets -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [32, 64])
def test_pipelined_sets_match_plain_int8(D):
    """Sets of 12 mixed-size queries, three sets in flight (test_int8_tables.py's jobs12 shape): every query of every set
    is bit-identical to plain int8's."""
    rng = np.random.RandomState(D + 80)
    T, B, L = 3, 48, 20
    rows = [2051, 2053, 2057]
    tables = [rng.uniform(-1, 1, (r, D)).astype(np.float32) for r in rows]
    idx, lens, Lmax = _inputs(rng, rows, D, L, B)
    dense = [rng.rand(B, 8).astype(np.float32) for _ in range(2)]
    plain = _engine(rows, D, Lmax, B, 0, slots=3)
    lines = _engine(rows, D, Lmax, B, 1, slots=3)
    try:
        for eng in (plain, lines):
            _load(eng, tables, D)
            for b in range(2):
                eng.stage_batch(b, dense[b], idx[b], lens[b])
        sets = [[((k + s) % 2, (B, 1, 17, 0)[(k + s) % 4]) for k in range(12)] for s in range(3)]
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
                assert ("i8l" in " ".join(eng.last_dispatch(2))) == (eng is lines)
            for s, jobs in enumerate(sets):
                v = 0
                for b, m in jobs:
                    assert np.array_equal(_bits(got[lines][s][v:v + m]), _bits(got[plain][s][v:v + m])), (exact, s, b, m)
                    v += (m + 63) // 64 * 64
    finally:
        plain.close()
        lines.close()
