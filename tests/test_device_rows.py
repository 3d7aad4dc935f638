"""Table rows updated and read back from device arrays on the GPU (-m gpu): drs_update_rows_device / drs_get_rows_device.

tests/test_row_updates.py's twin method with the HOST update as the reference: engines A and B load the same tables and take
the same options; A takes the device update (torch tensors on the GPU), B takes Engine.update_rows with the same ids and the
same values widened to fp32.  get_rows over EVERY row of EVERY table must be bit-identical between the two, and so must one
forward.  No tolerance is involved anywhere.
"""
import ctypes as C

import numpy as np
import pytest

from deeprecsys_amd import _native as N
from tests import helpers as H
from tests import large_table_shapes as S
from tests import row_update_ref as R
from tests.test_row_updates import B, CASES, LINES_KEY, MID, ROWS, T, _bits, all_rows, engine, expect_equal_engines, forward, options, same, stage, tables

pytestmark = pytest.mark.gpu

SENTINEL = -77.0


def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch


def dev(a):
    torch = torch_cuda()
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def code_of(t):
    torch = torch_cuda()
    return {torch.float32: N.TABLE_FP32, torch.float16: N.TABLE_FP16, torch.bfloat16: N.TABLE_BF16}[t.dtype]


def dev_update(eng, t, ids_t, V_t, stream=None):
    """the device update of rows ids_t (int64 tensor) with V_t ([n, D] tensor of any of the three types, rows at their stride)"""
    if stream is None:
        torch_cuda().cuda.synchronize()                 # `ordered` 0: the arrays are complete when the call is made
    n = int(ids_t.numel())
    eng.update_rows_device(t, ids_t.data_ptr(), n, V_t.data_ptr(), V_t.stride(0) if n > 1 else V_t.shape[1], code_of(V_t), stream=stream)


def dev_get(eng, t, ids_t, out=None, stream=None):
    torch = torch_cuda()
    n = int(ids_t.numel())
    if out is None:
        out = torch.full((n, eng.D), SENTINEL, dtype=torch.float32, device="cuda:0")
    if stream is None:
        torch.cuda.synchronize()
    eng.get_rows_device(t, ids_t.data_ptr(), n, out.data_ptr(), out.stride(0) if n > 1 else eng.D, stream=stream)
    return out


def host(t):
    return t.detach().float().cpu().contiguous().numpy()


def pair(D, Ws, dtype, lines, rows=ROWS, slots=2, staged=True):
    a, b = engine(D, Ws, rows=rows, slots=slots), engine(D, Ws, rows=rows, slots=slots)
    for e in (a, b):
        options(e, dtype, lines)
        if staged:
            stage(e, D)
    return a, b


def same_tables(a, b, rows, what):
    ra, rb = all_rows(a, rows), all_rows(b, rows)
    for t in range(len(rows)):
        assert same(ra[t], rb[t]), (what, "table %d" % t, np.argwhere(_bits(ra[t]) != _bits(rb[t]))[:4].tolist())
    return ra


# ---- every type, width and layout -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,D,lines", CASES)
def test_the_device_update_gives_the_host_updates_engine(dtype, D, lines):
    """R.IDS: row 0, row 300 (the partly filled last line), two neighbours in one 128-byte line, unsorted, one id three
    times.  A == B over every row and one forward; tables 0 and 2 keep their bits; the read-back equals get_rows."""
    Ws = tables(D)
    V = R.update_values(R.IDS.size, D, seed=100 + D)
    a, b = pair(D, Ws, dtype, lines)
    try:
        before = all_rows(a)
        dev_update(a, MID, dev(R.IDS), dev(V))
        b.update_rows(MID, R.IDS, V)
        got = expect_equal_engines(a, b, D, (dtype, D, lines))
        assert same(got[0], before[0]) and same(got[2], before[2]) and not same(got[MID], before[MID])
        assert same(got[MID], R.served_after_update(Ws[MID], R.IDS, V, dtype))
        every = np.arange(R.ROWS, dtype=np.int64)
        assert same(host(dev_get(a, MID, dev(every))), got[MID])
        if dtype == R.FP8:
            assert a.table_fp8_exponent(MID) == b.table_fp8_exponent(MID) == R.table_exponent(Ws[MID])
    finally:
        a.close()
        b.close()


# ---- the forms the values come in -------------------------------------------------------------------------------------------
FORMS = ["fp16", "bf16", "block_fp32", "block_fp16", "block_bf16", "one_row_nonsense_stride", "no_row"]


@pytest.mark.parametrize("dtype", R.DTYPES)
@pytest.mark.parametrize("form", FORMS)
def test_value_types_strides_one_row_and_no_row(dtype, form):
    """fp16 / bf16 values are the fp32 update of their widened values; a column block of a wider tensor goes down as it is (the
    pointer aligned to its element, no more); the stride of a single row is not read; n == 0 does nothing.  D 30, line-packed
    where the type has lines."""
    torch = torch_cuda()
    D, lines = 30, int(dtype in LINES_KEY)
    Ws = tables(D)
    a, b = pair(D, Ws, dtype, lines)
    try:
        before = all_rows(a)
        half = {"fp16": torch.float16, "bf16": torch.bfloat16, "fp32": torch.float32}
        if form == "no_row":
            assert N.lib().drs_update_rows_device(a._h, MID, 0, None, None, 0, N.TABLE_FP32, None, 0) == N.OK
            assert dev_get(a, MID, dev(np.zeros(0, np.int64))).shape == (0, D)
        elif form == "one_row_nonsense_stride":
            ids = np.array([R.ROWS - 1], np.int64)
            ids_t, V_t = dev(ids), dev(R.update_values(1, D, seed=9))
            out = torch.full((1, D), SENTINEL, dtype=torch.float32, device="cuda:0")
            torch.cuda.synchronize()
            for stride in (-12345, 1 << 61):
                a.update_rows_device(MID, ids_t.data_ptr(), 1, V_t.data_ptr(), stride, N.TABLE_FP32)
            b.update_rows(MID, ids, host(V_t))
            a.get_rows_device(MID, ids_t.data_ptr(), 1, out.data_ptr(), -5)
            assert same(host(out), b.get_rows(MID, ids))
        else:
            V = dev(R.update_values(R.IDS.size, D, seed=21))
            if form.startswith("block_"):
                wide = torch.full((R.IDS.size, 3 + D + 6), SENTINEL, dtype=half[form[6:]], device="cuda:0")
                V_t = wide[:, 3:3 + D]
                V_t.copy_(V)
                assert V_t.stride(0) == D + 9 and V_t.data_ptr() % 8 != 0
            else:
                V_t = V.to(half[form])
            dev_update(a, MID, dev(R.IDS), V_t)
            b.update_rows(MID, R.IDS, host(V_t))                          # the same values, widened
            if form.startswith("block_"):
                assert (host(wide[:, :3]) == SENTINEL).all() and (host(wide[:, 3 + D:]) == SENTINEL).all()
        got = expect_equal_engines(a, b, D, (dtype, form))
        assert same(got[0], before[0]) and same(got[2], before[2])
        assert same(got[MID], before[MID]) == (form == "no_row")
    finally:
        a.close()
        b.close()


# ---- the edges of the passes ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [R.FP32, R.I8])
def test_pass_edges_on_a_small_d_table(dtype):
    """D 4, one table of 70 000 rows: n on both sides of a wave (64, 65) and of a workgroup of the per-id passes (256, 257);
    65 537 rows, past the place kernel's grid cap of 16 384 workgroups of 4 rows; every position naming one id; a random
    list with about 30 % repeats.  One pair of engines takes them all in turn."""
    D, rows = 4, [70000]
    rng = np.random.RandomState(17)
    Ws = [R.table(rows[0], D, seed=5)]
    lists = [("n=%d" % n, rng.permutation(rows[0])[:n].astype(np.int64)) for n in (64, 65, 256, 257, 65537)]
    lists.append(("one id 257 times", np.full(257, 4242, np.int64)))
    rep = rng.randint(0, 1500, size=1000).astype(np.int64)
    assert 0.2 < 1.0 - np.unique(rep).size / rep.size < 0.4
    lists.append(("30 % repeats", rep))
    a, b = pair(D, Ws, dtype, 0, rows=rows, slots=1, staged=False)
    try:
        for k, (name, ids) in enumerate(lists):
            V = R.update_values(ids.size, D, seed=40 + k)
            dev_update(a, 0, dev(ids), dev(V))
            b.update_rows(0, ids, V)
            got = same_tables(a, b, rows, name)
            assert same(host(dev_get(a, 0, dev(ids))), got[0][ids]), name
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("dtype", [R.FP32, R.I8])
def test_updates_larger_than_one_chunk(dtype):
    """D 260: a chunk holds 64 527 rows (16 M elements), the update names one more.  One id loses in chunk 0 and wins in
    chunk 1, one pair lies inside chunk 0.  The read-back of the same ids spans two chunks too."""
    rows, D = 66000, 260
    n = (16 << 20) // D + 1
    rng = np.random.RandomState(12)
    W = rng.uniform(-1, 1, (rows, D)).astype(np.float32)
    ids = rng.permutation(rows)[:n].astype(np.int64)
    ids[n - 1] = ids[5]                                                      # loser in chunk 0, winner in chunk 1
    ids[100] = ids[50]
    V = rng.uniform(-1, 1, (n, D)).astype(np.float32)
    assert n * D > 16 << 20 and (n - 1) * D <= 16 << 20 and np.unique(ids).size == n - 2
    a, b = pair(D, [W], dtype, 0, rows=[rows], slots=1, staged=False)
    try:
        ids_t = dev(ids)
        dev_update(a, 0, ids_t, dev(V))
        b.update_rows(0, ids, V)
        got = same_tables(a, b, [rows], dtype)
        assert same(host(dev_get(a, 0, ids_t)), got[0][ids])
    finally:
        a.close()
        b.close()


def test_rows_beyond_piece_2_pow_31_and_byte_2_pow_32():
    """tests/large_table_shapes.py's [214 752 461, 1000] int8 tables at D 32, line-packed, filled on the device: rows among the
    last 4096 of table 0 lie at pieces in [2^31, 2^32) and beyond byte 2^32.  Rows on both sides of the boundary are updated
    and read back through the new kernel: the updated rows serve the reference's values, their neighbours the fill's.  Skips,
    with both numbers, only when the device cannot hold the arena and its conversion."""
    from tests.test_large_tables import gate
    dtype, lines = R.I8, 1
    D, rows = S.D_MAIN, list(S.ROWS_A)
    lo, hi, seed = S.FILL
    gate("device row updates", S.free_needed(((S.FP32, False), (dtype, bool(lines))), rows, D))
    last = rows[0] - 1
    edge = S.R_STAR_LINES
    assert S.row_piece(dtype, D, last - 4095, True) >= 1 << 31 and S.row_piece(dtype, D, edge - 1, True) < 1 << 31 <= S.row_piece(dtype, D, edge, True)
    eng = N.Engine(N.MODEL_DLRM, rows, D, [8, D], [D * 3, 4, 1], N.INTERACT_CAT, sigmoid_top=2, max_batch=B, max_lookups=4,
                   num_staged_batches=1, num_slots=1)
    try:
        options(eng, dtype, lines)
        for t in range(2):
            eng.fill_table_uniform(t, lo, hi, seed)
        rng = np.random.RandomState(31)
        ids = np.array([last, last - 4095, last - 7, last - 6, edge - 1, edge, edge + 1, 3, last - 7], np.int64)     # one id twice
        V = rng.uniform(lo, hi, (ids.size, D)).astype(np.float32)
        look = np.unique(np.concatenate([ids + d for d in (-6, -2, -1, 0, 1, 2, 6)]))
        look = look[(look >= 0) & (look < rows[0])]
        fill = S.fill_rows(look, D, 0, lo, hi, seed)
        dev_update(eng, 0, dev(ids), dev(V))
        exp = R.served_after_update(fill, S.positions(look, ids), V, dtype)
        got = host(dev_get(eng, 0, dev(look)))
        assert same(got, exp), look[np.argwhere((_bits(got) != _bits(exp)).any(axis=1))[:, 0]].tolist()
        assert same(got, eng.get_rows(0, look))
    finally:
        eng.close()


# ---- the read-back -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", R.DTYPES)
def test_the_read_back_equals_get_rows_and_leaves_the_gaps(dtype):
    torch = torch_cuda()
    D, lines = 30, int(dtype in LINES_KEY)
    a = engine(D, tables(D))
    try:
        options(a, dtype, lines)
        ids = np.array([300, 0, 150, 150, 7, 300, 6, 299], np.int64)      # any order, repeats
        want = a.get_rows(MID, ids)
        assert same(host(dev_get(a, MID, dev(ids))), want)
        wide = torch.full((ids.size, 3 + D + 6), SENTINEL, dtype=torch.float32, device="cuda:0")
        out = wide[:, 3:3 + D]
        assert dev_get(a, MID, dev(ids), out=out) is out
        w = host(wide)
        assert same(w[:, 3:3 + D], want) and (w[:, :3] == SENTINEL).all() and (w[:, 3 + D:] == SENTINEL).all()
        for t in (0, 2):
            every = np.arange(ROWS[t], dtype=np.int64)
            assert same(host(dev_get(a, t, dev(every))), a.get_rows(t, every))
    finally:
        a.close()


# ---- errors found on the device ------------------------------------------------------------------------------------------------
def expect_error(fn, code, *words):
    with pytest.raises(N.DrsError) as err:
        fn()
    assert err.value.code == code, err.value
    for w in words:
        assert w in err.value.detail, (w, err.value.detail)


@pytest.mark.parametrize("dtype", [R.FP32, R.I4, R.FP8])
def test_errors_found_on_the_device_change_nothing(dtype):
    """the right code, the lowest offending position in the message, every row of every table as it was; a failed read-back
    leaves d_V's sentinel"""
    D = 32
    Ws = tables(D)
    a = engine(D, Ws)
    try:
        options(a, dtype, int(dtype in LINES_KEY))
        before = all_rows(a)

        def unchanged(what):
            now = all_rows(a)
            assert all(same(now[t], before[t]) for t in range(T)), what

        bad_lists = [([R.ROWS, 5, 6, R.ROWS], 0, R.ROWS),                   # the first position (and a later one: the lowest reports)
                     ([5, 6, 7, R.ROWS], 3, R.ROWS),                        # the last position
                     ([5, -1, 6, -1], 1, -1),
                     ([5, 6, 7, (1 << 32) + 5, R.ROWS], 3, (1 << 32) + 5)]  # (narrowed to 32 bits it would be row 5)
        for ids, pos, val in bad_lists:
            ids = np.array(ids, np.int64)
            V = R.update_values(ids.size, D, seed=1)
            msg = "ids[%d] = %d" % (pos, val)
            expect_error(lambda: dev_update(a, MID, dev(ids), dev(V)), N.ERR_INDEX_RANGE, "drs_update_rows_device", msg)
            unchanged(("update", ids.tolist()))
            out = dev(np.full((ids.size, D), SENTINEL, np.float32))
            expect_error(lambda: dev_get(a, MID, dev(ids), out=out), N.ERR_INDEX_RANGE, "drs_get_rows_device", msg)
            assert (host(out) == SENTINEL).all(), ids.tolist()
        if dtype == R.FP8:
            torch = torch_cuda()
            k = a.table_fp8_exponent(MID)
            edge = np.float32(448 * 2.0 ** -k)
            over = R.update_values(4, D, seed=2)
            over[1, 7] = np.nextafter(edge, np.float32(np.inf))
            over[3, 0] = -4 * edge
            ids = np.array([5, 6, 7, 8], np.int64)
            expect_error(lambda: dev_update(a, MID, dev(ids), dev(over)), N.ERR_BAD_ARG, "row 1", "drs_set_table")
            unchanged("fp8 fit")
            over[1, 7] = 2 * edge                                              # (bf16 holds it; the next float above the edge it would round onto the edge)
            expect_error(lambda: dev_update(a, MID, dev(ids), dev(over).to(torch.bfloat16)), N.ERR_BAD_ARG, "row 1", "drs_set_table")
            unchanged("fp8 fit, bf16 values")
            # an id out of range beside a value that does not fit: the ids are judged first, as on the host
            expect_error(lambda: dev_update(a, MID, dev(np.array([5, 6, 7, R.ROWS], np.int64)), dev(over)), N.ERR_INDEX_RANGE, "ids[3]")
            unchanged("both")
            # the edge itself fits; non-finite elements are stored as drs_set_table stores them: the host update's bits
            ok = R.update_values(4, D, seed=2)
            ok[1, 7], ok[2, 0], ok[2, 1] = -edge, np.inf, np.nan
            b = engine(D, Ws)
            try:
                options(b, dtype, 0)
                dev_update(a, MID, dev(ids), dev(ok))
                b.update_rows(MID, ids, ok)
                ga, gb = a.get_rows(MID, ids), b.get_rows(MID, ids)
                assert np.array_equal(np.isnan(ga), np.isnan(gb)) and same(np.nan_to_num(ga), np.nan_to_num(gb)) and ga[1, 7] == -edge
                assert a.table_fp8_exponent(MID) == k
            finally:
                b.close()
    finally:
        a.close()


@pytest.mark.parametrize("dtype", [R.FP32, R.I8])
def test_a_bad_id_in_the_second_chunk_changes_nothing(dtype):
    """D 260, one row more than a chunk, the last id out of range: the first chunk's rows are not placed either"""
    D = 260
    n = (16 << 20) // D + 1
    Ws = tables(D)
    a = engine(D, Ws)
    try:
        options(a, dtype, int(dtype in LINES_KEY))
        before = all_rows(a)
        rng = np.random.RandomState(3)
        ids = rng.randint(0, R.ROWS, size=n).astype(np.int64)
        ids[n - 1] = R.ROWS
        V_t = dev(R.update_values(1, D, seed=8)).expand(n, D).contiguous()
        expect_error(lambda: dev_update(a, MID, dev(ids), V_t), N.ERR_INDEX_RANGE, "ids[%d] = %d" % (n - 1, R.ROWS))
        now = all_rows(a)
        assert all(same(now[t], before[t]) for t in range(T))
    finally:
        a.close()


# ---- what the host refuses before anything is enqueued -------------------------------------------------------------------------
def test_host_visible_refusals_change_nothing():
    torch = torch_cuda()
    D = 32
    Ws = tables(D)
    Ws[2] = None                                                          # table 2 is never set or filled
    a = engine(D, Ws)
    try:
        options(a, R.I8, 1)
        every = np.arange(R.ROWS, dtype=np.int64)
        before = a.get_rows(MID, every)
        n = 4
        ids_h, V_h = np.array([5, 6, 7, 8], np.int64), R.update_values(n, D, seed=1)
        ids_t, V_t = dev(ids_h), dev(V_h)
        out_t = dev(np.full((n, D), SENTINEL, np.float32))
        V16 = V_t.to(torch.float16)
        torch.cuda.synchronize()
        L = N.lib()
        vp = lambda p: C.c_void_p(p) if p else None

        def refused(what, t=MID, n=n, ids=ids_t.data_ptr(), V=V_t.data_ptr(), stride=D, dt=N.TABLE_FP32, stream=0, ordered=0, out=None):
            rc = L.drs_update_rows_device(a._h, t, n, vp(ids), vp(V), stride, dt, vp(stream), ordered)
            assert rc == N.ERR_BAD_ARG, ("update", what, rc)
            if dt == N.TABLE_FP32:                                           # (the read-back has no val_dtype)
                rc = L.drs_get_rows_device(a._h, t, n, vp(ids), vp(out_t.data_ptr() if out is None else out), stride, vp(stream), ordered)
                assert rc == N.ERR_BAD_ARG, ("get", what, rc)
            assert same(a.get_rows(MID, every), before), what
            assert (host(out_t) == SENTINEL).all(), what

        refused("host ids", ids=ids_h.ctypes.data)
        refused("host values", V=V_h.ctypes.data, out=V_h.ctypes.data)
        refused("ids past their allocation", n=1 << 24)                                 # (ids_t holds n: 128 MB of ids end far behind it)
        refused("values past their allocation", stride=1 << 40)                         # (an extent below 2^60 bytes that ends far behind V_t)
        refused("misaligned values", V=V_t.data_ptr() + 2, out=out_t.data_ptr() + 2)
        refused("misaligned ids", ids=ids_t.data_ptr() + 4)
        refused("stride < D", stride=D - 1)
        refused("negative stride", stride=-D)
        refused("a stride beyond any allocation", stride=1 << 59)
        refused("val_dtype 3", dt=3)
        refused("val_dtype fp8", dt=N.TABLE_FP8_E4M3)
        refused("ordered 2", ordered=2)
        refused("ordered -1", ordered=-1)
        refused("table -1", t=-1)
        refused("table T", t=T)
        refused("a table never set", t=2)
        refused("null ids", ids=0)
        refused("null values", V=0, out=0)
        refused("n < 0", n=-1)
        refused("n beyond the cap", n=N.DEVICE_ROWS_MAX + 1)
        # misaligned fp16 values: aligned to 2 bytes is enough, 1 byte off is not
        assert L.drs_update_rows_device(a._h, MID, n, vp(ids_t.data_ptr()), vp(V16.data_ptr() + 1), D, N.TABLE_FP16, None, 0) == N.ERR_BAD_ARG
        assert same(a.get_rows(MID, every), before)
        # what all of that was refused about is fine
        assert L.drs_update_rows_device(a._h, MID, n, vp(ids_t.data_ptr()), vp(V_t.data_ptr()), D, N.TABLE_FP32, None, 0) == N.OK
        assert not same(a.get_rows(MID, every), before)
    finally:
        a.close()


# ---- ordering ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [R.FP32, R.I8])
def test_an_ordered_update_runs_behind_the_callers_stream(dtype):
    """On a side stream: a delay, then the copies that write the final ids and rows over placeholders, then the update with
    `ordered` 1 and no synchronisation.  The table must hold the final rows (the placeholders name row 0 alone).  The ordered
    read-back likewise."""
    from tests.test_device_outputs import sleep_cycles
    torch = torch_cuda()
    D, lines = 32, int(dtype in LINES_KEY)
    Ws = tables(D)
    V = R.update_values(R.IDS.size, D, seed=33)
    a, b = pair(D, Ws, dtype, lines)
    try:
        final_ids, final_V = dev(R.IDS), dev(V)
        ids_t, V_t = torch.zeros_like(final_ids), torch.full_like(final_V, 0.5)
        cycles = sleep_cycles(torch, 150.0)
        side = torch.cuda.Stream()
        assert side.cuda_stream != 0
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            torch.cuda._sleep(cycles)
            ids_t.copy_(final_ids, non_blocking=True)
            V_t.copy_(final_V, non_blocking=True)
            dev_update(a, MID, ids_t, V_t, stream=side.cuda_stream)
        b.update_rows(MID, R.IDS, V)
        got = expect_equal_engines(a, b, D, dtype)
        ids2 = torch.zeros_like(final_ids)
        out = torch.full((R.IDS.size, D), SENTINEL, dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            torch.cuda._sleep(cycles)
            ids2.copy_(final_ids, non_blocking=True)
            dev_get(a, MID, ids2, out=out, stream=side.cuda_stream)
        assert same(host(out), got[MID][R.IDS])                                # (complete when the call has returned)
        # the null stream is a stream like any other
        dev_update(a, MID, final_ids, final_V, stream=0)
        same_tables(a, b, ROWS, "null stream")
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("dtype", [R.FP32, R.I8])
def test_a_set_in_flight_is_served_from_the_old_rows(dtype):
    D = 64
    Ws = tables(D)
    V = R.update_values(R.IDS.size, D, seed=4)
    a, b = pair(D, Ws, dtype, int(dtype in LINES_KEY))
    try:
        old = a.forward(0, B).copy()
        ids_t, V_t = dev(R.IDS), dev(V)
        torch_cuda().cuda.synchronize()
        a.forward_async(1, 0, B)
        a.update_rows_device(MID, ids_t.data_ptr(), R.IDS.size, V_t.data_ptr(), D, N.TABLE_FP32)
        assert same(a.wait(1, B), old)
        b.update_rows(MID, R.IDS, V)
        new = a.forward(0, B)
        assert same(new, b.forward(0, B)) and not same(new, old)
    finally:
        a.close()
        b.close()


# ---- the six model kinds, through the model wrapper --------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["dlrm_rm1_mini", "wnd_mini", "ncf_mini", "mtwnd_mini", "din_mini", "dien_mini"])
def test_every_model_kind_serves_device_updated_rows(case):
    """one row that a bag names, updated through net.update_embedding_rows with torch tensors on the GPU (a) and with
    numpy arrays (b): output and interaction buffer equal bit for bit and the interaction buffer differs from the one before;
    net.embedding_rows returns a device tensor with the host route's bits"""
    torch = torch_cuda()
    meta, _ = H.load_fixture(case)

    def build():
        net, lX, lS_l, lS_i, lT = H.materialize(H.args_from(meta["args"]))
        net.create(lX[0], lS_l[0], lS_i[0], lT[0])
        net.stage_batches(lX, lS_l, lS_i)
        return net, lS_i, len(lS_l[0][0])

    a, lS_i, n = build()
    b, _, _ = build()
    try:
        D = a.emb_w[0].shape[1]
        # (DIN and DIEN: the candidate-ad table, whose pooled row stands in the interaction buffer as it is; a behaviour row
        # reaches it through ReLU units that may be dead in the mini models)
        t = len(a.emb_w) - 2 if case in ("din_mini", "dien_mini") else 1
        row = int(lS_i[0][t][0])
        v = np.random.RandomState(2).uniform(-0.5, 0.5, (1, D)).astype(np.float32)
        old = a.run_staged(0, n).copy(), a.engine.fetch_interaction(n).copy()
        ids_t = dev(np.array([row], np.int64))
        a.update_embedding_rows(t, ids_t, dev(v))
        b.update_embedding_rows(t, [row], v)
        back = a.embedding_rows(t, ids_t)
        assert isinstance(back, torch.Tensor) and back.is_cuda and same(host(back), b.embedding_rows(t, [row])) and same(host(back), v)
        got = a.run_staged(0, n).copy(), a.engine.fetch_interaction(n).copy()
        exp = b.run_staged(0, n).copy(), b.engine.fetch_interaction(n).copy()
        assert same(got[0], exp[0]) and same(got[1], exp[1])
        assert not same(got[1], old[1])
        # the rules the wrapper checks on device tensors
        with pytest.raises(ValueError):
            a.update_embedding_rows(t, ids_t.to(torch.int32), dev(v))
        with pytest.raises(ValueError):
            a.update_embedding_rows(t, ids_t, dev(v).to(torch.float64))
        with pytest.raises(ValueError):
            a.update_embedding_rows(t, ids_t, v)                               # device ids, host values
    finally:
        a.engine.close()
        b.engine.close()
