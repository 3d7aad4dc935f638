"""Single table rows updated and read back on the GPU (-m gpu): Engine.update_rows / Engine.get_rows in every stored type.

The twin-engine method: engine A loads W, takes its options and then update_rows(ids, V); engine B is built from W' (W with
those rows replaced, the last occurrence of an id winning -- tests/row_update_ref.py) in the same option order.  get_rows over
EVERY row of EVERY table must be bit-identical between the two, and so must one forward (DLRM cat, T 3, B 32, bags naming
updated and untouched rows).  Updates go to the middle table; tables 0 and 2 must keep their bits.  The stored bytes are
torch's: get_rows also equals the reference module's served values bit for bit, and what a path that predates it shows --
one-row bags through fetch_interaction.  tests/test_row_updates_cpu.py proves the property the method rests on.
"""
import ctypes as C

import numpy as np
import pytest

from deeprecsys_amd import _native as N
from tests import helpers as H
from tests import large_table_shapes as S
from tests import row_update_ref as R
from tests.test_int8_tables import _fc

pytestmark = pytest.mark.gpu

ROWS = [120, R.ROWS, 77]
T, MID, B, L, B_ONE = 3, 1, 32, 4, 320          # B_ONE one-row bags cover every row of every table
LINES_KEY = {R.I8: "table_int8_lines", R.I4: "table_int4_lines"}
CASES = [(dt, D, ln) for dt in R.DTYPES for D in R.DS for ln in ((0, 1) if dt in LINES_KEY else (0,))]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def tables(D, seed=0):
    return [R.table(r, D, seed=seed + 10 * t + D) for t, r in enumerate(ROWS)]


def batches(D):
    """batch 0: 32 bags of 4 rows; the middle table's bags name every updated row and untouched ones.  batch 1: 320 one-row
    bags, every row of every table."""
    rng = np.random.RandomState(7 + D)
    idx = [rng.randint(0, r, size=B * L).astype(np.int64) for r in ROWS]
    idx[MID][:R.IDS.size] = R.IDS
    idx[MID][R.IDS.size:R.IDS.size + 3] = [1, 8, 298]                     # (neighbours of updated rows)
    one = [(np.arange(B_ONE) % r).astype(np.int64) for r in ROWS]
    return (rng.rand(B, 8).astype(np.float32), idx, [np.full(B, L, np.int32)] * T), (np.zeros((B_ONE, 8), np.float32), one, [np.ones(B_ONE, np.int32)] * T)


def options(eng, dtype, lines):
    if lines:
        eng.set_option(LINES_KEY[dtype], 1)
    if dtype != R.FP32:
        eng.set_option("table_dtype", dtype)


def engine(D, Ws, rows=ROWS, slots=2):
    eng = N.Engine(N.MODEL_DLRM, rows, D, [8, D], [D * (len(rows) + 1), 4, 1], N.INTERACT_CAT, sigmoid_top=2, max_batch=B_ONE,
                   max_lookups=L, num_staged_batches=2, num_slots=slots)
    for t, W in enumerate(Ws):
        if W is not None:
            eng.set_table(t, W)
    _fc(eng, D, len(rows))
    eng.set_option("sls_exact", 1)
    return eng


def stage(eng, D):
    for b, (dense, idx, lens) in enumerate(batches(D)):
        eng.stage_batch(b, dense, idx, lens)


def all_rows(eng, rows=ROWS):
    return [eng.get_rows(t, np.arange(r, dtype=np.int64)) for t, r in enumerate(rows)]


def forward(eng):
    out = eng.forward(0, B)
    return out.copy(), eng.fetch_interaction(B).copy()


def one_row_bags(eng, D):
    """every row of every table as the gather serves it to a bag of that row alone (the path that predates get_rows)"""
    eng.forward(1, B_ONE)
    Rm = eng.fetch_interaction(B_ONE)[:, D:]
    return [Rm[:r, t * D:(t + 1) * D].copy() for t, r in enumerate(ROWS)]


def expect_equal_engines(a, b, D, what):
    ra, rb = all_rows(a), all_rows(b)
    for t in range(T):
        assert same(ra[t], rb[t]), (what, "table %d" % t, np.argwhere(_bits(ra[t]) != _bits(rb[t]))[:4].tolist())
    (oa, Ra), (ob, Rb) = forward(a), forward(b)
    assert same(Ra, Rb) and same(oa, ob), (what, "forward")
    return ra


# ---- 1, 2: every type, width and layout ---------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,D,lines", CASES)
def test_update_rows_gives_the_engine_built_from_the_updated_table(dtype, D, lines):
    """ids: row 0, row 300 (the whole partly filled last line), two neighbours in one 128-byte line, unsorted, one id three
    times.  A == B over every row and one forward; get_rows == torch's served values == one-row bags, bit for bit; tables 0
    and 2 keep their bits; the forward differs from the one before the update."""
    Ws = tables(D)
    V = R.update_values(R.IDS.size, D, seed=100 + D)
    W2 = [W if t != MID else R.replaced(W, R.IDS, V) for t, W in enumerate(Ws)]
    a, b = engine(D, Ws), engine(D, W2)
    try:
        for e in (a, b):
            options(e, dtype, lines)
            stage(e, D)
        before_rows, before_fwd = all_rows(a), forward(a)
        for t in range(T):
            assert same(before_rows[t], R.served(Ws[t], dtype)), ("before the update", t)
        a.update_rows(MID, R.IDS, V)
        got = expect_equal_engines(a, b, D, (dtype, D, lines))
        assert same(got[0], before_rows[0]) and same(got[2], before_rows[2])
        assert not same(forward(a)[1], before_fwd[1])
        # 2. the stored bytes are torch's, and the read-back is what the gather serves
        exp = [R.served(Ws[0], dtype), R.served_after_update(Ws[MID], R.IDS, V, dtype), R.served(Ws[2], dtype)]
        bags = one_row_bags(a, D)
        for t in range(T):
            assert same(got[t], exp[t]), ("reference", t, np.argwhere(_bits(got[t]) != _bits(exp[t]))[:4].tolist())
            assert same(got[t], bags[t]), ("one-row bags", t)
        # any order, duplicates allowed in a read-back
        ids = np.array([300, 0, 150, 150, 7, 300], np.int64)
        assert same(a.get_rows(MID, ids), exp[MID][ids])
        if dtype == R.FP8:
            assert a.table_fp8_exponent(MID) == b.table_fp8_exponent(MID) == R.table_exponent(Ws[MID])
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("dtype", R.DTYPES)
@pytest.mark.parametrize("n", ["rows", 1, 0])
def test_every_row_one_row_and_no_row(dtype, n):
    """n == rows (every row, the absmax row's magnitude kept in the new values so that fp8 keeps its scale), n == 1, n == 0 at
    D 30, line-packed where the type has lines (3 and 6 rows per line)"""
    D, lines = 30, int(dtype in LINES_KEY)
    Ws = tables(D)
    if n == "rows":
        ids = np.random.RandomState(5).permutation(R.ROWS).astype(np.int64)
        V = R.update_values(R.ROWS, D, seed=9)
        V[0, 3] = 1.5
    else:
        ids, V = np.array([R.ROWS - 1] * n, np.int64), R.update_values(n, D, seed=9)
    W2 = [W if t != MID else R.replaced(W, ids, V) for t, W in enumerate(Ws)]
    a, b = engine(D, Ws), engine(D, W2)
    try:
        for e in (a, b):
            options(e, dtype, lines)
            stage(e, D)
        a.update_rows(MID, ids, V)
        got = expect_equal_engines(a, b, D, (dtype, n))
        assert same(got[MID], R.served_after_update(Ws[MID], ids, V, dtype))
        assert a.get_rows(MID, np.zeros(0, np.int64)).shape == (0, D)
    finally:
        a.close()
        b.close()


# ---- 3: order with conversions ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [R.I8, R.I4, R.FP8, R.FP16])
def test_update_under_fp32_then_convert(dtype):
    D, lines = 32, int(dtype in LINES_KEY)
    Ws = tables(D)
    V = R.update_values(R.IDS.size, D, seed=3)
    W2 = [W if t != MID else R.replaced(W, R.IDS, V) for t, W in enumerate(Ws)]
    a, b = engine(D, Ws), engine(D, W2)
    try:
        a.update_rows(MID, R.IDS, V)
        for e in (a, b):
            options(e, dtype, lines)
            stage(e, D)
        got = expect_equal_engines(a, b, D, dtype)
        assert same(got[MID], R.served(W2[MID], dtype))
    finally:
        a.close()
        b.close()


def test_update_under_int8_then_convert_to_fp32():
    D = 32
    Ws = tables(D)
    V = R.update_values(R.IDS.size, D, seed=3)
    a = engine(D, Ws)
    try:
        options(a, R.I8, 1)
        a.update_rows(MID, R.IDS, V)
        a.set_option("table_dtype", R.FP32)
        got = all_rows(a)
        assert same(got[MID], R.served_after_update(Ws[MID], R.IDS, V, R.I8))
        assert same(got[0], R.served(Ws[0], R.I8)) and same(got[2], R.served(Ws[2], R.I8))
    finally:
        a.close()


# ---- 4: work in flight ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [R.FP32, R.I8])
def test_a_set_in_flight_is_served_from_the_old_rows(dtype):
    D = 64
    Ws = tables(D)
    V = R.update_values(R.IDS.size, D, seed=4)
    W2 = [W if t != MID else R.replaced(W, R.IDS, V) for t, W in enumerate(Ws)]
    a, b = engine(D, Ws), engine(D, W2)
    try:
        for e in (a, b):
            options(e, dtype, 1 if dtype in LINES_KEY else 0)
            stage(e, D)
        old = a.forward(0, B).copy()
        a.forward_async(1, 0, B)
        a.update_rows(MID, R.IDS, V)
        assert same(a.wait(1, B), old)
        new = a.forward(0, B)
        assert same(new, b.forward(0, B)) and not same(new, old)
    finally:
        a.close()
        b.close()


# ---- 5: refusals change nothing ---------------------------------------------------------------------------------------------
def _raw(eng, fn, t, n, ids, V):
    """the C call itself, so that a null pointer and a negative n can be passed"""
    return getattr(N.lib(), fn)(eng._h, t, n, None if ids is None else ids.ctypes.data_as(C.POINTER(C.c_int64)),
                                None if V is None else V.ctypes.data_as(C.POINTER(C.c_float)))


@pytest.mark.parametrize("dtype", [R.FP32, R.I4, R.FP8])
def test_refusals_change_nothing(dtype):
    D = 32
    Ws = tables(D)
    Ws[2] = None                                                          # table 2 is never set or filled
    a = engine(D, Ws)
    try:
        options(a, dtype, 1 if dtype in LINES_KEY else 0)
        before = a.get_rows(MID, np.arange(R.ROWS, dtype=np.int64))
        good = R.update_values(3, D, seed=1)

        def refused(code, t, n, ids, V, fn="drs_update_rows"):
            assert _raw(a, fn, t, n, ids, V) == code, (fn, t, n)
            assert same(a.get_rows(MID, np.arange(R.ROWS, dtype=np.int64)), before), (fn, t, n)

        for fn in ("drs_update_rows", "drs_get_rows"):
            for bad in ([-1, 5, 6], [5, R.ROWS, 6], [5, 6, 1 << 40]):
                refused(N.ERR_INDEX_RANGE, MID, 3, np.array(bad, np.int64), good.copy(), fn)
            one = np.array([5], np.int64)
            refused(N.ERR_BAD_ARG, -1, 1, one, good.copy(), fn)
            refused(N.ERR_BAD_ARG, T, 1, one, good.copy(), fn)
            refused(N.ERR_BAD_ARG, MID, 1, None, good.copy(), fn)
            refused(N.ERR_BAD_ARG, MID, 1, one, None, fn)
            refused(N.ERR_BAD_ARG, MID, -1, one, good.copy(), fn)
            refused(N.ERR_BAD_ARG, 2, 1, one, good.copy(), fn)             # never set or filled
            assert _raw(a, fn, MID, 0, None, None) == N.OK                 # n == 0: nothing to do, nothing read
        with pytest.raises(ValueError):
            a.update_rows(MID, [1, 2], good)                              # the binding checks the shapes first
        if dtype == R.FP8:
            k = a.table_fp8_exponent(MID)
            edge = np.float32(448 * 2.0 ** -k)
            over = good.copy()
            over[1, 7] = np.nextafter(edge, np.float32(np.inf))
            with pytest.raises(N.DrsError) as e:
                a.update_rows(MID, [5, 6, 7], over)
            assert e.value.code == N.ERR_BAD_ARG and "drs_set_table" in e.value.detail
            assert same(a.get_rows(MID, np.arange(R.ROWS, dtype=np.int64)), before)
            ok = good.copy()
            ok[1, 7], ok[2, 0], ok[2, 1] = -edge, np.inf, np.nan              # the edge itself fits; non-finite elements are stored as NaN
            ok[0, 0], ok[0, 1] = -1e-9, 1e-9                                  # rounds to a zero code: the stored sign comes back
            a.update_rows(MID, [5, 6, 7], ok)
            got = a.get_rows(MID, np.array([5, 6, 7], np.int64))
            assert got[1, 7] == -edge and np.isnan(got[2, 0]) and np.isnan(got[2, 1])
            assert _bits(got[0, :2]).tolist() == [0x80000000, 0]
            exp = R.served(ok, R.FP8, k)                                       # (a NaN's payload is not part of the contract)
            assert np.array_equal(np.isnan(got), np.isnan(exp)) and same(np.nan_to_num(got), np.nan_to_num(exp))
            assert a.table_fp8_exponent(MID) == k
    finally:
        a.close()


# ---- 6: the chunk edge --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [R.FP32, R.I8])
def test_updates_larger_than_one_staging_chunk(dtype):
    """One table of 66 000 rows at D 256: a chunk holds 65 536 rows (16 M elements), the update names 65 540 -- two ids twice,
    one pair on either side of the chunk boundary"""
    rows, D, n = 66000, 256, 65540
    rng = np.random.RandomState(12)
    W = rng.uniform(-1, 1, (rows, D)).astype(np.float32)
    ids = rng.permutation(rows)[:n].astype(np.int64)
    ids[65536] = ids[65535]
    ids[n - 1] = ids[10]
    V = rng.uniform(-1, 1, (n, D)).astype(np.float32)
    assert n * D > 16 << 20 and np.unique(ids).size == n - 2
    a, b = engine(D, [W], rows=[rows], slots=1), engine(D, [R.replaced(W, ids, V)], rows=[rows], slots=1)
    try:
        for e in (a, b):
            options(e, dtype, 0)
        a.update_rows(0, ids, V)
        ga, gb = all_rows(a, [rows])[0], all_rows(b, [rows])[0]
        assert same(ga, gb), np.argwhere(_bits(ga) != _bits(gb))[:4].tolist()
        assert same(a.get_rows(0, ids), gb[ids])                           # a read-back of more than one chunk
    finally:
        a.close()
        b.close()


# ---- 7: offsets beyond the 32nd bit --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,lines", [(R.I8, 0), (R.I8, 1), (R.I4, 0), (R.I4, 1)])
def test_rows_beyond_piece_2_pow_31_and_byte_2_pow_32(dtype, lines):
    """tests/large_table_shapes.py's [214 752 461, 1000] tables at D 32, filled on the device: rows among the last 4096 of table
    0 lie at pieces in [2^31, 2^32), table 1 lies behind 2^32 bytes.  Updated rows serve the reference's values, their
    neighbours the fill's.  Skips, with both numbers, only when the device cannot hold the arena and its conversion."""
    from tests.test_large_tables import gate
    D, rows = S.D_MAIN, list(S.ROWS_A)
    lo, hi, seed = S.FILL
    gate("row updates %d/%d" % (dtype, lines), S.free_needed(((S.FP32, False), (dtype, bool(lines))), rows, D))
    assert S.row_piece(dtype, D, rows[0] - 4096, bool(lines)) >= 1 << 31 and S.table_offsets(dtype, rows, D, bool(lines))[0][1] >= 1 << 32
    eng = N.Engine(N.MODEL_DLRM, rows, D, [8, D], [D * 3, 4, 1], N.INTERACT_CAT, sigmoid_top=2, max_batch=B, max_lookups=L,
                   num_staged_batches=1, num_slots=1)
    try:
        options(eng, dtype, lines)
        for t in range(2):
            eng.fill_table_uniform(t, lo, hi, seed)
        rng = np.random.RandomState(31)
        last = rows[0] - 1
        ids0 = np.array([last, last - 4095, last - 7, last - 6, last - 2000, last - 7], np.int64)       # neighbours in a line; one id twice
        ids1 = np.array([999, 0, 500], np.int64)
        for t, ids in ((0, ids0), (1, ids1)):
            V = rng.uniform(lo, hi, (ids.size, D)).astype(np.float32)
            look = np.unique(np.concatenate([ids + d for d in (-6, -2, -1, 0, 1, 2, 6)]))
            look = look[(look >= 0) & (look < rows[t])]
            fill = S.fill_rows(look, D, t, lo, hi, seed)
            eng.update_rows(t, ids, V)
            exp = R.served_after_update(fill, S.positions(look, ids), V, dtype)
            got = eng.get_rows(t, look)
            assert same(got, exp), (t, look[np.argwhere((_bits(got) != _bits(exp)).any(axis=1))[:, 0]].tolist())
    finally:
        eng.close()


# ---- 8: DIN and DIEN ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["din_mini", "dien_mini"])
def test_din_and_dien_serve_updated_rows(case):
    """one row that a behaviour bag names and one that the candidate-ad table names: output and interaction buffer equal a twin
    built from W', bit for bit, and differ from the output before"""
    meta, _ = H.load_fixture(case)

    def build(patch):
        net, lX, lS_l, lS_i, lT = H.materialize(H.args_from(meta["args"]))
        for t, r, v in patch:
            net.emb_w[t][r] = v
        net.create(lX[0], lS_l[0], lS_i[0], lT[0])
        net.stage_batches(None, lS_l, lS_i)
        return net, lS_l, lS_i, len(lS_l[0][0])

    a, lS_l, lS_i, n = build([])
    try:
        nT, D = len(a.emb_w), a.emb_w[0].shape[1]
        old = a.run_staged(0, n).copy(), a.engine.fetch_interaction(n).copy()
        # (the mini models' outputs are ReLU outputs, many of them 0: the rows come from a sample whose output is alive)
        smp = int(np.argwhere(old[0].any(axis=1))[0, 0])
        rng = np.random.RandomState(2)
        patch = []
        for t in (1, nT - 2):                                               # a behaviour table, the candidate ad
            first = int(np.asarray(lS_l[0][t][:smp]).sum())
            assert lS_l[0][t][smp] > 0
            patch.append((t, int(lS_i[0][t][first]), rng.uniform(-0.5, 0.5, D).astype(np.float32)))
        b, _, _, _ = build(patch)
        try:
            for t, r, v in patch:
                a.update_embedding_rows(t, [r], v[None, :])
                assert same(a.embedding_rows(t, [r]), v[None, :])
            got = a.run_staged(0, n).copy(), a.engine.fetch_interaction(n).copy()
            exp = b.run_staged(0, n).copy(), b.engine.fetch_interaction(n).copy()
            assert same(got[0], exp[0]) and same(got[1], exp[1])
            assert not same(got[0], old[0]) and not same(got[1], old[1])
        finally:
            b.engine.close()
    finally:
        a.engine.close()


# ---- 9: the wrapper ---------------------------------------------------------------------------------------------------------------
def test_the_model_wrapper_round_trips():
    meta, _ = H.load_fixture("dlrm_rm1_mini")
    net, lX, lS_l, lS_i, lT = H.materialize(H.args_from(meta["args"]))
    net.create(lX[0], lS_l[0], lS_i[0], lT[0])
    try:
        rows, D = net.emb_w[0].shape
        ids = np.array([rows - 1, 0, 1], np.int64)
        V = np.random.RandomState(1).uniform(-1, 1, (3, D)).astype(np.float32)
        net.update_embedding_rows(0, ids, V)
        assert same(net.embedding_rows(0, ids), V)
        assert same(net.embedding_rows(0, [2]), net.emb_w[0][2:3])
    finally:
        net.engine.close()
