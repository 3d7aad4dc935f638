"""Tables whose row offsets need the 32nd bit, on the GPU (-m gpu).

Every gather kernel addresses a row as an unsigned 32-bit count of pieces from its table's base; only the rowwise types
(int8, int4, line-packed or not) reach piece offsets in [2^31, 2^32).  The cases here put bags on the table's LAST rows (bit
31 set), on its first, across every edge (the first row with bit 31 set in the plain and in the line-packed layouts, the rows
where a half-precision and an fp8 byte offset cross 2^32) and on random rows, with a second table behind the big one (its
offset beyond 2^32 bytes / elements), and walk one engine through every stored type, so that each conversion kernel of
csrc/table_convert.hip runs once over billions of elements.  tests/large_table_shapes.py holds the shapes,
tests/test_large_tables_cpu.py proves that they sit on their edges and that a wrong address would read different numbers.

Every table is filled ON THE DEVICE (fill_table_uniform); no host array of a big table exists.  The expectations are built
from the picked rows alone: orc_fill_value element by element (S.fill_rows), then the checkers of the per-type tests --
torch's embedding_bag_byte / 4bit prepack and rowwise_offsets (bitwise for the sequential forms and the one-row bags), numpy's
fp16 / torch's bf16 and float8_e4m3fn roundings, the oracle's sequential fp32 sum -- and the bar those files use for the other
forms, H.close(rtol=1e-5, atol_scale=2e-6) against the sequential result.

These cases are large by nature (27.5 GB of fp32 beside 8.6 GB of int8 at the peak of Case A; convert_tables wants the new
arena to fit a quarter of the free memory): each case reads the free device memory first and skips, with both numbers in the
message, when the device cannot hold its walk -- the only reason for a skip here.  No GPU work follows a HIP error: the case
that met one is remembered and the remaining ones fail without touching the GPU (tests/test_gather_boundaries.py's pattern).
DRS_LARGE_TABLES_REPORT=<file>: one JSON line per step (forms shown, seconds), profiles/r23_large_tables.md.
"""
import functools
import json
import os
import time

import numpy as np
import pytest

from deeprecsys_amd import _native as N
from oracle import oracle as orc
from tests import gather_shapes as GS
from tests import helpers as H
from tests import large_table_shapes as S
from tests import test_int4_tables as T4
from tests import test_int8_tables as T8
from tests.test_fp8_tables_cpu import fp8_exponent
from tests.test_half_tables import upcast
from tests.test_sls_weights_cpu import torch_weighted_rowwise

pytestmark = pytest.mark.gpu

FAULT = []          # the case that met a HIP error: the cases behind it do not touch the GPU
LO, HI, SEED = S.FILL
# (sls_exact, sls_flat, sls_one) of the per-type tests, bags per wave left to the engine -- and one setting with one bag per
# wave: with T = 2 the engine pairs the bags of a sample (flat ... bpw2), "sls_bpw" 1 shows the coalesced flat form
SETTINGS = [dict(sls_exact=e, sls_flat=f, sls_one=o, sls_bpw=0) for e, f, o in T8.SETTINGS] + [dict(sls_exact=0, sls_flat=1, sls_one=1, sls_bpw=1)]
BAG_L = (1, S.L_MAX, GS.RAGGED)            # the bag length of staged batch 0, 1, 2


def _report(**kw):
    print(json.dumps(kw))
    path = os.environ.get("DRS_LARGE_TABLES_REPORT")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(kw) + "\n")


def free_bytes():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return int(torch.cuda.mem_get_info()[0])


def gate(test, need):
    free = free_bytes()
    _report(test=test, free_bytes=free, needed_bytes=need)
    if free < need:
        pytest.skip("%d bytes of device memory are free, this case needs %d" % (free, need))
    return free


def guarded(name, body):
    if FAULT:
        pytest.fail("not run: %s met a HIP error, nothing more is started on that GPU" % FAULT[0])
    try:
        body()
    except N.DrsError as e:
        if e.code == N.ERR_HIP:
            FAULT.append(name)
        raise


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def sequential(form):
    return form == "any" or form.startswith("one") or form.endswith("sequential")


def form_of(D, T, L, opts):
    case = GS.Case("large", "sls", D, T, (), (), (L,), (S.B,), tuple(sorted(opts.items())), 0, "", "at", "", (), (), None, "")
    return case, GS.expected_gather_form(case)


@functools.lru_cache(maxsize=None)
def picked(rows, D):
    """What the tests over tables of `rows` rows share, computed once and never written to: the staged batches, the picked
    rows of every table (table 0: the rows the batches name; the small tables behind it: every row), the batches' indices
    re-indexed into them, and those rows as the fill writes them."""
    bs = S.batches_a(D) if rows == S.ROWS_A else S.batches_limit(rows[0])
    picks = [S.picked_rows(bs, 0)] + [np.arange(r, dtype=np.int64) for r in rows[1:]]
    pos = [[S.positions(picks[t], idx[t]) for t in range(len(rows))] for idx, _ in bs]
    fill = [S.fill_rows(picks[0], D, 0, LO, HI, SEED)] + [orc.fill_table_uniform(rows[t], D, t, LO, HI, SEED, nthreads=0) for t in range(1, len(rows))]
    return bs, picks, pos, fill


class Case(object):
    """One engine over device-filled tables and its three staged batches."""

    def __init__(self, rows, D):
        self.rows, self.D, self.T = list(rows), D, len(rows)
        self.bs, self.picks, self.pos, self.fill = picked(tuple(rows), D)
        self.eng = N.Engine(N.MODEL_DLRM, self.rows, D, [8, D], [D * (self.T + 1), 4, 1], N.INTERACT_CAT, sigmoid_top=2, max_batch=S.B,
                            max_lookups=S.L_MAX, num_staged_batches=3, num_slots=1)
        self.eng.set_option("dispatch_log", 1)
        self.eng.set_option("sls_nt", 0)
        T8._fc(self.eng, D, self.T)
        self.dense = np.random.RandomState(3).rand(S.B, 8).astype(np.float32)
        self.stage()
        self.t0 = time.time()

    def stage(self):
        for b, (idx, lens) in enumerate(self.bs):
            self.eng.stage_batch(b, self.dense, idx, lens)

    def fill_tables(self):
        for t in range(self.T):
            self.eng.fill_table_uniform(t, LO, HI, SEED)

    def lap(self):
        t, self.t0 = time.time() - self.t0, time.time()
        return round(t, 2)

    # ---- references: [B, T * D] per staged batch ------------------------------------------------------------------------
    def refs_rowwise(self, bits, src):
        """src: the fp32 rows the quantizer read (per table, the picked rows) -> (refs, every picked row's value)"""
        M = T8 if bits == 8 else T4
        P = [M.prepack(W) for W in src]
        V = [M.dequant(W) for W in src]
        refs = []
        for b, (_, lens) in enumerate(self.bs):
            refs.append(np.concatenate([V[t][self.pos[b][t]] if b == 0 else M.pool(P[t], self.pos[b][t], lens[t]) for t in range(self.T)], axis=1))
        return refs, V, P

    def refs_plain(self, V):
        """V: the stored values, widened to fp32 -> the oracle's sequential fp32 sums"""
        return [np.concatenate([V[t][self.pos[b][t]] if b == 0 else orc.sls(V[t], self.pos[b][t], lens[t]) for t in range(self.T)], axis=1)
                for b, (_, lens) in enumerate(self.bs)]

    # ---- one state of the walk --------------------------------------------------------------------------------------------
    def check(self, step, dtype, packed, tag, refs, settings=SETTINGS, batches=(0, 1, 2), same_as=None, same_seq_only=False):
        """Under every setting and for every batch: the dispatch log names exactly the expected form with the type's tag; a
        sequential form (and every one-row bag) is bitwise the reference, any other form within the bar of the sequential
        result; same_as: the bits an earlier state gave under the same setting.  -> {(setting, batch): pooled columns}"""
        eng, D = self.eng, self.D
        assert eng.get_option("table_dtype") == dtype, step
        assert eng.get_option("table_bytes") == S.arena_bytes(dtype, self.rows, D, packed), step
        out, forms = {}, set()
        for k, opts in enumerate(settings):
            for key, v in sorted(opts.items()):
                eng.set_option(key, v)
            for b in batches:
                case, form = form_of(D, self.T, BAG_L[b], opts)
                eng.forward(b, S.B)
                log = eng.last_dispatch()
                got = eng.fetch_interaction(S.B)[:, D:].copy()
                bad = GS.check_dispatch(case, log, form=form, tag=tag)
                assert not bad, (step, opts, b, bad, log)
                forms.update(t.split("[")[0] for t in log if t.startswith(GS.GATHER_TOKENS))
                where = (step, tag, opts, "batch %d" % b, form)
                if sequential(form):
                    if not np.array_equal(_bits(got), _bits(refs[b])):
                        wrong = np.argwhere(_bits(got) != _bits(refs[b]))
                        raise AssertionError((where, "not the reference's bits", "bags %r" % sorted(set(wrong[:, 0]))[:12],
                                              "columns %r" % sorted(set(wrong[:, 1]))[:12], float(np.abs(got - refs[b]).max())))
                else:
                    assert H.close(got, refs[b], rtol=1e-5, atol_scale=2e-6), (where, float(np.abs(got - refs[b]).max()))
                if same_as is not None and (sequential(form) or not same_seq_only):
                    assert np.array_equal(_bits(got), _bits(same_as[(k, b)])), (where, "not the bits of the earlier state")
                out[(k, b)] = got
        _report(step=step, D=D, rows=self.rows[0], tag=tag or "f32", forms=sorted(forms), seconds=self.lap())
        return out

    def check_weighted(self, step, bits, tag, P):
        """batch 1 (L_MAX rows per bag) with a weight per row, "sls_weighted_flat" 1: torch's rowwise_offsets with
        per_sample_weights, bitwise in the sequential form, within the bar in the flat one"""
        eng, D = self.eng, self.D
        idx, lens = self.bs[1]
        rng = np.random.RandomState(5)
        wts = [rng.uniform(0, 1, size=i.size).astype(np.float32) for i in idx]
        ref = np.concatenate([torch_weighted_rowwise(P[t], self.pos[1][t], lens[t], wts[t], bits) for t in range(self.T)], axis=1)
        eng.stage_batch_weights(1, wts)
        eng.set_option("sls_weighted_flat", 1)
        forms = set()
        for opts in (dict(sls_exact=1, sls_flat=1, sls_one=1, sls_bpw=0), dict(sls_exact=0, sls_flat=1, sls_one=1, sls_bpw=1)):
            for key, v in sorted(opts.items()):
                eng.set_option(key, v)
            case, form = form_of(D, self.T, S.L_MAX, opts)
            eng.forward(1, S.B)
            log = eng.last_dispatch()
            got = eng.fetch_interaction(S.B)[:, D:].copy()
            bad = GS.check_dispatch(case, log, form=form, tag=tag + ",w")
            assert not bad, (step, opts, bad, log)
            forms.update(t.split("[")[0] for t in log if t.startswith(GS.GATHER_TOKENS))
            if sequential(form):
                assert np.array_equal(_bits(got), _bits(ref)), (step, opts, form, float(np.abs(got - ref).max()))
            else:
                assert H.close(got, ref, rtol=1e-5, atol_scale=2e-6), (step, opts, form, float(np.abs(got - ref).max()))
        eng.set_option("sls_weighted_flat", 0)
        self.stage()                                                    # staged again: unweighted again
        _report(step=step, D=D, rows=self.rows[0], tag=tag + ",w", forms=sorted(forms), seconds=self.lap())


# ---- Case A: every stored type over a table whose last rows have bit 31 set ----------------------------------------------
# One walk, in two tests: steps 1 - 4 (the rowwise types) and, from step 4's state built again, steps 5 - 8 (fp16, fp32, bf16,
# fp8).  Each step frees its source arena before the next large one exists.  (Measured as one test, the walk takes many
# times test_table_beyond_2_pow_32_floats' time -- profiles/r23_large_tables.md -- hence the split; no state is trimmed.)
def walk_rowwise(D):
    rows, I8, I4 = S.ROWS_A, N.TABLE_INT8_ROWWISE, N.TABLE_INT4_ROWWISE
    test = "rowwise walk D %d" % D
    free = gate(test, S.free_needed(S.WALK_A1, rows, D))
    t_start = time.time()
    c = Case(rows, D)
    eng = c.eng
    try:
        _report(step="engine created", D=D, rows=rows[0], seconds=c.lap())
        # 1. table_dtype 8 (quantize_rows_kernel<SrcElems> over the arena as drs_create left it), then the fill (<SrcFill>)
        eng.set_option("table_dtype", I8)
        c.fill_tables()
        refs8, V8, P8 = c.refs_rowwise(8, c.fill)
        r1 = c.check("1: 8, fill", I8, False, "i8", refs8)
        c.check_weighted("1: 8, weighted", 8, "i8", P8)
        # 2. the line-packed layout and back (relayout_rows_kernel, both ways): the bits of step 1
        eng.set_option("table_int8_lines", 1)
        c.check("2: int8 lines 1", I8, True, "i8l", refs8, same_as=r1)
        eng.set_option("table_int8_lines", 0)
        c.check("2: int8 lines 0", I8, False, "i8", refs8, same_as=r1)
        # 3. 8 -> 9 (pack4_rows_kernel<SrcI8>): every int8 row's value, quantized again; then its line-packed layout
        eng.set_option("table_dtype", I4)
        refs48, _, P48 = c.refs_rowwise(4, V8)
        r3 = c.check("3: 8 -> 9", I4, False, "i4", refs48)
        c.check_weighted("3: 9, weighted", 4, "i4", P48)
        eng.set_option("table_int4_lines", 1)
        c.check("3: int4 lines 1", I4, True, "i4l", refs48, same_as=r3)
        # 4. the fill under 9 (pack4_rows_kernel<SrcFill>, into the line-packed layout): one-row bags
        c.fill_tables()
        refs4, _, _ = c.refs_rowwise(4, c.fill)
        c.check("4: fill under 9", I4, True, "i4l", refs4, batches=(0,))
    finally:
        eng.close()
    _report(test=test, free_bytes=free, seconds=round(time.time() - t_start, 2))


def walk_plain(D):
    rows, I4 = S.ROWS_A, N.TABLE_INT4_ROWWISE
    test = "plain walk D %d" % D
    free = gate(test, S.free_needed(S.WALK_A2, rows, D))
    t_start = time.time()
    c = Case(rows, D)
    eng = c.eng
    try:
        _report(step="engine created", D=D, rows=rows[0], seconds=c.lap())
        # 4 again: the state walk_rowwise ended in -- line-packed int4 tables, filled under 9
        eng.set_option("table_int4_lines", 1)
        eng.set_option("table_dtype", I4)
        c.fill_tables()
        refs4, V4, _ = c.refs_rowwise(4, c.fill)
        c.check("4: fill under 9 (again)", I4, True, "i4l", refs4, batches=(0,))
        # 5. 9 -> 1 (write_elems_kernel<SrcI4>, more than 2^32 elements): the fp16 rounding of step 4's values
        eng.set_option("table_dtype", N.TABLE_FP16)
        V16 = [upcast(V, N.TABLE_FP16) for V in V4]
        refs16 = c.refs_plain(V16)
        r5 = c.check("5: 9 -> 1", N.TABLE_FP16, False, "f16", refs16, batches=(0, 1))
        # 6. 1 -> 0 (the flat convert_table_kernel, n above 2^32): widening is exact -- step 5's bits; 0 -> 2: their bf16 rounding
        eng.set_option("table_dtype", N.TABLE_FP32)
        c.check("6: 1 -> 0", N.TABLE_FP32, False, "", refs16, batches=(0, 1), same_as=r5, same_seq_only=True)
        eng.set_option("table_dtype", N.TABLE_BF16)
        c.check("6: 0 -> 2", N.TABLE_BF16, False, "bf16", c.refs_plain([upcast(V, N.TABLE_BF16) for V in V16]), batches=(0, 1))
        # 7. fp32 again, the fill under 0 (fill_uniform_kernel), 0 -> 4 (absmax_rows_kernel, to_fp8_rows_kernel)
        eng.set_option("table_dtype", N.TABLE_FP32)
        c.fill_tables()
        c.check("7: fill under 0", N.TABLE_FP32, False, "", c.refs_plain(c.fill), batches=(0, 1))
        assert fp8_exponent(0.05) == 13
        eng.set_option("table_dtype", N.TABLE_FP8_E4M3)
        assert [eng.table_fp8_exponent(t) for t in range(c.T)] == [13] * c.T
        import torch
        Vf8 = [torch.from_numpy(W * np.float32(2.0 ** 13)).to(torch.float8_e4m3fn).to(torch.float32).numpy() * np.float32(2.0 ** -13) for W in c.fill]
        refsf8 = c.refs_plain(Vf8)
        c.check("7: 0 -> 4", N.TABLE_FP8_E4M3, False, "f8", refsf8)
        # 8. the fill under 4 (to_fp8_rows_kernel<SrcFill>; the scale from the bounds, the same k)
        c.fill_tables()
        assert [eng.table_fp8_exponent(t) for t in range(c.T)] == [13] * c.T
        c.check("8: fill under 4", N.TABLE_FP8_E4M3, False, "f8", refsf8)
    finally:
        eng.close()
    _report(test=test, free_bytes=free, seconds=round(time.time() - t_start, 2))


@pytest.mark.parametrize("D", [S.D_MAIN, S.D_ANY])
def test_rowwise_types_read_the_rows_beyond_bit_31(D):
    """Case A, steps 1 - 4: rows [214 752 461, 1000]; D 32 shows the copy, flat-coalesced, flat (two bags per wave), sequential
    and split ring forms, D 30 sls_any_kernel -- each with the i8, i8l, i4 and i4l tags, weighted bags with i8 and i4."""
    guarded("Case A, rowwise, D %d" % D, lambda: walk_rowwise(D))


@pytest.mark.parametrize("D", [S.D_MAIN, S.D_ANY])
def test_conversions_out_of_the_rowwise_types_beyond_2_pow_32_elements(D):
    """Case A, steps 5 - 8: 9 -> 1 -> 0 -> 2 -> 0 -> 4 over 6.9 G elements, and the fills under 0 and 4; the f16, bf16 and f8
    tags and fp32 tables, byte offsets beyond 2^32 and table 1 behind them."""
    guarded("Case A, plain, D %d" % D, lambda: walk_plain(D))


# ---- Case B: the limit and the refusals -------------------------------------------------------------------------------------
LIMIT_SETTINGS = [dict(sls_exact=1, sls_flat=1, sls_one=1, sls_bpw=0), dict(sls_exact=0, sls_flat=1, sls_one=1, sls_bpw=0)]


def refusals():
    D, rows = S.D_LIMIT, (S.ROWS_REFUSED,)
    gate("refusals", S.arena_bytes(S.FP32, rows, D) + S.SLACK)
    c = Case(rows, D)
    eng = c.eng
    try:
        before = eng.get_option("table_bytes")
        assert before == S.arena_bytes(S.FP32, rows, D) == (1 << 34)
        for dt in (N.TABLE_INT8_ROWWISE, N.TABLE_INT4_ROWWISE):
            with pytest.raises(N.DrsError) as e:
                eng.set_option("table_dtype", dt)
            assert e.value.code == N.ERR_UNSUPPORTED, e.value
            assert "table 0 " in e.value.detail and "too large to address" in e.value.detail and "table_dtype %d" % dt in e.value.detail
            assert eng.get_option("table_dtype") == N.TABLE_FP32 and eng.get_option("table_bytes") == before
        c.fill_tables()                                                 # exactly 2^32 floats
        c.check("refused: fp32 still served", N.TABLE_FP32, False, "", c.refs_plain(c.fill), settings=LIMIT_SETTINGS)
    finally:
        eng.close()


def test_tables_too_large_to_address_are_refused_and_nothing_changes():
    """rows 2^30 at D 4: 2^32 pieces in either rowwise type.  Both conversions are refused (ERR_UNSUPPORTED, the message names
    the table), the engine keeps its fp32 arena and serves the last rows of its 2^32 floats, bitwise."""
    guarded("Case B, refusals", refusals)


def limit(dtype):
    D, rows = S.D_LIMIT, (S.ROWS_LIMIT,)
    bits, tag = (8, "i8") if dtype == N.TABLE_INT8_ROWWISE else (4, "i4")
    gate("limit %s" % tag, S.free_needed(((S.FP32, False), (dtype, False)), rows, D))
    c = Case(rows, D)
    try:
        c.eng.set_option("table_dtype", dtype)                          # accepted: 2^32 - 4 pieces
        c.fill_tables()
        refs, _, _ = c.refs_rowwise(bits, c.fill)
        c.check("limit: %s" % tag, dtype, False, tag, refs, settings=LIMIT_SETTINGS)
    finally:
        c.eng.close()


@pytest.mark.parametrize("dtype", [N.TABLE_INT4_ROWWISE, N.TABLE_INT8_ROWWISE])
def test_the_largest_addressable_rowwise_table(dtype):
    """rows 2^30 - 1 at D 4: the last row starts at piece 2^32 - 8.  Bags of the last 20 rows, the first ones, rows around 2^29
    (piece 2^31) and random ones: bitwise torch's pooled sums in the sequential walk, within the bar in the split one."""
    guarded("Case B, limit %d" % dtype, lambda: limit(dtype))
