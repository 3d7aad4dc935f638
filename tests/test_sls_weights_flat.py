"""Weights inside the flat, flat-coalesced and one-lookup gather forms on the GPU (-m gpu): engine option
"sls_weighted_flat" 1.

Every shape of tests/test_sls_weights_flat_cpu.py's catalogue, for each stored type: the weighted launch set takes the
form of its unweighted twin with the `w` tag, and its pooled columns equal the numpy restatement of that form's order
bit for bit (`flat_order_ref`; the sequential `weighted_ref` on the one-lookup shapes), within the split order's
tolerance of the sequential chain.  Weights of 1.0 (or NULL) give the unweighted engine's bits, and the unweighted query
of a mixed set keeps the bits it has alone.

L 81 at D 64 is the first length past the flat forms: the set keeps the weighted ring walk, split order (81 > 2048 / D), whose
bits are not the sequential chain's.  There the bit-for-bit checks are: the option changes nothing (the same bits with
"sls_weighted_flat" 0), and under "sls_exact" 1 the pooled columns are `weighted_ref`'s.
"""
import functools

import numpy as np
import pytest

from deeprecsys_amd import _native as N
from tests import helpers as H
from tests.test_half_tables import _load
from tests.test_sls_weights import JOBS12, JOBS16, TYPES, _engine, _fixed, _log, _run_set, _stored
from tests.test_sls_weights_cpu import same_bits
from tests.test_sls_weights_flat_cpu import (B, CATALOGUE, KEY, SIZES, expected_form, flat_order_ref, log_token, order_of, rows_of,
                                             seq_ref, shape_id)

pytestmark = pytest.mark.gpu


def dtype_tag(kind, D):
    """the dispatch log's dtype token: the line-packed kernels only where the layout is not the plain one (S < 128 that does
    not divide 128, docs/OPTIONS.md)"""
    if kind == "int8_lines":
        S = (D + 7) // 8 * 8 + 8
        return "i8l" if S < 128 and 128 % S else "i8"
    if kind == "int4_lines":
        S = (D // 2 + 3) // 4 * 4 + 4
        return "i4l" if S < 128 and 128 % S else "i4"
    return {"fp32": "", "fp16": "f16", "bf16": "bf16", "int8": "i8", "int4": "i4"}[kind]


@functools.lru_cache(maxsize=None)
def _case(n, base):
    """inputs and references of catalogue shape n for the stored values of `base` (fp32 | fp16 | bf16 | int8 | int4),
    computed once: the line-packed types share their plain twin's.  Batch 0 weighted, batch 1 weighted with table 1 left
    NULL, batch 2 the indices of batch 0 without weights."""
    D, T, L, opts = CATALOGUE[n]
    rows = rows_of(T)
    rng = np.random.RandomState(100 * n + 7)
    tables = [rng.uniform(-1, 1, (r, D)).astype(np.float32) for r in rows]
    stored = [_stored(base, W) for W in tables]
    idx = []
    for _ in range(2):
        ix = [rng.randint(0, rows[t], size=B * L).astype(np.int64) for t in range(T)]
        for t in range(T):
            ix[t][0], ix[t][-1] = 0, rows[t] - 1
        idx.append(ix)
    idx.append(idx[0])
    lens = [np.full(B, L, np.int32) for _ in range(T)]
    dense = [rng.rand(B, 8).astype(np.float32) for _ in range(2)]
    dense.append(dense[0])
    wts = [[rng.uniform(0, 1, size=B * L).astype(np.float32) for t in range(T)] for b in range(2)]
    wts[1][1] = None

    def eff(b, t):
        return np.ones(B * L, np.float32) if b == 2 or wts[b][t] is None else wts[b][t]

    form = expected_form(CATALOGUE[n])
    order = order_of(form)
    seq = [np.concatenate([seq_ref(stored[t], idx[b][t], lens[t], eff(b, t)) for t in range(T)], axis=1) for b in range(3)]
    if order is None:
        ref = None if form.endswith("split") else seq                          # (the split ring walk: no restatement of its order)
    else:
        NG, bpw = order
        ref = [np.concatenate([flat_order_ref(stored[t], idx[b][t], eff(b, t), B, L, NG, bpw, t % bpw) for t in range(T)], axis=1)
               for b in range(3)]
    for a in tables + seq + (ref or []):
        a.setflags(write=False)
    return dict(tables=tables, idx=idx, lens=lens, dense=dense, wts=wts, form=form, seq=seq, ref=ref)


def _tokens(eng, slot=0):
    return [t for t in eng.last_dispatch(slot) if t.startswith("sls_")]


# ------------------------------------------------------------------------------------------------------------------------
# 1. the catalogue
@pytest.mark.parametrize("kind", sorted(TYPES))
@pytest.mark.parametrize("n", range(len(CATALOGUE)), ids=[shape_id(s) for s in CATALOGUE])
def test_weighted_flat_forms_against_their_order_restated(kind, n):
    D, T, L, opts = CATALOGUE[n]
    c = _case(n, kind.split("_")[0])
    tables, idx, lens, dense, wts, form, seq, ref = (c[k] for k in ("tables", "idx", "lens", "dense", "wts", "form", "seq", "ref"))
    tag = dtype_tag(kind, D)
    ones = [np.ones(B * L, np.float32) for _ in range(T)]
    wf, on, un = (_engine(rows_of(T), D, L, B, kind) for _ in range(3))
    try:
        for eng in (wf, on, un):
            _load(eng, 11, tables, D, T)
            eng.set_option("dispatch_log", 1)
            eng.set_option("sls_nt", 1)
            for k, v in sorted(opts.items()):
                eng.set_option(k, v)
        wf.set_option(KEY, 1)
        on.set_option(KEY, 1)
        for b in range(3):
            wf.stage_batch(b, dense[b], idx[b], lens, weights=wts[b] if b < 2 else None)
            on.stage_batch(b, dense[b], idx[b], lens, weights=(ones, [None] * T, None)[b])
            un.stage_batch(b, dense[b], idx[b], lens)
        assert (wf.get_option(KEY), on.get_option(KEY), un.get_option(KEY)) == (1, 1, 0)
        with_w, without = log_token(form, 1, tag), log_token(form, 1, tag, weighted=False)
        alone = {}
        worst = 0.0
        for b in range(3):
            for bs in SIZES:
                where = (kind, shape_id(CATALOGUE[n]), b, bs)
                wf.forward(b, bs)
                Rw = wf.fetch_interaction(bs)
                tw = _tokens(wf)
                on.forward(b, bs)
                Ro = on.fetch_interaction(bs)
                un.forward(b, bs)
                Ru = un.fetch_interaction(bs)
                tu = _tokens(un)
                alone[(b, bs)] = Ru.copy()
                # 1. the form of the unweighted twin, with `w` where the batch carries weights
                assert len(tw) == 1 and tw[0].startswith(with_w if b < 2 else without), (where, tw, with_w)
                assert len(tu) == 1 and tu[0].startswith(without), (where, tu, without)
                assert tw[0].split("[")[1] == tu[0].split("[")[1], (where, tw, tu)             # ... and the same grid
                # 2. the form's order restated, bit for bit (the split ring walk: the bits it has without the option)
                if ref is None:
                    wf.set_option(KEY, 0)
                    wf.forward(b, bs)
                    assert same_bits(Rw, wf.fetch_interaction(bs)) and _tokens(wf) == tw, where
                    wf.set_option(KEY, 1)
                else:
                    assert same_bits(Rw[:, D:], ref[b][:bs]), where
                # 3. the split order's tolerance of the sequential chain
                worst = max(worst, float(np.abs(Rw[:, D:].astype(np.float64) - seq[b][:bs]).max()))
                assert H.close(Rw[:, D:], seq[b][:bs], rtol=1e-5, atol_scale=2e-6), (where, worst)
                # 4. weights of 1.0 / NULL: the unweighted bits;  6. the bottom MLP's columns
                assert same_bits(Ro, Ru), where
                assert same_bits(Rw[:, :D], Ru[:, :D]), where
        for jobs in (JOBS12, JOBS16):
            got_w, got_o, got_u = _run_set(wf, jobs), _run_set(on, jobs), _run_set(un, jobs)
            tw, tu = _tokens(wf, 1), _tokens(un, 1)
            if ref is None:
                wf.set_option(KEY, 0)
                assert all(same_bits(x, y) for x, y in zip(got_w, _run_set(wf, jobs))) and _tokens(wf, 1) == tw, (kind, n)
                wf.set_option(KEY, 1)
            assert len(tw) == 1 and tw[0].startswith(with_w), (kind, n, tw, with_w)
            assert len(tu) == 1 and tu[0].startswith(without), (kind, n, tu, without)
            for (b, q), Rw, Ro, Ru in zip(jobs, got_w, got_o, got_u):
                if not q:
                    continue
                where = (kind, shape_id(CATALOGUE[n]), len(jobs), b, q)
                assert ref is None or same_bits(Rw[:, D:], ref[b][:q]), where
                assert H.close(Rw[:, D:], seq[b][:q], rtol=1e-5, atol_scale=2e-6), where
                assert same_bits(Ro, Ru) and same_bits(Rw[:, :D], Ru[:, :D]), where
                if b == 2 and (b, q) in alone:                                 # 5. the unweighted query of a mixed set: its bits served alone
                    assert same_bits(Rw, alone[(b, q)]), where
        # the instances without the non-temporal hint: the same bits
        for b in range(2):
            wf.set_option("sls_nt", 1)
            wf.forward(b, B)
            R1 = wf.fetch_interaction(B).copy()
            wf.set_option("sls_nt", 0)
            wf.forward(b, B)
            tw = _tokens(wf)
            assert len(tw) == 1 and tw[0].startswith(log_token(form, 0, tag)), (kind, n, tw)
            assert same_bits(wf.fetch_interaction(B), R1), (kind, n, b, "sls_nt 0")
        if ref is None:                                                        # the sequential order: weighted_ref's bits
            wf.set_option("sls_exact", 1)
            for b in range(3):
                wf.forward(b, B)
                assert _tokens(wf)[0].startswith(log_token("ring %s,sequential" % form.split()[1].split(",")[0], 0, tag, weighted=b < 2))
                assert same_bits(wf.fetch_interaction(B)[:, D:], seq[b]), (kind, n, b, "sls_exact 1")
        print("worst |got - sequential| = %.3g (%s, %s, %s)" % (worst, kind, shape_id(CATALOGUE[n]), form))
    finally:
        for eng in (wf, on, un):
            eng.close()


# ------------------------------------------------------------------------------------------------------------------------
# 2. the dispatch log
def test_dispatch_log_of_the_option():
    D, Bq = 64, 64
    eng, tables, X, ix, ln, wt = _fixed(D, 20)
    try:
        eng.stage_batch(0, X, ix, ln)
        eng.forward(0, Bq)
        first = _log(eng)
        assert "sls_flatc_kernel<16,5,nt>[" in first, first
        eng.stage_batch_weights(0, wt)
        eng.forward(0, Bq)
        ring = _log(eng)
        assert "sls_kernel<16,sequential,w>[" in ring and "flat" not in ring, ring     # the default: the ring walk
        assert eng.get_option(KEY) == 0
        eng.set_option(KEY, 1)
        eng.forward(0, Bq)
        assert "sls_flatc_kernel<16,5,nt,w>[" in _log(eng) and "sls_kernel<" not in _log(eng), _log(eng)
        eng.set_option("sls_exact", 1)
        eng.forward(0, Bq)
        assert "sls_kernel<16,sequential,w>[" in _log(eng) and "flat" not in _log(eng), _log(eng)
        eng.set_option("sls_exact", 0)
        eng.set_option("table_dtype", N.TABLE_FP16)
        eng.forward(0, Bq)
        assert "sls_flatc_kernel<16,5,nt,f16,w>[" in _log(eng), _log(eng)
        eng.set_option("table_dtype", N.TABLE_FP32)
        eng.set_option(KEY, 0)
        eng.forward(0, Bq)
        assert _log(eng) == ring
        for bad in (2, -1):
            with pytest.raises(N.DrsError) as e:
                eng.set_option(KEY, bad)
            assert e.value.code == N.ERR_BAD_ARG and eng.get_option(KEY) == 0
        eng.set_option(KEY, 1)
        eng.stage_batch(0, X, ix, ln)                                          # staged again: unweighted again
        eng.forward(0, Bq)
        assert _log(eng) == first
    finally:
        eng.close()
    eng, tables, X, ix, ln, wt = _fixed(D, 1)
    try:
        eng.stage_batch(0, X, ix, ln)
        eng.forward(0, Bq)
        first = _log(eng)
        assert "sls_one_kernel<16,16>[" in first, first
        eng.stage_batch_weights(0, wt)
        eng.set_option(KEY, 1)
        eng.forward(0, Bq)
        assert "sls_one_kernel<16,16,w>[" in _log(eng) and "sls_kernel<" not in _log(eng), _log(eng)
        eng.set_option("sls_exact", 1)
        eng.forward(0, Bq)
        assert "sls_one_kernel<16,16,w>[" in _log(eng), _log(eng)                 # (the copy form is the sequential order)
        eng.set_option("table_dtype", N.TABLE_FP16)
        eng.forward(0, Bq)
        assert "sls_one_kernel<16,16,f16,w>[" in _log(eng), _log(eng)
        eng.set_option("table_dtype", N.TABLE_FP32)
        eng.set_option("sls_exact", 0)
        eng.set_option(KEY, 0)
        eng.forward(0, Bq)
        assert "sls_kernel<16,sequential,w>[" in _log(eng) and "sls_one_kernel" not in _log(eng), _log(eng)
        eng.set_option(KEY, 1)
        eng.stage_batch(0, X, ix, ln)
        eng.forward(0, Bq)
        assert _log(eng) == first
    finally:
        eng.close()
    eng, tables, X, ix, ln, wt = _fixed(10, 5)                                 # a width outside the 16-byte forms
    try:
        eng.set_option(KEY, 1)
        eng.stage_batch(0, X, ix, ln, weights=wt)
        eng.forward(0, Bq)
        assert "sls_any_kernel<w>[" in _log(eng), _log(eng)
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------------------------------
# 3. an out-of-range index
@pytest.mark.parametrize("L,token", [(20, "sls_flatc_kernel<16,5,nt,w>["), (1, "sls_one_kernel<16,16,w>[")])
def test_out_of_range_index_is_refused_and_the_next_good_call_keeps_its_bits(L, token):
    """Caffe2's ENFORCE.  Every path that hands indices to a weighted launch of these forms stages them, and staging checks
    the range on the host: the call returns ERR_INDEX_RANGE and the batch staged before is served with the bits it had.
    (The kernels' own flag, the unweighted forms' `bad` word unchanged, is the backstop behind that check.)"""
    D, Bq = 64, 64
    eng, tables, X, ix, ln, wt = _fixed(D, L)
    try:
        eng.set_option(KEY, 1)
        eng.stage_batch(0, X, ix, ln, weights=wt)
        eng.forward(0, Bq)
        assert token in _log(eng), _log(eng)
        R0 = eng.fetch_interaction(Bq).copy()
        bad = [i.copy() for i in ix]
        bad[1][5] = 5000                                                       # one past the table
        with pytest.raises(N.DrsError) as e:
            eng.stage_batch(0, X, bad, ln, weights=wt)
        assert e.value.code == N.ERR_INDEX_RANGE and eng.get_option("sls_weighted") == 1
        eng.forward(0, Bq)
        assert token in _log(eng) and same_bits(eng.fetch_interaction(Bq), R0)
    finally:
        eng.close()
