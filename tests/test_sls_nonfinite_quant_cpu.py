"""CPU side of poison rows in the quantized tables (tests/test_sls_nonfinite_quant.py runs the layout below on the GPU).

tests/test_sls_nonfinite_cpu.py covers the plain stored types.  The quantized ones have poison of their own:
  * fp8 e4m3 ("table_dtype" 4): e4m3fn has no infinity and two NaN codes; +-inf and NaN all quantize to them;
  * int8 / int4 rowwise ("table_dtype" 8 / 9): a FINITE fp32 row whose range overflows the header -- (max - min) above
    fp32's largest value for int8, (max - bias) / 15 above fp16's for int4 -- takes the scale +inf and the codes 0, as
    torch's embedding_bag_byte_prepack / embedding_bag_4bit_prepack write it, and decodes to inf * 0 = NaN in every column.
    torch's embedding_bag_*_rowwise_offsets pools NaN for a bag that names such a row (also with the weight 0 on it) and for
    no other bag.
The layout is tests/test_sls_nonfinite_cpu.py's (`_layout`: which bags name which of rows 0 .. 7, the weights, the empty
bags), with a poison table per kind; rows from 8 on are the clean table's.

What is pinned here:
  * the poison rows' bytes are torch's, and the class map of `class_ref` on the decoded table is the class map of torch's
    quantized operators, weighted and not;
  * the conditions that keep the GPU test from passing vacuously;
  * why a kernel may not mask a ROWWISE row by its weight: s = 0 * inf is NaN; the products are formed with the row's own
    weight and dropped afterwards.
"""
import functools

import numpy as np
import pytest

from tests.test_fp8_tables_cpu import fp8_decoded, fp8_exponent
from tests.test_int4_lines_cpu import rows_per_line as rows_per_line4
from tests.test_int4_tables_cpu import quantize_rows4
from tests.test_int8_lines_cpu import rows_per_line as rows_per_line8
from tests.test_int8_tables_cpu import quantize_rows
from tests.test_sls_nonfinite_cpu import (N_BATCHES, N_POISON, NAN, RAGGED, SHAPES, _layout, class_ref, classes, form_of, named_columns,
                                          nf_shape_id, poison_rows, seq_bits_ref, token_of)
from tests.test_sls_weights_cpu import (codes4, codes8, fma32, same_bits, torch_weighted_rowwise, weighted_ref_rowwise)
from tests.test_sls_weights_flat_cpu import B

QUANT_KINDS = ("fp8", "int8", "int8_lines", "int4", "int4_lines")
QTAG = {"fp8": "f8", "int8": "i8", "int8_lines": "i8l", "int4": "i4", "int4_lines": "i4l"}
CONTROL = 5                                       # the rowwise kinds' finite control row: an outlier just inside the header's range


def base_of(kind):
    return kind[:-len("_lines")] if kind.endswith("_lines") else kind


# ---- the poison layouts --------------------------------------------------------------------------------------------------------
def poison_rows_fp8(W):
    """poison_rows, but row 5's element is NaN instead of 1e5: a finite outlier would move the table's scale exponent
    (the absmax is taken over the finite elements) and with it every clean row's code"""
    poison_rows(W)
    W[5, 3] = NAN
    return W


def poison_rows_int8(W):
    """rows 0 .. 7, in place: +3e38 and -3e38 at two columns per row -- max - min = inf: scale +inf, every code 0; row 5
    (the control) +-1e38: the range 2e38 is finite"""
    D = W.shape[1]
    for r in range(N_POISON):
        v = np.float32(1e38 if r == CONTROL else 3e38)
        W[r, r], W[r, D - 1 - r] = v, -v
    return W


def poison_rows_int4(W):
    """rows 0 .. 7, in place: one element of 1e6, at column r -- (1e6 - bias) / 15 rounds to +inf in fp16: every code 0;
    row 5 (the control) 9.7e5: the scale 64672"""
    for r in range(N_POISON):
        W[r, r] = np.float32(9.7e5 if r == CONTROL else 1e6)
    return W


POISON = {"fp8": poison_rows_fp8, "int8": poison_rows_int8, "int4": poison_rows_int4}


def decode_rowwise(q, scale, bias):
    """each element's value as the kernels and torch form it: fmaf(scale, q, 0.0f + bias); inf * 0 is NaN"""
    with np.errstate(all="ignore"):
        return fma32(scale[:, None], q, (np.float32(0) + bias)[:, None])


def restated_codes(base, W):
    """(codes [rows, D] fp32, scale, bias) out of the numpy restatements quantize_rows / quantize_rows4"""
    D = W.shape[1]
    with np.errstate(all="ignore"):
        p = quantize_rows(W) if base == "int8" else quantize_rows4(W)
    if base == "int8":
        return p[:, :D].astype(np.float32), p[:, D:D + 4].copy().view(np.float32)[:, 0], p[:, D + 4:D + 8].copy().view(np.float32)[:, 0]
    h = D // 2
    q = np.empty((p.shape[0], D), np.float32)
    q[:, 0::2] = p[:, :h] & 15
    q[:, 1::2] = p[:, :h] >> 4
    return (q, p[:, h:h + 2].copy().view(np.float16).astype(np.float32)[:, 0],
            p[:, h + 2:h + 4].copy().view(np.float16).astype(np.float32)[:, 0])


def lines_pack(kind, D):
    """does the line-packed layout of a `_lines` kind differ from its plain twin's at this D (n >= 1 rows to a line)?"""
    return bool((rows_per_line8 if kind == "int8_lines" else rows_per_line4)(D, 1))


def shapes_of(kind):
    """the SHAPES entries a kind runs on: all of them, but for the `_lines` kinds those whose layout really packs"""
    ns = range(len(SHAPES))
    return [n for n in ns if lines_pack(kind, SHAPES[n][0])] if kind.endswith("_lines") else list(ns)


@functools.lru_cache(maxsize=None)
def _qcase(n, base):
    lay = _layout(n)
    c = dict(lay)
    T = len(c["rows"])
    c["poisoned"] = [POISON[base](W.copy()) for W in lay["clean"]]
    if base == "fp8":
        c["codes"] = None
        c["stored"] = [fp8_decoded(W)[0] for W in c["poisoned"]]
    else:
        with np.errstate(all="ignore"):
            c["codes"] = [(codes8 if base == "int8" else codes4)(W)[1:] for W in c["poisoned"]]
        c["stored"] = [decode_rowwise(*qsb) for qsb in c["codes"]]
    for a in c["poisoned"]:
        a.setflags(write=False)
    c["cls"], c["seq"] = {}, {}
    for mode in ("sum", "mean", "w"):
        cls, seq = [], []
        for b in range(N_BATCHES):
            cl, sq = [], []
            for t in range(T):
                idx, lens = c["idx"][b][t], c["lens"][b][t]
                w = c["wts"][b][t] if mode == "w" else None
                cl.append(class_ref(c["stored"][t], idx, lens, w, mode == "mean"))
                if base == "fp8":
                    sq.append(seq_bits_ref(c["stored"][t], idx, lens, w, mode == "mean"))
                else:
                    with np.errstate(all="ignore"):
                        s = weighted_ref_rowwise(*c["codes"][t], idx, lens, np.ones(idx.size, np.float32) if w is None else w)
                        if mode == "mean":
                            s = s / np.maximum(np.asarray(lens), 1).astype(np.float32)[:, None]
                    assert s.dtype == np.float32
                    sq.append(s)
            cls.append(np.concatenate(cl, axis=1))
            seq.append(np.concatenate(sq, axis=1))
        c["cls"][mode], c["seq"][mode] = cls, seq
        for a in cls + seq:
            a.setflags(write=False)
    return c


def quant_case(shape, kind):
    """tests/test_sls_nonfinite_cpu.poison_case for a quantized kind: `poisoned` are the kind's fp32 poison tables (what
    set_table takes), `stored` their decoded values, `codes` (rowwise kinds) torch's (codes, scale, bias) per table;
    cls / seq as there -- seq is weighted_ref_rowwise on the codes for the rowwise kinds"""
    return _qcase(SHAPES.index(shape), base_of(kind))


# ---- 1. the checker against torch -----------------------------------------------------------------------------------------------
def test_tokens_carry_the_kinds_tags():
    assert [QTAG[k] for k in QUANT_KINDS] == ["f8", "i8", "i8l", "i4", "i4l"]
    assert token_of("flatc 16,5", 1, QTAG["fp8"], "w") == "sls_flatc_kernel<16,5,nt,f8,w>["
    assert token_of("ring 16,split", 1, QTAG["int8_lines"], "mean") == "sls_kernel<16,split,nt,i8l,mean>["
    assert token_of("one 8,16", 1, QTAG["int4"], "sum") == "sls_one_kernel<8,16,i4>["
    assert token_of("any", 1, QTAG["int4_lines"], "w") == "sls_any_kernel<i4l,w>["
    assert token_of("flat 8,5,bpw2", 0, QTAG["int8"], "w") == "sls_flat_kernel<8,5,bpw2,i8,w>["


@pytest.mark.parametrize("D", [16, 64])
@pytest.mark.parametrize("base", ["int8", "int4"])
def test_rowwise_poison_rows_are_torchs_bytes_and_decode_to_nan(base, D):
    import torch
    rng = np.random.RandomState(D)
    W = POISON[base](rng.uniform(-1, 1, (32, D)).astype(np.float32))
    assert np.all(np.isfinite(W))                                              # finite fp32 input throughout
    op = torch.ops.quantized.embedding_bag_byte_prepack if base == "int8" else torch.ops.quantized.embedding_bag_4bit_prepack
    ref = op(torch.from_numpy(W)).numpy()
    with np.errstate(all="ignore"):
        mine = quantize_rows(W) if base == "int8" else quantize_rows4(W)
    assert np.array_equal(mine, ref)
    q, s, b = restated_codes(base, W)
    tq, ts, tb = (codes8 if base == "int8" else codes4)(W)[1:]
    assert np.array_equal(q, tq) and same_bits(s, ts) and same_bits(b, tb)
    dec = decode_rowwise(q, s, b)
    for r in range(N_POISON):
        if r == CONTROL:
            assert np.isfinite(s[r]) and np.all(np.isfinite(dec[r])), r
            assert s[r] == (np.float32(64672) if base == "int4" else np.float32(np.float32(2e38) / np.float32(255))), s[r]
        else:
            assert np.isposinf(s[r]) and np.isfinite(b[r]) and not np.any(q[r]) and np.all(np.isnan(dec[r])), r
    assert np.all(np.isfinite(dec[N_POISON:])) and np.all(np.isfinite(s[N_POISON:]))


def _ragged_n():
    return SHAPES.index((64, 3, RAGGED, {}))


@pytest.mark.parametrize("base", ["int8", "int4"])
def test_rowwise_class_map_is_torchs(base):
    """one ragged case: class_ref on the decoded table against embedding_bag_*_rowwise_offsets, with per_sample_weights
    (the weight 0 and a negative weight on a poison row among them) and without; finite elements: torch's bits"""
    c = _qcase(_ragged_n(), base)
    bits = 8 if base == "int8" else 4
    for b in range(N_BATCHES):
        hot_w = np.concatenate([c["wts"][b][t][(c["idx"][b][t] < N_POISON) & (c["idx"][b][t] != CONTROL)] for t in range(len(c["rows"]))])
        assert np.any(hot_w == 0) and np.any(hot_w < 0) and np.any(hot_w > 0)
        for t in range(len(c["rows"])):
            idx, lens, w = c["idx"][b][t], c["lens"][b][t], c["wts"][b][t]
            with np.errstate(all="ignore"):
                P = (codes8 if base == "int8" else codes4)(c["poisoned"][t].copy())[0]
                tw = torch_weighted_rowwise(P, idx, lens, w, bits)
                tu = torch_weighted_rowwise(P, idx, lens, np.ones(idx.size, np.float32), bits)
            D = c["shape"][0]
            for mode, got in (("w", tw), ("sum", tu)):
                cref = c["cls"][mode][b][:, t * D:(t + 1) * D]
                sref = c["seq"][mode][b][:, t * D:(t + 1) * D]
                assert np.array_equal(classes(cref), classes(got)), (base, mode, b, t)
                assert np.array_equal(classes(sref), classes(got)), (base, mode, b, t)
                fin = classes(got) == 0
                assert fin.any() and np.array_equal(sref[fin].view(np.uint32), got[fin].view(np.uint32)), (base, mode, b, t)
                assert set(np.unique(classes(got))) == {0, 3}                  # a rowwise poison row is all NaN: no +-inf class


@pytest.mark.parametrize("D", [10, 16, 64])
def test_fp8_decoded_poison_table_is_torchs_round_trip(D):
    import torch
    rng = np.random.RandomState(D)
    W = rng.uniform(-1, 1, (64, D)).astype(np.float32)
    P = poison_rows_fp8(W.copy())
    dec, k = fp8_decoded(P)
    fin = np.abs(P[np.isfinite(P)])
    assert k == fp8_exponent(fin.max()) == fp8_exponent(np.abs(W[N_POISON:]).max())
    with np.errstate(all="ignore"):
        rt = torch.from_numpy(P * np.float32(2.0 ** k)).to(torch.float8_e4m3fn).to(torch.float32).numpy() * np.float32(2.0 ** -k)
    assert np.array_equal(np.isnan(dec), np.isnan(rt)) and np.array_equal(np.isnan(dec), ~np.isfinite(P))   # every inf became NaN
    assert same_bits(np.nan_to_num(dec), np.nan_to_num(rt))
    assert same_bits(dec[N_POISON:], fp8_decoded(W)[0][N_POISON:])


# ---- 2. why the weight may not mask a rowwise row -------------------------------------------------------------------------------
def addw_restated(acc, keep, w, scale, bias, q, select_after):
    """I8::addw / I4::addw on one row: select_after False -- the weight is masked (w = keep ? w : 0) before the two products;
    True -- the products are formed with the row's own weight and dropped afterwards"""
    w, scale, bias, zero = np.float32(w), np.float32(scale), np.float32(bias), np.float32(0)
    with np.errstate(all="ignore"):
        if select_after:
            s = np.float32(w * scale) if keep else zero
            b = np.float32(w * bias) if keep else zero
        else:
            w = w if keep else zero
            s, b = np.float32(w * scale), np.float32(w * bias)
        return fma32(s, q, (acc + b).astype(np.float32))


def test_a_masked_weight_does_not_mask_a_rowwise_row_whose_scale_overflowed():
    acc = np.array([0.0, 1.5, -2.25, 1e-40], np.float32)
    q0, inf = np.zeros(4, np.float32), np.float32(np.inf)
    # the parent's form: 0 * inf is NaN, and fma(NaN, 0, acc + b) with it
    assert np.all(np.isnan(addw_restated(acc, False, 0.75, inf, -0.5, q0, select_after=False)))
    assert np.all(np.isnan(addw_restated(acc, False, 0.75, 3.0, -inf, q0, select_after=False)))      # ... and an infinite bias
    # the kept form: acc's bits, whatever the header holds
    for scale, bias in ((inf, -0.5), (3.0, -inf), (np.float32(np.nan), np.float32(np.nan)), (0.25, -1.0)):
        for w in (0.75, 0.0, -0.5):
            assert same_bits(addw_restated(acc, False, w, scale, bias, q0 + 7, select_after=True), acc), (scale, bias, w)
    # a row that counts is NaN under both forms, also with the weight 0 on it (torch's class)
    for w in (0.75, 0.0, -0.5):
        for after in (False, True):
            assert np.all(np.isnan(addw_restated(acc, True, w, inf, -0.5, q0, select_after=after))), (w, after)
    # finite headers: a kept row has the same bits under both forms, and a masked row adds nothing under either
    rng = np.random.RandomState(3)
    q = rng.randint(0, 256, 4).astype(np.float32)
    for w in (0.75, 0.0, -0.5, 1.0):
        for s, b in ((0.0039, -0.9), (7.8e35, -1e38), (64672.0, -1.0)):
            assert same_bits(addw_restated(acc, True, w, s, b, q, False), addw_restated(acc, True, w, s, b, q, True))
            assert same_bits(addw_restated(acc, False, w, s, b, q, False), acc) and same_bits(addw_restated(acc, False, w, s, b, q, True), acc)


# ---- 3. the layout is not vacuous -----------------------------------------------------------------------------------------------
def test_the_lines_kinds_run_on_shapes_that_pack_in_every_form():
    assert [D for D in (64, 32, 24, 128, 16, 10) if lines_pack("int8_lines", D)] == [64, 32, 16, 10]
    assert [D for D in (64, 32, 24, 128, 16, 10) if lines_pack("int4_lines", D)] == [64, 32, 128, 16, 10]
    for kind in ("int8_lines", "int4_lines"):
        forms = {form_of(SHAPES[n], (B,)).split(" ")[0] for n in shapes_of(kind)}
        assert {"ring", "flat", "flatc", "one", "any"} <= forms, (kind, forms)
        weighted_default = {form_of(SHAPES[n], (B,), weighted_default=True) for n in shapes_of(kind)}
        assert {"ring 16,split", "ring 16,sequential", "ring 8,sequential"} <= weighted_default, (kind, weighted_default)
    for kind in ("fp8", "int8", "int4"):
        assert shapes_of(kind) == list(range(len(SHAPES)))
    assert all(s[0] % 2 == 0 for s in SHAPES)                                   # int4 takes even widths only


@pytest.mark.parametrize("n", range(len(SHAPES)), ids=[nf_shape_id(s) for s in SHAPES])
def test_the_quantized_poison_layouts_cannot_pass_vacuously(n):
    shape = SHAPES[n]
    D, T, L, opts = shape
    lay = _layout(n)
    for base in ("fp8", "int8", "int4"):
        c = _qcase(n, base)
        for t in range(T):
            W, P, st = lay["clean"][t], c["poisoned"][t], c["stored"][t]
            assert same_bits(W[N_POISON:], P[N_POISON:]) and np.all(np.isfinite(st[N_POISON:])), (base, t)
            if base == "fp8":
                assert fp8_exponent(np.abs(W).max()) == fp8_decoded(W)[1] == fp8_decoded(P)[1], t      # the clean rows keep their codes
                assert same_bits(st[N_POISON:], fp8_decoded(W)[0][N_POISON:])
                assert np.all(np.isnan(st[:N_POISON]).any(axis=1)) and np.all(np.isnan(st[0]))          # a NaN code in every poison row
                assert not np.any(np.isinf(st))                                 # e4m3fn has no infinity
            else:
                assert np.all(np.isfinite(P))                                   # finite fp32 input
                q, s, b = c["codes"][t]
                rq, rs, rb = restated_codes(base, P)
                assert np.array_equal(q, rq) and same_bits(s, rs) and same_bits(b, rb), (base, t)   # torch's bytes are the restated ones
                hot = [r for r in range(N_POISON) if r != CONTROL]
                assert np.all(np.isposinf(rs[hot])) and np.all(np.isnan(st[hot])), (base, t)
                assert np.isfinite(rs[CONTROL]) and np.all(np.isfinite(st[CONTROL])), (base, t)
                clean_codes = (codes8 if base == "int8" else codes4)(W.copy())[1:]
                assert all(same_bits(x[N_POISON:], y[N_POISON:]) for x, y in zip(c["codes"][t], clean_codes))
        for b in range(N_BATCHES):
            idx, lens, wts, named = lay["idx"][b], lay["lens"][b], lay["wts"][b], lay["named"][b]
            offs = [np.concatenate([[0], np.cumsum(ln)]).astype(np.int64) for ln in lens]
            nan_rows = [r for r in range(1, N_POISON) if base == "fp8" or r != CONTROL]
            poisoned_bags = zero_w = control = 0
            really = np.zeros((T, B), bool)                                    # bags that name a row with a NaN in it
            for t in range(T):
                assert not np.any(idx[t] == 0)                                  # no bag names row 0
                for s in np.nonzero(named[t])[0]:
                    r, w = idx[t][offs[t][s]:offs[t][s + 1]], wts[t][offs[t][s]:offs[t][s + 1]]
                    really[t, s] = np.any(np.isin(r, nan_rows))
                    poisoned_bags += int(really[t, s])
                    zero_w += int(np.any((w == 0) & np.isin(r, nan_rows)))
                    control += int(CONTROL in r and not really[t, s])
            assert poisoned_bags >= 8 and zero_w >= 1 and (control >= 1 or base == "fp8"), (base, b, poisoned_bags, zero_w, control)
            if not isinstance(L, int):                                         # an empty bag directly beside a poisoned one
                assert any(lens[t][s] == 0 and (really[t, s - 1] or really[t, s + 1]) for t in range(T) for s in range(1, B - 1)), (base, b)
            hot = named_columns(named, D, B)
            really_cols = named_columns(really, D, B)
            for mode in ("sum", "mean", "w"):
                cls, seq = classes(c["cls"][mode][b]), classes(c["seq"][mode][b])
                assert np.array_equal(cls, seq), (base, mode, b)
                assert not np.any(cls[~hot]), (base, mode, b)                   # poison stays in the bags that name it
                assert np.any(cls[really_cols] == 3) and np.any(cls[hot] == 0), (base, mode, b)
                if base != "fp8":
                    assert np.all(cls[really_cols] == 3) and not np.any(cls[~really_cols]), (base, mode, b)   # all NaN, control finite
                    assert np.any(np.abs(c["cls"][mode][b][hot & ~really_cols]) > 1e3)                # ... and it is there
            # nothing finite overflows fp32: the rowwise control row's elements are at most 1e38 and a bag names it once
            fin = c["seq"]["w"][b][classes(c["seq"]["w"][b]) == 0]
            assert np.abs(fin).max() < (1e6 if base == "fp8" else 2e38)
