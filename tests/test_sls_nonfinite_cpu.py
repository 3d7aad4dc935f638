"""CPU side of inf and NaN table rows in the gather (tests/test_sls_nonfinite.py runs the layout below on the GPU).

The gather kernels keep control flow wave-uniform by loading rows a bag does not own -- a short bag's last row again, row 0
for an empty bag, the rows of the wave's other bags, row R - 1 past the wave's rows -- and making them count for nothing.
A non-finite element of a plain table (fp32 / fp16 / bf16: "NaN stays NaN, overflow gives +-inf") must therefore reach
the bags that name its row, as torch's operators propagate it, and no other bag.

What is pinned here:
  * the checker: `classes` (0 finite, 1 +inf, 2 -inf, 3 NaN) of `class_ref` (the float64 sum of w * row per bag) is the
    class map of torch's CPU embedding_bag and of tests/test_sls_weights_cpu.weighted_ref, whose finite elements are
    torch's bits.  With finite weights and no overflow the class of a sum does not depend on its order, so the one
    reference serves every gather form;
  * why a kernel may not mask a row by its weight: fma(0, x, acc) is acc for a finite x only;
  * the poison layout `poison_case` the GPU test runs, and the conditions that keep that test from passing vacuously.
"""
import functools
import zlib

import numpy as np
import pytest

from tests import gather_shapes as GS
from tests.test_half_tables import upcast
from tests.test_sls_weights_cpu import fma32, same_bits, torch_weighted, weighted_ref
from tests.test_sls_weights_flat_cpu import B, CATALOGUE, expected_form, log_token, rows_of, shape_id

INF = np.float32(np.inf)
NAN = np.float32(np.nan)
N_POISON = 8                                      # rows 0 .. 7 of every table: row 0 all NaN (no bag names it), 1 .. 7 poison rows
KINDS = ("fp32", "fp16", "bf16")                  # the plain stored types: non-finite elements are inside their contract
RAGGED, RAGGED4 = "ragged", "ragged4"             # lengths 0 .. 11 / 0 .. 4, empty bags planted

# the shapes beside the catalogue: the sequential ring walk whose bags end inside a ring round (L % 4 != 0), the ragged
# ring walk in both orders (sequential: an empty bag shares its wave with longer ones) and the any-width form
EXTRA = [
    (64, 3, 5, {"sls_exact": 1}),                 # ring 16,sequential: four bags per wave, one round and a quarter
    (32, 3, 3, {"sls_exact": 1}),                 # ring 8,sequential: eight bags per wave, less than one round
    (64, 3, RAGGED, {}),                          # ring 16,split: a wave per bag
    (64, 3, RAGGED, {"sls_exact": 1}),            # ring 16,sequential: empty, short and long bags in one wave
    (10, 3, RAGGED4, {}),                         # any
]
SHAPES = list(CATALOGUE) + EXTRA


def nf_shape_id(shape):
    D, T, L, opts = shape
    return shape_id(shape) if isinstance(L, int) else "D%d-T%d-%s%s" % (D, T, L, "".join("-%s%d" % kv for kv in sorted(opts.items())))


# ---- the checker ---------------------------------------------------------------------------------------------------------------
def classes(a):
    """0 finite, 1 +inf, 2 -inf, 3 NaN, elementwise"""
    a = np.asarray(a)
    c = np.zeros(a.shape, np.int8)
    c[np.isposinf(a)] = 1
    c[np.isneginf(a)] = 2
    c[np.isnan(a)] = 3
    return c


def class_ref(stored, idx, lens, w, mean=False):
    """[bags, D] float64: per bag the sum of w * row over its indices (w None: 1), divided by its length under `mean`;
    an empty bag is +0"""
    stored = np.asarray(stored, np.float64)
    idx, lens = np.asarray(idx, np.int64), np.asarray(lens, np.int64)
    w = np.ones(idx.size) if w is None else np.asarray(w, np.float64)
    bag = np.repeat(np.arange(lens.size), lens)
    out = np.zeros((lens.size, stored.shape[1]), np.float64)
    with np.errstate(all="ignore"):
        np.add.at(out, bag, w[:, None] * stored[idx])
        if mean:
            out = out / np.maximum(lens, 1)[:, None]
    return out


def seq_bits_ref(stored, idx, lens, w, mean=False):
    """[bags, D] fp32: the sequential chain (weighted_ref; w None: weights of 1.0, i.e. plain additions), under `mean`
    divided by the length with one fp32 division -- the bits of the sequential, one-lookup and any-width forms"""
    idx = np.asarray(idx, np.int64)
    with np.errstate(all="ignore"):
        out = weighted_ref(stored, idx, lens, np.ones(idx.size, np.float32) if w is None else w)
        if mean:
            out = out / np.maximum(np.asarray(lens), 1).astype(np.float32)[:, None]
    assert out.dtype == np.float32
    return out


def stored_plain(kind, W):
    return np.ascontiguousarray(W, np.float32) if kind == "fp32" else upcast(W, kind)


def close_finite(got, ref, rtol=1e-5, atol_scale=2e-6):
    """tests/helpers.close on the elements whose reference is finite: the floor is taken over those only"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    fin = np.isfinite(ref)
    if not fin.any():
        return True
    g, r = got[fin], ref[fin]
    return bool(np.all(np.abs(g - r) <= atol_scale * np.abs(r).max() + rtol * np.abs(r)))


# ---- the poison layout -----------------------------------------------------------------------------------------------------------
def poison_rows(W):
    """rows 0 .. 7 of the uniform table W, in place: row 0 all NaN; one column +inf, the same column -inf, one NaN element,
    a whole row of +inf, one element 1e5 (+inf in fp16 only), -inf in another column, +inf in the last column"""
    D = W.shape[1]
    c = 1
    W[0] = NAN
    W[1, c] = INF
    W[2, c] = -INF
    W[3, 2] = NAN
    W[4] = INF
    W[5, 3] = np.float32(1e5)
    W[6, D - 2] = -INF
    W[7, D - 1] = INF
    return W


# what a poisoned bag holds: (first row or None, its weight or None, last row, its weight or None); None: as drawn.
# A bag of one row takes the last row only.
RECIPES = [
    (None, None, 1, None),                        # +inf row last in the bag
    (None, None, 2, None),                        # -inf row last
    (None, None, 3, None),                        # a NaN element
    (1, None, 2, None),                           # +inf and -inf meet in one column: NaN
    (None, None, 1, 0.0),                         # weight 0 on an inf row: NaN, as torch has it
    (None, None, 2, -0.5),                        # a negative weight on a -inf row: +inf
    (None, None, 4, None),                        # a whole row of +inf
    (None, None, 5, None),                        # 1e5: finite but in fp16
    (6, None, 7, None),                           # -inf and +inf in different columns
    (None, None, 7, None),
    (None, None, 1, -0.25),                       # a negative weight on a +inf row: -inf
    (3, None, 4, 0.0),                            # NaN first, then weight 0 on a whole row of +inf
]
N_BATCHES = 2                                     # staged batches 0 and 1 differ; batch 2 is batch 0 again


def lengths_of(shape, rng, T):
    D, Tn, L, opts = shape
    if isinstance(L, int):
        return [np.full(B, L, np.int32) for _ in range(T)]
    hi = 12 if L == RAGGED else 5
    lens = [rng.randint(0, hi, size=B).astype(np.int32) for _ in range(T)]
    for t in range(T):
        lens[t][[1, 14, 23, B - 1]] = 0               # empty bags ...
        lens[t][[13, 22]] = hi - 1                # ... directly between two bags of hi - 1 (ragged: 11) rows
        lens[t][[15, 24]] = hi - 1
    return lens


def _build(shape):
    D, T, L, opts = shape
    rows = rows_of(T)
    rng = np.random.RandomState(zlib_seed(shape))
    clean = [rng.uniform(-1, 1, (r, D)).astype(np.float32) for r in rows]
    poisoned = [poison_rows(W.copy()) for W in clean]
    idx, lens, wts, named = [], [], [], []
    for b in range(N_BATCHES):
        ln = lengths_of(shape, rng, T)
        hot = np.zeros((T, B), bool)                  # bags that name a poison row
        plan = {}
        for k, s in enumerate(range(b, B, 3)):        # every third sample, one table of it: the neighbours stay clean
            if k >= len(RECIPES) + 4:
                break
            t = k % T
            plan[(t, s)] = RECIPES[k % len(RECIPES)]
            hot[t, s] = True
            if not isinstance(L, int):
                ln[t][s] = max(int(ln[t][s]), 2 + k % 4)      # (a poisoned bag is not empty; 2 .. 5 rows at least)
        ix, wt = [], []
        for t in range(T):
            off = np.concatenate([[0], np.cumsum(ln[t])]).astype(np.int64)
            i_t = rng.randint(N_POISON, rows[t], size=int(off[-1])).astype(np.int64)   # ordinary indices: [8, rows)
            w_t = rng.uniform(0.1, 1, size=int(off[-1])).astype(np.float32)
            for (tt, s), (r0, w0, r1, w1) in plan.items():
                if tt != t:
                    continue
                first, last = off[s], off[s + 1] - 1
                if r0 is not None and last > first:
                    i_t[first] = r0
                    if w0 is not None:
                        w_t[first] = w0
                i_t[last] = r1
                if w1 is not None:
                    w_t[last] = w1
            ix.append(i_t)
            wt.append(w_t)
        idx.append(ix)
        lens.append(ln)
        wts.append(wt)
        named.append(hot)
    for a in clean + poisoned:
        a.setflags(write=False)
    return dict(shape=shape, rows=rows, clean=clean, poisoned=poisoned, idx=idx, lens=lens, wts=wts, named=named)


def zlib_seed(shape):
    return zlib.crc32(nf_shape_id(shape).encode()) & 0x7FFFFFFF


@functools.lru_cache(maxsize=None)
def _layout(n):
    return _build(SHAPES[n])


@functools.lru_cache(maxsize=None)
def _case(n, kind):
    c = dict(_layout(n))
    T = len(c["rows"])
    c["stored"] = [stored_plain(kind, W) for W in c["poisoned"]]
    # per mode: [batch] -> [B, T * D]; "cls" float64 (the class map), "seq" fp32 (the sequential chain's bits)
    c["cls"], c["seq"] = {}, {}
    for mode in ("sum", "mean", "w"):
        w = (lambda b, t: c["wts"][b][t]) if mode == "w" else (lambda b, t: None)
        c["cls"][mode] = [np.concatenate([class_ref(c["stored"][t], c["idx"][b][t], c["lens"][b][t], w(b, t), mode == "mean")
                                          for t in range(T)], axis=1) for b in range(N_BATCHES)]
        c["seq"][mode] = [np.concatenate([seq_bits_ref(c["stored"][t], c["idx"][b][t], c["lens"][b][t], w(b, t), mode == "mean")
                                          for t in range(T)], axis=1) for b in range(N_BATCHES)]
        for a in c["cls"][mode] + c["seq"][mode]:
            a.setflags(write=False)
    return c


def poison_case(shape, kind):
    """The layout of SHAPES entry `shape` for the stored type `kind`, computed once and shared:
      rows, clean / poisoned: the fp32 tables (they differ in rows 0 .. 7 only), stored: what the poisoned engine holds, upcast
      idx, lens, wts: [batch][table]; named: [batch] -> bool [T, B], the bags that name a poison row
      cls / seq: [mode in sum | mean | w][batch] -> [B, T * D], class_ref and seq_bits_ref of the poisoned tables"""
    return _case(SHAPES.index(shape), kind)


def named_columns(named_b, D, bs):
    """bool [bs, T * D]: the pooled columns of the bags that name a poison row"""
    return np.repeat(named_b[:, :bs].T, D, axis=1)


# ---- the forms a case must show -----------------------------------------------------------------------------------------------
def form_of(shape, sizes, weighted_default=False):
    """the form (tests/gather_shapes.py's shorthand) of a launch set of this shape; weighted_default: a weighted set under
    "sls_weighted_flat" 0, which takes neither the flat nor the one-lookup forms"""
    D, T, L, opts = shape
    if D % 4:
        return "any"
    o = dict(opts)
    if weighted_default:
        o.update(sls_flat=0, sls_one=0)
    Lq = L if isinstance(L, int) else GS.RAGGED
    case = GS.Case(nf_shape_id(shape), "sls", D, T, (), (), (Lq,) * len(sizes), tuple(sizes), tuple(sorted(o.items())), 0, "", "at",
                   "", (), (), None, "")
    return GS.expected_gather_form(case)


def token_of(form, nt, dtype_tag, mode):
    """the dispatch-log token's prefix of `form` for a run of mode sum | mean | w"""
    tags = ",".join(x for x in (dtype_tag, "mean" if mode == "mean" else "", "w" if mode == "w" else "") if x)
    if form == "any":
        return "sls_any_kernel%s[" % ("<%s>" % tags if tags else "")
    return log_token(form, nt, tags, weighted=False)


def sequential_order(form):
    """does the form sum a bag in index order (the bits of seq_bits_ref)?"""
    return form == "any" or form.startswith("one ") or form.endswith("sequential")


# ---- 1. the checker ------------------------------------------------------------------------------------------------------------
def _small_poisoned(D):
    rng = np.random.RandomState(D)
    W = poison_rows(rng.uniform(-1, 1, (64, D)).astype(np.float32))
    c = 1
    bags = [([20, 31, 1], [.5, .7, .3]),          # a +inf row last in the bag
            ([2, 40], [.9, .2]),                  # a -inf row
            ([12, 3, 13], [.4, .6, .8]),          # a NaN element
            ([1, 22, 2], [.5, .5, .5]),           # +inf and -inf meet in one column
            ([30, 1], [.3, 0.0]),                 # weight 0 on an inf row
            ([2, 33], [-.5, .4]),                 # a negative weight on an inf row
            ([], []),                             # an empty bag
            ([4], [.25]), ([5, 9], [1.0, .5]), ([6, 7], [.2, .3]), ([44, 45, 46, 47], [.1, .2, .3, .4])]
    idx = np.array([i for b, _ in bags for i in b], np.int64)
    w = np.array([x for _, ws in bags for x in ws], np.float32)
    lens = np.array([len(b) for b, _ in bags], np.int32)
    return W, idx, lens, w, c


@pytest.mark.parametrize("D", [8, 10, 32, 64, 128])
def test_class_map_is_torchs_and_the_sequential_chains(D):
    import torch
    import torch.nn.functional as F
    W, idx, lens, w, c = _small_poisoned(D)
    with np.errstate(all="ignore"):
        tw = torch_weighted(W, idx, lens, w)
        off = np.concatenate([[0], np.cumsum(lens)])[:-1].astype(np.int64)
        tm = F.embedding_bag(torch.from_numpy(idx), torch.from_numpy(W), torch.from_numpy(off), mode="mean").numpy()
        ts = F.embedding_bag(torch.from_numpy(idx), torch.from_numpy(W), torch.from_numpy(off), mode="sum").numpy()
    ones = np.ones(idx.size, np.float32)
    for name, t, cref, sref in (("w", tw, class_ref(W, idx, lens, w), seq_bits_ref(W, idx, lens, w)),
                                ("sum", ts, class_ref(W, idx, lens, None), seq_bits_ref(W, idx, lens, None)),
                                ("mean", tm, class_ref(W, idx, lens, None, mean=True), seq_bits_ref(W, idx, lens, None, mean=True))):
        assert np.array_equal(classes(cref), classes(t)), (D, name)
        assert np.array_equal(classes(cref), classes(sref)), (D, name)
        fin = classes(t) == 0
        assert fin.any() and np.array_equal(sref[fin].view(np.uint32), t[fin].view(np.uint32)), (D, name)
    assert same_bits(seq_bits_ref(W, idx, lens, ones), seq_bits_ref(W, idx, lens, None))
    # the planted cases read as intended (weighted sum, column c)
    cw = classes(class_ref(W, idx, lens, w))
    assert [int(cw[k, c]) for k in range(7)] == [1, 2, 0, 3, 3, 1, 0]
    assert cw[2, 2] == 3 and np.all(cw[7] == 1) and not np.any(cw[6]) and not np.any(cw[10])
    assert not np.any(class_ref(W, idx, lens, w)[6].view(np.uint64))           # the empty bag: +0


def test_a_weight_of_zero_does_not_mask_a_non_finite_row():
    """fma(0, x, acc) has acc's bits for a finite x (tests/test_sls_weights_flat_cpu.py pins it) and is NaN for x in
    {+inf, -inf, NaN}: a kernel that loads a row it does not own must drop the VALUE, not the weight"""
    acc = np.array([0.0, 1.5, -2.25, 1e-40], np.float32)
    zero = np.float32(0)
    with np.errstate(all="ignore"):
        assert same_bits(fma32(zero, np.float32(0.75), acc), acc)
        for x in (INF, -INF, NAN):
            assert np.all(np.isnan(fma32(zero, x, acc))), x
        # the kept form: the value is zeroed and the weight may be anything finite
        for wv in (0.0, 1.0, -0.5, 3e38):
            assert same_bits(fma32(np.float32(wv), zero, acc), acc), wv


# ---- 2. the layout is not vacuous ----------------------------------------------------------------------------------------------
def test_the_shapes_take_the_forms_they_stand_for():
    assert len(SHAPES) == 27
    want = ["ring 16,sequential", "ring 8,sequential", "ring 16,split", "ring 16,sequential", "any"]
    for shape, form in zip(EXTRA, want):
        for sizes in ((B,), (1,), (29,), (B, 1, 29) * 3):
            assert form_of(shape, sizes) == form, (shape, sizes)
            assert form_of(shape, sizes, weighted_default=True) == form, (shape, sizes)
    for shape in CATALOGUE:
        assert form_of(shape, (B,)) == expected_form(shape)
        assert form_of(shape, (B,), weighted_default=True).startswith("ring "), shape
    assert token_of("any", 1, "", "w") == "sls_any_kernel<w>[" and token_of("any", 1, "f16", "sum") == "sls_any_kernel<f16>["
    assert token_of("any", 0, "", "sum") == "sls_any_kernel["
    assert token_of("flatc 16,5", 1, "bf16", "mean") == "sls_flatc_kernel<16,5,nt,bf16,mean>["
    assert token_of("ring 16,sequential", 1, "", "w") == "sls_kernel<16,sequential,w>["
    assert token_of("one 8,16", 1, "", "sum") == "sls_one_kernel<8,16>["
    assert sequential_order("one 8,16") and sequential_order("any") and not sequential_order("flat 8,5,bpw2")


@pytest.mark.parametrize("n", range(len(SHAPES)), ids=[nf_shape_id(s) for s in SHAPES])
def test_the_poison_layout_cannot_pass_vacuously(n):
    shape = SHAPES[n]
    D, T, L, opts = shape
    lay = _layout(n)
    for W, P in zip(lay["clean"], lay["poisoned"]):
        assert np.all(np.isnan(P[0])) and np.all(np.isfinite(W))               # row 0: all NaN; the clean twin: finite
        assert same_bits(W[N_POISON:], P[N_POISON:]) and not np.all(np.isfinite(P[1:N_POISON]).all(axis=1))
        assert np.all(np.isfinite(P[N_POISON:]))
    for b in range(N_BATCHES):
        idx, lens, wts, named = lay["idx"][b], lay["lens"][b], lay["wts"][b], lay["named"][b]
        offs = [np.concatenate([[0], np.cumsum(ln)]).astype(np.int64) for ln in lens]
        bag_rows = lambda t, s: idx[t][offs[t][s]:offs[t][s + 1]]
        bag_wts = lambda t, s: wts[t][offs[t][s]:offs[t][s + 1]]
        both = zero_w = neg_w = 0
        for t in range(T):
            assert not np.any(idx[t] == 0) and idx[t].min() >= 1 and idx[t].max() < lay["rows"][t]   # no bag names row 0; in range
            assert np.all(np.isfinite(wts[t])) and np.all(np.abs(wts[t]) <= 1)
            is_named = np.array([np.any(bag_rows(t, s) < N_POISON) for s in range(B)])
            assert np.array_equal(is_named, named[t])
            assert any(named[t, s] and bag_rows(t, s)[-1] < N_POISON for s in range(B)), t     # a poison row last in a bag
            for s in np.nonzero(named[t])[0]:
                assert not named[(t + 1) % T, s] and not named[t, (s + 1) % B], (t, s)          # clean neighbours
                r, w = bag_rows(t, s), bag_wts(t, s)
                both += int(1 in r and 2 in r)
                zero_w += int(np.any((w == 0) & np.isin(r, (1, 2, 4, 6, 7))))
                neg_w += int(np.any((w < 0) & np.isin(r, (1, 2, 4, 6, 7))))
        assert zero_w >= 1 and neg_w >= 1
        if not (isinstance(L, int) and L == 1):                                # (a bag of one row holds no two rows)
            assert both >= 1
        if L == RAGGED:
            for t in range(T):
                assert any(lens[t][s] == 0 and lens[t][s - 1] >= 5 and lens[t][s + 1] >= 5 for s in range(1, B - 1)), t
        if not isinstance(L, int):                                            # an empty bag beside a poisoned one, in the same table
            assert any(lens[t][s] == 0 and (named[t, s - 1] or named[t, s + 1]) for t in range(T) for s in range(1, B - 1))
        assert 2 * named.sum() <= named.size and 4 * np.sum(~named.any(axis=0)) >= B
        assert not named[:, 1 - b].any() and named[:, b].any()                # batch b: sample b poisoned, its neighbour clean
    for kind in KINDS:
        c = poison_case(shape, kind)
        for mode in ("sum", "mean", "w"):
            for b in range(N_BATCHES):
                cls = classes(c["cls"][mode][b])
                assert set(np.unique(cls)) == {0, 1, 2, 3}, (kind, mode, b)
                assert np.array_equal(cls, classes(c["seq"][mode][b])), (kind, mode, b)
                hot = named_columns(c["named"][b], D, B)
                assert not np.any(cls[~hot]), (kind, mode, b)                  # poison stays in the bags that name it
                fin = c["cls"][mode][b][cls == 0]
                assert np.abs(fin).max() < 1e6
        # nothing overflows: no finite weight times a finite element, nor any finite partial sum, exceeds 1e6
        for t in range(T):
            st = c["stored"][t]
            big = np.abs(np.where(np.isfinite(st), st, 0)).max(axis=1)
            for b in range(N_BATCHES):
                assert np.abs(c["wts"][b][t]).max() * big.max() <= 1e6
                assert int(c["lens"][b][t].max()) * big[N_POISON:].max() + 2 * big.max() <= 1e6
