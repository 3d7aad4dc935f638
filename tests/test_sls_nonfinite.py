"""inf and NaN table rows in every gather form on the GPU (-m gpu).

Every kernel of the gather loads rows a bag does not own (its own last row again, row 0 for an empty bag, the rows of
the wave's other bags, the row past the wave's rows) and must make them count for nothing.  Here those rows are poison:
tests/test_sls_nonfinite_cpu.py's `poison_case` puts NaN into row 0 of every table (no bag names it) and +-inf / NaN / 1e5
elements into rows 1 .. 7, which every third sample names in one of its tables -- last in the bag, with a weight of 0, with
a negative weight, +inf and -inf in one bag -- while its neighbours in the wave (the next table of the sample, the next
sample of the table, the empty bag beside it) name rows from 8 on only.

Two engines per case differ in their tables alone: `poisoned`, and `clean` whose rows 0 .. 7 are finite.  For the
unweighted sum, the mean and the weighted sum under "sls_weighted_flat" 0 and 1, for single queries of 48, 29 and 1
samples and one coalesced set, on the pooled columns of the interaction matrix, no element left out:
  * the class (finite, +inf, -inf, NaN) of every element is class_ref's, i.e. torch's;
  * the finite elements are the sequential chain's bits where the form sums in index order (the sequential ring walk,
    the one-lookup and any-width forms), and within the split order's tolerance of it otherwise;
  * every bag that names no poison row has the clean engine's bits, the empty bags +0.0;
  * the launch is the form the case stands for (dispatch log), and forward raises nothing: poison is no index error.
And on the outputs: the rows of samples none of whose bags is poisoned are the clean engine's bits -- NaN pooled rows stay
in their own rows of the MLP.
"""
import numpy as np
import pytest

from deeprecsys_amd import _native as N
from tests.test_half_tables import _load
from tests.test_sls_nonfinite_cpu import (KINDS, N_BATCHES, SHAPES, classes, close_finite, form_of, named_columns, nf_shape_id,
                                          poison_case, sequential_order, token_of)
from tests.test_sls_weights import JOBS12, _engine, _run_set
from tests.test_sls_weights_cpu import same_bits
from tests.test_sls_weights_flat_cpu import B, SIZES

pytestmark = pytest.mark.gpu

TAG = {"fp32": "", "fp16": "f16", "bf16": "bf16"}


def _tokens(eng, slot=0):
    return [t for t in eng.last_dispatch(slot) if t.startswith("sls_")]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _check_pooled(where, form, got, clean, cls_ref, seq, hot, empty):
    """got / clean: the pooled columns [bs, T * D] of the poisoned / the clean engine; cls_ref, seq: the references' rows;
    hot / empty: bool [bs, T * D], the columns of the bags that name a poison row / that are empty"""
    want = classes(cls_ref)
    have = classes(got)
    assert np.array_equal(have, want), (where, "classes differ at", np.argwhere(have != want)[:8].tolist(),
                                        have[have != want][:8].tolist(), want[have != want][:8].tolist())
    fin = want == 0
    if sequential_order(form):
        assert np.array_equal(_bits(got)[fin], _bits(seq)[fin]), (where, "finite elements: not the sequential chain's bits")
    else:
        # (two groups, each with its own floor: the 1e5 element of a poisoned bag must not widen the clean bags' floor)
        assert close_finite(got[~hot], seq[~hot]), (where, "clean bags outside the split tolerance")
        assert close_finite(got[hot], seq[hot]), (where, "finite elements of poisoned bags outside the split tolerance")
    assert np.array_equal(_bits(got)[~hot], _bits(clean)[~hot]), (where, "a bag that names no poison row differs from the clean engine",
                                                                 np.argwhere((_bits(got) != _bits(clean)) & ~hot)[:8].tolist())
    assert not np.any(_bits(got)[empty]), (where, "an empty bag is not +0.0")


def run_poison_case(c, n, kind, tag, after_load=None):
    """every run mode, query size and launch set of SHAPES[n] on two engines of stored type `kind` (tests/test_sls_weights.py's
    _engine) that hold c["poisoned"] and c["clean"]; c: poison_case's layout and references, tag: the kind's dispatch token;
    after_load(poisoned engine, clean engine): a check of the loaded tables (tests/test_sls_nonfinite_quant.py)"""
    shape = SHAPES[n]
    D, T, L, opts = shape
    fixed = isinstance(L, int)
    Lmax = max(int(ln.max()) for b in range(N_BATCHES) for ln in c["lens"][b])
    rng = np.random.RandomState(n)
    dense = [rng.rand(B, 8).astype(np.float32) for _ in range(N_BATCHES)]
    batch = lambda b: b % N_BATCHES                                            # staged batch 2 is batch 0 again, never weighted
    empty = [np.concatenate([np.repeat((c["lens"][b][t] == 0)[:, None], D, axis=1) for t in range(T)], axis=1) for b in range(N_BATCHES)]
    po, cl = (_engine(c["rows"], D, Lmax, B, kind) for _ in range(2))
    engines = (po, cl)
    try:
        _load(po, 11, c["poisoned"], D, T)
        _load(cl, 11, c["clean"], D, T)
        if after_load:
            after_load(po, cl)
        for eng in engines:
            eng.set_option("dispatch_log", 1)
            for k, v in sorted(opts.items()):
                eng.set_option(k, v)

        def stage(weighted):
            for eng in engines:
                for b in range(3):
                    eng.stage_batch(b, dense[batch(b)], c["idx"][batch(b)], c["lens"][batch(b)],
                                    weights=c["wts"][b] if weighted and b < N_BATCHES else None)

        def run(mode, nt, wflat=0, sizes=SIZES, sets=True):
            for eng in engines:
                eng.set_option("sls_nt", nt)
            for b in range(3):
                m = mode if b < N_BATCHES or mode != "w" else "sum"            # batch 2 carries no weights
                for bs in sizes:
                    where = (kind, nf_shape_id(shape), mode, "nt%d" % nt, "wflat%d" % wflat, b, bs)
                    form = form_of(shape, (bs,), weighted_default=(m == "w" and not wflat))
                    outs, Rs = [], []
                    for eng in engines:
                        outs.append(eng.forward(b, bs))                        # (raises on any error: poison is none)
                        Rs.append(eng.fetch_interaction(bs))
                        tok = _tokens(eng)
                        assert len(tok) == 1 and tok[0].startswith(token_of(form, nt, tag, m)), (where, tok, form)
                    bb = batch(b)
                    hot = named_columns(c["named"][bb], D, bs)
                    _check_pooled(where, form, Rs[0][:, D:], Rs[1][:, D:], c["cls"][m][bb][:bs], c["seq"][m][bb][:bs], hot, empty[bb][:bs])
                    assert same_bits(Rs[0][:, :D], Rs[1][:, :D]), (where, "the bottom MLP's columns")
                    ok = ~c["named"][bb][:, :bs].any(axis=0)                   # samples none of whose bags is poisoned
                    assert np.array_equal(_bits(outs[0])[ok], _bits(outs[1])[ok]), (where, "outputs of clean samples differ", np.nonzero(ok)[0][:8])
            if not sets:
                return
            live = [bs for _, bs in JOBS12 if bs]
            form = form_of(shape, live, weighted_default=(mode == "w" and not wflat))
            got_p, got_c = _run_set(po, JOBS12), _run_set(cl, JOBS12)
            for eng in engines:
                tok = _tokens(eng, 1)
                assert len(tok) == 1 and tok[0].startswith(token_of(form, nt, tag, mode)), (kind, n, mode, tok, form)
            for (b, q), Rp, Rc in zip(JOBS12, got_p, got_c):
                if not q:
                    continue
                m = mode if b < N_BATCHES or mode != "w" else "sum"            # (an unweighted query of a weighted set: weights of 1)
                bb = batch(b)
                where = (kind, nf_shape_id(shape), mode, "nt%d" % nt, "wflat%d" % wflat, "set of 12", b, q)
                _check_pooled(where, form, Rp[:, D:], Rc[:, D:], c["cls"][m][bb][:q], c["seq"][m][bb][:q], named_columns(c["named"][bb], D, q),
                              empty[bb][:q])
                assert same_bits(Rp[:, :D], Rc[:, :D]), where

        def run_all(mode, wflat=0):
            run(mode, 1, wflat)
            if fixed:                                                          # the instances without the non-temporal hint
                run(mode, 0, wflat, sizes=(B, 29), sets=False)

        stage(False)
        run_all("sum")
        for eng in engines:
            eng.set_option("sls_pool", 1)
        run_all("mean")
        for eng in engines:
            eng.set_option("sls_pool", 0)
        stage(True)
        for wflat in (0, 1):
            for eng in engines:
                eng.set_option("sls_weighted_flat", wflat)
            run_all("w", wflat)
    finally:
        for eng in engines:
            eng.close()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", range(len(SHAPES)), ids=[nf_shape_id(s) for s in SHAPES])
def test_non_finite_rows_reach_the_bags_that_name_them_and_no_other(kind, n):
    run_poison_case(poison_case(SHAPES[n], kind), n, kind, TAG[kind])


# ------------------------------------------------------------------------------------------------------------------------
# the stand-alone operator
@pytest.mark.parametrize("D", [10, 64])
def test_drs_sls_weighted_keeps_poison_in_the_bags_that_name_it(D):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    shape = [s for s in SHAPES if s[0] == D and not isinstance(s[2], int) and not s[3]][0]
    c = poison_case(shape, "fp32")
    idx, lens, w = c["idx"][0][0].astype(np.int32), c["lens"][0][0], c["wts"][0][0]
    rows, bags = c["rows"][0], lens.size
    hot = np.repeat(c["named"][0][0][:, None], D, axis=1)
    empty = np.repeat((lens == 0)[:, None], D, axis=1)
    form = {True: "any" if D % 4 else "ring 16,sequential", False: "any" if D % 4 else "ring 16,split"}
    eng = N.Engine(N.MODEL_DLRM, [16, 16], 8, [4, 8], [24, 4, 1], N.INTERACT_CAT, sigmoid_top=2,
                   max_batch=4, max_lookups=2, num_staged_batches=1, num_slots=1)
    try:
        dP, dC, di, dl, dw = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (c["poisoned"][0], c["clean"][0], idx, lens, w))
        for weighted in (True, False):
            mode = "w" if weighted else "sum"
            cls_ref, seq = c["cls"][mode][0][:, :D], c["seq"][mode][0][:, :D]
            for exact in (True, False):
                got = []
                for dW in (dP, dC):
                    out = torch.full((bags, D), float("nan"), device="cuda")
                    torch.cuda.synchronize()   # inputs/outputs were produced on torch's stream, the op runs on the engine's
                    eng.sls(dW.data_ptr(), rows, D, di.data_ptr(), dl.data_ptr(), bags, idx.size, out.data_ptr(), exact_order=exact,
                            wgt_ptr=dw.data_ptr() if weighted else None)
                    got.append(out.cpu().numpy())
                _check_pooled((D, mode, exact), form[exact], got[0], got[1], cls_ref, seq, hot, empty)
    finally:
        eng.close()
