"""inf and NaN table rows in DIN's and DIEN's own kernels on the GPU (-m gpu).

tests/test_din_dien_nonfinite_cpu.py holds the layout, the float64 references, the hot sets and the bar; here the engine runs
it.  Two engines per engine key differ in their tables alone: `poisoned` (row 0 of every table all NaN and named by every
staged bag BEYOND a query's size; rows 1 .. 7 hold +-inf, a NaN element, 1e5, a whole row of +inf, and one bag of every third
sample names them) and `clean` (the same tables with rows 0 .. 7 finite).  Per case -- one launch set of the boundary
catalogue -- under the case's own options and under "sls_exact" 1, for the whole set and for every query alone:
  1. forward raises nothing (poison is no index error) and the dispatch log shows the case's form;
  2. the pass-through blocks of the top MLP's input row (profile, candidate ad, context) have class_ref's classes, the
     sequential chain's bits where the form sums a bag in index order (else its tolerance), the clean engine's bits in
     every bag that names no poison row, +0.0 in the empty ones;
  3. the attention block / the recurrent state: every sample outside the hot set has the clean engine's bits -- the other
     samples of a poisoned sample's workgroup, lane group or MFMA tile are untouched, and DIEN's Reshape carries poison to
     sample (s U + u) % n and nowhere else; every sample has the float64 reference's class map and its finite elements
     are within tests/test_gather_boundaries.py's bar, the floor taken per sample row;
  4. the outputs: the same three statements, against the C oracle;
  5. the case's option sweeps (DIN: "din_s" 0 / 1 / 2 / 4 x "din_pipe" 1 / 0; DIEN: "dien_mfma" x "dien_fuse_top") give the
     poisoned engine's own result: equal bits where finite or infinite, NaN where NaN (fmaxf and the compare-select may
     differ in a NaN's payload); a query alone gives the bits it gave in the set wherever the catalogue promises bits;
  6. nothing stays behind: the same batches with every marked bag pointed at ordinary rows, on the POISONED engine in the
     same slot, give the clean engine's bits -- no stale inf / NaN in the slot's interaction and scratch buffers or in pad
     columns.
DRS_DIN_DIEN_NONFINITE_REPORT=<file>: one JSON line per case (profiles/r24_din_dien_nonfinite.md).
"""
import time

import numpy as np
import pytest

from deeprecsys_amd import _native as N
from tests import gather_shapes as S
from tests.test_din_dien_nonfinite_cpu import (ORDER, bar_fraction, block_columns, classes, layout, models_of, out_bar, passthrough_columns,
                                               references, report, row_bar, tables_of)
from tests.test_gather_boundaries import make_engine, run_set, sequential, set_options
from tests.test_sls_nonfinite import _check_pooled

pytestmark = pytest.mark.gpu


class Ctx(object):
    """tests/test_gather_boundaries.Ctx with a PAIR of engines per engine key: (poisoned, clean)"""

    def __init__(self):
        self.cur = {}
        self.seen = {}        # case name -> every token it showed
        self.fault = []       # the case that met a HIP error: the cases behind it do not touch the GPU
        self.wall = 0.0

    def close(self):
        for e in self.cur.get("engines", []):
            e.close()
        self.cur.clear()

    def engines(self, key):
        if self.cur.get("key") != key:
            self.close()
            clean, poisoned = tables_of(key)
            w = models_of(key)[0]
            self.cur.update(key=key, engines=[])
            for tab in (poisoned, clean):
                self.cur["engines"].append(make_engine(key, tab, w, N.TABLE_FP32))
        return self.cur["engines"]


@pytest.fixture(scope="module")
def ctx():
    c = Ctx()
    yield c
    c.close()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_or_nan(a, b):
    """equal bits where finite or infinite, NaN where NaN"""
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(_bits(a)[~na], _bits(b)[~nb]))


def stage(engines, lay, plain=False):
    for eng in engines:
        for b in sorted(lay.need):
            eng.stage_batch(b, None, lay.plain[b] if plain else lay.idx[b], lay.lens[b])


def check_query(where, case, form, exact, lay, b, n, r, Rp, Rc, Op, Oc, worst):
    """one query's input rows and outputs of the poisoned (Rp, Op) and the clean engine (Rc, Oc) against its references r"""
    D = case.D
    hot = r["hot"]
    fused = case.kind == "din" and S.din_class(case) == "fused" and not exact
    bag_form = "any" if fused or exact else form.split(" + ")[0]          # (the fused DIN forms pool a bag in index order)
    # 2. the pass-through blocks
    for k, (t, c0) in enumerate(passthrough_columns(case)):
        cols = slice(c0, c0 + D)
        _check_pooled(where + ("table %d" % t,), bag_form, Rp[:, cols], Rc[:, cols], r["R64"][:, cols], r["seq"][k],
                      np.repeat(hot["passthrough"][k][:, None], D, axis=1), np.repeat((lay.lens[b][t][:n] == 0)[:, None], D, axis=1))
    # 3. the attention block / the recurrent state
    lo, hi = block_columns(case)
    got, ref = Rp[:, lo:hi], r["R64"][:, lo:hi]
    cold = ~hot["block"]
    assert np.array_equal(_bits(got)[cold], _bits(Rc[:, lo:hi])[cold]), (where, "block: a sample outside the hot set differs from the clean engine",
                                                                        np.nonzero((_bits(got) != _bits(Rc[:, lo:hi])).any(axis=1) & cold)[0][:8].tolist())
    have, want = classes(got), classes(ref)
    assert np.array_equal(have, want), (where, "block: classes differ at", np.argwhere(have != want)[:8].tolist(), have[have != want][:8].tolist(),
                                        want[have != want][:8].tolist())
    frac = bar_fraction(got, ref, **row_bar(case))
    print("%r block: %.3f of the bar (hot rows %.3f)" % (where, frac.max(), frac[hot["block"]].max() if hot["block"].any() else 0.0))
    assert frac.max() <= 1, (where, "block: a finite element outside the bar, sample %d" % int(frac.argmax()), float(frac.max()))
    if hot["block"].any():
        worst["block"] = max(worst["block"], float(frac[hot["block"]].max()))
    order_exact = case.kind == "din" and (exact or (S.din_class(case) == "any" and sequential(form)))
    if order_exact:
        # the two-launch and any-shape forms behind a sequential gather: the oracle's bits
        fin = want == 0
        assert np.array_equal(_bits(got)[fin], _bits(r["R_orc"][:, lo:hi])[fin]), (where, "block: not the oracle's bits")
    # 4. the outputs
    cold = ~hot["out"]
    assert np.array_equal(_bits(Op)[cold], _bits(Oc)[cold]), (where, "outputs: a sample outside the hot sets differs from the clean engine",
                                                              np.nonzero((_bits(Op) != _bits(Oc)).any(axis=1) & cold)[0][:8].tolist())
    have, want = classes(Op), classes(r["out_orc"])
    assert np.array_equal(have, want), (where, "outputs: classes differ at", np.argwhere(have != want)[:8].tolist(), have[have != want][:8].tolist(),
                                        want[have != want][:8].tolist())
    frac = bar_fraction(Op, r["out_orc"], **out_bar(case, exact=order_exact))
    print("%r outputs: %.3f of the bar (hot rows %.3f)" % (where, frac.max(), frac[hot["out"]].max() if hot["out"].any() else 0.0))
    assert frac.max() <= 1, (where, "outputs: a finite element outside the bar, sample %d" % int(frac.argmax()), float(frac.max()))
    if hot["out"].any():
        worst["out"] = max(worst["out"], float(frac[hot["out"]].max()))
    assert np.all(np.isfinite(Rc)) and np.all(np.isfinite(Oc)), (where, "the clean engine returned a non-finite element")


def poison_case(ctx, name):
    lay = layout(name)
    case = lay.case
    refs = references(name)
    po, cl = engines = ctx.engines(lay.key)
    jobs = lay.jobs
    seen = ctx.seen.setdefault(name, set())
    worst = dict(block=0.0, out=0.0)
    stage(engines, lay)
    own_set = None
    for mode in ("exact", "own"):
        exact = mode == "exact"
        over = {"sls_exact": 1} if exact else {}
        for eng in engines:
            own = set_options(eng, case, **over)
        form = S.EXPECTED[case.kind](own)
        (Rp, Op, logp), (Rc, Oc, logc) = run_set(po, jobs), run_set(cl, jobs)       # 1. (raises on any error: poison is none)
        print("%s %s: %s" % (name, mode, " ".join(logp)))
        for log in (logp, logc):
            bad = S.check_dispatch(own, log, form=form)
            assert not bad, (name, mode, bad, log)
        if not exact:
            seen.update(logp)
            own_set = (Rp, Op)
        for i, (b, n) in enumerate(jobs):
            if n:
                check_query((name, mode, "set", i, n), case, form, exact, lay, b, n, refs[(b, n)], Rp[i], Rc[i], Op[i], Oc[i], worst)
        # every query alone
        if len([n for _, n in jobs if n]) < 2:
            continue
        done = set()
        for i, (b, n) in enumerate(jobs):
            if n == 0 or (b, n) in done:
                continue
            done.add((b, n))
            (R1, O1, log1), (R1c, O1c, log1c) = run_set(po, [(b, n)]), run_set(cl, [(b, n)])
            form_i = S.EXPECTED[case.kind](own, only=i)
            for log in (log1, log1c):
                bad = S.check_dispatch(own._replace(exclude=()), log, form=form_i)
                assert not bad, (name, mode, "query %d alone" % i, bad, log)
            if not exact:
                seen.update(log1)
            check_query((name, mode, "alone", i, n), case, form_i, exact, lay, b, n, refs[(b, n)], R1[0], R1c[0], O1[0], O1c[0], worst)
            if case.alone in S.BITS_PROMISED or form_i == form:
                assert same_or_nan(R1[0], Rp[i]) and same_or_nan(O1[0], Op[i]), (name, mode, "query %d alone: not the bits it gave in the set" % i, log1)
    # 5. the sweeps, on the poisoned engine (which holds the case's own options again)
    Rq, Oq = own_set
    for over in S.sweeps(case):
        swept = set_options(po, case, **over)
        R2, O2, log2 = run_set(po, jobs)
        seen.update(log2)
        bad = S.check_dispatch(swept, log2, form=S.EXPECTED[case.kind](swept))
        assert not bad, (name, over, bad, log2)
        for i in range(len(jobs)):
            assert same_or_nan(R2[i], Rq[i]) and same_or_nan(O2[i], Oq[i]), (name, over, "query %d: not the result of the case's own options" % i, log2)
    # 6. nothing stays behind: every marked bag pointed at ordinary rows, the poisoned engine in the same slot
    stage(engines, lay, plain=True)
    for eng in engines:
        set_options(eng, case)
    (Rp, Op, logp), (Rc, Oc, _) = run_set(po, jobs), run_set(cl, jobs)
    for i, (b, n) in enumerate(jobs):
        assert np.array_equal(_bits(Rp[i]), _bits(Rc[i])) and np.array_equal(_bits(Op[i]), _bits(Oc[i])), (name, "query %d: the poisoned engine on ordinary "
                                                                                                             "rows differs from the clean one" % i, logp)
        assert np.all(np.isfinite(Rp[i])) and np.all(np.isfinite(Op[i])), (name, "query %d: a non-finite element stayed behind" % i)
    return worst


def run_case(ctx, name):
    if ctx.fault:
        pytest.fail("not run: %s met a HIP error, nothing more is started on that GPU" % ctx.fault[0])
    t0 = time.time()
    try:
        worst = poison_case(ctx, name)
    except N.DrsError as e:
        if e.code == N.ERR_HIP:
            ctx.fault.append(name)
        raise
    finally:
        ctx.wall += time.time() - t0
    lay = layout(name)
    forms = sorted({t.split("[")[0] for t in ctx.seen[name] if t.startswith(S.KERNEL_NAMES)})
    report(test="gpu", case=name, kind=lay.case.kind, forms=forms, seconds=round(time.time() - t0, 3),
           queries=[dict(n=n, hot=int(references(name)[(b, n)]["hot"]["out"].sum()), clean=int((~references(name)[(b, n)]["hot"]["out"]).sum()))
                    for b, n in lay.jobs if n],
           worst_block=worst["block"], worst_out=worst["out"])


@pytest.mark.parametrize("name", ORDER)
def test_poison_reaches_the_samples_that_name_it_and_no_other(ctx, name):
    run_case(ctx, name)


def test_the_cases_reach_every_din_and_dien_kernel(ctx):
    """every kernel name mlp_din and mlp_dien can log (S.SECOND_TOKENS) was shown by a case of this module"""
    for name in ORDER:
        if name not in ctx.seen:          # (this test selected without the per-case test)
            run_case(ctx, name)
    tokens = set().union(*ctx.seen.values())
    for k in S.SECOND_TOKENS:
        assert any(t.startswith((k + "<", k + "[")) for t in tokens), (k, sorted(tokens))
    print("wall time of the %d cases: %.1f s" % (len(ORDER), ctx.wall))
    report(test="gpu_wall", cases=len(ORDER), seconds=round(ctx.wall, 1))
