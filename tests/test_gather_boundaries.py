"""The gather, DIN and DIEN launch choosers on both sides of every form boundary (-m gpu): the engine against float64 and the
CPU oracle at every launch set of the boundary catalogue (tests/gather_shapes.py; tests/test_gather_boundaries_cpu.py holds
the catalogue to its rules and the oracle to float64 there).

For every case (one launch set):
  * the dispatch log shows the form the case stands for and no other gather / DIN / DIEN form: a case that has slipped off its
    boundary fails instead of quietly testing something else;
  * output and interaction buffers start as NaN, the staged bags beyond a query's size name a table row that is all NaN, and
    no NaN comes back;
  * gather cases, integer pass (table rows of small integers: every summation order is exact): the pooled tensor is BITWISE
    the float64 sum under every form, with fp32 and with fp16 tables; real pass (rows uniform in [-1, 1]): within the derived
    bound (L - 1) 2^-24 sum|x_i| of float64, and against the oracle bitwise for the sequential forms (any / copy / sequential
    ring walk) and within DESIGN.md 6's bar (1e-5 rel + 2e-6 max) for the split and flat forms;
  * DIN / DIEN: under "sls_exact" 1 the top MLP's input row and the outputs against the oracle at the bars of
    test_gpu_parity.py, the case's own (default-mode) options within the default-mode tolerance; DIEN's pass-through columns
    bitwise, every "dien_mfma" x "dien_fuse_top" the same bits; DIN: "din_pipe" 0 and every forced "din_s" the same bits;
  * a query's bits do not depend on its set: every query served alone gives the bits it gave in the set -- except across a
    change of summation order, which the case states (`alone`), where the tolerance holds instead.
The closing test asserts that the catalogue reached every gather / DIN / DIEN kernel name and lists the template-argument
combinations no case showed.  DRS_GATHER_BOUNDARY_REPORT=<file>: the forms each case showed, one JSON line per case
(profiles/r12_gather_boundaries.md).

One engine serves the cases of one (kind, D, T, hidden widths, top MLP): the cases run in the order of that key (the module's
`ctx` fixture holds the current key's engines), batches are restaged and options flipped per case.
"""
import json
import os

import numpy as np
import pytest

from deeprecsys_amd import _native as N
from tests import gather_shapes as S
from tests import helpers as H

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
ORDER = sorted(S.NAMES, key=lambda n: (repr(S.engine_key(S.BY_NAME[n])), S.NAMES.index(n)))
KIND = {"sls": N.MODEL_DLRM, "din": N.MODEL_DIN, "dien": N.MODEL_DIEN}
# the bars model_case holds the top MLP's input row and the outputs to (H.close's arguments; tests/test_din_dien_nonfinite*.py
# import them): DIN in the case's own mode (rtol alone on the outputs: test_din_fused_and_two_launch_forms_match_oracle's
# default-mode bar) and under "sls_exact" 1, DIEN in either mode
DIN_ROW = dict(rtol=1e-5, atol_scale=2e-6)
DIN_OUT = dict(rtol=H.RTOL_OUT)
DIN_OUT_EXACT = dict(rtol=1e-6, atol=1e-7)
DIEN_ROW = dict(rtol=2e-5, atol=2e-6)
DIEN_OUT = dict(rtol=max(2e-5, H.RTOL_OUT), atol=2e-6)


def _report(**kw):
    path = os.environ.get("DRS_GATHER_BOUNDARY_REPORT")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(kw) + "\n")


class Ctx(object):
    """What the cases of this module share: the engines of the current engine key (the cases are ordered by key, the previous
    key's engines are closed), the dispatch tokens every case showed, and the case that met a HIP error."""

    def __init__(self):
        self.cur = {}
        self.seen = {}        # case name -> every token it showed (its own options, the sweeps, the queries alone)
        self.fault = []       # the case that met a HIP error: the cases behind it do not touch the GPU

    def close(self):
        for e in self.cur.get("engines", {}).values():
            e.close()
        self.cur.clear()

    def bundle(self, key):
        """tables, weights, oracle model and the engines of a key"""
        if self.cur.get("key") != key:
            self.close()
            tab, w = S.Tables(key), S.Weights(key)
            self.cur.update(key=key, tab=tab, w=w, om=w.oracle_model(tab.W), engines={})
        return self.cur

    def engine(self, key, dtype=N.TABLE_FP32):
        b = self.bundle(key)
        if dtype not in b["engines"]:
            b["engines"][dtype] = make_engine(key, b["tab"], b["w"], dtype)
        return b["engines"][dtype]


@pytest.fixture(scope="module")
def ctx():
    c = Ctx()
    yield c
    c.close()


def make_engine(key, tab, w, dtype):
    kind, D, T, Hh, top = key
    eng = N.Engine(KIND[kind], tab.table_rows(), D, w.ln_bot, w.ln_top, N.INTERACT_CAT, sigmoid_top=2 if kind == "sls" else -1,
                   max_batch=S.B_MAX, max_lookups=S.max_lookups(key), num_staged_batches=S.N_BATCH, num_slots=1)
    try:
        if dtype != N.TABLE_FP32:
            eng.set_option("table_dtype", dtype)          # first, while the arena is empty
        eng.set_option("dispatch_log", 1)
        for t, W in enumerate(tab.W):
            eng.set_table(t, W)
        if kind == "sls":
            for l, (W, b) in enumerate(w.bot):
                eng.set_fc(N.MLP_BOT, l, W, b)
        if kind == "din":
            for u, unit in enumerate(w.att):
                for l, (W, b) in enumerate(unit):
                    eng.set_fc(N.MLP_ATT0 + u, l, W, b)
        if kind == "dien":
            for l, mlp in enumerate((N.MLP_RNN0, N.MLP_RNN1)):
                for i, (W, b) in enumerate(w.rnn[l]):
                    eng.set_fc(mlp, i, W, b)
        for l, (W, b) in enumerate(w.top):
            eng.set_fc(N.MLP_TOP, l, W, b)
    except Exception:
        eng.close()
        raise
    return eng


def set_options(eng, case, **over):
    opts = S.options(case)
    opts.update(over)
    for k, v in opts.items():
        eng.set_option(k, v)
    return case._replace(opts=tuple(sorted(opts.items())))


def stage(eng, st, w, integer=False):
    for b, n in sorted(st.need().items()):
        idx, lens = st.stage(b, n, integer)
        dense = None
        if w.kind == "sls":
            dense = w.dense.copy()
            dense[n:] = np.nan
        eng.stage_batch(b, dense, idx, lens)


def run_set(eng, jobs):
    """one launch set into NaN buffers -> (per-query interaction rows, per-query outputs, dispatch log)"""
    eng.forward_multi_async(0, [b for b, _ in jobs], [n for _, n in jobs])
    total = sum(n for _, n in jobs)
    out = np.full((total, eng.n_out), np.nan, dtype=np.float32)
    eng._check(N.lib().drs_wait(eng._h, 0, out.ctypes.data_as(N._f32p), out.size), "drs_wait")
    log = eng.last_dispatch(0)
    vrows = sum((n + 63) // 64 * 64 for _, n in jobs)
    R = np.full((vrows, eng.num_int), np.nan, dtype=np.float32)
    eng._check(N.lib().drs_fetch_interaction(eng._h, 0, vrows, R.ctypes.data_as(N._f32p)), "drs_fetch_interaction")
    Rq, Oq, v, o = [], [], 0, 0
    for _, n in jobs:
        Rq.append(R[v:v + n])
        Oq.append(out[o:o + n])
        v += (n + 63) // 64 * 64
        o += n
    return Rq, Oq, log


def no_nan(name, what, arrays):
    for i, a in enumerate(arrays):
        assert not np.any(np.isnan(a)), (name, what, "query %d: a NaN came back, rows %r" % (i, sorted(set(np.argwhere(np.isnan(a))[:, 0]))[:8]))


def sequential(form):
    g = form.split(" + ")[0]
    return g == "any" or g.startswith("one") or g.endswith("sequential")


def pooled_refs(case, st, tab, b, n, integer):
    """float64 pooled tensor [n, T D], the magnitudes' sums, the bags' lengths per element, and the oracle's fp32 tensor"""
    idx, lens = st.query(b, n, integer)
    r64, mag, Ls, o32 = [], [], [], []
    for t in range(case.T):
        e, m = S.sls64(tab.W[t], idx[t], lens[t])
        r64.append(e)
        mag.append(m)
        Ls.append(np.repeat(lens[t], case.D).reshape(n, case.D))
        o32.append(S.orc.sls(tab.W[t], idx[t], lens[t]))
    return np.concatenate(r64, 1), np.concatenate(mag, 1), np.concatenate(Ls, 1), np.concatenate(o32, 1)


def alone_checks(case, eng, st, jobs, Rq, Oq, own, tag, seen, close_R, close_out):
    """every query of the set served alone: its own form (by the rules), and the bits it gave in the set -- unless serving
    THIS query alone changes the order of its sums (its own form differs from the set's, and the case says that the change
    is one of order): then interaction rows and outputs within the tolerances"""
    if len([n for _, n in jobs if n]) < 2:
        return
    done = {}
    for i, (b, n) in enumerate(jobs):
        if n == 0 or (b, n) in done:
            continue
        done[(b, n)] = i
        R1, O1, log = run_set(eng, [(b, n)])
        seen.update(log)
        # (`exclude` speaks of the set: alone, the query takes whatever the rules give it)
        form = S.EXPECTED[case.kind](own, only=i)
        bad = S.check_dispatch(own._replace(exclude=()), log, form=form, tag=tag)
        assert not bad, (case.name, "query %d alone" % i, bad, log)
        if case.alone in S.BITS_PROMISED or form == S.EXPECTED[case.kind](own):
            assert np.array_equal(R1[0], Rq[i]), (case.name, "query %d alone: interaction rows differ from the set's" % i, log)
            assert np.array_equal(O1[0], Oq[i]), (case.name, "query %d alone: outputs differ from the set's" % i, log)
        else:
            assert close_R(R1[0], Rq[i]), (case.name, "query %d alone (a form change)" % i, float(np.abs(R1[0] - Rq[i]).max()))
            assert close_out(O1[0], Oq[i]), (case.name, "query %d alone (a form change): outputs" % i, float(np.abs(O1[0] - Oq[i]).max()))


def gather_case(ctx, case):
    key = S.engine_key(case)
    b = ctx.bundle(key)
    tab, w = b["tab"], b["w"]
    st = S.Staged(case, tab)
    jobs = st.jobs()
    D = case.D
    seen = ctx.seen.setdefault(case.name, set())
    for tag, dtype in (("", N.TABLE_FP32), ("f16", N.TABLE_FP16)):
        eng = ctx.engine(key, dtype)
        own = set_options(eng, case)
        for integer in ((False, True) if not tag else (True,)):
            stage(eng, st, w, integer)
            Rq, Oq, log = run_set(eng, jobs)
            print("%s %s %s: %s" % (case.name, tag or "f32", "integer" if integer else "real", " ".join(log)))
            bad = S.check_dispatch(case, log, tag=tag)
            assert not bad, (case.name, tag, bad, log)
            if not tag:
                seen.update(log)
            no_nan(case.name, "interaction rows", Rq)
            no_nan(case.name, "outputs", Oq)
            for i, (bt, n) in enumerate(jobs):
                if n == 0:
                    continue
                r64, mag, Ls, o32 = pooled_refs(case, st, tab, bt, n, integer)
                got = Rq[i][:, D:]
                if integer:
                    if not np.array_equal(got, r64):
                        wrong = np.argwhere(got != r64)
                        raise AssertionError((case.name, tag, "integer pass, query %d: not the exact sum" % i, "samples %r" % sorted(set(wrong[:, 0]))[:12],
                                              "columns %r" % sorted(set(wrong[:, 1]))[:12], log))
                    continue
                bound = np.maximum(Ls - 1, 0) * U * mag
                err = np.abs(got - r64)
                assert np.all(err <= bound), (case.name, "query %d: beyond (L - 1) u sum|x| of float64" % i, float((err - bound).max()), log)
                if sequential(case.form):
                    assert np.array_equal(got, o32), (case.name, "query %d: a sequential form is bitwise the oracle's" % i, float(np.abs(got - o32).max()), log)
                else:
                    assert H.close(got, o32, rtol=1e-5, atol_scale=2e-6), (case.name, "query %d" % i, float(np.abs(got - o32).max()), log)
            alone_checks(case, eng, st, jobs, Rq, Oq, own, tag, seen if not tag else set(),
                         lambda a, c: H.close(a[:, D:], c[:, D:], rtol=1e-5, atol_scale=2e-6),
                         lambda a, c: H.close(a, c, rtol=H.RTOL_OUT, atol=1e-7))     # (smoke()'s bar for the split gather's outputs)
            if integer and case.alone not in S.BITS_PROMISED:
                # (integer rows: exact under either form, so the bits agree across the form change too)
                for i, (bt, n) in enumerate(jobs):
                    if n:
                        assert np.array_equal(run_set(eng, [(bt, n)])[0][0][:, D:], Rq[i][:, D:]), (case.name, tag, i)


def model_case(ctx, case):
    key = S.engine_key(case)
    b = ctx.bundle(key)
    tab, w, om = b["tab"], b["w"], b["om"]
    eng = ctx.engine(key)
    st = S.Staged(case, tab)
    jobs = st.jobs()
    D, Hh = case.D, (case.H[0] if case.kind == "dien" else 0)
    seen = ctx.seen.setdefault(case.name, set())
    stage(eng, st, w)
    exp = {}
    for bt, n in set(jobs):
        if n:
            idx, lens = st.query(bt, n)
            exp[(bt, n)] = om.forward(None, idx, lens, bs=n, want_R=True)
    din_any = case.kind == "din" and S.din_class(case) == "any"
    seq_gather = sequential(case.form)
    for mode in ("exact", "own"):
        own = set_options(eng, case, **({"sls_exact": 1} if mode == "exact" else {}))
        Rq, Oq, log = run_set(eng, jobs)
        print("%s %s: %s" % (case.name, mode, " ".join(log)))
        bad = S.check_dispatch(own, log, form=S.EXPECTED[case.kind](own))
        assert not bad, (case.name, mode, bad, log)
        if mode == "own":
            seen.update(log)
        no_nan(case.name, "interaction rows", Rq)
        no_nan(case.name, "outputs", Oq)
        for i, (bt, n) in enumerate(jobs):
            if n == 0:
                continue
            out_exp, R_exp = exp[(bt, n)]
            R, out = Rq[i], Oq[i]
            d = float(np.abs(R - R_exp).max())
            if case.kind == "din":
                if mode == "exact" or (din_any and seq_gather):
                    assert np.array_equal(R, R_exp), (case.name, mode, i, d, log)
                    assert H.close(out, out_exp, **DIN_OUT_EXACT), (case.name, mode, i)
                else:
                    assert H.close(R, R_exp, **DIN_ROW), (case.name, mode, i, d, log)
                    assert H.close(out, out_exp, **DIN_OUT), (case.name, mode, i)
                if mode == "exact" or seq_gather or S.din_class(case) == "fused":
                    # the pass-through features are pooled in index order: bitwise
                    for lo in (0, 2 * D, 3 * D):
                        assert np.array_equal(R[:, lo:lo + D], R_exp[:, lo:lo + D]), (case.name, mode, i, lo)
            else:
                if mode == "exact" or seq_gather:
                    assert np.array_equal(R[:, Hh:], R_exp[:, Hh:]), (case.name, mode, i, "pass-through columns")
                    assert H.close(R, R_exp, **DIEN_ROW), (case.name, mode, i, d, log)
                    assert H.close(out, out_exp, **DIEN_OUT), (case.name, mode, i)
                else:
                    # (ragged bags: the split ring walk pools the pass-through columns in another order -- the same bar,
                    #  without the bitwise claim)
                    assert H.close(R, R_exp, **DIEN_ROW), (case.name, mode, i, d, log)
                    assert H.close(out, out_exp, **DIEN_OUT), (case.name, mode, i)
    # (the engine holds the case's own options again)
    for over in S.sweeps(case):
        swept = set_options(eng, case, **over)
        R2, O2, log2 = run_set(eng, jobs)
        seen.update(log2)
        bad = S.check_dispatch(swept, log2, form=S.EXPECTED[case.kind](swept))
        assert not bad, (case.name, over, bad, log2)
        for i in range(len(jobs)):
            assert np.array_equal(O2[i], Oq[i]) and np.array_equal(R2[i], Rq[i]), (case.name, over, "query %d: not the bits of the case's own options" % i, log2)
    own = set_options(eng, case)
    tol = (lambda a, c: H.close(a, c, rtol=1e-5, atol_scale=2e-6)) if case.kind == "din" else (lambda a, c: H.close(a, c, rtol=2e-5, atol=2e-6))
    alone_checks(case, eng, st, jobs, Rq, Oq, own, "", seen, tol, lambda a, c: H.close(a, c, rtol=H.RTOL_OUT))


def run_case(ctx, name):
    case = S.BY_NAME[name]
    if ctx.fault:
        pytest.fail("not run: %s met a HIP error, nothing more is started on that GPU" % ctx.fault[0])
    try:
        (gather_case if case.kind == "sls" else model_case)(ctx, case)
    except N.DrsError as e:
        if e.code == N.ERR_HIP:
            ctx.fault.append(name)
        raise
    forms = sorted({t.split("[")[0] for t in ctx.seen[name] if t.startswith(S.KERNEL_NAMES)})
    _report(test="gpu_forms", case=name, kind=case.kind, rule=case.rule, thr=case.thr, side=case.side, forms=forms)


@pytest.mark.parametrize("name", ORDER)
def test_set_takes_the_expected_form_and_matches_the_references(ctx, name):
    run_case(ctx, name)


def test_the_catalogue_reaches_every_gather_din_and_dien_kernel(ctx):
    """Every kernel name launch_sls_e, launch_din_fused, mlp_din and mlp_dien can log was shown by a case, and is named in
    the `expect` of one; the template-argument combinations of the product build that the run did NOT show are exactly the
    list the catalogue pins (S.NOT_SHOWN): a form that silently stops being reached -- or starts to be -- fails here."""
    for name in ORDER:
        if name not in ctx.seen:          # (this test selected without the per-case test)
            run_case(ctx, name)
    seen = ctx.seen
    tokens = set().union(*seen.values())
    for k in S.KERNEL_NAMES:
        shown = [n for n, toks in seen.items() if any(t.startswith((k + "<", k + "[")) for t in toks)]
        named = [n for n in shown if any(p.startswith((k + "<", k + "[")) for p in S.BY_NAME[n].expect)]
        assert named, (k, shown)
    missing = [f for f in S.PRODUCT_FORMS if not any(t.startswith(f) for t in tokens)]
    print("template-argument combinations no case showed: %r" % missing)
    _report(test="not_shown", forms=missing)
    assert missing == list(S.NOT_SHOWN), (sorted(set(missing) - set(S.NOT_SHOWN)), sorted(set(S.NOT_SHOWN) - set(missing)))
