"""The MLP launch planner on both sides of every form boundary (-m gpu): the engine against the CPU oracle at every shape of
the boundary catalogue (tests/mlp_shapes.py; tests/test_mlp_boundaries_cpu.py holds the oracle itself to float64 there).

For every case, with "sls_exact" 1:
  * the interaction tensor is bitwise the oracle's; the outputs are bitwise the oracle's where the last layer has no sigmoid
    and within rtol 1e-6 / atol 1e-7 where it has one (the bars of test_gpu_parity.py);
  * the dispatch log shows every form the case stands for and none it excludes: a case that no longer stands on its
    boundary fails instead of quietly testing something else;
  * every product launch structure that applies gives the same bits, three launch sets in flight;
  * a coalesced set of 12 queries equals the same queries served alone;
  * output buffers start as NaN, and everything of the staged batch beyond the query's rows is NaN (dense rows; bags that
    name a NaN table row): a kernel that reads a row or a pad column it should not read shows up.
The closing test asserts that the catalogue reaches every MLP form launch_plan can name.
DRS_MLP_BOUNDARY_REPORT=<file>: the forms each case showed, one JSON line per case (profiles/r10_mlp_boundaries.md).
"""
import json
import os

import numpy as np
import pytest

from deeprecsys_amd import _native as N
from tests import helpers as H
from tests import mlp_shapes as S

pytestmark = pytest.mark.gpu

LAB_SEEN = set()   # tokens seen under the lab-only structures


@pytest.fixture(scope="module")
def seen():
    """case name -> the dispatch-log tokens of its own options (single queries): filled by the per-case test, read by the closing
    coverage test (which runs the cases it does not find here itself)"""
    return {}


def _report(**kw):
    path = os.environ.get("DRS_MLP_BOUNDARY_REPORT")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(kw) + "\n")


def make_engine(net, slots=3):
    c = net.case
    eng = N.Engine(net.kind, net.table_rows(), c.D, net.ln_bot, list(c.top), N.INTERACT_DOT if net.dot else N.INTERACT_CAT,
                   sigmoid_top=net.sigmoid_top, max_batch=S.B_MAX, max_lookups=c.L, num_staged_batches=2, num_slots=slots,
                   ln_task=list(c.task) if c.task else None, num_tasks=c.num_tasks)
    try:
        eng.set_option("sls_exact", 1)
        eng.set_option("dispatch_log", 1)
        for k, v in S.options(c).items():
            eng.set_option(k, v)
        for t, W in enumerate(net.tables):
            eng.set_table(t, W)
        for (which, l), (W, b) in sorted(net.w.items()):
            eng.set_fc(which, l, W, b)
        eng.stage_batch(0, net.dense, net.idx, net.lens)
        eng.stage_batch(1, *net.stage(S.B_MAX))
    except Exception:
        eng.close()
        raise
    return eng


def forward_into_nan(eng, batch, bs):
    out = np.full((bs, eng.n_out), np.nan, dtype=np.float32)
    eng._check(N.lib().drs_forward(eng._h, batch, bs, out.ctypes.data_as(N._f32p)), "drs_forward")
    return out


def interaction_into_nan(eng, bs):
    R = np.full((bs, eng.num_int), np.nan, dtype=np.float32)
    eng._check(N.lib().drs_fetch_interaction(eng._h, 0, bs, R.ctypes.data_as(N._f32p)), "drs_fetch_interaction")
    return R


def same_outputs(net, got, exp):
    if net.sigmoid_top < 0:
        return np.array_equal(got, exp)
    return got.shape == exp.shape and bool(np.all(np.isfinite(got))) and np.allclose(got, exp, rtol=1e-6, atol=1e-7)


def forms_of(log):
    return sorted({t.split("[")[0] for t in log if t.startswith(S.MLP_TOKENS)})


@pytest.mark.parametrize("name", S.NAMES)
def test_engine_matches_oracle_and_takes_the_expected_form(name, seen):
    case = S.BY_NAME[name]
    net = S.Built(case)
    om = net.oracle_model()
    eng = make_engine(net, slots=1)
    reads_in_place = any("sbase,split" in p for p in case.expect)
    try:
        for bs in case.rows:
            exp, R_exp = net.oracle_forward(om, bs)
            eng.stage_batch(1, *net.stage(bs))                 # rows beyond bs: NaN
            got = forward_into_nan(eng, 1, bs)
            log = eng.last_dispatch(0)
            print("%s bs %d: %s" % (name, bs, " ".join(log)))
            bad = S.check_dispatch(case, log)
            assert not bad, (name, bs, bad, log)
            seen.setdefault(name, set()).update(log)
            assert not np.any(np.isnan(got)), (name, bs, "a NaN reached the outputs: rows %r" % sorted(set(np.argwhere(np.isnan(got))[:, 0]))[:8])
            if not same_outputs(net, got, exp):
                d = np.abs(got.astype(np.float64) - exp)
                r, col = np.unravel_index(int(np.argmax(d)), d.shape)
                wrong = np.argwhere(got != exp)
                raise AssertionError((name, bs, "outputs differ from the oracle", float(d.max()), "at row %d column %d" % (r, col),
                                      "rows %r" % sorted(set(wrong[:, 0]))[:16], "columns %r" % sorted(set(wrong[:, 1]))[:16], log))
            if reads_in_place:
                # (the first layer read the dense columns from the queries' arrays: the interaction tensor was never
                #  materialised -- the same query once more through the copy launch)
                with pytest.raises(N.DrsError) as err:
                    eng.fetch_interaction(bs)
                assert err.value.code == N.ERR_STATE
                eng.set_option("gemm_split", 0)
                again = forward_into_nan(eng, 1, bs)
                assert np.array_equal(again, got), (name, bs, "gemm_split 0 / 1")
            R = interaction_into_nan(eng, bs)
            if reads_in_place:
                eng.set_option("gemm_split", 1)
            if not np.array_equal(R, R_exp):
                wrong = np.argwhere(~((R == R_exp) | (np.isnan(R) & np.isnan(R_exp))))
                raise AssertionError((name, bs, "interaction tensor differs", "rows %r" % sorted(set(wrong[:, 0]))[:16],
                                      "columns %r" % sorted(set(wrong[:, 1]))[:16], log))
        _report(test="gpu_forms", case=name, rule=case.rule, side=case.side, forms=forms_of(seen[name]))
    finally:
        eng.close()


# the product launch structures of test_mlp_launch_structures_are_bit_identical, each on top of the case's own options; the
# lab build adds the forms that lost their measurement (H.runs_here)
STRUCTURES = [
    ("stream_packed", dict(mlp_stream=2)),
    ("stream4", dict(mlp_stream=4)),
    ("unfused", dict(mlp_fuse=0)),
    ("unfused_stream_packed", dict(mlp_stream=2, mlp_fuse=0)),
    ("no_standalone_layers", dict(mlp_split=0)),
    ("two_per_cu", dict(mlp_stream_2cu=1)),
    ("stream_packed_two_per_cu", dict(mlp_stream=2, mlp_stream_2cu=1)),
    ("rows32", dict(mlp_rows32=1)),
    ("unfused_rows32", dict(mlp_rows32=1, mlp_fuse=0)),
    ("nsplit2", dict(mlp_nsplit=2, mlp_nsplit_rows=1 << 20)),
    ("nsplit4", dict(mlp_nsplit=4, mlp_nsplit_rows=1 << 20)),
    ("rows32_nsplit4", dict(mlp_rows32=1, mlp_nsplit=4, mlp_nsplit_rows=1 << 20)),
    ("one_stream", dict(shared_stream=1)),
    ("one_stream_unfused", dict(shared_stream=1, mlp_fuse=0)),
    ("stream_lds", dict(mlp_stream=1)),
    ("chain", dict(mlp_stream=0)),
    ("unfused_chain", dict(mlp_stream=0, mlp_fuse=0)),
    ("standalone_layers", dict(mlp_stream=1, mlp_fuse=0, mlp_wide_kn=1)),
    ("preloaded_chain", dict(mlp_stream=0, mlp_preload=1)),
    ("early_stream4", dict(mlp_stream=4, mlp_early=1)),
]


@pytest.mark.parametrize("name", S.NAMES)
def test_launch_structures_and_coalescing_are_bit_identical(name):
    case = S.BY_NAME[name]
    net = S.Built(case)
    eng = make_engine(net, slots=3)
    try:
        eng.stage_batch(1, *net.stage(65))
        own = dict(S.options(case), shared_stream=2)
        if H.LAB:
            own.update(mlp_preload=0, mlp_early=0)
        jobs = [(0, S.B_MAX), (1, 1), (0, 37), (1, 64), (0, 17)]
        n_rows = sum(bs for _, bs in jobs)

        def three_sets(tag):
            for slot in (0, 1, 2):
                eng.forward_multi_async(slot, [b for b, _ in jobs], [bs for _, bs in jobs])
            outs = [eng.wait(slot, n_rows) for slot in (0, 1, 2)]
            assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2]), (name, tag, "sets in flight differ")
            return outs[0]
        base = three_sets("own")
        assert np.all(np.isfinite(base)), name
        # the same queries one at a time
        v = 0
        for b, bs in jobs:
            assert np.array_equal(base[v:v + bs], eng.forward(b, bs)), (name, "coalesced 5", b, bs)
            v += bs
        for tag, opts in STRUCTURES:
            if not H.runs_here(opts):
                continue                                        # (a lab option: DRS_TEST_LAB=1 runs it)
            for k, v_ in opts.items():
                eng.set_option(k, v_)
            got = three_sets(tag)
            log = eng.last_dispatch(0)
            if H.LAB:
                LAB_SEEN.update(log)
            for k, v_ in own.items():
                eng.set_option(k, v_)
            if not np.array_equal(got, base):
                wrong = np.argwhere(got != base)
                raise AssertionError((name, tag, "differs from the case's own structure", "rows %r" % sorted(set(wrong[:, 0]))[:16],
                                      "columns %r" % sorted(set(wrong[:, 1]))[:16], log))
        # 12 queries of mixed sizes in one set against the same queries alone
        jobs12 = [(1, 1), (1, 16), (1, 17), (0, S.B_MAX), (1, 33), (1, 64), (0, 15), (0, S.B_MAX), (0, 1), (1, 32), (0, 17), (1, 65)]
        eng.forward_multi_async(1, [b for b, _ in jobs12], [bs for _, bs in jobs12])
        out = eng.wait(1, sum(bs for _, bs in jobs12))
        alone = {}
        v = 0
        for b, bs in jobs12:
            if (b, bs) not in alone:
                alone[(b, bs)] = forward_into_nan(eng, b, bs)
            assert np.array_equal(out[v:v + bs], alone[(b, bs)]), (name, "coalesced 12", b, bs, eng.last_dispatch(1))
            v += bs
    finally:
        eng.close()


def test_the_catalogue_reaches_every_mlp_form(seen):
    """The union of the kernel names the cases showed (their own options, single queries) holds every MLP form of the product
    build that launch_plan names; stream_kernel<lds> exists in the lab build only."""
    for name in S.NAMES:
        if name in seen:
            continue
        case = S.BY_NAME[name]            # (this test selected without the per-case test: the case's queries, dispatch only)
        net = S.Built(case)
        eng = make_engine(net, slots=1)
        try:
            for bs in case.rows:
                eng.forward(0, bs)
                seen.setdefault(name, set()).update(eng.last_dispatch(0))
        finally:
            eng.close()
    tokens = set().union(*seen.values())
    missing = [f for f in S.PRODUCT_FORMS if f not in S.UNREACHABLE and not any(t.startswith(f) for t in tokens)]
    assert not missing, missing
    for f, why in S.UNREACHABLE.items():
        assert why and not any(t.startswith(f) for t in tokens), (f, "is listed as unreachable but was seen")
    # a form that only ONE case shows: removing that case must not go unnoticed -- it is named in its `expect`
    for f in S.PRODUCT_FORMS:
        shown = [n for n, toks in seen.items() if any(t.startswith(f) for t in toks)]
        named = [n for n in shown if any(p.split(" .. ")[0].startswith(f) for p in S.BY_NAME[n].expect)]
        assert named, (f, shown)
    if H.LAB:
        net = S.Built(S.BY_NAME["hidden_64"])
        eng = make_engine(net, slots=1)
        try:
            eng.set_option("mlp_stream", 1)
            eng.forward(0, 17)
            LAB_SEEN.update(eng.last_dispatch(0))
        finally:
            eng.close()
        for f in S.LAB_FORMS:
            assert any(t.startswith(f) for t in LAB_SEEN), f
