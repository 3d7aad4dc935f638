"""DLRM's one-launch form with its bf16 layers inside (-m gpu): engine option "mlp_bf16_fuse" 1 on top of "mlp_dtype" 2.

The expected values are never the launch under test: they are the layer-by-layer path of "mlp_dtype" 2 alone (one
gemm_bf16_kernel launch per bf16 layer) and the forward composed from operator calls (Net.compose: drs_fc, drs_sls), both
held to the derived bound by tests/test_bf16_mlp.py.  An output's bits depend on its row of x and its row of W only
(DESIGN 4.2), so the fused launch must return the same bits: every comparison below is np.array_equal.

Every engine runs with sls_exact 1 and dispatch_log 1.
"""
import numpy as np
import pytest

from deeprecsys_amd import _native as N
from tests import helpers as H
from tests.test_bf16_mlp import BF16, Net, count_bf16, nets

pytestmark = pytest.mark.gpu

GRID = [(0, 200), (1, 37), (0, 1), (1, 15), (0, 16), (1, 17), (0, 64), (1, 65)]


def count_fused(log):
    return sum(1 for t in log if t.startswith("fused_bf16_kernel"))


def logged(eng):
    eng.set_option("dispatch_log", 1)
    return eng


def unfused_engine(net, **kw):
    return logged(net.engine(BF16, **kw))


def fused_engine(net, order="after", **kw):
    """order: when mlp_bf16_fuse is set -- "first": before mlp_dtype and the weights | "before_weights": behind mlp_dtype,
    before the weights | "after": behind both."""
    if order == "after":
        eng = net.engine(BF16, **kw)
        eng.set_option("mlp_bf16_fuse", 1)
        return logged(eng)
    eng = net.engine(0, load=False, **kw)
    try:
        if order == "first":
            eng.set_option("mlp_bf16_fuse", 1)
            eng.set_option("mlp_dtype", BF16)
        else:
            eng.set_option("mlp_dtype", BF16)
            eng.set_option("mlp_bf16_fuse", 1)
        net.load(eng)
    except Exception:
        eng.close()
        raise
    return logged(eng)


def threshold_net(top):
    """D 16, T 3: bottom 64-64-16 (a bf16 first layer that reads the dense rows, then a narrow one), cat top 64-..."""
    return Net(N.MODEL_DLRM, 16, 3, [64, 64, 16], top, sigmoid_top=len(top) - 1, seed=11)


class World(object):
    """Per model: the fused engine, the layer-by-layer bf16 engine and an fp32 engine, and the reference outputs of GRID
    computed once."""

    def __init__(self, names):
        self.net, self.fused, self.unfused, self.fp32, self.ref = {}, {}, {}, {}, {}
        self._all = nets()
        self.names = names

    def get(self, name):
        if name not in self.net:
            net = self._all[name]
            self.net[name] = net
            self.fused[name], self.unfused[name], self.fp32[name] = fused_engine(net), unfused_engine(net), logged(net.engine(0))
            self.ref[name] = {}
        return self.net[name], self.fused[name], self.unfused[name], self.fp32[name]

    def reference(self, name, batch, bs):
        """(outputs, interaction tensor, dispatch log) of the layer-by-layer bf16 engine."""
        key = (batch, bs)
        if key not in self.ref[name]:
            eng = self.unfused[name]
            out = eng.forward(batch, bs)
            self.ref[name][key] = (out, eng.fetch_interaction(bs), eng.last_dispatch(0))
        return self.ref[name][key]

    def close(self):
        for d in (self.fused, self.unfused, self.fp32):
            for e in d.values():
                e.close()


@pytest.fixture(scope="module")
def world():
    w = World(("dlrm_dot", "dlrm_cat"))
    yield w
    w.close()


def check_same_bits(net, fused, unfused, fp32, batch, bs, reference=None):
    got = fused.forward(batch, bs)
    log = fused.last_dispatch(0)
    inter = fused.fetch_interaction(bs)
    assert count_fused(log) == 1 and count_bf16(log) == 0, log
    # one MLP-side launch: nothing but the set's header, the gather and the fused launch
    assert sum(1 for t in log if "kernel" in t and not t.startswith(("sls", "fused_bf16_kernel"))) == 0, log
    if reference is None:
        exp = unfused.forward(batch, bs)
        reference = (exp, unfused.fetch_interaction(bs), unfused.last_dispatch(0))
    exp, exp_inter, exp_log = reference
    assert count_bf16(exp_log) == net.n_eligible() and count_fused(exp_log) == 0, exp_log
    assert np.array_equal(got, exp), (batch, bs, float(np.abs(got - exp).max()))
    assert np.array_equal(inter, exp_inter), (batch, bs)
    comp, _ = net.compose(unfused, batch, bs)
    assert np.array_equal(got, comp), (batch, bs, float(np.abs(got - comp).max()))
    plain = fp32.forward(batch, bs)
    assert count_fused(fp32.last_dispatch(0)) == 0
    assert not np.array_equal(got, plain), "the bf16 layers did not run"


# ------------------------------------------------------------------------------------------------
# 1. the option
def test_option_is_read_back_refused_out_of_range_and_inert_elsewhere():
    e = N.Engine(N.MODEL_DLRM, [16, 16], 8, [4, 8], [24, 4, 1], N.INTERACT_CAT, sigmoid_top=2,
                 max_batch=4, max_lookups=2, num_staged_batches=1, num_slots=1)
    try:
        assert e.get_option("mlp_bf16_fuse") == 0
        e.set_option("mlp_bf16_fuse", 1)
        assert e.get_option("mlp_bf16_fuse") == 1
        for bad in (2, -1):
            with pytest.raises(N.DrsError) as err:
                e.set_option("mlp_bf16_fuse", bad)
            assert err.value.code == N.ERR_BAD_ARG
            assert e.get_option("mlp_bf16_fuse") == 1
        e.set_option("mlp_bf16_fuse", 0)
        assert e.get_option("mlp_bf16_fuse") == 0
    finally:
        e.close()
    # W&D (with bf16 layers of its own): accepted, nothing changes
    net = nets()["wnd"]
    eng = unfused_engine(net)
    try:
        before = eng.forward(0, net.B), eng.last_dispatch(0)
        eng.set_option("mlp_bf16_fuse", 1)
        assert eng.get_option("mlp_bf16_fuse") == 1
        after = eng.forward(0, net.B), eng.last_dispatch(0)
        assert np.array_equal(before[0], after[0]) and before[1] == after[1]
        assert count_bf16(after[1]) == net.n_eligible() and count_fused(after[1]) == 0
    finally:
        eng.close()
    # DIN: accepted, nothing changes
    meta, _ = H.load_fixture("din_mini")
    args = H.args_from(meta["args"])
    din, lX, lS_l, lS_i, lT = H.materialize(args)
    din.create(lX[0], lS_l[0], lS_i[0], lT[0])
    try:
        din.engine.set_option("dispatch_log", 1)
        din.stage_batches(lX, lS_l, lS_i)
        n = len(lS_l[0][0])
        before = din.run_staged(0, n).copy(), din.engine.last_dispatch(0)
        din.engine.set_option("mlp_bf16_fuse", 1)
        assert din.engine.get_option("mlp_bf16_fuse") == 1
        after = din.run_staged(0, n).copy(), din.engine.last_dispatch(0)
        assert np.array_equal(before[0], after[0]) and before[1] == after[1]
    finally:
        din.engine.close()


# ------------------------------------------------------------------------------------------------
# 2. same bits as the layer-by-layer path
@pytest.mark.parametrize("batch,bs", GRID)
@pytest.mark.parametrize("name", ["dlrm_dot", "dlrm_cat"])
def test_fused_launch_returns_the_bits_of_the_unfused_path(world, name, batch, bs):
    net, fused, unfused, fp32 = world.get(name)
    check_same_bits(net, fused, unfused, fp32, batch, bs, world.reference(name, batch, bs))


# ------------------------------------------------------------------------------------------------
# 3. the 64 threshold inside the launch
def test_threshold_between_fp32_and_bf16_layers_inside_the_launch():
    # top 64-63-64-65-1: 64 x 63 and 63 x 64 stay fp32, 64 x 65 is bf16 with an N that is no multiple of 16
    net = threshold_net([64, 63, 64, 65, 1])
    assert net.n_eligible() == 2
    fused, unfused, fp32 = fused_engine(net), unfused_engine(net), logged(net.engine(0))
    try:
        fused.forward(0, net.B)
        if count_fused(fused.last_dispatch(0)) == 0:
            # the planner declines 63 / 65: then the set must run exactly as without the option ...
            for batch, bs in [(0, 1), (1, 16), (0, 17), (1, 200)]:
                got, exp = fused.forward(batch, bs), unfused.forward(batch, bs)
                assert fused.last_dispatch(0) == unfused.last_dispatch(0)
                assert np.array_equal(got, exp)
            for e in (fused, unfused, fp32):
                e.close()
            # ... and the fused case is checked on widths that are multiples of 4
            net = threshold_net([64, 60, 64, 68, 1])
            assert net.n_eligible() == 2
            fused, unfused, fp32 = fused_engine(net), unfused_engine(net), logged(net.engine(0))
        for batch, bs in [(0, 1), (1, 16), (0, 17), (1, 200)]:
            check_same_bits(net, fused, unfused, fp32, batch, bs)
    finally:
        for e in (fused, unfused, fp32):
            e.close()


# ------------------------------------------------------------------------------------------------
# 4. coalescing, two sets in flight
@pytest.mark.parametrize("name", ["dlrm_dot", "dlrm_cat"])
def test_coalesced_queries_are_bit_identical_to_single_runs(world, name):
    net, fused, unfused, fp32 = world.get(name)
    sizes = [net.B, 1, 37, 64, 65, 128, 5, 200]
    sets = [[((k + n_q) % 2, sizes[(k * 3 + n_q) % len(sizes)]) for k in range(n_q)] for n_q in (1, 5, 12, 16)]
    alone = {}

    def check(slot, jobs):
        out = fused.wait(slot, sum(n for _, n in jobs))
        log = fused.last_dispatch(slot)
        assert count_fused(log) == 1 and count_bf16(log) == 0, log
        v = 0
        for b, n in jobs:
            if (b, n) not in alone:
                alone[(b, n)] = unfused.forward(b, n)        # the query alone, on the layer-by-layer path
            assert np.array_equal(out[v:v + n], alone[(b, n)]), (name, len(jobs), b, n)
            v += n
    # two slots in flight: both sets are enqueued before either is waited for, each signs off by itself
    for first, second in [(sets[0], sets[1]), (sets[2], sets[3]), (sets[3], sets[0])]:
        fused.forward_multi_async(0, [b for b, _ in first], [n for _, n in first])
        fused.forward_multi_async(1, [b for b, _ in second], [n for _, n in second])
        check(1, second)
        check(0, first)
    # ... and the same query alone on the fused path
    for (b, n), exp in sorted(alone.items())[:4]:
        assert np.array_equal(fused.forward(b, n), exp)


# ------------------------------------------------------------------------------------------------
# 5. NaN and infinity stay in their rows
def test_nan_and_infinite_dense_rows_stay_in_their_rows():
    net = nets()["dlrm_cat"]
    bs, r_nan, r_inf = 40, 3, 17
    fused, unfused = fused_engine(net), unfused_engine(net)
    try:
        clean = fused.forward(0, bs)
        assert np.all(np.isfinite(clean))
        dense = net.dense[0].copy()
        dense[r_nan, 5] = np.nan
        dense[r_inf, 0] = np.inf
        for e in (fused, unfused):
            e.stage_batch(0, dense, net.idx[0], net.lens[0])
        got = fused.forward(0, bs)
        assert count_fused(fused.last_dispatch(0)) == 1
        exp = unfused.forward(0, bs)
        assert count_bf16(unfused.last_dispatch(0)) == net.n_eligible()
        differs = np.array([not np.array_equal(got[i], clean[i], equal_nan=True) for i in range(bs)])
        want = np.zeros(bs, bool)
        want[[r_nan, r_inf]] = True
        assert np.array_equal(differs, want), np.nonzero(differs)[0]
        assert np.array_equal(np.isnan(got), np.isnan(exp))
        assert np.array_equal(got, exp, equal_nan=True)
    finally:
        fused.close()
        unfused.close()


# ------------------------------------------------------------------------------------------------
# 6. composition and order
@pytest.mark.parametrize("order", ["first", "before_weights", "after"])
@pytest.mark.parametrize("dtype", [N.TABLE_FP16, N.TABLE_INT8_ROWWISE])
def test_composes_with_table_dtypes_in_any_option_order(dtype, order):
    net = nets()["dlrm_dot"]
    fused, unfused = fused_engine(net, order, table_dtype=dtype), unfused_engine(net, table_dtype=dtype)
    try:
        assert fused.get_option("table_dtype") == dtype and fused.get_option("mlp_dtype") == BF16
        assert fused.get_option("mlp_bf16_fuse") == 1
        for batch, bs in [(0, net.B), (1, 37)]:
            got, exp = fused.forward(batch, bs), unfused.forward(batch, bs)
            log = fused.last_dispatch(0)
            assert count_fused(log) == 1 and count_bf16(log) == 0, log
            assert count_bf16(unfused.last_dispatch(0)) == net.n_eligible()
            assert np.array_equal(got, exp), (dtype, order, batch, bs)
            assert np.array_equal(fused.fetch_interaction(bs), unfused.fetch_interaction(bs))
    finally:
        fused.close()
        unfused.close()


@pytest.mark.parametrize("name", ["dlrm_dot", "dlrm_cat"])
def test_layer_replacement_and_back_to_fp32(name):
    net = nets()[name]
    fused, unfused, fp32 = fused_engine(net, "first"), unfused_engine(net), logged(net.engine(0))
    try:
        base = fused.forward(0, net.B)
        assert np.array_equal(base, unfused.forward(0, net.B))
        # replace a bf16 layer and an fp32 layer: the same history on both engines
        layers = net.layers()
        for which, l, K, N_ in ([x for x in layers if x[2] >= 64 and x[3] >= 64][:1] + [x for x in layers if x[3] < 64][:1]):
            W, b = net.w[(which, l)]
            for e in (fused, unfused):
                e.set_fc(which, l, W * 0.5, b + 0.25)
            got, exp = fused.forward(0, net.B), unfused.forward(0, net.B)
            assert count_fused(fused.last_dispatch(0)) == 1
            assert np.array_equal(got, exp) and not np.array_equal(got, base)
            for e in (fused, unfused):
                e.set_fc(which, l, W, b)
            assert np.array_equal(fused.forward(0, net.B), base)
        # mlp_dtype 0: an fp32 engine's outputs and log, the option still set
        fused.set_option("mlp_dtype", 0)
        assert fused.get_option("mlp_bf16_fuse") == 1
        assert np.array_equal(fused.forward(1, 77), fp32.forward(1, 77))
        assert fused.last_dispatch(0) == fp32.last_dispatch(0)
        fused.set_option("mlp_dtype", BF16)
        assert np.array_equal(fused.forward(0, net.B), base)
        assert count_fused(fused.last_dispatch(0)) == 1
    finally:
        for e in (fused, unfused, fp32):
            e.close()


# ------------------------------------------------------------------------------------------------
# 7. fallback: where the one-launch form does not apply the set runs as without the option
@pytest.mark.parametrize("key,value", [("mlp_fuse", 0), ("mlp_wide_kn", 128 * 96)])
def test_fallback_is_the_unfused_path(key, value):
    net = nets()["dlrm_cat"]              # (mlp_wide_kn 12 288: its 128 x 96 top layer is wide)
    fused, unfused = fused_engine(net), unfused_engine(net)
    try:
        for e in (fused, unfused):
            e.set_option(key, value)
        for batch, bs in [(0, net.B), (1, 17)]:
            got, exp = fused.forward(batch, bs), unfused.forward(batch, bs)
            assert fused.last_dispatch(0) == unfused.last_dispatch(0)
            assert count_fused(fused.last_dispatch(0)) == 0
            assert np.array_equal(got, exp)
    finally:
        fused.close()
        unfused.close()
