"""NCF's one-launch form (Sum + MLP branch + predictor) with its bf16 layers inside (-m gpu): engine option
"mlp_bf16_fuse" 1 on top of "mlp_dtype" 2, fused_bf16_sum_kernel, logged as fused_bf16_kernel<sum>[...].

The expected values are never the launch under test: they are the layer-by-layer path of "mlp_dtype" 2 alone
(add_rows_kernel, one gemm_bf16_kernel launch per bf16 layer, chains in between) and the forward composed from operator
calls (Net.compose: drs_sls, drs_fc; mf = emb0 + emb1 in numpy, one fp32 add per element like the kernels').  An
output's bits depend on its row of x and its row of W only, so the fused launch must return the same bits:
every comparison below is np.array_equal, none has a tolerance.

The shapes are the smallest that stand on each edge of the kernel (SHAPES).  The LDS budget cases are computed from the
planner's layout (lds_bytes: X0 | RS | P | Q, slabs of 16 rows, 64 m + 4 floats apart, the DLRM kernel's pitch): with it
D 32, branch 64-2304-16, predictor 48 -> 1 takes 156 416 of the 159 744 bytes and fits, branch 64-2368-16 takes 160 512
and does not (both first layers are below mlp_wide_kn).

Every engine runs with sls_exact 1 and dispatch_log 1.
"""
import numpy as np
import pytest

from deeprecsys_amd import _native as N
from tests.test_bf16_fused import count_fused, fused_engine, unfused_engine
from tests.test_bf16_mlp import BF16, Net, count_bf16, eligible, nets

pytestmark = pytest.mark.gpu

SIZES = [1, 15, 16, 17, 64]
LDS_BUDGET = 156 * 1024


def ncf(D, branch, fin, seed, B=64):
    return Net(N.MODEL_NCF, D, 4, [1], branch, fin=fin, L=1, B=B, seed=seed)


def shapes():
    return {
        # bf16, fp32 (N < 64), fp32 (K < 64), and a bf16 LAST layer that writes the outputs
        "ncf": nets()["ncf"],
        # the reference's shape: an fp32 last layer with N = 1
        "ncf_ref_shape": ncf(64, [128, 256, 128, 64], 1, 31),
        # a bf16 predictor with K = 92 padded to 128 (slab columns 92 .. 127 must read zero); an fp32 first layer (K = 40)
        "ncf_pad": ncf(20, [40, 64, 72], 64, 32),
        # D % 4 != 0: scalar staging, and the branch's bf16 last layer stores behind 10 columns of mf
        "ncf_scalar": ncf(10, [20, 64, 64], 1, 33),
        # the shortest chain
        "ncf_one_layer": ncf(32, [64, 64], 1, 34),
        # DRS_MAX_CHAIN layers: bf16, bf16, fp32, fp32, bf16, fp32
        "ncf_six": ncf(32, [64, 128, 64, 32, 64, 64, 16], 1, 35),
    }


NAMES = sorted(shapes())


def pad64(n):
    return (n + 63) // 64 * 64


def lds_bytes(D, branch):
    """plan_fused_bf16_sum's layout: X0 (the branch input) | RS (the predictor's input) | P | Q (ping-pong layer outputs)."""
    floats = 16 * (pad64(branch[0]) + 4) + 16 * (pad64(D + branch[-1]) + 4)
    mids = branch[1:-1]
    for half in (mids[0::2], mids[1::2]):
        if half:
            floats += 16 * (max(pad64(w) for w in half) + 4)
    return 4 * floats


def fused_tokens(log):
    return [t for t in log if t.startswith("fused_bf16_kernel")]


def mlp_side(log):
    """Every launch of the set but the gather (the log's first token is the set's header)."""
    return [t for t in log if "kernel" in t and not t.startswith("sls")]


def assert_one_launch(net, log):
    assert len(fused_tokens(log)) == 1 and fused_tokens(log)[0].startswith("fused_bf16_kernel<sum>["), log
    assert count_bf16(log) == 0 and not [t for t in log if t.startswith("add_rows_kernel")], log
    assert mlp_side(log) == fused_tokens(log), log
    tok = fused_tokens(log)[0]
    assert "%d layers, %d bf16, %d B lds]" % (len(net.layers()), net.n_eligible(), lds_bytes(net.D, net.ln_top)) in tok, tok


def assert_unfused_log(net, log):
    assert count_fused(log) == 0 and count_bf16(log) == net.n_eligible(), log
    assert len([t for t in log if t.startswith("add_rows_kernel")]) == 1, log


class World(object):
    """Per shape: the fused engine and the layer-by-layer bf16 engine, and the latter's results per (batch, size), computed once."""

    def __init__(self):
        self.all = shapes()
        self.eng, self.ref = {}, {}

    def get(self, name):
        if name not in self.eng:
            net = self.all[name]
            self.eng[name] = (fused_engine(net), unfused_engine(net))
            self.ref[name] = {}
        return (self.all[name],) + self.eng[name]

    def reference(self, name, batch, bs):
        """(outputs, interaction tensor, dispatch log) of the layer-by-layer engine."""
        key = (batch, bs)
        if key not in self.ref[name]:
            unfused = self.eng[name][1]
            out = unfused.forward(batch, bs)
            self.ref[name][key] = (out, unfused.fetch_interaction(bs), unfused.last_dispatch(0))
        return self.ref[name][key]

    def close(self):
        for pair in self.eng.values():
            for e in pair:
                e.close()


@pytest.fixture(scope="module")
def world():
    w = World()
    yield w
    w.close()


# ------------------------------------------------------------------------------------------------
# 1. it happens
@pytest.mark.parametrize("name", NAMES)
def test_ncf_set_is_one_launch_whenever_the_option_was_set(world, name):
    net, fused, unfused = world.get(name)
    assert net.n_eligible() >= 1 and lds_bytes(net.D, net.ln_top) <= LDS_BUDGET
    assert [eligible(K, N_) for _, _, K, N_ in net.layers()].count(True) == net.n_eligible()
    logs = []
    for order in ("after", "first", "before_weights"):
        eng = fused if order == "after" else fused_engine(net, order)
        try:
            assert eng.get_option("mlp_bf16_fuse") == 1 and eng.get_option("mlp_dtype") == BF16
            for batch, bs in [(0, net.B), (1, 17)]:
                eng.forward(batch, bs)
                log = eng.last_dispatch(0)
                assert_one_launch(net, log)
                logs.append((order, batch, bs, log))
        finally:
            if eng is not fused:
                eng.close()
    for i, (order, batch, bs, log) in enumerate(logs):        # the same log in every order
        assert log == logs[i % 2][3], (order, batch, bs, log, logs[i % 2][3])
    # ... and without the option: the layer-by-layer path
    assert_unfused_log(net, world.reference(name, 0, net.B)[2])


# ------------------------------------------------------------------------------------------------
# 2. same bits
@pytest.mark.parametrize("name", NAMES)
def test_same_bits_as_the_layer_by_layer_path_and_the_composed_forward(world, name):
    net, fused, unfused = world.get(name)
    for i, bs in enumerate(SIZES):
        batch = i % 2
        got = fused.forward(batch, bs)
        log = fused.last_dispatch(0)
        inter = fused.fetch_interaction(bs)
        assert_one_launch(net, log)
        exp, exp_inter, exp_log = world.reference(name, batch, bs)
        assert_unfused_log(net, exp_log)
        print("%s bs %d: max |fused - unfused| = %g" % (name, bs, float(np.abs(got - exp).max())))
        assert got.shape == (bs, net.fin) and inter.shape == (bs, net.D + net.ln_top[-1])
        assert np.array_equal(got, exp), (name, batch, bs)
        assert np.array_equal(inter, exp_inter), (name, batch, bs)
        comp, _ = net.compose(unfused, batch, bs)
        print("%s bs %d: max |unfused - composed| = %g" % (name, bs, float(np.abs(exp - comp).max())))
        assert np.array_equal(got, comp), (name, batch, bs)
        assert np.all(np.isfinite(got))


def test_the_bf16_layers_ran(world):
    net, fused, unfused = world.get("ncf_ref_shape")
    fp32 = net.engine(0)
    try:
        assert not np.array_equal(fused.forward(0, net.B), fp32.forward(0, net.B))
    finally:
        fp32.close()


# ------------------------------------------------------------------------------------------------
# 3. coalescing, two sets in flight
@pytest.mark.parametrize("name", ["ncf", "ncf_pad", "ncf_scalar"])
def test_coalesced_queries_are_bit_identical_to_single_runs(world, name):
    net, fused, unfused = world.get(name)
    draw = (1, 17, 0, 64, 16)
    sets = [[((k + n_q) % 2, draw[(2 * k + n_q) % len(draw)]) for k in range(n_q)] for n_q in (3, 16)]
    assert all(any(n == 0 for _, n in jobs) and any(n == 64 for _, n in jobs) for jobs in sets)
    alone = {}

    def check(slot, jobs):
        total = sum(n for _, n in jobs)
        out = fused.wait(slot, total)
        assert_one_launch(net, fused.last_dispatch(slot))
        rows = sum((n + 63) // 64 * 64 for _, n in jobs)
        inter = fused.fetch_interaction(rows, slot)
        unfused.forward_multi_async(slot, [b for b, _ in jobs], [n for _, n in jobs])
        exp = unfused.wait(slot, total)
        assert_unfused_log(net, unfused.last_dispatch(slot))
        exp_inter = unfused.fetch_interaction(rows, slot)
        assert np.array_equal(out, exp)
        v = r = 0
        for b, n in jobs:
            if n and (b, n) not in alone:
                alone[(b, n)] = unfused.forward(b, n)        # the query alone, on the layer-by-layer path
            if n:
                assert np.array_equal(out[v:v + n], alone[(b, n)]), (name, len(jobs), b, n)
                assert np.array_equal(inter[r:r + n], exp_inter[r:r + n]), (name, len(jobs), b, n)
            v += n
            r += (n + 63) // 64 * 64
    # both sets are enqueued before either is waited for, each signs off by itself
    for first, second in [(sets[0], sets[1]), (sets[1], sets[0])]:
        fused.forward_multi_async(0, [b for b, _ in first], [n for _, n in first])
        fused.forward_multi_async(1, [b for b, _ in second], [n for _, n in second])
        check(1, second)
        check(0, first)
    for (b, n), exp in sorted(alone.items()):
        assert np.array_equal(fused.forward(b, n), exp)


# ------------------------------------------------------------------------------------------------
# 4. NaN and infinity stay in their rows
def test_nan_and_infinite_embedding_rows_stay_in_their_samples():
    net = shapes()["ncf"]
    bs, r_mf, r_x2, r_x3 = 40, 3, 17, 22
    # one table row per sample, so that a poisoned row belongs to one sample only
    idx = [np.arange(net.B, dtype=np.int64) for _ in range(net.T)]
    fused, unfused = fused_engine(net), unfused_engine(net)
    try:
        for e in (fused, unfused):
            e.stage_batch(0, None, idx, net.lens[0])
        clean = fused.forward(0, bs)
        assert np.all(np.isfinite(clean)) and np.array_equal(clean, unfused.forward(0, bs))
        tables = [W.copy() for W in net.tables]
        tables[0][r_mf, 5] = np.nan
        tables[2][r_x2, net.D - 1] = np.nan
        tables[3][r_x3, 0] = np.inf
        for e in (fused, unfused):
            for t in (0, 2, 3):
                e.set_table(t, tables[t])
        got, inter = fused.forward(0, bs), fused.fetch_interaction(bs)
        assert_one_launch(net, fused.last_dispatch(0))
        exp, exp_inter = unfused.forward(0, bs), unfused.fetch_interaction(bs)
        assert_unfused_log(net, unfused.last_dispatch(0))
        differs = np.array([not np.array_equal(got[i], clean[i], equal_nan=True) for i in range(bs)])
        want = np.zeros(bs, bool)
        want[[r_mf, r_x2, r_x3]] = True
        assert np.array_equal(differs, want), np.nonzero(differs)[0]
        assert np.array_equal(np.isnan(got), np.isnan(exp)) and np.array_equal(got, exp, equal_nan=True)
        assert np.array_equal(np.isnan(inter), np.isnan(exp_inter)) and np.array_equal(inter, exp_inter, equal_nan=True)
        assert np.isnan(inter[r_mf, 5]) and np.isnan(inter[:, :net.D]).sum() == 1      # mf = emb0 + emb1, in the sample's row only
    finally:
        fused.close()
        unfused.close()


# ------------------------------------------------------------------------------------------------
# 5. fallbacks are the path without the option
def check_fallback(net, fused, plain, fp32_form=False):
    for batch, bs in [(0, net.B), (1, 17), (0, 1)]:
        got, exp = fused.forward(batch, bs), plain.forward(batch, bs)
        log = fused.last_dispatch(0)
        assert log == plain.last_dispatch(0), (log, plain.last_dispatch(0))
        assert count_fused(log) == 0, log
        assert np.array_equal(got, exp)
        assert np.array_equal(fused.fetch_interaction(bs), plain.fetch_interaction(bs))
        if fp32_form:       # the fp32 one-launch form: Sum, branch and predictor in one stream-kernel launch
            assert len(mlp_side(log)) == 1 and mlp_side(log)[0].startswith("stream") and count_bf16(log) == 0, log
        else:
            assert count_bf16(log) == net.n_eligible() and len(mlp_side(log)) > 1, log


def with_engines(net, check, before=None):
    fused, plain = fused_engine(net), unfused_engine(net)
    try:
        for e in (fused, plain):
            if before:
                e.set_option(*before)
        check(fused, plain)
    finally:
        fused.close()
        plain.close()


@pytest.mark.parametrize("key,value", [("mlp_fuse", 0), ("mlp_wide_kn", 128 * 256)])
def test_fallback_by_option_is_the_unfused_path(key, value):
    net = shapes()["ncf"]                   # (mlp_wide_kn 32 768: its 128 x 256 branch layer is wide)
    with_engines(net, lambda fused, plain: check_fallback(net, fused, plain), before=(key, value))


def test_fallback_seven_layer_branch():
    net = ncf(32, [64, 128, 64, 32, 64, 64, 16, 16], 1, 36)
    assert len(net.ln_top) - 1 == 7 and net.n_eligible() == 3
    with_engines(net, lambda fused, plain: check_fallback(net, fused, plain))


def test_model_without_a_bf16_layer_keeps_the_fp32_one_launch_form():
    net = ncf(16, [32, 16, 8], 1, 37)
    assert net.n_eligible() == 0
    with_engines(net, lambda fused, plain: check_fallback(net, fused, plain, fp32_form=True))


def test_mlp_dtype_0_with_the_option_still_set_is_an_fp32_engine():
    net = shapes()["ncf"]
    fused, fp32 = fused_engine(net), net.engine(0)
    try:
        fp32.set_option("dispatch_log", 1)
        base = fused.forward(0, net.B)
        assert_one_launch(net, fused.last_dispatch(0))
        fused.set_option("mlp_dtype", 0)
        assert fused.get_option("mlp_bf16_fuse") == 1
        for batch, bs in [(0, net.B), (1, 17)]:
            assert np.array_equal(fused.forward(batch, bs), fp32.forward(batch, bs))
            assert fused.last_dispatch(0) == fp32.last_dispatch(0) and count_fused(fused.last_dispatch(0)) == 0
        fused.set_option("mlp_dtype", BF16)
        assert np.array_equal(fused.forward(0, net.B), base)
        assert_one_launch(net, fused.last_dispatch(0))
    finally:
        fused.close()
        fp32.close()


def test_lds_budget_one_shape_on_each_side():
    fits, over = [64, 2304, 16], [64, 2368, 16]
    assert lds_bytes(32, fits) == 156416 <= LDS_BUDGET < lds_bytes(32, over) == 160512
    for branch in (fits, over):
        assert branch[0] * branch[1] < 256 * 1024            # (not a wide layer: below the default mlp_wide_kn)
    net = ncf(32, fits, 1, 38)
    fused, plain = fused_engine(net), unfused_engine(net)
    try:
        for batch, bs in [(0, net.B), (1, 17)]:
            got, exp = fused.forward(batch, bs), plain.forward(batch, bs)
            assert_one_launch(net, fused.last_dispatch(0))
            assert np.array_equal(got, exp)
            assert np.array_equal(fused.fetch_interaction(bs), plain.fetch_interaction(bs))
    finally:
        fused.close()
        plain.close()
    net = ncf(32, over, 1, 39)
    with_engines(net, lambda fused, plain: check_fallback(net, fused, plain))


# ------------------------------------------------------------------------------------------------
# 6. composes with the table types
@pytest.mark.parametrize("order", ["first", "after"])
@pytest.mark.parametrize("dtype", [N.TABLE_FP16, N.TABLE_INT8_ROWWISE])
def test_composes_with_table_dtypes_in_either_option_order(dtype, order):
    net = shapes()["ncf_pad"]
    fused, unfused = fused_engine(net, order, table_dtype=dtype), unfused_engine(net, table_dtype=dtype)
    try:
        assert fused.get_option("table_dtype") == dtype and fused.get_option("mlp_dtype") == BF16
        assert fused.get_option("mlp_bf16_fuse") == 1
        for batch, bs in [(0, net.B), (1, 17)]:
            got, exp = fused.forward(batch, bs), unfused.forward(batch, bs)
            assert_one_launch(net, fused.last_dispatch(0))
            assert_unfused_log(net, unfused.last_dispatch(0))
            assert np.array_equal(got, exp), (dtype, order, batch, bs)
            assert np.array_equal(fused.fetch_interaction(bs), unfused.fetch_interaction(bs))
    finally:
        fused.close()
        unfused.close()


# ------------------------------------------------------------------------------------------------
# 7. layer replacement
def test_layer_replacement_after_the_first_forward():
    net = shapes()["ncf"]
    fused, unfused = fused_engine(net, "first"), unfused_engine(net)
    try:
        base = fused.forward(0, net.B)
        assert np.array_equal(base, unfused.forward(0, net.B))
        # a bf16 branch layer, then the (bf16) predictor: the same history on both engines
        for which, l in [(N.MLP_TOP, 0), (N.MLP_FINAL, 0)]:
            W, b = net.w[(which, l)]
            assert eligible(W.shape[1], W.shape[0])
            for e in (fused, unfused):
                e.set_fc(which, l, W * 0.5, b + 0.25)
            got, exp = fused.forward(0, net.B), unfused.forward(0, net.B)
            assert_one_launch(net, fused.last_dispatch(0))
            assert np.array_equal(got, exp) and not np.array_equal(got, base)
            assert np.array_equal(fused.fetch_interaction(net.B), unfused.fetch_interaction(net.B))
            for e in (fused, unfused):
                e.set_fc(which, l, W, b)
            assert np.array_equal(fused.forward(0, net.B), base)
            assert_one_launch(net, fused.last_dispatch(0))
    finally:
        fused.close()
        unfused.close()
