"""The wide FC layers on the bf16 matrix cores (-m gpu): engine option "mlp_dtype" 2.

The rule: with mlp_dtype 2 an FC layer of the bottom, top, final or task MLP with K >= 64 and N >= 64 computes
y = act(sum_k bf16(x[k]) * bf16(W[n][k]) + b[n]) -- operands rounded to bf16 (nearest even, NaN stays NaN), exact
products, fp32 accumulation, fp32 bias / activation / output; everything else is as with mlp_dtype 0.

The checker is the numpy restatement below (float64 accumulation over operands rounded with torch's bfloat16); it shares
no code with the engine.  A bf16 layer is held to the textbook bound of an fp32 sum of K exact terms in any order, with
the unit roundoff doubled (the matrix core's internal adder is not documented to round to nearest):

    |got - exp| <= K 2^-23 sum_k |bf16(x_k) bf16(W_nk)| + 2^-23 |exp|        (before the activation)

ReLU and sigmoid do not enlarge it (Lipschitz 1 and 1/4); the sigmoid gets the allowance of the fp32 drs_fc parity test
(rtol 1e-6, atol 1e-7: expf differs by a few ulp between libm and the device).  Whole models are checked layer by layer
with no measured tolerance: the engine's output is bit-identical to the same forward composed from operator calls on
the same handle, and every bf16 layer of that composition meets the bound on the input it actually got.

ReLU maps a NaN to 0 in every FC kernel of this library (v > 0 ? v : 0, fp32 and bf16 alike), so "NaN in -> NaN out" is
checked without activation and through the sigmoid.  (The fp32 forms are held to that rule, every one of them, by
tests/test_mlp_nonfinite.py; stream4_kernel's fmaxf(v, 0.f) gives the same 0.)

profiles/r09_bf16_mlp.md records what DRS_BF16_REPORT=<file> makes these tests write: per shape the largest measured
fraction of the bound, per model the largest difference from the fp32 engine.
"""
import json
import os

import numpy as np
import pytest

from deeprecsys_amd import _native as N
from tests import helpers as H

pytestmark = pytest.mark.gpu

BF16 = 2
U = 2.0 ** -23


def _report(**kw):
    path = os.environ.get("DRS_BF16_REPORT")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(kw) + "\n")


def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch


def bf(a):
    """a rounded to bfloat16 (nearest even) and widened back to fp32."""
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16).to(torch.float32).numpy()


def eligible(K, N_):
    return K >= 64 and N_ >= 64


def restate(x, W, b):
    """(sum + bias in float64, sum of |products|) of a bf16 layer, before the activation."""
    xa, Wa = bf(x).astype(np.float64), bf(W).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        s = xa @ Wa.T
        mag = np.abs(xa) @ np.abs(Wa).T
    if b is not None:
        s = s + np.asarray(b, np.float64)[None, :]
    return s, mag


def act64(s, act):
    if act == N.ACT_RELU:
        return np.maximum(s, 0.0)
    if act == N.ACT_SIGMOID:
        with np.errstate(over="ignore"):
            return 1.0 / (1.0 + np.exp(-s))
    return s


def bound_ratio(got, x, W, b, act):
    """max over the elements of |got - exp| / bound (<= 1 passes); rows holding a NaN or an infinity are left to the caller."""
    K = np.asarray(x).shape[1]
    s, mag = restate(x, W, b)
    exp = act64(s, act)
    bound = K * U * mag + U * np.abs(s)
    if act == N.ACT_SIGMOID:
        bound = bound + 1e-7 + 1e-6 * np.abs(exp)
    fin = np.isfinite(s)
    err = np.abs(got.astype(np.float64) - exp)
    tiny = np.finfo(np.float64).tiny
    ratio = np.where(fin, err / np.maximum(bound, tiny), 0.0)
    ratio = np.where(fin & (err == 0), 0.0, ratio)
    assert np.all(np.isfinite(got[fin])), "a finite sum came out as NaN / infinity"
    return float(ratio.max()) if ratio.size else 0.0


def fc_op(eng, x, W, b, act):
    """drs_fc on the handle: follows its mlp_dtype and the shape rule."""
    torch = torch_cuda()
    x = np.ascontiguousarray(x, np.float32)
    M, K = x.shape
    N_ = W.shape[0]
    dx, dW = torch.from_numpy(x).cuda(), torch.from_numpy(np.ascontiguousarray(W, np.float32)).cuda()
    db = torch.from_numpy(np.ascontiguousarray(b, np.float32)).cuda() if b is not None else None
    y = torch.full((M, N_), float("nan"), device="cuda")
    torch.cuda.synchronize()   # inputs/outputs were produced on torch's stream, the op runs on the engine's
    eng.fc(dx.data_ptr(), M, K, dW.data_ptr(), db.data_ptr() if db is not None else None, N_, act, y.data_ptr())
    return y.cpu().numpy()


def sls_op(eng, W, idx, lens):
    torch = torch_cuda()
    W = np.ascontiguousarray(W, np.float32)
    lens = np.ascontiguousarray(lens, np.int32)
    idx = np.ascontiguousarray(np.asarray(idx)[:int(lens.sum())], np.int32)
    dW, dl = torch.from_numpy(W).cuda(), torch.from_numpy(lens).cuda()
    di = torch.from_numpy(idx if idx.size else np.zeros(1, np.int32)).cuda()
    out = torch.full((lens.size, W.shape[1]), float("nan"), device="cuda")
    torch.cuda.synchronize()
    eng.sls(dW.data_ptr(), W.shape[0], W.shape[1], di.data_ptr(), dl.data_ptr(), lens.size, idx.size, out.data_ptr(),
            exact_order=True)
    return out.cpu().numpy()


def dot_op(eng, T, F, D, itself):
    torch = torch_cuda()
    B = T.shape[0]
    P = F * (F + 1) // 2 if itself else F * (F - 1) // 2
    dT = torch.from_numpy(np.ascontiguousarray(T, np.float32)).cuda()
    R = torch.full((B, D + P), float("nan"), device="cuda")
    torch.cuda.synchronize()
    eng.interact_dot(dT.data_ptr(), B, F, D, itself, R.data_ptr())
    return R.cpu().numpy()


@pytest.fixture(scope="module")
def op_engine():
    """A tiny engine used as the handle of the operator-level calls, with mlp_dtype 2."""
    e = N.Engine(N.MODEL_DLRM, [16, 16], 8, [4, 8], [24, 4, 1], N.INTERACT_CAT, sigmoid_top=2,
                 max_batch=4, max_lookups=2, num_staged_batches=1, num_slots=1)
    e.set_option("mlp_dtype", BF16)
    yield e
    e.close()


# ------------------------------------------------------------------------------------------------
# 1. the option exists
def test_option_is_accepted_read_back_and_refused_where_it_does_not_apply():
    e = N.Engine(N.MODEL_DLRM, [16, 16], 8, [4, 8], [24, 4, 1], N.INTERACT_CAT, sigmoid_top=2,
                 max_batch=4, max_lookups=2, num_staged_batches=1, num_slots=1)
    try:
        assert N.MLP_FP32 == 0 and N.MLP_BF16 == 2
        assert e.get_option("mlp_dtype") == 0
        e.set_option("mlp_dtype", 2)
        assert e.get_option("mlp_dtype") == 2
        for bad in (1, 3, -1, 8):
            with pytest.raises(N.DrsError) as err:
                e.set_option("mlp_dtype", bad)
            assert err.value.code == N.ERR_BAD_ARG
            assert e.get_option("mlp_dtype") == 2
        e.set_option("mlp_dtype", 0)
        assert e.get_option("mlp_dtype") == 0
    finally:
        e.close()
    din = N.Engine(N.MODEL_DIN, [50] * 5, 8, [24, 4, 8], [32, 8, 1], max_batch=4, max_lookups=2, num_staged_batches=1)
    dien = N.Engine(N.MODEL_DIEN, [50] * 5, 16, [16, 8], [56, 8, 1], max_batch=4, max_lookups=2, num_staged_batches=1)
    for eng in (din, dien):
        try:
            with pytest.raises(N.DrsError) as err:
                eng.set_option("mlp_dtype", 2)
            assert err.value.code == N.ERR_UNSUPPORTED
            assert "mlp_dtype" in str(err.value)
            assert eng.get_option("mlp_dtype") == 0
            eng.set_option("mlp_dtype", 0)          # (the value it has: nothing to refuse)
        finally:
            eng.close()


# ------------------------------------------------------------------------------------------------
# 2. one layer against the derived bound
KN = [(64, 64), (65, 96), (96, 65), (100, 256), (256, 100), (1000, 64), (64, 1000), (1376, 1000), (2560, 1376), (1000, 2560),
      (256, 256), (1376, 96), (65, 65), (2560, 64), (100, 100)]
MS = [1, 15, 64, 200, 3072]


@pytest.mark.parametrize("act", [N.ACT_NONE, N.ACT_RELU, N.ACT_SIGMOID])
@pytest.mark.parametrize("K,N_", KN)
def test_one_layer_meets_the_derived_bound(op_engine, K, N_, act):
    worst = 0.0
    for i, M in enumerate(MS):
        if M == 3072 and K * N_ > 1376 * 1000 and act != N.ACT_RELU:
            continue                                  # (the largest shapes at 3 072 rows once)
        rng = np.random.RandomState(K * 31 + N_ * 7 + M + act)
        x = rng.uniform(-2, 2, (M, K)).astype(np.float32)
        W = rng.normal(0, 1.0 / np.sqrt(K), (N_, K)).astype(np.float32)
        b = rng.normal(0, 0.1, N_).astype(np.float32) if (i + K) % 2 == 0 else None
        got = fc_op(op_engine, x, W, b, act)
        r = bound_ratio(got, x, W, b, act)
        worst = max(worst, r)
        print("K %d N %d M %d act %d bias %s: |err| / bound = %.4f" % (K, N_, M, act, b is not None, r))
        assert r <= 1.0, (K, N_, M, act, r)
    _report(test="one_layer", K=K, N=N_, act=act, worst_fraction_of_bound=worst)


@pytest.mark.parametrize("act", [N.ACT_NONE, N.ACT_SIGMOID, N.ACT_RELU])
@pytest.mark.parametrize("M,K,N_", [(15, 65, 96), (200, 256, 100), (64, 1000, 64)])
def test_nan_and_infinite_rows_stay_in_their_rows(op_engine, M, K, N_, act):
    rng = np.random.RandomState(M + K + N_)
    x = rng.uniform(-1, 1, (M, K)).astype(np.float32)
    W = rng.normal(0, 0.1, (N_, K)).astype(np.float32)
    b = rng.normal(0, 0.1, N_).astype(np.float32)
    r_nan, r_pinf, r_ninf = 1, M // 2, M - 1
    x[r_nan, K - 1] = np.nan                 # (the last k: inside the K tail's chunk)
    x[r_pinf, 0] = np.inf
    x[r_ninf, K // 2] = -np.inf
    got = fc_op(op_engine, x, W, b, act)
    s, _ = restate(x, W, b)
    exp = act64(s, act)
    special = np.zeros(M, bool)
    special[[r_nan, r_pinf, r_ninf]] = True
    if act != N.ACT_RELU:                    # (ReLU maps NaN to 0, like every FC kernel here)
        assert np.all(np.isnan(got[r_nan])), "NaN in -> NaN out"
        assert np.array_equal(np.isnan(got[special]), np.isnan(exp[special]))
        ok = ~np.isnan(exp[special])
        assert np.array_equal(got[special][ok], exp[special][ok].astype(np.float32))   # +-inf, or the sigmoid's 0 / 1
    clean = ~special
    assert np.all(np.isfinite(got[clean]))
    assert bound_ratio(got[clean], x[clean], W, b, act) <= 1.0


@pytest.mark.parametrize("M,K,N_", [(33, 63, 256), (200, 256, 63), (64, 32, 32), (5, 1000, 1), (300, 16, 1024)])
def test_layers_below_64_are_bit_identical_to_fp32(op_engine, M, K, N_):
    ref = N.Engine(N.MODEL_DLRM, [16, 16], 8, [4, 8], [24, 4, 1], N.INTERACT_CAT, sigmoid_top=2,
                   max_batch=4, max_lookups=2, num_staged_batches=1, num_slots=1)
    try:
        rng = np.random.RandomState(M + K + N_)
        x = rng.uniform(-1, 1, (M, K)).astype(np.float32)
        W = rng.normal(0, 0.1, (N_, K)).astype(np.float32)
        b = rng.normal(0, 0.1, N_).astype(np.float32)
        for act in (N.ACT_NONE, N.ACT_RELU, N.ACT_SIGMOID):
            assert np.array_equal(fc_op(op_engine, x, W, b, act), fc_op(ref, x, W, b, act)), (M, K, N_, act)
    finally:
        ref.close()


# ------------------------------------------------------------------------------------------------
# 3a. every tile shape gives the same bits
@pytest.mark.parametrize("M,K,N_", [(300, 896, 1024), (65, 68, 130), (2048, 1024, 512), (31, 132, 64), (129, 64, 200),
                                    (257, 1376, 96), (4096, 65, 65), (1, 100, 1000)])
def test_every_tile_shape_gives_the_same_bits(op_engine, M, K, N_):
    rng = np.random.RandomState(M * 7 + K + N_)
    x = rng.uniform(-1, 1, (M, K)).astype(np.float32)
    W = rng.normal(0, 0.1, (N_, K)).astype(np.float32)
    b = rng.normal(0, 0.1, N_).astype(np.float32)
    outs = {}
    try:
        for tile in (0, 44, 22, 12):
            op_engine.set_option("mlp_bf16_tile", tile)
            outs[tile] = fc_op(op_engine, x, W, b, N.ACT_RELU)
    finally:
        op_engine.set_option("mlp_bf16_tile", 0)
    assert bound_ratio(outs[0], x, W, b, N.ACT_RELU) <= 1.0
    for tile in (44, 22, 12):
        assert np.array_equal(outs[tile], outs[0]), tile


# ------------------------------------------------------------------------------------------------
# whole models
class Net(object):
    """One small model: its shapes, weights, tables and staged inputs; engines are built from it with any options."""

    def __init__(self, kind, D, T, ln_bot, ln_top, sigmoid_top=-1, dot=False, itself=False, ln_task=None, num_tasks=0,
                 fin=0, L=2, B=200, seed=0, n_batches=2):
        self.kind, self.D, self.T, self.ln_bot, self.ln_top = kind, D, T, list(ln_bot), list(ln_top)
        self.sigmoid_top, self.dot, self.itself, self.ln_task, self.num_tasks = sigmoid_top, dot, itself, ln_task, num_tasks
        self.fin, self.L, self.B = fin, L, B
        rng = np.random.RandomState(seed)
        self.rows = [301 + 17 * t for t in range(T)]
        self.tables = [rng.uniform(-1, 1, (r, D)).astype(np.float32) for r in self.rows]
        self.w = {}

        def mlp(which, ln):
            for l in range(len(ln) - 1):
                self.w[(which, l)] = (rng.normal(0, 1.0 / np.sqrt(ln[l]), (ln[l + 1], ln[l])).astype(np.float32),
                                      rng.normal(0, 0.1, ln[l + 1]).astype(np.float32))
        mlp(N.MLP_BOT, self.ln_bot)
        mlp(N.MLP_TOP, self.ln_top)
        for k in range(num_tasks):
            mlp(N.MLP_TASK0 + k, ln_task)
        if kind == N.MODEL_NCF:
            mlp(N.MLP_FINAL, [D + ln_top[-1], fin])
        self.m_den = ln_bot[0] if kind != N.MODEL_NCF else 0
        self.dense, self.idx, self.lens = [], [], []
        for _ in range(n_batches):
            self.dense.append(rng.uniform(-1, 1, (B, self.m_den)).astype(np.float32) if self.m_den else None)
            ln = [np.full(B, L, np.int32) for _ in range(T)]
            self.idx.append([rng.randint(0, self.rows[t], size=B * L).astype(np.int64) for t in range(T)])
            self.lens.append(ln)

    def layers(self):
        """Every FC layer of the model in the order a forward runs them: (mlp, layer, K, N)."""
        out = []
        for which, ln in [(N.MLP_BOT, self.ln_bot), (N.MLP_TOP, self.ln_top)] + \
                         [(N.MLP_TASK0 + k, self.ln_task) for k in range(self.num_tasks)]:
            out += [(which, l, ln[l], ln[l + 1]) for l in range(len(ln) - 1)]
        if self.kind == N.MODEL_NCF:
            out.append((N.MLP_FINAL, 0, self.D + self.ln_top[-1], self.fin))
        return out

    def n_eligible(self):
        return sum(1 for _, _, K, N_ in self.layers() if eligible(K, N_))

    def engine(self, mlp_dtype=0, table_dtype=0, slots=2, option_first=True, load=True, tables=None):
        eng = N.Engine(self.kind, self.rows, self.D, self.ln_bot, self.ln_top,
                       N.INTERACT_DOT if self.dot else N.INTERACT_CAT, interaction_itself=self.itself,
                       sigmoid_top=self.sigmoid_top, max_batch=self.B, max_lookups=self.L,
                       num_staged_batches=len(self.dense), num_slots=slots, ln_task=self.ln_task, num_tasks=self.num_tasks)
        try:
            eng.set_option("sls_exact", 1)
            if table_dtype:
                eng.set_option("table_dtype", table_dtype)
            if mlp_dtype and option_first:
                eng.set_option("mlp_dtype", mlp_dtype)
            if load:
                self.load(eng, tables)
            if mlp_dtype and not option_first:
                eng.set_option("mlp_dtype", mlp_dtype)
        except Exception:
            eng.close()
            raise
        return eng

    def load(self, eng, tables=None):
        for t, W in enumerate(tables or self.tables):
            eng.set_table(t, W)
        for (which, l), (W, b) in sorted(self.w.items()):
            eng.set_fc(which, l, W, b)
        for i in range(len(self.dense)):
            eng.stage_batch(i, self.dense[i], self.idx[i], self.lens[i])

    def act(self, which, l):
        if which == N.MLP_BOT or self.kind == N.MODEL_NCF:
            return N.ACT_RELU
        if self.kind == N.MODEL_MTWND and which == N.MLP_TOP:
            return N.ACT_RELU
        return N.ACT_SIGMOID if l + 1 == self.sigmoid_top else N.ACT_RELU

    def compose(self, eng, batch, bs, tables=None):
        """The forward from operator calls on `eng`'s handle -> (outputs, [(K, N, act, input, W, b, output)] per layer)."""
        tables = tables or self.tables
        rec = []
        L = self.L

        def run(which, ln, x):
            for l in range(len(ln) - 1):
                W, b = self.w[(which, l)]
                y = fc_op(eng, x, W, b, self.act(which, l))
                rec.append((ln[l], ln[l + 1], self.act(which, l), x, W, b, y))
                x = y
            return x
        pooled = [sls_op(eng, tables[t], self.idx[batch][t][:bs * L], self.lens[batch][t][:bs]) for t in range(self.T)]
        if self.kind == N.MODEL_NCF:
            mf = pooled[0] + pooled[1]
            h = run(N.MLP_TOP, self.ln_top, np.concatenate([pooled[2], pooled[3]], axis=1))
            return run(N.MLP_FINAL, [self.D + self.ln_top[-1], self.fin], np.concatenate([mf, h], axis=1)), rec
        dense = self.dense[batch][:bs]
        if self.kind == N.MODEL_DLRM:
            x = run(N.MLP_BOT, self.ln_bot, dense)
            Tm = np.concatenate([x] + pooled, axis=1)
            z = dot_op(eng, Tm, self.T + 1, self.D, self.itself) if self.dot else Tm
            return run(N.MLP_TOP, self.ln_top, z), rec
        z = np.concatenate([dense] + pooled, axis=1)
        h = run(N.MLP_TOP, self.ln_top, z)
        if self.kind == N.MODEL_WND:
            return h, rec
        return np.concatenate([run(N.MLP_TASK0 + k, self.ln_task, h) for k in range(self.num_tasks)], axis=1), rec


def nets():
    """At least two eligible layers each, a non-eligible layer between or behind them, one eligible LAST layer (ncf)."""
    return {
        # RM3-shaped DLRM: wide bottom MLP (eligible 128-256, 256-64), dot interaction, top 100-128-64-1: eligible 100-128, 128-64
        "dlrm_dot": Net(N.MODEL_DLRM, 64, 8, [128, 256, 64], [64 + 36, 128, 64, 1], sigmoid_top=3, dot=True, seed=1),
        # ... a non-eligible layer BETWEEN two eligible ones in the top MLP (200-32-...), cat interaction
        "dlrm_cat": Net(N.MODEL_DLRM, 32, 3, [13, 64, 32], [128, 96, 32, 80, 64, 1], sigmoid_top=5, seed=2),
        # W&D: odd dense width (rows only 4-byte aligned), eligible 147-256, 256-128, 128-64, then 64-1
        "wnd": Net(N.MODEL_WND, 32, 4, [19], [19 + 128, 256, 128, 64, 1], sigmoid_top=4, seed=3),
        # MT-WnD: shared top 140-256-64 eligible, task heads 64-64 (eligible) -32-2
        "mtwnd": Net(N.MODEL_MTWND, 32, 4, [12], [12 + 128, 256, 64], sigmoid_top=3, ln_task=[64, 64, 32, 2], num_tasks=3,
                     seed=4),
        # NCF: MLP branch 128-256-16-64 (eligible, not, not), predictor (64 + 64)-64: an eligible LAST layer
        "ncf": Net(N.MODEL_NCF, 64, 4, [1], [128, 256, 16, 64], fin=64, L=1, seed=5),
    }


def single(eng, batch, bs, slot=0):
    return eng.forward(batch, bs)


def count_bf16(log):
    return sum(1 for t in log if t.startswith("gemm_bf16_kernel"))


# 4. layer by layer, 5. the option does something
@pytest.mark.parametrize("name", sorted(nets()))
def test_whole_model_is_the_composition_of_its_layers(name):
    net = nets()[name]
    assert net.n_eligible() >= 2 and net.n_eligible() < len(net.layers())
    eng, ref = net.engine(BF16), net.engine(0)
    try:
        worst_rel = 0.0
        for batch, bs in [(0, net.B), (1, 37), (0, 1), (1, 64)]:
            got = eng.forward(batch, bs)
            log = eng.last_dispatch(0)
            assert count_bf16(log) == net.n_eligible(), log
            exp, rec = net.compose(eng, batch, bs)
            assert got.shape == exp.shape
            assert np.array_equal(got, exp), (name, batch, bs, float(np.abs(got - exp).max()))
            n_b = 0
            for K, N_, act, x, W, b, y in rec:
                if not eligible(K, N_):
                    continue
                n_b += 1
                r = bound_ratio(y, x, W, b, act)
                print("%s batch %d bs %d layer %dx%d: |err| / bound = %.4f" % (name, batch, bs, K, N_, r))
                assert r <= 1.0, (name, K, N_, r)
            assert n_b == net.n_eligible()
            # 5: it does something, stays finite, and what it costs
            fp32 = ref.forward(batch, bs)
            assert count_bf16(ref.last_dispatch(0)) == 0
            assert np.all(np.isfinite(got))
            assert not np.array_equal(got, fp32), "mlp_dtype 2 changed nothing"
            # (relative to the run's largest fp32 output: ReLU outputs hold exact zeros)
            worst_rel = max(worst_rel, float(np.abs(got - fp32).max() / np.abs(fp32).max()))
            _report(test="model", model=name, batch=batch, bs=bs, max_abs_diff_from_fp32=float(np.abs(got - fp32).max()),
                    max_abs_fp32=float(np.abs(fp32).max()))
        print("%s: largest difference from the fp32 engine, relative to the largest output: %.3e" % (name, worst_rel))
        _report(test="model_summary", model=name, max_rel_diff_from_fp32=worst_rel)
    finally:
        eng.close()
        ref.close()


# 3b. a query's bits do not depend on what it was coalesced with
@pytest.mark.parametrize("name", sorted(nets()))
def test_coalesced_queries_are_bit_identical_to_single_runs(name):
    net = nets()[name]
    eng = net.engine(BF16, slots=2)
    try:
        sizes = [net.B, 1, 37, 64, 65, 128, 5, 200]
        alone = {}
        for n_q in (1, 5, 12, 16):
            jobs = [((k + n_q) % 2, sizes[(k * 3 + n_q) % len(sizes)]) for k in range(n_q)]
            eng.forward_multi_async(1, [b for b, _ in jobs], [n for _, n in jobs])
            out = eng.wait(1, sum(n for _, n in jobs))
            log = eng.last_dispatch(1)
            assert count_bf16(log) == net.n_eligible(), log
            v = 0
            for b, n in jobs:
                if (b, n) not in alone:
                    alone[(b, n)] = eng.forward(b, n)
                assert np.array_equal(out[v:v + n], alone[(b, n)]), (name, n_q, b, n)
                v += n
    finally:
        eng.close()


# 3c. nothing to do: nothing changes
def test_model_without_an_eligible_layer_is_unchanged():
    net = Net(N.MODEL_DLRM, 16, 3, [13, 32, 16], [64, 48, 32, 1], sigmoid_top=3, seed=9)
    assert net.n_eligible() == 0
    a, b = net.engine(BF16), net.engine(0)
    try:
        for batch, bs in [(0, net.B), (1, 33)]:
            assert np.array_equal(a.forward(batch, bs), b.forward(batch, bs))
            assert a.last_dispatch(0) == b.last_dispatch(0)
    finally:
        a.close()
        b.close()


# 6. composes with the table types; option order; replacing a layer; there and back
def _stored(tables, dtype):
    if dtype == N.TABLE_FP32:
        return tables
    if dtype == N.TABLE_FP16:
        with np.errstate(over="ignore"):
            return [W.astype(np.float16).astype(np.float32) for W in tables]
    if dtype == N.TABLE_BF16:
        return [bf(W) for W in tables]
    import torch
    out = []
    for W in tables:      # torch's CPU implementation of the 8-bit rowwise format: a row's value is its one-row bag
        P = torch.ops.quantized.embedding_bag_byte_prepack(torch.from_numpy(W))
        rows = W.shape[0]
        out.append(torch.ops.quantized.embedding_bag_byte_rowwise_offsets(
            P, torch.arange(rows, dtype=torch.int64), torch.arange(rows, dtype=torch.int64), mode=0,
            include_last_offset=False).numpy().astype(np.float32))
    return out


@pytest.mark.parametrize("dtype", [N.TABLE_FP16, N.TABLE_BF16, N.TABLE_INT8_ROWWISE])
@pytest.mark.parametrize("name", ["dlrm_dot", "wnd"])
def test_composes_with_every_table_dtype(name, dtype):
    net = nets()[name]
    net = Net(net.kind, net.D, net.T, net.ln_bot, net.ln_top, sigmoid_top=net.sigmoid_top, dot=net.dot, L=1, seed=21)
    eng = net.engine(BF16, table_dtype=dtype)
    try:
        assert eng.get_option("table_dtype") == dtype and eng.get_option("mlp_dtype") == BF16
        stored = _stored(net.tables, dtype)      # (one-lookup bags: a pooled row is the stored row's value)
        for batch, bs in [(0, net.B), (1, 37)]:
            got = eng.forward(batch, bs)
            assert count_bf16(eng.last_dispatch(0)) == net.n_eligible()
            exp, rec = net.compose(eng, batch, bs, tables=stored)
            assert np.array_equal(got, exp), (name, dtype, batch, bs)
            for K, N_, act, x, W, b, y in rec:
                if eligible(K, N_):
                    assert bound_ratio(y, x, W, b, act) <= 1.0
    finally:
        eng.close()


@pytest.mark.parametrize("name", ["dlrm_cat", "mtwnd", "ncf"])
def test_option_order_layer_replacement_and_back_to_fp32(name):
    net = nets()[name]
    first, later, ref = net.engine(BF16, option_first=True), net.engine(BF16, option_first=False), net.engine(0)
    try:
        outs = [first.forward(0, net.B), later.forward(0, net.B)]
        assert np.array_equal(outs[0], outs[1])
        assert first.last_dispatch(0) == later.last_dispatch(0)
        # replace an eligible layer with other weights, then with the original ones again
        which, l, K, N_ = [x for x in net.layers() if eligible(x[2], x[3])][0]
        W, b = net.w[(which, l)]
        for eng in (first, later):
            eng.set_fc(which, l, W * 0.5, b + 0.25)
        changed = [first.forward(0, net.B), later.forward(0, net.B)]
        assert np.array_equal(changed[0], changed[1]) and not np.array_equal(changed[0], outs[0])
        for eng in (first, later):
            eng.set_fc(which, l, W, b)
            assert np.array_equal(eng.forward(0, net.B), outs[0])
        # there and back: bit-identical to an engine that never had it, dispatch log included
        fp32 = ref.forward(1, 77)
        for eng in (first, later):
            eng.set_option("mlp_dtype", 0)
            assert np.array_equal(eng.forward(1, 77), fp32)
            assert eng.last_dispatch(0) == ref.last_dispatch(0)
            eng.set_option("mlp_dtype", BF16)
            assert np.array_equal(eng.forward(0, net.B), outs[0])
    finally:
        first.close()
        later.close()
        ref.close()
