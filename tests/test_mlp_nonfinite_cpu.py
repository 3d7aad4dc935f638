"""NaN, infinity and fp32 overflow through the fp32 MLP: the CPU oracle against an independent statement, at every shape of
the boundary catalogue with the poison layout of tests/mlp_shapes.py (poisoned).  No GPU.

tests/test_mlp_nonfinite.py holds every launch form of the engine to the oracle on these inputs; this file is what makes
the oracle worth that, and shows that the GPU test cannot pass vacuously.  For every case at bs = max(case.rows):

  * the class (finite, +inf, -inf, NaN) of EVERY output element of EVERY operator call of the oracle's forward
    (Built.compose(OracleOps): orc.fc, orc.sls, orc.interact_dot), in the samples of kinds nan / pinf / ninf / both, is the class
    a float64 restatement gives on the inputs that call actually got (operator by operator: a sign flip near zero in an earlier
    layer cannot move the comparison).  The restatement forms the products elementwise and applies
        a sum is NaN if a term is NaN or +inf and -inf terms meet, else +-inf if a term is, else the finite sum
        ReLU(s) = where(s > 0, s, 0)  (so ReLU(NaN) = 0; NOT np.maximum, which propagates NaN)
        sigmoid(s) = 1 / (1 + exp(-s)): exactly 1 at +inf, exactly 0 at -inf, NaN at NaN;
  * `huge` (finite +-3e38 whose sums overflow): the class depends on fp32's summation order, float64 says nothing; for three
    small cases the oracle's fc is held bit for bit to a numpy fp32 restatement of its k-ordered fma chain (fma32 of
    tests/test_sls_weights_cpu.py; a step with a non-finite operand takes IEEE's own inf / NaN rules) on those samples;
  * the conditions CONDITIONS names hold (the poison does something, ReLU brings a NaN row back, overflow is born inside the
    MLP, an infinity and a finite value meet in the output layer's input): conditions, not measurements.  A case that cannot
    meet one because of its structure is excused BY NAME in EXCUSED, with the reason;
  * the clean samples of the poisoned run have the bits of the all-clean run, and oracle.Model.forward equals the composition.

DRS_MLP_NONFINITE_REPORT=<file>: one JSON line per case, which conditions it met (profiles/r31_mlp_nonfinite.md).
"""
import json
import os

import numpy as np
import pytest

from deeprecsys_amd import _native as N
from oracle import oracle as orc
from tests import mlp_shapes as S
from tests.test_sls_weights_cpu import fma32

FINITE, PINF, NINF, NAN = 0, 1, 2, 3
CLASS_KINDS = ("nan", "pinf", "ninf", "both")     # the kinds whose class float64 can state

CONDITIONS = ("kinds", "differs", "relu_restores", "overflow_inside", "inf_meets_finite")
# condition -> {case name: why its structure cannot meet it}
EXCUSED = {"kinds": {}, "differs": {}, "relu_restores": {}, "inf_meets_finite": {},
           "overflow_inside": {
               "rows32_q_own_slab": "the dense input is 16 of the first layer's 64 columns (weights normal(0, 1/8)): a sum of 16 terms "
                                    "of +-3e38 w has sigma 1.5e38 and overflows beyond 2.3 sigma only; of this case's 64 sums the largest "
                                    "is 3.14e38 < FLT_MAX, and behind ReLU the next layers' sums are smaller (2.43e38, 3.4e37)"}}


def _report(**kw):
    path = os.environ.get("DRS_MLP_NONFINITE_REPORT")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(kw) + "\n")


def classes(a):
    a = np.asarray(a)
    return np.where(np.isnan(a), NAN, np.where(a == np.inf, PINF, np.where(a == -np.inf, NINF, FINITE))).astype(np.int8)


def sum64(P, axis):
    """the sum of the float64 terms P along `axis`, by the rule of the docstring (stated, not left to numpy's adds)"""
    nan = np.isnan(P).any(axis=axis)
    pinf, ninf = (P == np.inf).any(axis=axis), (P == -np.inf).any(axis=axis)
    fin = np.where(np.isfinite(P), P, 0.0).sum(axis=axis)
    return np.where(nan | (pinf & ninf), np.nan, np.where(pinf, np.inf, np.where(ninf, -np.inf, fin)))


def act64(s, act):
    with np.errstate(over="ignore", invalid="ignore"):
        if act == N.ACT_RELU:
            return np.where(s > 0, s, 0.0)
        if act == N.ACT_SIGMOID:
            return 1.0 / (1.0 + np.exp(-s))
    return s


def fc64(x, W, b, act):
    """act(x W^T + b) in float64.  A row of x with a non-finite element: its products elementwise ([N, K] per row), summed
    by sum64; a row of finite elements: the sum of its (finite) products is the matrix product's."""
    x, W, b = np.asarray(x, np.float64), np.asarray(W, np.float64), np.asarray(b, np.float64)
    plain = np.isfinite(x).all(axis=1)
    s = np.empty((x.shape[0], W.shape[0]))
    s[plain] = x[plain] @ W.T + b
    with np.errstate(invalid="ignore"):
        for m in np.nonzero(~plain)[0]:
            s[m] = sum64(np.concatenate([W * x[m], b[:, None]], axis=1), 1)
    assert np.all(np.isfinite(s[plain])), "float64 overflowed: no reference"
    return act64(s, act)


def sls64(W, idx, lens):
    W = np.asarray(W, np.float64)
    out = np.zeros((len(lens), W.shape[1]))
    o = 0
    for i, n in enumerate(lens):
        out[i] = sum64(W[idx[o:o + n]], 0)
        o += n
    return out


def dot64(T3):
    T3 = np.asarray(T3, np.float64)
    li, lj = S.pair_index(T3.shape[1])
    with np.errstate(invalid="ignore", over="ignore"):
        Z = sum64(T3[:, li, :] * T3[:, lj, :], 2)
    return np.concatenate([T3[:, 0, :], Z], axis=1)


class Float64Ops(object):
    """S.Float64Ops with the rules above: the whole forward in float64 (the conditions read it)"""
    sls = staticmethod(sls64)
    fc = staticmethod(fc64)
    dot = staticmethod(dot64)
    cat = staticmethod(lambda xs: np.concatenate([np.asarray(x, np.float64) for x in xs], axis=1))

    @staticmethod
    def add(a, b):
        with np.errstate(invalid="ignore"):
            return np.asarray(a, np.float64) + np.asarray(b, np.float64)


def fma32_any(a, b, c):
    """fma32 where all three operands are finite; elsewhere a * b (exact in float64) + c follows IEEE's rules for inf and NaN,
    which are fmaf's"""
    a, b, c = (np.asarray(v, np.float32) for v in np.broadcast_arrays(a, b, c))
    ok = np.isfinite(a) & np.isfinite(b) & np.isfinite(c)
    with np.errstate(invalid="ignore", over="ignore"):
        out = (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)
        out[ok] = fma32(a[ok], b[ok], c[ok])
    return out


def chain32(x, W, b):
    """[M, N] fp32: per output the k-ordered chain acc = fma(x_k, W_nk, acc) from +0.0, then one fp32 add of the bias"""
    x, W, b = np.asarray(x, np.float32), np.asarray(W, np.float32), np.asarray(b, np.float32)
    acc = np.zeros((x.shape[0], W.shape[0]), np.float32)
    for k in range(x.shape[1]):
        acc = fma32_any(x[:, k:k + 1], W[None, :, k], acc)
    with np.errstate(invalid="ignore", over="ignore"):
        return acc + b


def poisoned_run(name):
    case = S.BY_NAME[name]
    bs = max(case.rows)
    net = S.Built(case, poison=True)
    pnet = S.poisoned(net, bs)
    return case, bs, net, pnet


def samples_of(pnet, kinds):
    return np.array([s for s in range(pnet.hot.size) if pnet.hot_kind[s] in kinds], dtype=np.int64)


@pytest.mark.parametrize("name", S.NAMES)
def test_oracle_classes_match_float64_and_the_poison_bites(name):
    case, bs, net, pnet = poisoned_run(name)
    assert np.array_equal(np.nonzero(pnet.hot)[0], S.hot_samples(bs))
    om = net.oracle_model()
    out, R, rec = pnet.compose(S.OracleOps, bs)
    f_out, f_R = pnet.oracle_forward(om, bs)
    assert np.array_equal(out, f_out, equal_nan=True) and np.array_equal(R, f_R, equal_nan=True), (name, "forward is not its composition")
    clean_out, clean_R = net.oracle_forward(om, bs)
    assert np.all(np.isfinite(clean_out)) and np.all(np.isfinite(clean_R))
    # the clean samples of the poisoned run: the bits of the all-clean run
    cold = ~pnet.hot
    assert np.array_equal(out[cold], clean_out[cold]) and np.array_equal(R[cold], clean_R[cold]), name

    # ---- the class of every element of every operator call, in the samples float64 can speak for ----------------------------
    rows = samples_of(pnet, CLASS_KINDS)
    n_checked = 0
    for which, l, act, x, W, b, y in rec["fc"]:
        pre = fc64(x[rows], W, b, N.ACT_NONE)
        exp = act64(pre, act)
        got = classes(y[rows])
        assert np.array_equal(got, classes(exp)), (name, "fc", which, l, W.shape, np.argwhere(got != classes(exp))[:8])
        if act == N.ACT_SIGMOID:       # the three special results, as values
            assert np.all(y[rows][pre == np.inf] == 1.0) and np.all(y[rows][pre == -np.inf] == 0.0), (name, which, l)
            assert np.all(np.isnan(y[rows][np.isnan(pre)]))
        if act == N.ACT_RELU:
            assert np.all(y[rows][np.isnan(pre)] == 0.0), (name, which, l, "ReLU(NaN) = 0")
        n_checked += got.size
    for t, idx, lens, y in rec["sls"]:
        exp = sls64(net.tables[t], idx, lens)
        assert np.array_equal(classes(y[rows]), classes(exp[rows])), (name, "sls", t)
        n_checked += y[rows].size
    for T3, Rd in rec["dot"]:
        exp = dot64(T3[rows])
        assert np.array_equal(classes(Rd[rows]), classes(exp)), (name, "dot", np.argwhere(classes(Rd[rows]) != classes(exp))[:8])
        n_checked += Rd[rows].size
    assert n_checked > 0

    # ---- the conditions against a vacuous pass ------------------------------------------------------------------------------
    met = {}
    kinds_here = {k for k in pnet.hot_kind if k}
    met["kinds"] = kinds_here == set(S.KINDS[:min(len(S.KINDS), int(pnet.hot.sum()))])
    met["differs"] = any(not np.array_equal(out[s], clean_out[s], equal_nan=True) for s in np.nonzero(pnet.hot)[0])
    # a sample that held a NaN (the kind nan: in its dense row, or in its pooled row) has a finite output again
    held = [s for s in samples_of(pnet, ("nan",))
            if (pnet.hot_route[s] == "dense" and np.isnan(pnet.dense[s]).any()) or (pnet.hot_route[s] == "table" and any(np.isnan(y[s]).any() for _, _, _, y in rec["sls"]))]
    assert held, name
    met["relu_restores"] = any(np.isfinite(out[s]).any() for s in held)
    # overflow born inside the MLP: an operator whose inputs for a huge sample are all finite gives +-inf or NaN there
    huge = samples_of(pnet, ("huge",))
    born = False
    for which, l, act, x, W, b, y in rec["fc"]:
        born = born or any(np.isfinite(x[s]).all() and not np.isfinite(fc_pre(x[s:s + 1], W, b)).all() for s in huge)
    for T3, Rd in rec["dot"]:
        born = born or any(np.isfinite(T3[s]).all() and not np.isfinite(Rd[s]).all() for s in huge)
    met["overflow_inside"] = bool(born)
    n_layers = sum(1 for _ in rec["fc"])
    needs_overflow = net.m_den > 0 and n_layers >= 2
    # an infinity and a finite value in one row of the output layer's input, where the float64 forward says so
    both_in_row = lambda x, s: bool(np.isinf(x[s]).any() and np.isfinite(x[s]).any())
    pi = samples_of(pnet, ("pinf", "both"))
    _, _, rec64 = pnet.compose(Float64Ops, bs)
    says = any(both_in_row(x, s) for x in rec64["last_in"] for s in pi)
    met["inf_meets_finite"] = any(both_in_row(x, s) for x in rec["last_in"] for s in pi)

    required = {"kinds": True, "differs": True, "relu_restores": True, "overflow_inside": needs_overflow, "inf_meets_finite": says}
    print("%s: %r" % (name, met))
    _report(case=name, met=met, required=required, checked=n_checked)
    for cond in CONDITIONS:
        if name in EXCUSED[cond]:
            assert EXCUSED[cond][name] and not met[cond], (name, cond, "is excused but met")
        elif required[cond]:
            assert met[cond], (name, cond)


def fc_pre(x, W, b):
    return orc.fc(x, W, b, N.ACT_NONE)


HUGE_CASES = ("even_32_dot", "k_642", "ncf_sum_stream4", "mtwnd_heads")


@pytest.mark.parametrize("name", HUGE_CASES)
def test_oracle_fc_is_its_fp32_chain_on_the_huge_samples(name):
    """dlrm_dot (the overflow is born in the interaction: inf and NaN enter the top MLP), W&D with a scalar K tail, NCF (both
    joins), MT-WnD (heads)"""
    case, bs, net, pnet = poisoned_run(name)
    _, _, rec = pnet.compose(S.OracleOps, bs)
    rows = samples_of(pnet, ("huge",))
    assert rows.size
    seen = set()
    for which, l, act, x, W, b, y in rec["fc"]:
        pre = chain32(x[rows], W, b)
        got_pre = fc_pre(x[rows], W, b)
        assert np.array_equal(pre.view(np.uint32)[~np.isnan(pre)], got_pre.view(np.uint32)[~np.isnan(pre)]), (name, which, l)
        assert np.array_equal(np.isnan(pre), np.isnan(got_pre)), (name, which, l)
        seen.update(classes(pre).ravel().tolist())
        got = y[rows]
        if act == N.ACT_RELU:
            exp = np.where(pre > 0, pre, np.float32(0))
            assert np.array_equal(got.view(np.uint32), exp.view(np.uint32)), (name, which, l, "ReLU")
        else:
            with np.errstate(over="ignore"):
                exp = 1.0 / (1.0 + np.exp(-pre.astype(np.float64)))
            assert np.array_equal(classes(got), classes(exp)), (name, which, l)
            ok = np.isfinite(exp)
            assert np.allclose(got[ok], exp[ok], rtol=1e-6, atol=1e-7)
            assert np.all(got[pre == np.inf] == 1.0) and np.all(got[pre == -np.inf] == 0.0)
    print("%s: classes met before the activations: %r" % (name, sorted(seen)))
    assert seen - {FINITE}, (name, "no overflow anywhere: the case shows nothing")


def test_the_huge_cases_differ_in_kind():
    assert len({S.BY_NAME[n].kind for n in HUGE_CASES}) >= 3


def test_the_poison_layout():
    net = S.Built(S.BY_NAME["even_32_dot"], poison=True)
    plain = S.Built(S.BY_NAME["even_32_dot"])
    # the clean model is the boundary tests' own: the same weights, inputs and valid table rows
    assert all(np.array_equal(a[:-1], b[:r]) for a, b, r in zip(plain.tables, net.tables, net.rows))
    assert np.array_equal(plain.dense, net.dense) and all(np.array_equal(a, b) for a, b in zip(plain.idx, net.idx))
    assert all(np.array_equal(plain.w[k][0], net.w[k][0]) for k in plain.w)
    assert plain.table_rows() == [r + 1 for r in plain.rows]
    for t, W in enumerate(net.tables):
        assert np.all(np.isnan(W[net.nan_row[t]])) and net.nan_row[t] == W.shape[0] - 1
        assert np.all(np.isfinite(W[:net.rows[t]]))
    for bs, hot in ((1, [0]), (16, [0, 15]), (17, [0, 15, 16]), (33, [0, 15, 16, 31, 32]), (100, [0, 15, 16, 31, 32, 63, 64, 99])):
        p = S.poisoned(net, bs)
        assert list(np.nonzero(p.hot)[0]) == hot
        assert [p.hot_kind[s] for s in hot] == [S.KINDS[i % 5] for i in range(len(hot))]
        assert [p.hot_route[s] for s in hot] == ["table" if i % 2 else "dense" for i in range(len(hot))]
        assert np.all(np.isnan(p.dense[bs:])) and all(np.all(i[bs * 2:] == net.nan_row[t]) for t, i in enumerate(p.idx))
        cold = ~p.hot
        assert np.array_equal(p.dense[:bs][cold], net.dense[:bs][cold])
        for t in range(net.case.T):
            assert np.all(p.idx[t][:bs * 2] < net.nan_row[t])
            assert np.array_equal(p.idx[t][:bs * 2].reshape(bs, 2)[cold], net.idx[t][:bs * 2].reshape(bs, 2)[cold])
    p = S.poisoned(net, 100)
    # single elements: column 0 and the last column both carry one, by both routes
    dense_cols = [int(np.nonzero(~np.isfinite(p.dense[s]))[0][0]) for s in (0, 16, 64)]
    assert dense_cols == [0, net.m_den - 1, 0]
    assert np.all(np.abs(p.dense[32]) == np.float32(S.HUGE)) and len(set(np.sign(p.dense[32]))) == 2
    t = net.poison_tables()[0]
    named = [S.POISON_ROWS[int(p.idx[t][s * 2 + 1]) - net.poison_row[t]] for s in (15, 31, 63, 99)]
    assert named == [("pinf", 0), ("both", 1), ("nan", 0), ("ninf", 1)], named
    assert np.all(np.abs(net.tables[t][net.poison_row[t] + 8]) == np.float32(S.HUGE))
    # NCF: the summed pair and the concatenated pair, on different samples
    ncf = S.Built(S.BY_NAME["ncf_sum_stream4"], poison=True)
    q = S.poisoned(ncf, 100)
    at = {s: [t for t in range(4) if q.idx[t][s] >= ncf.rows[t]] for s in np.nonzero(q.hot)[0]}
    assert all(len(v) == 1 for v in at.values()) and {v[0] for v in at.values()} == {0, 2}
    assert all(r == "table" for r in q.hot_route if r)
