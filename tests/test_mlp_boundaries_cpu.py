"""The CPU oracle against a plain float64 forward at every shape of the boundary catalogue (tests/mlp_shapes.py), and the
catalogue's own hygiene.  No GPU.

The GPU suite holds the engine to the oracle bit for bit; this file is what makes that worth its claim at the new shapes.
For every case: oracle.Model.forward is bit-identical to the same forward composed from orc.sls / orc.fc /
orc.interact_dot and numpy concatenation, and every operator call of that composition meets a DERIVED bound against a
float64 restatement on the input it actually got:

    a k-ordered chain of K round-to-nearest fmaf steps plus the bias add:
        |got - exp| <= g(K) (sum_k |x_k W_nk| + |b_n|),   g(K) = (K + 1) u / (1 - (K + 1) u),   u = 2^-24
    before the activation; ReLU does not enlarge it (Lipschitz 1); the sigmoid (Lipschitz 1/4) gets the allowance of
    test_fc_matches_oracle_chain for expf (rtol 1e-6, atol 1e-7).  A pooled row summed in index order: the same with K =
    bag length over sum |rows|; a pair of the dot interaction: K = D over sum_k |a_k b_k|, no bias.

Nothing in the bound is measured.  DRS_MLP_BOUNDARY_REPORT=<file> makes the test append, per case, the largest measured
fraction of the bound (profiles/r10_mlp_boundaries.md quotes it).
"""
import json
import os

import numpy as np
import pytest

from deeprecsys_amd import _native as N
from tests import mlp_shapes as S

U = 2.0 ** -24


def gamma(K):
    return (K + 1) * U / (1.0 - (K + 1) * U)


def _report(**kw):
    path = os.environ.get("DRS_MLP_BOUNDARY_REPORT")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(kw) + "\n")


def _fraction(got, exp, bound):
    err = np.abs(np.asarray(got, np.float64) - exp)
    assert np.all(np.isfinite(got)), "the oracle produced a NaN / infinity"
    return float(np.max(np.where(err == 0, 0.0, err / np.maximum(bound, np.finfo(np.float64).tiny)))) if err.size else 0.0


def fc_fraction(x, W, b, act, y):
    x64, W64, b64 = np.asarray(x, np.float64), np.asarray(W, np.float64), np.asarray(b, np.float64)
    s = x64 @ W64.T + b64
    mag = np.abs(x64) @ np.abs(W64).T + np.abs(b64)
    exp = S.act64(s, act)
    bound = gamma(x64.shape[1]) * mag
    if act == N.ACT_SIGMOID:
        bound = bound + 1e-7 + 1e-6 * np.abs(exp)
    return _fraction(y, exp, bound)


def sls_fraction(W, idx, lens, y, L):
    exp = S.sls64(W, idx, lens)
    mag = S.sls64(np.abs(np.nan_to_num(W)), idx, lens)
    return _fraction(y, exp, gamma(L) * mag)


def dot_fraction(T3, R):
    D = T3.shape[2]
    assert np.array_equal(R[:, :D], T3[:, 0, :]), "the dense columns of the interaction tensor are a copy"
    li, lj = S.pair_index(T3.shape[1])
    a = np.asarray(T3, np.float64)
    exp = np.einsum("bik,bjk->bij", a, a)[:, li, lj]
    mag = np.einsum("bik,bjk->bij", np.abs(a), np.abs(a))[:, li, lj]
    return _fraction(R[:, D:], exp, gamma(D) * mag)


@pytest.mark.parametrize("name", S.NAMES)
def test_oracle_is_its_composition_and_meets_the_float64_bound(name):
    case = S.BY_NAME[name]
    net = S.Built(case)
    om = net.oracle_model()
    worst = {"fc": 0.0, "sls": 0.0, "dot": 0.0}
    for bs in sorted(set(case.rows) | {S.B_MAX}):
        out, R = net.oracle_forward(om, bs)
        cout, cR, rec = net.compose(S.OracleOps, bs)
        assert out.shape == cout.shape and R.shape == cR.shape
        assert np.array_equal(R, cR), (name, bs, "interaction tensor")
        assert np.array_equal(out, cout), (name, bs, float(np.abs(out - cout).max()))
        for which, l, act, x, W, b, y in rec["fc"]:
            r = fc_fraction(x, W, b, act, y)
            worst["fc"] = max(worst["fc"], r)
            assert r <= 1.0, (name, bs, which, l, W.shape, r)
        for t, idx, lens, y in rec["sls"]:
            r = sls_fraction(net.tables[t], idx, lens, y, case.L)
            worst["sls"] = max(worst["sls"], r)
            assert r <= 1.0, (name, bs, "table", t, r)
        for T3, Rd in rec["dot"]:
            r = dot_fraction(T3, Rd)
            worst["dot"] = max(worst["dot"], r)
            assert r <= 1.0, (name, bs, "dot", r)
    print("%s: largest fraction of the bound: fc %.3f, pooled rows %.3f, dot %.3f" % (name, worst["fc"], worst["sls"], worst["dot"]))
    _report(test="oracle_vs_float64", case=name, fc=worst["fc"], sls=worst["sls"], dot=worst["dot"])


@pytest.mark.parametrize("name", S.NAMES)
def test_the_network_is_alive_in_float64(name):
    """A condition on the catalogue, not a tolerance: in the float64 forward ALONE, the input of every layer that produces
    the model's outputs (the last hidden layer) is non-zero in at least half of its columns -- a network that died under
    ReLU would pass any comparison."""
    net = S.Built(S.BY_NAME[name])
    out, _, rec = net.compose(S.Float64Ops, S.B_MAX)
    assert np.all(np.isfinite(out))
    assert rec["last_in"]
    for x in rec["last_in"]:
        alive = int(np.count_nonzero(np.any(x != 0, axis=0)))
        assert 2 * alive >= x.shape[1], (name, alive, x.shape[1])
    assert float(np.abs(out).max()) < 1e6
    # the outputs are not all the same number either (a saturated sigmoid, a dead last layer)
    assert np.unique(np.round(out, 12)).size > 1


def test_catalogue_hygiene():
    assert len(set(S.NAMES)) == len(S.NAMES), "case names are unique"
    sides = {}
    for c in S.CASES:
        assert c.rule in range(1, 12) and c.side in S.SIDES, c.name
        assert c.expect, c.name + ": a case names the forms it must show"
        assert c.rows and max(c.rows) <= S.B_MAX and min(c.rows) >= 1, c.name
        assert c.T <= 8 and c.L <= 3, c.name
        if S.SIDES[c.side] is not None:          # ("shadowed": the threshold cannot be reached, the case counts for no side)
            sides.setdefault((c.rule, c.thr), set()).add(S.SIDES[c.side])
    # every threshold -- a rule, or each of the thresholds a rule bundles (`thr`) -- has a case on each side of it
    assert {r for r, _ in sides} == set(range(1, 12))
    for key, got in sorted(sides.items()):
        assert got == {"at", "other"}, "rule %d %s needs a case on each side of its threshold: %r" % (key[0], key[1], got)
    assert {("2", "steps"), ("2", "tiles"), ("3", "n")} <= {(str(r), thr) for r, thr in sides}
    # the far sides that only ONE case holds, by what they are
    assert any(c.top[-1] == 4081 and c.rule == 3 for c in S.CASES) and any(c.top[-1] == 4080 and c.rule == 3 for c in S.CASES)
    assert any(c.rule == 11 and c.side == "beyond" and c.kind == "ncf" for c in S.CASES)
    assert any(c.rule == 10 and c.side == "beyond" and c.top[0] * c.top[1] >= 262144 and c.top[0] % 4 for c in S.CASES), "fc_kernel<scalar>"
    assert any(c.rule == 10 and c.side == "beyond" and c.top[0] * c.top[1] < 262144 and c.top[0] > 640 and c.top[0] % 4 for c in S.CASES)
    assert any(c.rule == 9 and c.side == "below" and c.top[0] * c.top[1] == 262143 for c in S.CASES)
    for kc in (256, 192, 128, 64):
        assert any(("chain_kernel<scalar,%d>" % kc) in p or ("chain_kernel<vec,%d>" % kc) in p for c in S.CASES for p in c.expect), kc
    # the cases the catalogue must hold (by what they are, not by name)
    depth = lambda c, which: len(getattr(c, which)) - 1
    dlrm = [c for c in S.CASES if c.kind.startswith("dlrm")]
    assert any(depth(c, "bot") == 7 for c in dlrm) and any(depth(c, "top") == 7 for c in dlrm)
    assert any(depth(c, "bot") == 6 and depth(c, "top") == 6 for c in dlrm)
    assert any(depth(c, "bot") == 6 and depth(c, "top") == 7 for c in dlrm)
    assert any(c.kind == "wnd" and depth(c, "top") == 13 for c in S.CASES)
    assert any(c.kind == "mtwnd" and depth(c, "task") == 7 for c in S.CASES)
    for kind in ("dlrm_dot", "dlrm_cat"):
        for w in (30, 6):
            assert any(c.kind == kind and w in c.bot[1:-1] and w in c.top[1:-1] for c in S.CASES), (kind, w)
    for w in (64, 65, 128, 129, 256, 257):
        assert any(c.rule == 6 and w in c.top[1:-1] and w in c.bot[1:-1] for c in S.CASES), w
    for w in (128, 192, 256, 384, 512, 768, 1024):
        for s in (2, 4):
            assert any(c.rule == 7 and c.top[1] == w and dict(c.opts).get("mlp_nsplit") == s for c in S.CASES), (w, s)
    first_top = {(c.top[0], c.top[1]) for c in S.CASES}
    assert {(4000, 60), (60, 4000), (4096, 60), (4100, 60), (8192, 32), (512, 512), (512, 508)} <= first_top
    assert any(c.rule == 9 and (512, 512) in zip(c.bot[1:], c.bot[2:]) for c in S.CASES), "a wide layer in the middle of the bottom MLP"
    assert any(c.rule == 9 and c.top[-2] * c.top[-1] >= 262144 for c in S.CASES), "a wide layer as the model's last"
    r32 = [c for c in S.CASES if c.rule == 8]
    assert any(c.side == "beyond" and c.kind == "wnd" for c in r32) and any(c.side == "beyond" and c.kind == "dlrm_cat" for c in r32)
    for c in r32:
        assert {31, 32, 33, 63, 64, 65} <= set(c.rows), c.name
    # every product form is what at least one case expects; a form nobody can reach is listed with its reason
    for form in S.PRODUCT_FORMS:
        if form in S.UNREACHABLE:
            continue
        assert any(pat.split(" .. ")[0].startswith(form) for c in S.CASES for pat in c.expect), form


def test_the_pattern_language():
    tok = "stream4_kernel<rows32>[4 wg, 3 layers, 38224 B lds]"
    assert S.matches(tok, "stream4_kernel<rows32>[ .. , 3 layers")
    assert not S.matches(tok, "stream4_kernel[")
    assert not S.matches(tok, "stream4_kernel<rows32>[ .. , 13 layers")
    assert S.matches("stream4_kernel[7 wg, 12 layers, dot, 100 B lds]", "stream4_kernel[ .. , 12 layers, dot")
    assert not S.matches("stream4_kernel[7 wg, 12 layers, 100 B lds]", "stream4_kernel[ .. , 2 layers")
    assert S.matches("gemm32_kernel<2,2,sbase,split448>[1 x 4 wg, 512x512]", "gemm32_kernel<2,2,sbase,split448>[ .. 512x512]")
    assert not S.matches("gemm32_kernel<2,2,sbase>[1 x 4 wg, 512x512]", "gemm32_kernel<2,2>[")
    c = S.BY_NAME["depth_6_7_unfused"]
    good = ["set[1 queries, 64 rows, gather on own, mlp on own]", "sls_kernel<16,sequential>[3 wg]", "stream4_kernel[4 wg, 6 layers, 1 B lds]",
            "stream4_kernel[4 wg, 6 layers, 1 B lds]", "stream4_kernel[4 wg, 1 layers, 1 B lds]"]
    assert S.check_dispatch(c, good) == []
    assert S.check_dispatch(c, good[:-1])                                        # a launch short
    assert S.check_dispatch(c, good[:2] + ["stream4_kernel[4 wg, 13 layers, 1 B lds]"])
