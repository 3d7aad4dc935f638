"""The gather / DIN / DIEN boundary catalogue (tests/gather_shapes.py) against its own rules, and the CPU oracle against plain
float64 numpy at every catalogue shape.  No GPU.

  * hygiene: every rule 1 ... 16 and each of its thresholds has a case on each side; the form every case writes by hand is what
    the plain-Python restatement of the rules gives; no two cases are the same shape; every kernel name is expected by a case.
  * pooled sums: orc.sls against float64 within the DERIVED bound (L - 1) 2^-24 sum|x_i| per element (a chain of L - 1
    round-to-nearest additions); integer rows exactly.
  * DIN's top-MLP input row (pooled sums -> unit 3D-h-D, all ReLU -> Sum over the units) and DIEN's recurrence (two tanh layers
    over the Reshape'd sequence) against a float64 restatement written here, at the bars test_gpu_parity.py holds the engine to
    for the same quantities with xavier weights (rtol 2e-5, atol 2e-6).  The measured distance is printed and, with
    DRS_GATHER_BOUNDARY_REPORT=<file>, appended to the record (profiles/r12_gather_boundaries.md quotes it).
    A DIN row does not depend on the other samples of its query: models of more than 300 tables are compared on the first
    40 samples of each query (the float64 unit inputs of 160 samples x 1 534 units would take 190 MB).
"""
import json
import os

import numpy as np
import pytest

from tests import gather_shapes as S
from tests import helpers as H

U = 2.0 ** -24
_built = {}


def built(key):
    """tables, weights and the oracle model of an engine key (kept for the cases that share it)"""
    if key not in _built:
        _built.clear()
        tab, w = S.Tables(key), S.Weights(key)
        _built[key] = (tab, w, w.oracle_model(tab.W))
    return _built[key]


def _report(**kw):
    path = os.environ.get("DRS_GATHER_BOUNDARY_REPORT")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(kw) + "\n")


def relu(x):
    return np.maximum(x, 0.0)


def din_row64(w, E):
    """E: list of T float64 [n, D] pooled tensors -> the top MLP's input row [n, 4 D]"""
    T = len(E)
    ad = E[T - 2]
    att = np.zeros_like(ad)
    for i, unit in enumerate(w.att):
        x = np.concatenate([E[1 + i], ad, E[1 + i] + ad], axis=1)
        for W, b in unit:
            x = relu(x @ np.asarray(W, np.float64).T + np.asarray(b, np.float64))
        att += x
    return np.concatenate([E[0], att, ad, E[T - 1]], axis=1)


def dien_row64(w, E):
    """the Reshape quirk: step t of "sample" b reads behaviour embedding (t n + b) % U of sample (t n + b) // U"""
    T, n = len(E), E[0].shape[0]
    Ub = T - 3
    Hh = w.ln_bot[1]
    beh = np.stack(E[1:1 + Ub], axis=1)                     # [n, U, D]
    seq = beh.reshape(n * Ub, -1).reshape(Ub, n, -1)        # row-major reinterpretation
    f = lambda a: np.asarray(a, np.float64)
    (Wi0, bi0), (Wg0, bg0) = w.rnn[0]
    (Wi1, bi1), (Wg1, bg1) = w.rnn[1]
    h0, h1 = np.zeros((n, Hh)), np.zeros((n, Hh))
    for t in range(Ub):
        h0 = np.tanh((h0 @ f(Wg0).T + f(bg0)) + (seq[t] @ f(Wi0).T + f(bi0)))
        h1 = np.tanh((h1 @ f(Wg1).T + f(bg1)) + (h0 @ f(Wi1).T + f(bi1)))
    return np.concatenate([h1, E[0], E[T - 2], E[T - 1]], axis=1)


@pytest.mark.parametrize("name", S.NAMES)
def test_oracle_meets_float64_at_the_catalogue_shape(name):
    case = S.BY_NAME[name]
    tab, w, om = built(S.engine_key(case))
    st = S.Staged(case, tab)
    worst = {"sls": 0.0, "row_abs": 0.0, "row_rel": 0.0}
    for b, n in sorted(set(st.jobs())):
        if n == 0:
            continue
        if case.kind == "din" and case.T > 300:
            n = min(n, 40)
        for integer in (False, True):
            idx, lens = st.query(b, n, integer)
            E = []
            for t in range(case.T):
                got = S.orc.sls(tab.W[t], idx[t], lens[t])
                exp, mag = S.sls64(tab.W[t], idx[t], lens[t])
                E.append(exp)
                assert np.all(np.isfinite(got)), (name, t, "a bag named the NaN row")
                if integer:
                    assert np.array_equal(got, exp), (name, b, n, t, "integer rows sum exactly")
                    continue
                bound = np.maximum(np.repeat(lens[t], case.D).reshape(n, case.D) - 1, 0) * U * mag
                err = np.abs(got - exp)
                assert np.all(err <= bound), (name, b, n, t, float((err - bound).max()))
                worst["sls"] = max(worst["sls"], float(np.max(np.where(err > 0, err / np.maximum(bound, 1e-300), 0.0))))
            if integer or case.kind == "sls":
                continue
            _, R = om.forward(None, idx, lens, bs=n, want_R=True)
            R64 = (din_row64 if case.kind == "din" else dien_row64)(w, E)
            assert R.shape == R64.shape
            d = np.abs(R - R64)
            worst["row_abs"] = max(worst["row_abs"], float(d.max()))
            worst["row_rel"] = max(worst["row_rel"], float(np.max(d / np.maximum(np.abs(R64), 1e-3))))
            assert H.close(R, R64, rtol=2e-5, atol=2e-6), (name, b, n, float(d.max()))
            # the network is alive: a row of zeros would pass any comparison
            lo, hi = (case.D, 2 * case.D) if case.kind == "din" else (0, w.ln_bot[1])
            assert np.count_nonzero(R64[:, lo:hi]) * 4 >= R64[:, lo:hi].size, (name, "the attention / recurrent columns are mostly zero")
    print("%s: pooled rows at %.3f of the bound; row |d| %.3g, relative %.3g" % (name, worst["sls"], worst["row_abs"], worst["row_rel"]))
    _report(test="oracle_vs_float64", case=name, kind=case.kind, rule=case.rule, **worst)


def test_catalogue_hygiene():
    assert len(set(S.NAMES)) == len(S.NAMES), "case names are unique"
    shapes, sides = {}, {}
    for c in S.CASES:
        assert c.rule in S.RULES[c.kind], c.name
        assert c.side in ("at", "beyond", "shadowed"), c.name
        shape = (c.kind, c.D, c.T, c.H, c.top, c.L, c.sizes, c.opts)
        assert shape not in shapes, (c.name, shapes.get(shape), "the same shape twice")
        shapes[shape] = c.name
        assert 1 <= len(c.sizes) <= 16 and max(c.sizes) <= S.B_MAX and min(c.sizes) >= 0 and sum(c.sizes) >= 1, c.name
        assert all(L == S.RAGGED or L >= 1 for L in c.L), c.name
        # the form written by hand is what the rules give -- for the set, and for every query alone unless the case says
        # that serving it alone changes the form
        assert S.EXPECTED[c.kind](c) == c.form, (c.name, c.form, S.EXPECTED[c.kind](c))
        alone = {S.EXPECTED[c.kind](c, only=i) for i, n in enumerate(c.sizes) if n > 0}
        if c.alone is None:
            assert alone == {c.form}, (c.name, alone)
        else:
            assert alone != {c.form}, (c.name, "says a form change, but every query alone takes the set's form")
        if c.side != "shadowed":
            sides.setdefault((c.rule, c.thr), set()).add(c.side)
    assert {r for r, _ in sides} == set(range(1, 17))
    for key, got in sorted(sides.items()):
        assert got == {"at", "beyond"}, "rule %d %r needs a case on each side: %r" % (key[0], key[1], got)
    # what the issue names, by what the cases are
    sls = [c for c in S.CASES if c.kind == "sls"]
    assert {4, 8, 12, 16, 20, 32, 36, 64, 68, 128, 132, 252, 256, 260} <= {c.D for c in sls if c.rule == 1}
    for D, Ls in ((32, (40, 41, 80, 81, 160, 161)), (64, (20, 21, 40, 41, 80, 81)), (128, (10, 11, 20, 21, 40, 41)), (36, (40, 41)), (68, (20, 21))):
        assert set(Ls) <= {c.L[0] for c in sls if c.rule == 3 and c.D == D and dict(c.opts).get("sls_bpw") == 1}, D
    for D, Ls in ((32, (10, 11, 20, 21)), (64, (5, 6, 10, 11)), (128, (2, 3, 5, 6))):
        assert set(Ls) <= {c.L[0] for c in sls if c.rule == 4 and c.D == D and c.T == 4}, D
    assert {4, 5, 6} <= {c.T for c in sls if c.rule == 4}
    assert any(c.rule == 6 and 0 in c.sizes[1:-1] for c in sls), "an empty query in the middle of a set"
    assert any(c.rule == 6 and S.RAGGED in c.L and 20 in c.L for c in sls)
    waves = {c.T * -(-sum(c.sizes) // 64) for c in sls if c.rule == 7}
    assert {1023, 1024} <= waves, waves
    assert any(sum(c.sizes) == 1 for c in sls if c.rule == 7)
    din = [c for c in S.CASES if c.kind == "din"]
    assert {511, 512, 1023, 1024} <= {sum(c.sizes) for c in din if c.rule == 10}
    assert {256, 257, 877, 878, 1536, 1537} <= {c.T for c in din if c.rule == 12}
    assert {32, 33, 64, 65, 96, 97, 128, 129} <= {c.T - 3 for c in din if c.rule == 13 and c.D == 32}
    assert {16, 17, 32, 33, 48, 49} <= {c.T - 3 for c in din if c.rule == 13 and c.D == 64}
    dien = [c for c in S.CASES if c.kind == "dien"]
    assert {(16, 16), (16, 64), (64, 16), (64, 64), (16, 8), (64, 8)} <= {(c.D, c.H[0]) for c in dien if c.rule == 14}
    assert {15, 16, 17} <= {c.sizes[0] for c in dien if c.rule == 16 and len(c.sizes) == 1 and not c.opts}
    assert {3, 4, 5} <= {c.sizes[0] for c in dien if c.rule == 16 and dict(c.opts).get("dien_mfma") == 0}
    assert {1, 2, 4, 5} <= {c.T - 3 for c in dien if c.rule == 16}
    # every kernel NAME is what at least one case expects; the template-argument combinations nobody names are few and listed
    for k in S.KERNEL_NAMES:
        assert any(p.startswith(k + "<") or p.startswith(k + "[") for c in S.CASES for p in c.expect), k
    # ... and the combinations a run of the catalogue does not show (own options, sweeps, queries alone) are exactly the pinned list
    pred = S.predicted_tokens()
    assert [f for f in S.PRODUCT_FORMS if not any(t.startswith(f) for t in pred)] == list(S.NOT_SHOWN)
    assert set(S.NOT_SHOWN) <= set(S.not_shown())
    # "sls_exact" 1 at a case of each gather group: the same shape as a case of rules 1 ... 7, or that group's options
    exact = [c for c in sls if c.rule == 8 and dict(c.opts).get("sls_exact") == 1]
    assert any(c.L[0] == 10 and c.T == 4 and not dict(c.opts).get("sls_bpw") for c in exact), "group 4: automatic bags per wave"
    assert any(dict(c.opts).get("sls_bpw", 0) > 1 for c in exact) and any(dict(c.opts).get("sls_bpw") == 1 for c in exact)
    assert any(S.RAGGED in c.L for c in exact) and any(c.L[0] == 1 and c.T > 100 for c in exact) and any(c.D > 256 for c in exact)

def test_the_restatement_on_known_sets():
    """the shipped models' forms (DESIGN.md 3's table), by the restatement"""
    mk = lambda **kw: S.Case(**dict(dict(name="x", kind="sls", D=32, T=8, H=(), top=(), L=(80,), sizes=(256,), opts=(), rule=0, thr="", side="at",
                                         form="", expect=(), exclude=(), alone=None, note=""), **kw))
    assert S.expected_gather_form(mk(D=64, T=8, L=(80,))) == "flatc 16,20"                     # rmc1
    assert S.expected_gather_form(mk(D=32, T=8, L=(80,))) == "flatc 8,10"                      # dlrm_rm1.json
    assert S.expected_gather_form(mk(D=64, T=32, L=(120,))) == "ring 16,split"                 # rmc2: 30 loads per lane
    assert S.expected_gather_form(mk(D=32, T=10, L=(20,))) == "flat 8,5,bpw2"                  # rmc3
    assert S.expected_gather_form(mk(D=32, T=26, L=(1,))) == "one 8,16"                        # W&D, one query of 256
    assert S.expected_gather_form(mk(D=32, T=26, L=(1,) * 16, sizes=(256,) * 16)) == "one 8,64"
    din = dict(kind="din", D=32, T=254, H=(1,), top=(24, 2), L=(3,))
    assert S.expected_din_form(mk(**din)) == "din_pipe 8,S1"
    assert S.expected_din_form(mk(sizes=(256,) * 8, **dict(din, L=(3,) * 8))) == "din_pipe 8,S4"
    assert S.expected_dien_form(mk(kind="dien", D=32, T=43, H=(64,), top=(24, 2), L=(1,))) == "one 8,16 + dien_mfma 32,64,top"


def test_the_pattern_language():
    c = S.BY_NAME["bpw_32_L20"]
    good = ["set[2 queries, 192 rows, gather on own, mlp on own]", "sls_flat_kernel<8,5,bpw2>[152 wg, L=20]", "stream4_kernel[12 wg, 4 layers, 1 B lds]"]
    assert S.check_dispatch(c, good) == []
    assert S.check_dispatch(c, [good[0], "sls_flat_kernel<8,5,bpw4>[152 wg, L=20]"])
    assert S.check_dispatch(c, [good[0], "sls_flat_kernel<8,5,bpw2,nt>[152 wg, L=20]"])
    assert S.check_dispatch(c, good + ["sls_kernel<8,split>[3 wg]"])
    assert S.check_dispatch(c, [good[0], "sls_flat_kernel<8,5,bpw2,f16>[152 wg, L=20]"], tag="f16") == []
    c = S.BY_NAME["one_48_L1"]
    assert S.check_dispatch(c, ["sls_kernel<16,sequential>[9 wg]"]) == []
    assert S.check_dispatch(c, ["sls_kernel<16,sequential>[9 wg]", "sls_one_kernel<12,16>[3 wg]"])
    c = S.BY_NAME["top_5_layers"]
    assert S.check_dispatch(c, ["sls_one_kernel<8,16>[3 wg]", "dien_rnn_mfma_kernel<32,32>[3 wg]", "stream4_kernel[3 wg, 5 layers, 1 B lds]"]) == []
    assert S.check_dispatch(c, ["sls_one_kernel<8,16>[3 wg]", "dien_rnn_mfma_kernel<32,32>[3 wg]"]), "the top MLP must run somewhere"
    assert S.check_dispatch(c, ["sls_one_kernel<8,16>[3 wg]", "dien_rnn_mfma_kernel<32,32,top>[3 wg]"])
    c = S.BY_NAME["din_32_h3"]
    assert S.check_dispatch(c, ["sls_flat_kernel<8,5,bpw4>[1 wg, L=3]", "din_attention_kernel[19 wg]", "stream4_kernel[1 wg, 2 layers, 1 B lds]"]) == []
    assert S.check_dispatch(c, ["din_fused_kernel<8,S1,h4,C3>[75 wg]"])
