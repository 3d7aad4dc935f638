"""CPU side of weights inside the flat and one-lookup gather forms (engine option "sls_weighted_flat",
--accel_sls_weighted_flat): the shape catalogue the GPU tests (tests/test_sls_weights_flat.py) run, the numpy restatement
of the flat forms' summation order with weights (`flat_order_ref`), and the flag / option plumbing.

The order, for a wave that holds `bpw` bags of L rows each (R = bpw * L flattened rows, row j of the wave = row j % L of
bag j // L): lane group g of NG = 64 / G chains the flattened rows j = g, g + NG, g + 2 NG, ... in rising j with the
weighted step of tests/test_sls_weights_cpu.py -- acc = fma(w, x, acc), rowwise s = w * scale, b = w * bias,
acc = fma(s, q, acc + b) -- where a row of another bag (or past R) has the weight 0: the identity, so it is skipped
here.  Then the xor butterfly adds the groups' partial sums: m = 1, 2, ..., NG / 2, every group g taking
part[g] + part[g ^ m]."""
import os

import numpy as np
import pytest

from deeprecsys_amd import dlrm_s_hip
from deeprecsys_amd.utils.utils import FLAG_CHOICES, cli
from tests import gather_shapes as GS
from tests import helpers as H
from tests.test_bf16_mlp_cpu import _Recorder
from tests.test_sls_weights_cpu import codes4, codes8, fma32, same_bits, weighted_ref, weighted_ref_rowwise

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEY = "sls_weighted_flat"
B = 48                                            # samples per staged batch; queries of 48, 1 and 29 samples
SIZES = (B, 1, 29)


def rows_of(T):
    return [1501 + 13 * t for t in range(T)]


# ---- the shape catalogue: (D, T, L, options) -- the smallest shapes at each form's edges ------------------------------------
CATALOGUE = [
    (64, 3, 2, {}),                               # flatc 16,5: the shortest bag
    (64, 3, 20, {}),                              # flatc 16,5: five full loads
    (64, 3, 21, {}),                              # flatc 16,10: a partial last load
    (64, 3, 80, {}),                              # flatc 16,20: the last L that is flat
    (64, 3, 81, {}),                              # ring 16,split: the first L that is not
    (32, 3, 130, {}),                             # flatc 8,20: three index registers per lane, the last one partial
    (24, 3, 7, {}),                               # flatc 8,5: idle lanes, clamped columns
    (128, 3, 40, {}),                             # flatc 32,20: NG 2
    (32, 4, 10, {}),                              # flat 8,5,bpw4: four bags per wave
    (32, 4, 20, {}),                              # flat 8,5,bpw2: two bags per wave
    (64, 4, 5, {}),                               # flat 16,5,bpw4
    (128, 4, 5, {}),                              # flat 32,5,bpw2
    (32, 4, 20, {"sls_bpw": 4}),                  # flat 8,10,bpw4: forced BPW
    (64, 3, 41, {"sls_flat": 2}),                 # flat 16,20,bpw1: the forced phased form
] + [(D, 3, 1, {}) for D in (16, 32, 64, 128)] + [   # one D/4,16: tail lanes
    (D, 3, 1, {"sls_one": 64}) for D in (16, 32, 64, 128)]   # one D/4,64: sets of more than 64 samples, two tiles, the second partial
# what the issue's table states for them, in tests/gather_shapes.py's shorthand
STATED = (["flatc 16,5", "flatc 16,5", "flatc 16,10", "flatc 16,20", "ring 16,split", "flatc 8,20", "flatc 8,5", "flatc 32,20",
           "flat 8,5,bpw4", "flat 8,5,bpw2", "flat 16,5,bpw4", "flat 32,5,bpw2", "flat 8,10,bpw4", "flat 16,20,bpw1"] +
          ["one %d,16" % (D // 4) for D in (16, 32, 64, 128)] + ["one %d,64" % (D // 4) for D in (16, 32, 64, 128)])


def shape_id(shape):
    D, T, L, opts = shape
    return "D%d-T%d-L%d%s" % (D, T, L, "".join("-%s%d" % kv for kv in sorted(opts.items())))


def expected_form(shape, sizes=(B,)):
    """the unweighted launch's form by tests/gather_shapes.expected_gather_form (shorthand, e.g. "flatc 16,5")"""
    D, T, L, opts = shape
    case = GS.Case(shape_id(shape), "sls", D, T, (), (), (L,) * len(sizes), tuple(sizes), tuple(sorted(opts.items())), 0, "", "at",
                   "", (), (), None, "")
    return GS.expected_gather_form(case)


def log_token(form, nt, tag="", weighted=True):
    """shorthand -> the dispatch-log token's prefix: "sls_flatc_kernel<16,5,nt,f16,w>[" (nt: "sls_nt"; the sequential ring walk
    and the one-lookup form carry no nt)"""
    k, _, a = form.partition(" ")
    name = {"flatc": "sls_flatc_kernel", "flat": "sls_flat_kernel", "one": "sls_one_kernel", "ring": "sls_kernel"}[k]
    parts = [a]
    if nt and (k in ("flatc", "flat") or a.endswith("split")):
        parts.append("nt")
    if tag:
        parts.append(tag)
    if weighted:
        parts.append("w")
    return "%s<%s>[" % (name, ",".join(parts))


def order_of(form):
    """-> None (the sequential chain: weighted_ref) or (NG, bpw) of a flat / flatc form"""
    k, _, a = form.partition(" ")
    if k not in ("flat", "flatc"):
        return None
    f = a.split(",")
    return 64 // int(f[0]), int(f[2][3:]) if k == "flat" else 1


# ---- the restatement ---------------------------------------------------------------------------------------------------------
def flat_order_ref(stored, idx, w, B_, L, NG, bpw=1, k=0, plain_add=False, parts=False):
    """[B_, D] fp32: the flat forms' pooled vectors of ONE table whose bags are the k-th of `bpw` in their wave.
    stored: the fp32 table, or (codes, scale, bias) of a rowwise one; idx, w: [B_ * L] of that table (fixed L).
    plain_add: fp32 additions instead of the weighted step (w ignored); parts: return every lane group's result [NG, B_, D]."""
    rowwise = isinstance(stored, tuple)
    D = (stored[0] if rowwise else stored).shape[1]
    idx, w = np.asarray(idx, np.int64), np.asarray(w, np.float32)
    part = np.zeros((NG, B_, D), np.float32)
    for jj in range(L):                                                # rising j inside every group's chain
        g = (k * L + jj) % NG
        pos = np.arange(B_) * L + jj
        r, ww = idx[pos], w[pos]
        if plain_add:
            part[g] = (part[g] + stored[r]).astype(np.float32)
        elif rowwise:
            q, sc, bi = stored
            s = (ww * sc[r]).astype(np.float32)[:, None]
            b = (ww * bi[r]).astype(np.float32)[:, None]
            part[g] = fma32(s, q[r], (part[g] + b).astype(np.float32))
        else:
            part[g] = fma32(ww[:, None], stored[r], part[g])
    m = 1
    while m < NG:
        part = np.stack([(part[g] + part[g ^ m]).astype(np.float32) for g in range(NG)])
        m <<= 1
    return part if parts else part[0]


def seq_ref(stored, idx, lens, w):
    if isinstance(stored, tuple):
        return weighted_ref_rowwise(stored[0], stored[1], stored[2], idx, lens, w)
    return weighted_ref(stored, idx, lens, w)


def stored_cpu(kind, W):
    if kind == "fp32":
        return np.ascontiguousarray(W, np.float32)
    return (codes8(W) if kind == "int8" else codes4(W))[1:]


# ---- 1. the catalogue is the issue's table ------------------------------------------------------------------------------------
def test_the_catalogue_takes_the_forms_the_issue_states():
    assert len(CATALOGUE) == len(STATED) == 22
    for shape, form in zip(CATALOGUE, STATED):
        assert expected_form(shape) == form, shape
        for sizes in ((1,), (29,), (B, 1, 29) * 4):                    # ... alone and in sets
            assert expected_form(shape, sizes) == form, (shape, sizes)
    assert log_token("flatc 16,5", 1) == "sls_flatc_kernel<16,5,nt,w>["
    assert log_token("flat 8,5,bpw2", 1, "f16") == "sls_flat_kernel<8,5,bpw2,nt,f16,w>["
    assert log_token("one 16,16", 1) == "sls_one_kernel<16,16,w>["
    assert log_token("ring 16,split", 1, "i8") == "sls_kernel<16,split,nt,i8,w>["
    assert log_token("ring 16,sequential", 1, weighted=False) == "sls_kernel<16,sequential>["
    assert order_of("flat 8,10,bpw4") == (8, 4) and order_of("flatc 32,20") == (2, 1) and order_of("one 8,16") is None


# ---- 2. the restatement --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["fp32", "int8", "int4"])
@pytest.mark.parametrize("shape", [s for s, f in zip(CATALOGUE, STATED) if order_of(f)], ids=shape_id)   # (the others: weighted_ref itself)
def test_flat_order_restated(kind, shape):
    D, T, L, opts = shape
    NG, bpw = order_of(expected_form(shape))
    rng = np.random.RandomState(1000 * D + 10 * L + bpw)
    worst = 0.0
    for k in range(bpw):
        W = rng.uniform(-1, 1, (1500, D)).astype(np.float32)
        st = stored_cpu(kind, W)
        idx = rng.randint(0, 1500, size=B * L).astype(np.int64)
        w = rng.uniform(0, 1, size=B * L).astype(np.float32)
        lens = np.full(B, L)
        groups = flat_order_ref(st, idx, w, B, L, NG, bpw, k, parts=True)
        assert all(same_bits(groups[0], groups[g]) for g in range(NG)), (kind, shape, k)   # every group holds the sum
        got = groups[0]
        seq = seq_ref(st, idx, lens, w)
        worst = max(worst, float(np.abs(got.astype(np.float64) - seq).max()))
        assert H.close(got, seq, rtol=1e-5, atol_scale=2e-6), (kind, shape, k, worst)     # the split-order tolerance
        if L > NG:                                                     # ... and not the same bits: a bit comparison tells the forms apart
            assert not same_bits(got, seq), (kind, shape, k)
        if kind == "fp32":                                             # weights of 1.0: plain fp32 additions in the same order
            ones = np.ones(B * L, np.float32)
            assert same_bits(flat_order_ref(st, idx, ones, B, L, NG, bpw, k), flat_order_ref(st, idx, ones, B, L, NG, bpw, k, plain_add=True))
    print("worst |flat order - sequential| = %.3g (%s, %s)" % (worst, kind, shape_id(shape)))


def test_a_weight_of_zero_is_the_identity():
    """what lets flat_order_ref skip the rows a lane adds with the weight 0 (another bag's, past the wave's rows, out of
    range): fma(0, x, acc) == acc, and the rowwise step with s = b = +-0 likewise -- acc is never -0"""
    rng = np.random.RandomState(5)
    acc = np.concatenate([rng.uniform(-3, 3, 200), [0.0, 1e-40, -1e-40]]).astype(np.float32)
    x = rng.uniform(-1, 1, acc.size).astype(np.float32)
    assert same_bits(fma32(np.float32(0), x, acc), acc)
    for z in (np.float32(0.0), np.float32(-0.0)):                      # 0 * scale, 0 * bias of either sign
        assert same_bits(fma32(z, np.abs(x) * 15, (acc + z).astype(np.float32)), acc)


# ---- 3. flag and option plumbing ---------------------------------------------------------------------------------------------
def test_flag_defaults_to_off_and_takes_0_or_1():
    assert cli([]).accel_sls_weighted_flat == 0
    for v in (0, 1):
        assert cli(["--accel_sls_weighted_flat", str(v)]).accel_sls_weighted_flat == v
    assert FLAG_CHOICES["accel_sls_weighted_flat"] == (0, 1)
    for bad in ("2", "-1", "yes"):
        with pytest.raises(SystemExit):
            cli(["--accel_sls_weighted_flat", bad])
    args = cli([])
    for bad in (2, -1):
        args.accel_sls_weighted_flat = bad                             # (a JSON config can set anything: refused at engine build)
        with pytest.raises(ValueError):
            dlrm_s_hip._sls_weighted_flat(args)
    args.accel_sls_weighted_flat = 1
    assert dlrm_s_hip._sls_weighted_flat(args) == 1


def _engine_calls(monkeypatch, **flags):
    meta, _ = H.load_fixture("dlrm_dot_small")
    args = H.args_from(meta["args"], **flags)
    np.random.seed(args.numpy_rand_seed)
    net = H.NET_CLS[args.model_type](args)
    monkeypatch.setattr(dlrm_s_hip.N, "Engine", _Recorder)
    _Recorder.log = []
    net._create_engine()
    return list(_Recorder.log)


@pytest.mark.parametrize("flags", [{}, {"accel_sls_weights": "uniform"}, {"accel_table_dtype": "int4_rowwise", "accel_table_int4_lines": 1}])
def test_the_host_code_sets_the_option_only_when_the_flag_is_non_zero(monkeypatch, flags):
    """The CPU restatement of the ABI does not know the key: only a user who asked for it may reach it."""
    base = _engine_calls(monkeypatch, **flags)
    assert [c for c in base if c[0] == "set_fc"]
    assert [c for c in base if c[:2] == ("set_option", KEY)] == []
    assert _engine_calls(monkeypatch, accel_sls_weighted_flat=0, **flags) == base
    with_flag = _engine_calls(monkeypatch, accel_sls_weighted_flat=1, **flags)
    assert [c for c in with_flag if c[:2] == ("set_option", KEY)] == [("set_option", KEY, 1)] * len([c for c in with_flag if c[0] == "create"])
    assert [c for c in with_flag if c[:2] != ("set_option", KEY)] == base


def test_default_flags_set_nothing_on_the_cpu_abi(cpu_abi):
    meta, _ = H.load_fixture("dlrm_dot_small")
    net, lX, lS_l, lS_i, lT = H.materialize(H.args_from(meta["args"]))
    net.create(lX[0], lS_l[0], lS_i[0], lT[0])
    try:
        assert KEY not in net.engine.user_options
    finally:
        net.engine.close()


def test_documents_name_the_key():
    doc = open(os.path.join(ROOT, "docs", "OPTIONS.md")).read()
    assert "`sls_weighted_flat`" in doc and "--accel_sls_weighted_flat" in doc
    assert '"sls_weighted_flat" 0|1' in open(os.path.join(ROOT, "include", "drs.h")).read()
    assert "#define DRS_ABI_VERSION 5" in open(os.path.join(ROOT, "include", "drs.h")).read()
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "--accel_sls_weighted_flat" in readme and "`sls_weighted_flat`" in readme
    assert "sls_weighted_flat" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "sls_weighted_flat" in open(os.path.join(ROOT, "DESIGN.md")).read()
