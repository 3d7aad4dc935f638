"""DIN over fp16, bf16 and fp8 e4m3 tables on the GPU (-m gpu): engine option "din_table_dtype", din_pipe_narrow_kernel
(csrc/din_half.hip) and the two-launch form of the sets it does not cover.  The contract: a narrow engine serves, bit for
bit, what an fp32 engine serves on the upcast (fp8: decoded) tables.  A NaN equals a NaN (same_or_nan): the twin's tables come
from torch's converters, whose NaN carries another payload than the device's (bf16 0xffff0000 against 0x7fc00000, fp8
0x7ff00000 against 0xffc00000); every other element is compared by its bit pattern."""
import numpy as np
import pytest

from deeprecsys_amd import _native as N
from tests import gather_shapes as S
from tests import helpers as H
from tests.test_din_dien_nonfinite import same_or_nan
from tests.test_fp8_tables_cpu import fp8_decoded
from tests.test_gather_boundaries import DIN_OUT, DIN_ROW, run_set, stage
from tests.test_half_tables import upcast

pytestmark = pytest.mark.gpu
DT = {"fp16": (N.TABLE_FP16, "f16"), "bf16": (N.TABLE_BF16, "bf16"), "fp8": (N.TABLE_FP8_E4M3, "f8")}
TWO, THREE = (70, 5), (70, 5, 33)


def served(W, dtype):
    return W if dtype is None else fp8_decoded(W)[0] if dtype == "fp8" else upcast(W, DT[dtype][0])


def setup(D, U, L, sizes, h=(1,), poison=False, **opts):
    """-> (case, tables, weights, staged batches).  S.Tables with another magnitude per table (fp8: another exponent), table 2
    all zero; poison: the first integer row (no staged bag names it) of tables 0 and 1 is beyond fp16's range, that of table 2
    and of the last table holds a NaN, and bags of every third sample name them (a unit's ReLU may swallow either: the profile
    and context pass-throughs show them)"""
    L = (L,) * len(sizes) if isinstance(L, int) else tuple(L)
    case = S.Case("narrow", "din", D, U + 3, tuple(h), (24, 2), L, tuple(sizes), tuple(sorted(opts.items())), 0, "", "", "", (), (), None, "")
    tab, w = S.Tables(S.engine_key(case)), S.Weights(S.engine_key(case))
    for t, W in enumerate(tab.W):
        W[:-1] *= np.float32(1.25 * 2.0 ** (t % 7 - 3))
    tab.W[2][:-1] = 0.0
    st = S.Staged(case, tab)
    for t, first in (((0, 0), (1, 0), (2, 1), (-1, 1)) if poison else ()):
        tab.W[t][tab.rows[t]] = np.where(np.arange(D) % 3, 1.0e5, -1.0e5) if first == 0 else np.where(np.arange(D) == 5, np.nan, 0.0)
        for b in range(st.nb):
            st.idx[b][t][first * L[b]:S.B_MAX * L[b]:3 * L[b]] = tab.rows[t]
    return case, tab, w, st


def engine(case, W, w, st, option=None, before=True, **over):
    """a staged DIN engine on the tables W; option: its "din_table_dtype", set before the tables are written or after"""
    eng = N.Engine(N.MODEL_DIN, [x.shape[0] for x in W], case.D, w.ln_bot, w.ln_top, N.INTERACT_CAT, sigmoid_top=-1,
                   max_batch=S.B_MAX, max_lookups=S.RAGGED_MAX, num_staged_batches=S.N_BATCH, num_slots=1)
    try:
        for when in (True, False):
            if option is not None and before == when:
                eng.set_option("din_table_dtype", option)
            for t, x in (enumerate(W) if when else ()):
                eng.set_table(t, x)
        for mlp, layers in [(N.MLP_ATT0 + u, unit) for u, unit in enumerate(w.att)] + [(N.MLP_TOP, w.top)]:
            for l, (Wl, b) in enumerate(layers):
                eng.set_fc(mlp, l, Wl, b)
        for k, v in list(S.options(case).items()) + [("dispatch_log", 1)] + list(over.items()):
            eng.set_option(k, v)
        stage(eng, st, w)
    except Exception:
        eng.close()
        raise
    return eng


def twin_check(dtype, case, tab, w, st, nar=None, tables=None, **twin_over):
    """the narrow engine against an fp32 engine on the served tables, the set and every query alone -> the set's (R, out, log)"""
    tables = [served(W, dtype) for W in tab.W] if tables is None else tables
    nar_, twin = nar or engine(case, tab.W, w, st, DT[dtype][0]), None
    try:
        twin = engine(case, tables, w, st, **twin_over)
        jobs, first = st.jobs(), None
        for js in [jobs] + ([[j] for j in jobs] if len(jobs) > 1 else []):
            (Rn, On, log), (Rt, Ot, _) = run_set(nar_, js), run_set(twin, js)
            first = first or (Rn, On, log)
            assert all(same_or_nan(a, b) for a, b in zip(Rn + On, Rt + Ot)), (dtype, js, log)
        return first
    finally:
        for e in (twin, None if nar else nar_):
            if e is not None:
                e.close()


# D, U, L, sizes, options: both group_sum widths; din_s 1 | 2 | 4 with a ragged last workgroup and a one-sample set; every bag
# length; K = units per lane group on both sides of P and 2 P for P 2 and 4 (D 64: 16 lane groups); the second staging round
SHAPES = dict(
    [("d64_s%d" % s, (64, 5, 3, TWO, dict(din_s=s))) for s in (1, 2, 4)] +
    [("d32_s4", (32, 5, 3, TWO, dict(din_s=4, din_nt=1))), ("d32_s4_one", (32, 5, 3, (1,), dict(din_s=4))), ("d32_L1", (32, 5, 1, TWO, {})),
     ("d32_L2", (32, 5, 2, TWO, dict(din_s=2, din_nt=1))), ("d32_L123", (32, 6, (1, 2, 3), THREE, dict(din_s=4))),
     ("d32_U129", (32, 129, 3, TWO, dict(din_s=2))), ("d32_T257", (32, 254, (3, 1, 2), THREE, dict(din_s=4))),
     ("poison", (32, 5, 3, TWO, dict(din_s=4, poison=True)))] +
    [("d64_U%d" % u, (64, u, 3, TWO, dict(din_s=(1, 2, 4)[u % 3]))) for u in (33, 64, 65, 128, 129)])


@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("dtype", sorted(DT))
def test_narrow_pipe_launch_serves_the_fp32_twins_bits(dtype, shape):
    D, U, L, sizes, opts = SHAPES[shape]
    case, tab, w, st = setup(D, U, L, sizes, **opts)
    nar = engine(case, tab.W, w, st, DT[dtype][0])
    try:
        Rq, _, log = twin_check(dtype, case, tab, w, st, nar)
        hit = [t for t in log if t.startswith("din_pipe_narrow_kernel<%d,S%d,P" % (D // 4, opts.get("din_s", 1)))]
        assert len(hit) == 1 and (",%s>[" % DT[dtype][1]) in hit[0] and ("nt" in hit[0].split(",")) == bool(opts.get("din_nt")), log
        assert not any(t.startswith(("din_pipe_kernel", "din_fused_kernel", "sls_", "din_attention")) for t in log), log
        if dtype == "fp8":        # another exponent per table, 0 for the all-zero one
            ks = [nar.table_fp8_exponent(t) for t in range(case.T)]
            assert ks[2] == 0 and len(set(ks)) >= 4, ks
        if shape == "poison":     # samples 0, 3, ... carry the overflowing rows (inf in fp16 alone), 1, 4, ... the NaN; nobody else
            hot = np.arange(len(Rq[0])) % 3
            assert np.array_equal(~np.isfinite(Rq[0]).all(axis=1), (hot == 1) | ((hot == 0) & (dtype == "fp16")))
    finally:
        nar.close()


@pytest.mark.parametrize("D", [32, 64])
@pytest.mark.parametrize("dtype", sorted(DT))
def test_narrow_pipe_launch_against_float64(dtype, D):
    case, tab, w, st = setup(D, 5, 3, TWO, din_s=2)
    eng = engine(case, tab.W, w, st, DT[dtype][0])
    try:
        Rq, Oq, log = run_set(eng, st.jobs())
        assert any(t.startswith("din_pipe_narrow_kernel") for t in log), log
    finally:
        eng.close()
    f64 = lambda x: np.asarray(x, np.float64)    # noqa: E731
    for i, (b, n) in enumerate(st.jobs()):
        idx, lens = st.query(b, n)
        pooled = [S.sls64(served(tab.W[t], dtype), idx[t], lens[t])[0] for t in range(case.T)]
        att = sum(np.maximum(np.maximum(np.concatenate([u, pooled[-2], u + pooled[-2]], 1) @ f64(W1).T + f64(b1), 0) @ f64(W2).T + f64(b2), 0)
                  for u, ((W1, b1), (W2, b2)) in zip(pooled[1:-2], w.att))
        R64 = out64 = np.concatenate([pooled[0], att, pooled[-2], pooled[-1]], 1)
        for Wl, bl in w.top:
            out64 = np.maximum(out64 @ f64(Wl).T + f64(bl), 0)
        print(dtype, D, i, "max |R - R64| %.3g, max |out - out64| %.3g" % (np.abs(Rq[i] - R64).max(), np.abs(Oq[i] - out64).max()))
        for lo in range(0, 4 * D, D):      # profile | attention block | candidate ad | context
            assert H.close(Rq[i][:, lo:lo + D], R64[:, lo:lo + D], **DIN_ROW), (dtype, D, i, lo)
        assert H.close(Oq[i], out64, **DIN_OUT), (dtype, D, i)


# sets the narrow pipe form does not take: D, U, L, sizes, h, options, the attention kernel's token (None: T877 x 56 bytes fit
# the 48 KB the staged indices may take under "din_s" 4, and the set takes the narrow pipe form; T878 does not)
AK, AA = "din_attention_kernel[", "din_attention_any_kernel["
OTHER = {"h2": (32, 5, 3, TWO, (2,), {}, AK), "L4": (32, 5, 4, TWO, (1,), {}, AK), "ragged": (64, 5, S.RAGGED, TWO, (1,), {}, AK),
         "D16": (16, 5, 3, TWO, (1,), {}, AK), "D128": (128, 5, 3, TWO, (1,), {}, AK), "D30": (30, 5, 3, TWO, (1,), {}, AA),
         "pipe0": (32, 5, 3, TWO, (1,), dict(din_pipe=0), AK), "exact": (32, 5, 3, TWO, (1,), dict(sls_exact=1), AK),
         "T877": (32, 874, 3, (6,), (1,), dict(din_s=4), None), "T878": (32, 875, 3, (6,), (1,), dict(din_s=4), AK)}


@pytest.mark.parametrize("dtype,name", [(d, n) for n in sorted(OTHER) for d in ("fp16", "fp8") if d == "fp16" or not n.startswith("T87")])
def test_other_sets_take_the_gather_of_the_type_and_the_attention_kernel(dtype, name):
    D, U, L, sizes, h, opts, att = OTHER[name]
    case, tab, w, st = setup(D, U, L, sizes, h=h, **opts)
    _, _, log = twin_check(dtype, case, tab, w, st, din_fused=0 if att else 1)
    launches = [t for t in log if t.startswith(("sls_", "din_"))]
    if att is None:
        assert len(launches) == 1 and launches[0].startswith("din_pipe_narrow_kernel<8,S4,"), log
    else:
        assert len(launches) == 2 and launches[0].startswith("sls_") and DT[dtype][1] in launches[0] and launches[1].startswith(att), log


def test_the_key_on_a_din_engine():
    case, tab, w, st = setup(32, 5, 3, TWO)
    eng = engine(case, tab.W, w, st)

    def refused(key, v, code):
        before = run_set(eng, st.jobs())
        with pytest.raises(N.DrsError) as e:
            eng.set_option(key, v)
        after = run_set(eng, st.jobs())
        assert e.value.code == code and all(np.array_equal(a, b) for a, b in zip(before[0] + before[1], after[0] + after[1])), (key, v)
    try:
        for v in (3, 8, 9):
            refused("din_table_dtype", v, N.ERR_BAD_ARG)
        # 1 -> 0 -> 4 -> 0: the twin's bits at every stop (back at 0 the arena holds the rounded values)
        cur = tab.W
        for dtype, v in (("fp16", N.TABLE_FP16), (None, N.TABLE_FP32), ("fp8", N.TABLE_FP8_E4M3), (None, N.TABLE_FP32)):
            eng.set_option("din_table_dtype", v)
            assert eng.get_option("din_table_dtype") == eng.get_option("table_dtype") == v
            cur = [served(W, dtype) for W in cur]
            _, _, log = twin_check(dtype, case, tab, w, st, eng, tables=cur)
            assert any(t.startswith("din_pipe_narrow_kernel") for t in log) == bool(dtype), log
            for other in {N.TABLE_FP32, N.TABLE_FP16, N.TABLE_BF16} - {v}:
                refused("table_dtype", other, N.ERR_UNSUPPORTED)        # "table_dtype" still refuses on DIN ...
            eng.set_option("table_dtype", v)                            # ... and takes the arena's own type as nothing to do
        # the option before the tables are written and after: the same outputs
        early, late = [engine(case, tab.W, w, st, N.TABLE_BF16, before=b) for b in (True, False)]
        try:
            (Re, Oe, _), (Rl, Ol, _) = run_set(early, st.jobs()), run_set(late, st.jobs())
            assert all(np.array_equal(a, b) for a, b in zip(Re + Oe, Rl + Ol))
        finally:
            early.close()
            late.close()
        idx, lens = st.stage(0, 70)
        idx[3][4] = tab.W[3].shape[0]                                   # an index beyond its table
        with pytest.raises(N.DrsError) as e:
            eng.stage_batch(0, None, idx, lens)
            eng.forward(0, 70)
        assert e.value.code == N.ERR_INDEX_RANGE
    finally:
        eng.close()


@pytest.mark.parametrize("kind", ["dlrm", "dien"])
def test_the_key_on_other_models(kind):
    if kind == "dlrm":
        eng = N.Engine(N.MODEL_DLRM, [50, 60], 32, [8, 32], [96, 4, 1], N.INTERACT_CAT, sigmoid_top=2, max_batch=8, max_lookups=2)
    else:
        eng = N.Engine(N.MODEL_DIEN, [50] * 5, 32, [32, 16], [16 + 96, 4, 1], N.INTERACT_CAT, sigmoid_top=-1, max_batch=8, max_lookups=1)
    try:
        eng.set_option("din_table_dtype", N.TABLE_FP32)
        for v in (N.TABLE_FP16, N.TABLE_FP8_E4M3):
            with pytest.raises(N.DrsError) as e:
                eng.set_option("din_table_dtype", v)
            assert e.value.code == N.ERR_UNSUPPORTED and "table_dtype" in str(e.value)
        assert eng.get_option("din_table_dtype") == N.TABLE_FP32
    finally:
        eng.close()
