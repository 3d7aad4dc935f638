"""DIEN's recurrence on the bf16 matrix cores on the GPU (-m gpu): engine option "dien_bf16" 1, csrc/dien_bf16.hip.

tests/test_dien_bf16_cpu.py holds the cases, the inputs, the float64 reference of DESIGN.md 4.2's contract and TOL.  Per case,
one launch set: the dispatch log names dien_rnn_bf16_kernel; the last state (the first H columns of the interaction row) and
the scores are within TOL of the reference; "dien_fuse_top" 0 and 1 give the same bits; a query alone gives the bits it has
in the set; back at 0 the engine gives the bits it gave before the key was set.
"""
import numpy as np
import pytest

from deeprecsys_amd import _native as N
from tests import gather_shapes as S
from tests import test_dien_bf16_cpu as C
from tests.test_gather_boundaries import make_engine, run_set

pytestmark = pytest.mark.gpu


def engine_of(key, tab, w):
    _, D, T, _, _ = key
    eng = N.Engine(N.MODEL_DIEN, tab.table_rows(), D, w.ln_bot, w.ln_top, N.INTERACT_CAT, sigmoid_top=-1, max_batch=C.N_MAX, max_lookups=1,
                   num_staged_batches=3, num_slots=1)
    try:
        eng.set_option("dispatch_log", 1)
        for t, W in enumerate(tab.W):
            eng.set_table(t, W)
        for mlp, layers in ((N.MLP_RNN0, w.rnn[0]), (N.MLP_RNN1, w.rnn[1]), (N.MLP_TOP, w.top)):
            for l, (W, b) in enumerate(layers):
                eng.set_fc(mlp, l, W, b)
    except Exception:
        eng.close()
        raise
    return eng


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def run_bf16(eng, jobs, Hh):
    R, O, log = run_set(eng, jobs)
    assert any(t.startswith("dien_rnn_bf16_kernel<") for t in log) and not any(t.startswith("dien_rnn_mfma_kernel") for t in log), log
    return [r[:, :Hh] for r in R], O


@pytest.mark.parametrize("D,Hh,U,sizes", C.CASES, ids=C.IDS)
def test_bf16_recurrence_matches_the_contract(D, Hh, U, sizes):
    key = C.key_of(D, Hh, U)
    tab, w = C.model(key)
    staged = C.batches(key, tab)
    jobs = list(enumerate(sizes))
    eng = engine_of(key, tab, w)
    try:
        for b, (idx, lens) in enumerate(staged):
            eng.stage_batch(b, None, idx, lens)
        R0, O0, _ = run_set(eng, jobs)                                  # the fp32 engine
        eng.set_option("dien_bf16", 1)
        assert eng.get_option("dien_bf16") == 1
        Hs, Os = run_bf16(eng, jobs, Hh)
        for i, n in jobs:
            h64, o64 = C.reference(tab, w, staged[i][0], n)
            dh, do = float(np.abs(Hs[i] - h64).max()), float(np.abs(Os[i] - o64).max())
            print("query %d (%d samples): last state %.3g, scores %.3g of TOL %.3g" % (i, n, dh, do, C.TOL))
            assert dh <= C.TOL and do <= C.TOL, (i, n, dh, do)
            if len(jobs) > 1:                                           # alone: the bits it has in the set
                H1, O1 = run_bf16(eng, [(i, n)], Hh)
                assert np.array_equal(bits(H1[0]), bits(Hs[i])) and np.array_equal(bits(O1[0]), bits(Os[i])), i
        eng.set_option("dien_fuse_top", 0)
        Hf, Of = run_bf16(eng, jobs, Hh)
        eng.set_option("dien_fuse_top", 1)
        for i, _ in jobs:
            assert np.array_equal(bits(Hf[i]), bits(Hs[i])) and np.array_equal(bits(Of[i]), bits(Os[i])), i
        eng.set_option("dien_bf16", 0)
        R1, O1, _ = run_set(eng, jobs)
        for i, _ in jobs:
            assert np.array_equal(bits(R1[i]), bits(R0[i])) and np.array_equal(bits(O1[i]), bits(O0[i])), i
    finally:
        eng.close()


def test_nan_row_reaches_its_sample_and_no_other():
    """a padded-K shape (D + H = 48): the NaN row of behaviour table u, named by sample s of n, is step (s U + u) // n of
    sample (s U + u) % n (the Reshape)"""
    D, Hh, U, n, s, u = 16, 32, 5, 17, 3, 2
    key = C.key_of(D, Hh, U)
    tab, w = C.model(key)
    idx, lens = C.batches(key, tab)[0]
    eng = engine_of(key, tab, w)
    try:
        eng.set_option("dien_bf16", 1)
        eng.stage_batch(0, None, idx, lens)
        Hc, Oc = run_bf16(eng, [(0, n)], Hh)
        idx[1 + u][s] = 2 * tab.rows[1 + u]                            # the table's NaN row
        eng.stage_batch(0, None, idx, lens)
        Hp, Op = run_bf16(eng, [(0, n)], Hh)
    finally:
        eng.close()
    hot = np.zeros(n, bool)
    hot[(s * U + u) % n] = True
    assert np.isnan(Hp[0][hot]).all() and np.isfinite(Hc[0]).all() and np.isfinite(Oc[0]).all()
    assert np.array_equal(bits(Hp[0][~hot]), bits(Hc[0][~hot])) and np.array_equal(bits(Op[0][~hot]), bits(Oc[0][~hot]))


@pytest.mark.parametrize("name", ["w_32", "dien_16_8_mfma2"])
def test_other_models_and_shapes_refuse_the_key(name):
    key = S.engine_key(S.BY_NAME[name])
    eng = make_engine(key, S.Tables(key), S.Weights(key), N.TABLE_FP32)
    try:
        eng.set_option("dien_bf16", 0)
        with pytest.raises(N.DrsError) as ei:
            eng.set_option("dien_bf16", 1)
        assert ei.value.code == N.ERR_UNSUPPORTED and eng.get_option("dien_bf16") == 0
    finally:
        eng.close()
