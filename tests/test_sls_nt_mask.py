"""The gather's row-load cache policy table by table on the GPU (-m gpu): engine option "sls_nt_mask".

The contract (docs/OPTIONS.md): bit t of the mask says whether table t's rows are read with non-temporal or with plain
loads, and nothing else changes -- the pooled sums are bit-identical to the uniform engine's under every mask.  A mixed
mask is served by the per-table kernels of the one-bag-per-wave forms on fp32 rows -- the coalesced flat form and the split
ring walk (the dispatch record names them, with `ntm=0x..`); all zeros and all ones plan the uniform instances; every
other form keeps "sls_nt".  Three tables, so that
with sample-major bag numbering a wave's table changes from wave to wave.
"""
import numpy as np
import pytest

from deeprecsys_amd import _native as N
from tests.test_half_tables import _load

pytestmark = pytest.mark.gpu

ROWS, B = 2000, 5
MASKS = (0, 0b111, 0b101, 0b010)


def ring_from(D):
    """the first bag length plan_sls sends to the ring walk: more than 20 loads per lane in the flat forms"""
    return 20 * (64 // (D // 4)) + 1


def _engine(T, D, L):
    eng = N.Engine(N.MODEL_DLRM, [ROWS] * T, D, [8, D], [D * (T + 1), 4, 1], N.INTERACT_CAT, sigmoid_top=2,
                   max_batch=B, max_lookups=L, num_staged_batches=4, num_slots=2)
    eng.set_option("dispatch_log", 1)
    return eng


def _stage(eng, rng, T, D, L, tables):
    _load(eng, 11, tables, D, T)
    for b in range(3):
        lens = [np.full(B, L, np.int32) for _ in range(T)]
        idx = [rng.randint(0, ROWS, size=B * L).astype(np.int64) for _ in range(T)]
        for t in range(T):
            idx[t][0], idx[t][-1] = 0, ROWS - 1
        eng.stage_batch(b, rng.rand(B, 8).astype(np.float32), idx, lens)


def _run(eng, D, T):
    """a single-query set and a 3-query set: (outputs, pooled columns, gather tokens of the dispatch record) of each"""
    got = []
    out = eng.forward(0, B)
    got.append((out.view(np.uint32), eng.fetch_interaction(B).view(np.uint32), [t for t in eng.last_dispatch(0) if t.startswith("sls_")]))
    jobs = [(0, B), (1, 3), (2, 1)]
    eng.forward_multi_async(1, [b for b, _ in jobs], [n for _, n in jobs])
    out = eng.wait(1, sum(n for _, n in jobs))
    vrows = sum((n + 63) // 64 * 64 for _, n in jobs)
    R = eng.fetch_interaction(vrows, slot=1)
    keep = np.concatenate([np.arange(64 * k, 64 * k + n) for k, (_, n) in enumerate(jobs)])   # (pad rows between queries: not compared)
    got.append((out.view(np.uint32), R[keep].view(np.uint32), [t for t in eng.last_dispatch(1) if t.startswith("sls_")]))
    return got


@pytest.mark.parametrize("D", [64, 32])
@pytest.mark.parametrize("where", ["flatc", "ring"])
def test_every_mask_serves_the_uniform_engines_bits(D, where):
    T = 3
    L = 80 if where == "flatc" else ring_from(D)
    rng = np.random.RandomState(D + L)
    tables = [rng.uniform(-1, 1, (ROWS, D)).astype(np.float32) for _ in range(T)]
    eng = _engine(T, D, L)
    try:
        _stage(eng, rng, T, D, L, tables)
        eng.set_option("sls_nt", 0)
        assert eng.get_option("sls_nt_mask") == -1
        ref = _run(eng, D, T)
        form = "sls_flatc_kernel<%d,%d" % (D // 4, 20 if D == 64 else 10) if where == "flatc" else "sls_kernel<%d,split" % (D // 4)
        assert all(len(log) == 1 and log[0].startswith(form) and "ntm" not in log[0] for _, _, log in ref), ref[0][2]
        eng.set_option("sls_nt", 1)
        ref_nt = _run(eng, D, T)
        for mask in MASKS:
            eng.set_option("sls_nt_mask", mask)
            assert eng.get_option("sls_nt_mask") == mask
            got = _run(eng, D, T)
            for (o, R, log), (o0, R0, log0), (_, _, log1) in zip(got, ref, ref_nt):
                assert np.array_equal(R, R0) and np.array_equal(o, o0), (mask, log)
                if mask in (0b101, 0b010):                                    # the per-table kernels (sls_ntm.hip), by their names
                    masked = log0[0].replace("sls_flatc_kernel<", "sls_flatc_ntm_kernel<").replace("sls_kernel<", "sls_ntm_kernel<")
                    assert masked != log0[0] and log == [masked.replace(">[", ",ntm=0x%x>[" % mask)], log
                else:
                    assert log == (log1 if mask else log0), (mask, log)       # all zeros / all ones: the uniform instances
        # unset: the lines of an engine that never heard of the option
        eng.set_option("sls_nt_mask", -1)
        assert [log for _, _, log in _run(eng, D, T)] == [log for _, _, log in ref_nt]
        # a bit beyond the model's tables
        with pytest.raises(N.DrsError) as err:
            eng.set_option("sls_nt_mask", 1 << T)
        assert err.value.code == N.ERR_BAD_ARG and eng.get_option("sls_nt_mask") == -1
    finally:
        eng.close()


def test_an_out_of_range_index_is_flagged_under_either_policy_of_a_mixed_mask():
    """One bad index in a table read non-temporally and one in a table read with plain loads: the batch is refused with
    DRS_ERR_INDEX_RANGE exactly as under the uniform policy, nothing faults, and the engine serves on.  (A staged batch is
    range-checked on the host before it reaches the kernel; the per-table kernel keeps sls_flatc_kernel's own check -- the
    error word, the address clamped to row 0 -- for the paths that do not.)"""
    T, D, L = 3, 64, 80
    rng = np.random.RandomState(3)
    tables = [rng.uniform(-1, 1, (ROWS, D)).astype(np.float32) for _ in range(T)]
    eng = _engine(T, D, L)
    try:
        _stage(eng, rng, T, D, L, tables)

        def outcome(bad_table):
            lens = [np.full(B, L, np.int32) for _ in range(T)]
            idx = [rng.randint(0, ROWS, size=B * L).astype(np.int64) for _ in range(T)]
            idx[bad_table][L + 7] = ROWS + 5
            try:
                eng.stage_batch(3, rng.rand(B, 8).astype(np.float32), idx, lens)
                eng.forward(3, B)
            except N.DrsError as e:
                return e.code
            return N.OK

        for mask in (-1, 0b101):
            eng.set_option("sls_nt_mask", mask)
            for bad_table in (0, 1):                  # (under 0b101: a set bit, a clear bit)
                assert outcome(bad_table) == N.ERR_INDEX_RANGE, (mask, bad_table)
                eng.forward(0, B)                     # a good set afterwards is served
    finally:
        eng.close()


def test_two_bags_per_wave_keep_the_uniform_policy_under_a_mixed_mask():
    """Short bags share a wave (sls_flat_kernel, 2 bags of consecutive tables): a wave spans tables, the mask does not apply."""
    T, D, L = 4, 64, 8
    rng = np.random.RandomState(5)
    tables = [rng.uniform(-1, 1, (ROWS, D)).astype(np.float32) for _ in range(T)]
    eng = _engine(T, D, L)
    try:
        _stage(eng, rng, T, D, L, tables)
        ref = _run(eng, D, T)
        assert all(log[0].startswith("sls_flat_kernel<16,5,bpw2") for _, _, log in ref), ref[0][2]
        eng.set_option("sls_nt_mask", 0b0110)
        for (o, R, log), (o0, R0, log0) in zip(_run(eng, D, T), ref):
            assert log == log0 and np.array_equal(R, R0) and np.array_equal(o, o0)
    finally:
        eng.close()
