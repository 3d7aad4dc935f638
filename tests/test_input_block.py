"""The copies of the per-call input blocks at their edges (csrc/input_block.h plan_block_copies, issued by
drs_run_queues_multi_async and drs_forward_inputs_async): every set and query below gives the bits of the same queries served
alone from staged inputs, whichever copies carried it -- all blocks in one copy, up to the last block's used prefix, a
prefix per block with and without its prefix sums, and both sides of the size from which a single query is copied at all."""
import numpy as np
import pytest

from deeprecsys_amd import _native as N
from tests import helpers as H

pytestmark = pytest.mark.gpu

# "sls_uniform" 0 makes the kernels read the prefix sums of fixed-length bags too, so they have to travel with every copy: an
# option of the lab build alone (docs/OPTIONS.md) -- the product library refuses the key, and that half runs under DRS_TEST_LAB=1
UNIFORM = (1, 0) if H.LAB else (1,)


def make_engine(T, D, rows, m_den, max_batch, max_lookups, seed):
    rng = np.random.RandomState(seed)
    eng = N.Engine(N.MODEL_DLRM, [rows] * T, D, [m_den, D], [D * (T + 1), 8, 1], N.INTERACT_CAT, sigmoid_top=2,
                   max_batch=max_batch, max_lookups=max_lookups, num_staged_batches=1, num_slots=2)
    for t in range(T):
        eng.fill_table_uniform(t, -0.1, 0.1, 3 + t)
    eng.set_fc(N.MLP_BOT, 0, rng.randn(D, m_den).astype(np.float32), rng.randn(D).astype(np.float32))
    eng.set_fc(N.MLP_TOP, 0, rng.randn(8, D * (T + 1)).astype(np.float32) * 0.05, np.zeros(8, np.float32))
    eng.set_fc(N.MLP_TOP, 1, rng.randn(1, 8).astype(np.float32), np.zeros(1, np.float32))
    return eng, rng


def make_query(rng, T, rows, m_den, lens):
    """lens [T, bs] int32 (every table sums to the same count, as the 2-D form wants) -> (dense, ids, lens, bs)"""
    lens = np.ascontiguousarray(lens, dtype=np.int32)
    n = int(lens[0].sum())
    assert all(int(r.sum()) == n for r in lens)
    bs = lens.shape[1]
    return (rng.rand(bs, m_den).astype(np.float32), rng.randint(0, rows, size=(T, n)).astype(np.int64), lens, bs)


def set_uniform(eng, value):
    if H.LAB:
        eng.set_option("sls_uniform", value)


def staged(eng, q):
    """the query served alone from staged inputs: the yardstick (computed once per query, before any set runs)"""
    dense, ids, lens, bs = q
    eng.stage_batch(0, dense, list(ids), list(lens))
    return eng.forward(0, bs)


def check_sets(eng, sets, refs, slot, tag):
    for name, qs in sets.items():
        eng.run_queues_multi_async(qs, slot=slot)
        out = eng.wait(slot, sum(q[3] for q in qs))
        o = 0
        for i, q in enumerate(qs):
            assert np.array_equal(out[o:o + q[3]], refs[id(q)]), (tag, name, i)
            o += q[3]


def test_launch_sets_at_the_edges_of_the_copy_plan():
    """T = 3, 64 samples of up to 4 lookups: 2 full uniform queries, 2 full ragged ones, 3 uniform queries of one sample,
    3 of the smallest ragged queries there are, and a full ragged query beside a one-sample uniform one -- with the kernels
    taking the fixed length ("sls_uniform" 1) and reading the prefix sums (0); then a bad set and a good one on its slot.

    Two things about these cases, found while writing them.  A ragged query of ONE sample does not exist in the 2-D form:
    every table has n_idx_per_table indices, so the one bag of every table has that length; the smallest ragged query has
    two samples (lengths 1, 3 in one table and 3, 1 in the next), and that is what the fourth set holds.  And with three
    tables no set reaches the prefix-per-block copies: a used prefix always holds two whole index rows, more than half a
    block.  The test below, with one table, does."""
    T, D, rows, m_den, B, L = 3, 16, 1000, 4, 64, 4
    eng, rng = make_engine(T, D, rows, m_den, B, L, 5)
    try:
        base = rng.randint(0, L + 1, size=B)
        full_u = [make_query(rng, T, rows, m_den, np.full((T, B), L)) for _ in range(2)]
        full_r = [make_query(rng, T, rows, m_den, np.stack([rng.permutation(base) for _ in range(T)])) for _ in range(2)]
        one_u = [make_query(rng, T, rows, m_den, np.full((T, 1), 1 + k)) for k in range(3)]
        two_r = [make_query(rng, T, rows, m_den, [[1, 3], [3, 1], [2, 2]][k:] + [[1, 3], [3, 1], [2, 2]][:k]) for k in range(3)]
        assert all(not (q[2] == q[2][0, 0]).all() for q in full_r + two_r)
        sets = {"2 full uniform": full_u, "2 full ragged": full_r, "3 x 1 uniform": one_u, "3 x 2 ragged": two_r,
                "full ragged + 1 uniform": [full_r[0], one_u[1]]}
        refs = {id(q): staged(eng, q) for qs in sets.values() for q in qs}
        for uniform in UNIFORM:
            set_uniform(eng, uniform)
            check_sets(eng, sets, refs, 1, "sls_uniform %d" % uniform)
        set_uniform(eng, 1)
        bad = full_u[1][1].copy()
        bad[2, 77] = rows
        with pytest.raises(N.DrsError) as ei:
            eng.run_queues_multi_async([full_r[0], (full_u[1][0], bad, full_u[1][2], B), one_u[0]], slot=1)
        assert ei.value.code == N.ERR_INDEX_RANGE and "query 1: table 2" in ei.value.detail and "position 77" in ei.value.detail
        check_sets(eng, {"after the bad set": [full_r[1], one_u[2]]}, refs, 1, "same slot")
    finally:
        eng.close()


def test_launch_sets_copied_a_prefix_per_block():
    """one table, 4 dense columns: a block is 2 308 bytes (2 560 from block to block) and a query of a few indices uses
    little over 1 KB of it, so sets of such queries are copied block by block -- the prefix alone for fixed-length bags,
    the prefix and the prefix sums for ragged bags and under "sls_uniform" 0; a full query beside them tips the set back
    to one copy"""
    T, D, rows, m_den, B, L = 1, 16, 1000, 4, 64, 4
    eng, rng = make_engine(T, D, rows, m_den, B, L, 6)
    try:
        one_u = [make_query(rng, T, rows, m_den, [[1 + k]]) for k in range(3)]
        two_r = [make_query(rng, T, rows, m_den, [[1 + k, 3 - k]]) for k in (0, 2, 0)]
        full_u = make_query(rng, T, rows, m_den, np.full((T, B), L))
        sets = {"3 x 1 uniform": one_u, "3 x 2 ragged": two_r, "ragged + uniform": [two_r[0], one_u[0], two_r[1]],
                "1 alone": one_u[:1], "small + full": [one_u[2], full_u]}
        refs = {id(q): staged(eng, q) for qs in sets.values() for q in qs}
        for uniform in UNIFORM:
            set_uniform(eng, uniform)
            check_sets(eng, sets, refs, 0, "sls_uniform %d" % uniform)
    finally:
        eng.close()


def test_one_query_on_both_sides_of_the_size_it_is_copied_from():
    """"zero_copy_inputs" 3 reads a query in place below 128 KB of inputs and copies it from there on: at 4 * (16 + 8 * 80)
    bytes per sample that is between 49 and 50 samples; both sides, fixed-length and ragged bags, and the two forms by name"""
    T, D, rows, m_den, B, L = 8, 64, 10_000, 16, 256, 80
    eng, rng = make_engine(T, D, rows, m_den, B, L, 7)
    try:
        per_row = 4 * (m_den + T * L)
        assert 49 * per_row < 128 * 1024 <= 50 * per_row
        def ragged(bs):                    # four bags 20 short, in another place in every table
            base = np.full(bs, L)
            base[:4] -= 20
            return np.stack([rng.permutation(base) for _ in range(T)])
        for bs, lens, above in ((49, np.full((T, 49), L), False), (50, np.full((T, 50), L), True), (50, ragged(50), False), (52, ragged(52), True)):
            q = make_query(rng, T, rows, m_den, lens)
            assert (4 * (bs * m_den + T * q[1].shape[1]) >= 128 * 1024) == above
            ref = staged(eng, q)
            for mode in (3, 1, 2):
                eng.set_option("zero_copy_inputs", mode)
                for uniform in UNIFORM:
                    set_uniform(eng, uniform)
                    assert np.array_equal(eng.forward_inputs(q[0], q[1], q[2], bs, slot=1), ref), (bs, mode, uniform)
            set_uniform(eng, 1)
    finally:
        eng.close()
