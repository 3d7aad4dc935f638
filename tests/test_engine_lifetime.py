"""What an engine takes it gives back (-m gpu): the read-only option "live_device_objects" counts the GPU resources alive in
the process -- every owning handle of csrc/hip_owned.h and every table arena -- so an engine that stays open can state that
another one, created, used along every path that allocates on first use, and closed, left nothing behind.  Device-wide free
memory is not looked at: other processes on the device move it."""
import gc

import numpy as np
import pytest

from deeprecsys_amd import _native as N
from tests import helpers as H

pytestmark = pytest.mark.gpu

CASES = ["dlrm_rm1_mini", "wnd_mini", "mtwnd_mini", "ncf_mini", "din_mini", "dien_mini"]
SUM_ONLY = ("din", "dien")            # no per-sample weights, no stored type but fp32


@pytest.fixture(scope="module")
def watcher():
    """engine A: stays open only to read the count"""
    e = N.Engine(N.MODEL_DLRM, [16, 16], 8, [4, 8], [24, 4, 1], N.INTERACT_CAT, sigmoid_top=2,
                 max_batch=4, max_lookups=2, num_staged_batches=1, num_slots=1)
    yield e
    e.close()


def live(watcher):
    gc.collect()                      # (an engine some earlier test dropped without closing goes now, not between two readings)
    return watcher.get_option("live_device_objects")


def exercise(args, net, lX, lS_l, lS_i, golden):
    """one staged forward, then every first-use allocation the model allows; the forward's output before and after"""
    import torch
    e = net.engine
    kind = args.model_type
    dev = "cuda:%d" % e.device
    dense = None if kind in H.NO_DENSE else lX
    atol = 1e-5 if kind == "dien" else 0.0
    net.stage_batches(dense, lS_l, lS_i)
    n, L, last = len(lS_l[0][0]), int(args.num_indices_per_lookup), len(lS_l) - 1
    assert H.close(net.run_staged(0, n), golden, rtol=H.RTOL_OUT, atol=atol)

    def arrays(bid, bs):
        ids = np.ascontiguousarray(np.stack([np.asarray(i, dtype=np.int64) for i in lS_i[bid]])[:, :bs * L])
        lens = np.ascontiguousarray(np.stack([np.asarray(l, dtype=np.int32) for l in lS_l[bid]])[:, :bs])
        fc = None if dense is None else np.ascontiguousarray(np.asarray(lX[bid], dtype=np.float32)[:bs])
        return ids, lens, fc
    sizes = [(0, n), (last, max(1, n // 2))]
    # a host launch set of two queries: the slot's pinned and HBM blocks, the copy stream
    staged = net.run_staged_multi([b for b, _ in sizes], [s for _, s in sizes], slot=1)
    host = net.run_queued_multi([arrays(b, s) + (s,) for b, s in sizes], slot=1)
    assert all(np.array_equal(a, b) for a, b in zip(host, staged))
    # a device launch set, per-sample weights (all 1) on its first query: the other slot's HBM blocks and weight blocks
    reqs = []
    for k, (b, s) in enumerate(sizes):
        ids, lens, fc = arrays(b, s)
        w = torch.ones((e.T, s * L), dtype=torch.float32, device=dev) if k == 0 and kind not in SUM_ONLY else None
        reqs.append((torch.as_tensor(ids, device=dev), torch.as_tensor(lens, device=dev), None if fc is None else torch.as_tensor(fc, device=dev),
                     s, -1, w))
    got = net.run_queued_device_multi(reqs, slot=0)
    assert all(H.close(a, b, rtol=H.RTOL_OUT, atol=atol) for a, b in zip(got, staged))
    if kind not in SUM_ONLY:
        # staged batches with weights: each batch's weight array; staged again without, the batches are as they were
        ones = [[np.ones(len(i), dtype=np.float32) for i in per] for per in lS_i]
        net.stage_batches(dense, lS_l, lS_i, lS_w=ones)
        assert e.get_option("sls_weighted") == len(lS_l)
        net.stage_batches(dense, lS_l, lS_i)
    # one more copy of the tables, then only the one in use
    e.set_option("table_placement", -1)
    assert e.get_option("table_placements") == 2
    e.set_option("table_placement", -2)
    assert e.get_option("table_placements") == 1
    # rows on the device route, ids and strided values in device memory: read, and written back as read
    t = e.T - 2
    ids_t = torch.as_tensor(np.asarray(lS_i[0][t][:3], dtype=np.int64) if len(set(lS_i[0][t][:3])) == 3 else np.arange(3, dtype=np.int64), device=dev)

    def rows_round_trip():
        wide = torch.zeros((3, e.D + 5), dtype=torch.float32, device=dev)
        block = wide[:, 2:2 + e.D]
        assert net.embedding_rows(t, ids_t, out=block) is block
        net.update_embedding_rows(t, ids_t, block)
        assert torch.equal(net.embedding_rows(t, ids_t), block) and float(wide[:, :2].abs().max()) == 0.0
    if kind not in SUM_ONLY:
        # fp16 tables and back: a new arena each way; in between, the row calls take their packed and side buffers
        e.set_option("table_dtype", 1)
        rows_round_trip()
        e.set_option("table_dtype", 0)
        assert all(W is not None for W in net.emb_w)
        for k, W in enumerate(net.emb_w):          # (the round trip rounded the rows to fp16: the fixture's tables again)
            e.set_table(k, W)
    rows_round_trip()
    if kind == "dlrm":
        # the bf16 twins of the layers of at least 64 x 64 (dlrm_rm1_mini's 68 x 256 and 256 x 64 top layers), and away again
        assert any(a >= 64 and b >= 64 for a, b in zip(net.ln_top[:-1], net.ln_top[1:]))
        e.set_option("mlp_dtype", 2)
        net.run_staged(0, n)
        e.set_option("mlp_dtype", 0)
    assert H.close(net.run_staged(0, n), golden, rtol=H.RTOL_OUT, atol=atol)


@pytest.mark.parametrize("case", CASES)
def test_a_closed_engine_leaves_nothing_behind(watcher, case):
    meta, z = H.load_fixture(case)
    args = H.args_from(meta["args"], accel_slots=2)
    golden = H.golden_output(meta, z)
    c0 = live(watcher)
    for cycle in range(3):
        net, lX, lS_l, lS_i, lT = H.materialize(args)
        net.create(lX[0], lS_l[0], lS_i[0], lT[0])
        try:
            assert net.engine.num_slots == 2 and live(watcher) > c0
            exercise(args, net, lX, lS_l, lS_i, golden)
        finally:
            net.engine.close()
        assert live(watcher) == c0, (case, cycle)


def test_a_create_that_fails_at_its_last_allocation_leaves_nothing_behind(watcher):
    """24 tables of 2^26 rows at D 64 stay inside the per-table limit (rows * D < 2^33) and need 384 GiB, more than the
    device has in all: the slots, batches, streams and events are built, then the one arena allocation is refused -- the
    request is larger than the whole device, so no memory is taken from anyone"""
    c0 = live(watcher)
    T, D = 24, 64
    with pytest.raises(N.DrsError) as err:
        N.Engine(N.MODEL_DLRM, [1 << 26] * T, D, [4, D], [(T + 1) * D, 4, 1], N.INTERACT_CAT, sigmoid_top=2,
                 max_batch=4, max_lookups=2, num_staged_batches=2, num_slots=2)
    assert err.value.code == N.ERR_OOM, str(err.value)
    assert "arena_alloc" in str(err.value)          # it was the arena, the last step, that was refused
    assert live(watcher) == c0
