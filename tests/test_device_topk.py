"""Each query's top-k rows from the GPU (include/drs_device_topk.h, deeprecsys_amd/csrc/topk_pass.hip).  The reference is
numpy: the 64-bit keys of deeprecsys_amd/csrc/topk_plan.h restated here, sorted descending, the first k taken.  The rule makes
the result unique, so everything is compared bit for bit; on inputs without ties or NaN torch.topk on the CPU is a second
opinion.  The set call is compared on the scores the SAME requests leave through run_queues_device_io_multi_async, which
are the bits drs_wait hands out.  Nothing here can fault the card: every index is valid or is clamped by the input pass, and
the pointer check is shown with pinned memory, which the GPU could write."""
import numpy as np
import pytest

from deeprecsys_amd import _native as N
from tests import device_inputs_ref as R
from tests import helpers as H
from tests import test_device_inputs as DI
from tests import test_device_outputs as DO

pytestmark = pytest.mark.gpu

NAN_BITS = 0x7FC00000
IDX_GUARD, TOP_GUARD = -77, -77.25
GUARD = 8                                   # elements of sentinel in front of and behind each output
torch_cuda, bits, sleep_cycles = DO.torch_cuda, DO.bits, DO.sleep_cycles


# ------------------------------------------------------------------------------------------------
# the reference
def topk_keys(col_bits):
    """topk_plan.h's key of every row, restated: col_bits uint32 [rows] -> uint64 [rows]"""
    b = np.asarray(col_bits, dtype=np.uint32)
    nan = (b & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)
    word = np.where(nan, np.uint32(0xFFFFFFFF), np.where(b >> np.uint32(31) != 0, ~b, b | np.uint32(0x80000000))).astype(np.uint64)
    return (word << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - np.arange(b.size, dtype=np.uint64))


def topk_ref(score_bits, col, k):
    """score_bits uint32 [rows, n_out] -> (int32 [k] row numbers, uint32 [k, n_out] rows): the k largest keys, descending"""
    keys = topk_keys(score_bits[:, col])
    assert np.unique(keys).size == keys.size and keys.min() > 0
    order = np.argsort(keys, kind="stable")[::-1][:k]
    return order.astype(np.int32), score_bits[order]


def test_the_restated_keys_rank_as_the_header_says():
    f = lambda x: np.array([x], np.float32).view(np.uint32)[0]
    chain = [0xFFC00001, f(np.inf), f(3.0e38), f(1.0), 0x00000001, f(0.0), 0x80000000, 0x80000001, f(-1.0), f(-np.inf)]
    k = topk_keys(np.array(chain, np.uint32)) >> np.uint64(32)
    assert all(int(a) > int(b) for a, b in zip(k[:-1], k[1:])), k
    assert int(k[0]) == 0xFFFFFFFF and int(k[-1]) == 0x007FFFFF and int(k[5]) == 0x80000000 and int(k[6]) == 0x7FFFFFFF
    idx, _ = topk_ref(np.array([[f(2.0)], [0x7FC00000], [f(2.0)], [0xFFC12345]], np.uint32), 0, 4)
    assert idx.tolist() == [1, 3, 0, 2]               # NaN first (either sign), then equal scores by the lower row


# ------------------------------------------------------------------------------------------------
# outputs inside guard regions
class Top(object):
    """the two outputs of one query, each inside a buffer full of a sentinel: idx int32 [k], scores float32 [k, n_out]"""

    def __init__(self, k, n_out):
        torch = torch_cuda()
        self.k, self.n_out = k, n_out
        self.ibuf = torch.full((k + 2 * GUARD,), IDX_GUARD, dtype=torch.int32, device="cuda:0")
        self.sbuf = torch.full((k * n_out + 2 * GUARD,), TOP_GUARD, dtype=torch.float32, device="cuda:0")
        self.idx = self.ibuf[GUARD:GUARD + k]
        self.scores = self.sbuf[GUARD:GUARD + k * n_out].view(k, n_out)
        self.arg = (self.ibuf.data_ptr() + 4 * GUARD, self.sbuf.data_ptr() + 4 * GUARD)

    def read(self):
        return self.idx.cpu().numpy().copy(), bits(self.scores).reshape(self.k, self.n_out)

    def guards_untouched(self):
        i, s = self.ibuf.cpu().numpy(), bits(self.sbuf)
        want = np.float32(TOP_GUARD).view(np.uint32)
        return bool((i[:GUARD] == IDX_GUARD).all() and (i[GUARD + self.k:] == IDX_GUARD).all() and
                    (s[:GUARD] == want).all() and (s[GUARD + self.k * self.n_out:] == want).all())

    def untouched(self):
        return bool((self.ibuf.cpu().numpy() == IDX_GUARD).all() and (bits(self.sbuf) == np.float32(TOP_GUARD).view(np.uint32)).all())


# ------------------------------------------------------------------------------------------------
# the engine of the set tests: DLRM cat, T 2, D 16, a few hundred rows, max_lookups 2, max_batch 1088
ROWS, D, M_DEN, L = [300, 500], 16, 8, 2
LN_BOT, LN_TOP = [M_DEN, D], [D + len(ROWS) * D, 4, 1]
MAX_BATCH = 1088


@pytest.fixture(scope="module")
def eng():
    rng = np.random.RandomState(5)
    e = N.Engine(N.MODEL_DLRM, ROWS, D, LN_BOT, LN_TOP, N.INTERACT_CAT, sigmoid_top=2, max_batch=MAX_BATCH, max_lookups=L,
                 num_staged_batches=1, num_slots=2)
    e.set_option("dispatch_log", 1)
    for t, r in enumerate(ROWS):
        e.set_table(t, rng.uniform(-1, 1, (r, D)).astype(np.float32))
    for which, ln in ((N.MLP_BOT, LN_BOT), (N.MLP_TOP, LN_TOP)):
        for l in range(len(ln) - 1):
            e.set_fc(which, l, rng.normal(0, 1.0 / np.sqrt(ln[l]), (ln[l + 1], ln[l])).astype(np.float32),
                     rng.normal(0, 0.1, ln[l + 1]).astype(np.float32))
    yield e
    e.close()


def query(seed, bs, pairs=False):
    """a valid query of the engine above, every bag L long and promised; pairs: samples 2 j and 2 j + 1 are exact duplicates"""
    rng = np.random.RandomState(seed)
    ids = np.stack([rng.randint(0, r, size=(bs, L)).astype(np.int64) for r in ROWS])
    dense = rng.uniform(-1, 1, (bs, M_DEN)).astype(np.float32)
    if pairs:
        assert bs % 2 == 0
        ids[:, 1::2], dense[1::2] = ids[:, 0::2], dense[0::2]
    return R.Q(bs, np.ascontiguousarray(ids.reshape(len(ROWS), bs * L)), np.full((len(ROWS), bs), L, np.int32), dense, L)


# ------------------------------------------------------------------------------------------------
# 1. the kernel on chosen bits: Engine.topk_rows
SPECIAL = [0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF,      # +-0, +-inf, denormals
           0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001, 0x7FFFFFFF, 0xFFFFFFFF, 0x7FC12345, 0xFFA54321,      # NaNs of both signs, payloads
           0x3F800000, 0xBF800000, 0x7F7FFFFF, 0xFF7FFFFF]


def column(kind, rows, rng):
    """the ranking column's bits"""
    if kind == "runs":              # long runs of equal scores: the lower row wins
        vals = np.array([0.5, -1.0, 2.0, 0.5, 0.0], np.float32)
        return np.repeat(vals, rows // 5 + 1)[:rows].view(np.uint32).copy()
    if kind == "special":
        c = np.array(SPECIAL, np.uint32)[rng.randint(0, len(SPECIAL), rows)]
        some = rng.uniform(size=rows) < 0.3
        return np.where(some, rng.normal(size=rows).astype(np.float32).view(np.uint32), c).astype(np.uint32)
    if kind == "equal":
        return np.full(rows, 0x3F000000, np.uint32)
    assert kind == "distinct"       # no ties, no NaN: torch.topk agrees
    return ((rng.permutation(rows).astype(np.float32) - np.float32(rows // 2)) * np.float32(0.37)).view(np.uint32)


def run_rows(eng, table, col, k, stream=None):
    """table uint32 [rows, stride]; the first n_out columns are the rows' scores -> (idx, score bits, the Top)"""
    torch = torch_cuda()
    rows, stride, n_out = table[0].shape[0], table[0].shape[1], table[1]
    src = torch.from_numpy(table[0].view(np.float32)).to("cuda:0")
    top = Top(k, n_out)
    torch.cuda.synchronize()
    eng.topk_rows(src.data_ptr(), rows, n_out, stride, col, k, top.arg[0], top.arg[1], stream=stream)
    torch.cuda.synchronize()
    return top.read() + (top,)


@pytest.mark.parametrize("rows", [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049])
def test_topk_rows_equals_the_sorted_keys_bit_for_bit(eng, rows):
    torch = torch_cuda()
    rng = np.random.RandomState(rows)
    for n_out, extra in ((1, 0), (3, 0), (3, 2), (1, 3)):
        for kind in ("runs", "special", "equal", "distinct"):
            table = rng.randint(0, 2 ** 32, size=(rows, n_out + extra), dtype=np.uint64).astype(np.uint32)    # the other columns: any bits
            for col in sorted({0, n_out - 1}):
                table[:, col] = column(kind, rows, rng)
                for k in sorted({1, min(10, rows), min(rows, 1024)}):
                    idx, sc, top = run_rows(eng, (table, n_out), col, k)
                    want_idx, want_sc = topk_ref(table[:, :n_out], col, k)
                    what = (rows, n_out, extra, kind, col, k)
                    assert np.array_equal(idx, want_idx), what
                    assert np.array_equal(sc, want_sc), what
                    assert top.guards_untouched(), what
                    if kind == "distinct":
                        v, i = torch.topk(torch.from_numpy(table[:, col].copy().view(np.float32)), k)
                        assert np.array_equal(i.numpy().astype(np.int32), idx) and np.array_equal(bits(v), sc[:, col]), what
                    if kind == "equal":
                        assert idx.tolist() == list(range(k)), what


def test_topk_rows_is_enqueued_on_the_callers_stream(eng):
    torch = torch_cuda()
    rng = np.random.RandomState(3)
    a, b = column("distinct", 300, rng), column("special", 300, rng)
    src = torch.from_numpy(a.view(np.float32).reshape(300, 1)).to("cuda:0")
    later = torch.from_numpy(b.view(np.float32).reshape(300, 1)).to("cuda:0")
    top = Top(10, 1)
    S = torch.cuda.Stream()
    cycles = sleep_cycles(torch, 100.0)
    torch.cuda.synchronize()
    with torch.cuda.stream(S):
        torch.cuda._sleep(cycles)
        src.copy_(later, non_blocking=True)                      # the pass must see b: it runs behind the copy
        eng.topk_rows(src.data_ptr(), 300, 1, 1, 0, 10, top.arg[0], top.arg[1], stream=S.cuda_stream)
        got = top.idx.clone()
        still_running = not S.query()
    assert still_running, "the call waited on the host for the stream"
    S.synchronize()
    want_idx, want_sc = topk_ref(b.reshape(300, 1), 0, 10)
    assert np.array_equal(got.cpu().numpy(), want_idx) and np.array_equal(top.read()[1], want_sc) and top.guards_untouched()


def test_topk_rows_refuses_bad_arguments_and_writes_nothing(eng):
    torch = torch_cuda()
    rows, n_out, stride = 2049, 3, 5
    src = torch.zeros((rows, stride), device="cuda:0")
    top = Top(10, n_out)
    pin_f = torch.full((rows * stride,), TOP_GUARD).pin_memory()          # PINNED host memory: the GPU could write it
    pin_i = torch.full((16,), IDX_GUARD, dtype=torch.int32).pin_memory()
    good = dict(scores_ptr=src.data_ptr(), rows=rows, n_out=n_out, row_stride=stride, col=1, k=10, idx_ptr=top.arg[0], top_ptr=top.arg[1])
    cases = {"k_0": dict(k=0), "k_minus_1": dict(k=-1), "k_1025": dict(k=1025), "k_above_rows": dict(rows=5, k=6),
             "col_minus_1": dict(col=-1), "col_n_out": dict(col=n_out), "stride_below_n_out": dict(row_stride=n_out - 1),
             "stride_negative": dict(row_stride=-stride), "stride_2p62": dict(row_stride=2 ** 62), "rows_0": dict(rows=0, k=1),
             "rows_2p31": dict(rows=2 ** 31), "n_out_0": dict(n_out=0, col=0),
             "null_scores": dict(scores_ptr=0), "null_idx": dict(idx_ptr=0), "null_top": dict(top_ptr=0),
             "scores_plus_2": dict(scores_ptr=src.data_ptr() + 2), "idx_plus_2": dict(idx_ptr=top.arg[0] + 2),
             "top_plus_2": dict(top_ptr=top.arg[1] + 2),
             "pinned_scores": dict(scores_ptr=pin_f.data_ptr()), "pinned_idx": dict(idx_ptr=pin_i.data_ptr()),
             "pinned_top": dict(top_ptr=pin_f.data_ptr()),
             "idx_is_top": dict(idx_ptr=top.arg[1])}
    for name, change in cases.items():
        with pytest.raises(N.DrsError) as err:
            eng.topk_rows(**dict(good, **change))
        assert err.value.code == N.ERR_BAD_ARG, (name, str(err.value))
    torch.cuda.synchronize()
    assert top.untouched() and (pin_i.numpy() == IDX_GUARD).all() and (bits(pin_f) == np.float32(TOP_GUARD).view(np.uint32)).all()
    eng.topk_rows(**good)                                                  # the arguments the cases started from are served
    eng.topk_rows(**dict(good, rows=1, row_stride=-3, k=1))                # one row: the stride is not read
    torch.cuda.synchronize()
    assert top.guards_untouched() and top.read()[0].tolist() == [0] + list(range(1, 10))


# ------------------------------------------------------------------------------------------------
# 2. the set call against the scores the same requests leave through run_queues_device_io_multi_async
def call_topk(eng, tups, ks, col, tops, stream=None, slot=0, ordered=None, weights=None, null_k=False, null_tables=False):
    """drs_run_queues_device_topk_multi_async as the binding calls it, with every argument open to a refusal case"""
    C = N.C
    args, keep = eng._device_set(tups)
    n = len(tups)
    ka = np.zeros(max(n, 1), np.int32)
    ka[:len(ks)] = ks
    ip, sp = (C.c_void_p * max(n, 1))(), (C.c_void_p * max(n, 1))()
    for i, (a, b) in enumerate(tops):
        ip[i], sp[i] = a or None, b or None
    wargs, wkeep = ([None, None, None], None) if weights is None else eng._device_weights(n, weights)
    if ordered is None:
        ordered = 0 if stream is None else 1
    none_table = C.POINTER(C.c_void_p)()
    eng._check(N.lib().drs_run_queues_device_topk_multi_async(
        eng._h, slot, *(args + wargs + [None if null_k else ka.ctypes.data_as(N._i32p), col, none_table if null_tables else ip,
                                        none_table if null_tables else sp, stream or None, ordered])),
        "drs_run_queues_device_topk_multi_async")
    del keep, wkeep


def io_bits(eng, ups, qs, slot=0, weights=None):
    """the scores of the set through run_queues_device_io_multi_async -> (uint32 [bs, n_out] per query, dispatch tokens)"""
    torch = torch_cuda()
    outs = [torch.full((max(q.bs, 1), eng.n_out), TOP_GUARD, device="cuda:0") for q in qs]
    torch.cuda.synchronize()
    eng.run_queues_device_io_multi_async([u[1] for u in ups], [(o.data_ptr() if q.bs else 0, eng.n_out) for o, q in zip(outs, qs)],
                                         slot=slot, weights=weights)
    host = eng.wait(slot, sum(q.bs for q in qs))
    log = eng.last_dispatch(slot)
    got = [bits(o[:q.bs]).reshape(q.bs, eng.n_out) for o, q in zip(outs, qs)]
    assert np.array_equal(np.concatenate(got).reshape(-1), host.view(np.uint32).reshape(-1))       # the bits drs_wait hands out
    return got, log


def check_set(eng, qs, ks, col=0, slot=0, weights=None, upload_weights=None):
    torch = torch_cuda()
    ups = [DI.upload(q) for q in qs]
    want_scores, io_log = io_bits(eng, ups, qs, slot, weights)
    tops = [Top(k, eng.n_out) for k in ks]
    torch.cuda.synchronize()
    eng.run_queues_device_topk_multi_async([u[1] for u in ups], ks, col, [t.arg if k else (0, 0) for t, k in zip(tops, ks)], slot=slot,
                                           weights=weights)
    host = eng.wait(slot, sum(q.bs for q in qs))
    log = eng.last_dispatch(slot)
    assert np.array_equal(host.view(np.uint32).reshape(-1), np.concatenate(want_scores).reshape(-1))  # the host still receives every score
    for i, (q, k, t) in enumerate(zip(qs, ks, tops)):
        idx, sc = t.read()
        assert t.guards_untouched(), i
        if k == 0:
            assert t.untouched(), i
            continue
        want_idx, want_sc = topk_ref(want_scores[i], col, k)
        assert np.array_equal(idx, want_idx), (i, q.bs, k)
        assert np.array_equal(sc, want_sc), (i, q.bs, k)
    n_pass = sum(1 for q, k in zip(qs, ks) if q.bs and k)
    assert not any(t.startswith("topk_pass") for t in io_log)
    if n_pass:
        assert log[-1] == "topk_pass[%d x 256]" % n_pass and log[:-1] == io_log[:-1] and io_log[-1].startswith("output_pass["), (log, io_log)
    else:
        assert not any(t.startswith("topk_pass") for t in log)
    # a following device-output set on the same slot: the bits it had before, no token of the pass
    again, again_log = io_bits(eng, ups, qs, slot, weights)
    assert DI.same_bits(again, want_scores) and again_log == io_log
    return want_scores, tops


def test_a_set_of_mixed_sizes_an_empty_query_and_a_k_of_zero(eng):
    qs = [query(10, 0), query(11, 65), query(12, 1), query(13, 1025), query(14, 256), query(15, 300)]
    check_set(eng, qs, [0, 10, 1, 1024, 0, 300])
    check_set(eng, qs, [0, 65, 1, 1, 256, 10], slot=1)
    check_set(eng, qs, [0, 0, 0, 0, 0, 0])                      # nothing asked for: no pass, nothing written


def test_a_set_of_16_queries(eng):
    sizes = (1, 63, 64, 65, 255, 256, 257, 300)
    qs = [query(20 + i, sizes[i % 8]) for i in range(16)]
    check_set(eng, qs, [min(10, q.bs) for q in qs])
    check_set(eng, qs, [q.bs if i % 2 else 1 for i, q in enumerate(qs)], slot=1)


def test_duplicate_samples_rank_by_their_row(eng):
    q = query(30, 128, pairs=True)
    scores, tops = check_set(eng, [q], [64])
    assert np.array_equal(scores[0][0::2], scores[0][1::2]), "the duplicates must score alike for the test to show anything"
    idx = tops[0].read()[0]
    assert (idx[0::2] % 2 == 0).all() and np.array_equal(idx[1::2], idx[0::2] + 1)      # each pair together, the lower row first


def test_weighted_and_unweighted_queries_in_one_set(eng):
    torch = torch_cuda()
    qs = [query(40, 65), query(41, 256), query(42, 64)]
    rng = np.random.RandomState(43)
    w = [torch.from_numpy(rng.uniform(0, 1, q.ids.shape).astype(np.float32)).to("cuda:0") for q in qs]
    plain, _ = check_set(eng, qs, [10, 10, 10])
    mixed = [(w[0].data_ptr(), w[0].stride(0), N.WEIGHT_FP32), None, (w[2].data_ptr(), w[2].stride(0), N.WEIGHT_FP32)]
    weighted, _ = check_set(eng, qs, [10, 256, 1], weights=mixed)
    assert not np.array_equal(weighted[0], plain[0]) and not np.array_equal(weighted[2], plain[2]), "the weights must change the scores"
    check_set(eng, qs[:1], [65], weights=mixed[:1])               # a weighted request alone
    check_set(eng, qs, [10, 10, 10], weights=[None, None, None])  # a weight table of NULL entries: the unweighted set


@pytest.mark.parametrize("case", ["din_mini", "dien_mini", "mtwnd_mini"])
def test_one_fixture_model_of_the_other_kinds(case):
    meta, z = H.load_fixture(case)
    args = H.args_from(meta["args"], accel_slots=2)
    net, lX, lS_l, lS_i, lT = H.materialize(args)
    net.create(lX[0], lS_l[0], lS_i[0], lT[0])
    e = net.engine
    try:
        e.set_option("dispatch_log", 1)
        assert e.n_out > 1 or case != "mtwnd_mini"
        qs = DI.model_queries(e, lX, lS_l, lS_i, int(args.num_indices_per_lookup), promise=True)
        check_set(e, qs, [min(5, q.bs) for q in qs], col=e.n_out - 1, slot=1)
        check_set(e, qs, [q.bs for q in qs], col=0, slot=1)
    finally:
        e.close()


# ------------------------------------------------------------------------------------------------
# 3. ordering on the caller's stream
def test_ordered_1_runs_behind_the_callers_stream_and_the_consumer_behind_the_set(eng):
    torch = torch_cuda()
    A, B = query(50, 257), query(51, 257)
    upa, upb = [DI.upload(A)], [DI.upload(B)]
    (wa,), _ = io_bits(eng, upa, [A])
    (wb,), _ = io_bits(eng, upb, [B])
    assert not np.array_equal(topk_ref(wa, 0, 10)[0], topk_ref(wb, 0, 10)[0]), "A and B must differ for the test to show anything"
    (ids, lens, dense), tup = upa[0]
    b_ids, b_dense = upb[0][0][0], upb[0][0][2]
    top = Top(10, eng.n_out)
    cycles = sleep_cycles(torch, 150.0)
    S = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(S):
        torch.cuda._sleep(cycles)
        ids.copy_(b_ids, non_blocking=True)
        dense.copy_(b_dense, non_blocking=True)
        eng.run_queues_device_topk_multi_async([tup], [10], 0, [top.arg], stream=S.cuda_stream, slot=0)
        got_idx, got_sc = top.idx.clone(), top.scores.clone()          # the consumer: enqueued behind the call, no host wait
        still_running = not S.query()
    assert still_running, "the call (or the clones behind it) waited on the host for the stream"
    S.synchronize()
    want_idx, want_sc = topk_ref(wb, 0, 10)
    assert np.array_equal(got_idx.cpu().numpy(), want_idx), "the rows cloned on the stream are not B's"
    assert np.array_equal(bits(got_sc).reshape(10, -1), want_sc)
    assert eng.wait(0) is None and top.guards_untouched()
    # ordered 0: complete inputs, drs_wait is the completion (ids and dense hold B now)
    top0 = Top(10, eng.n_out)
    torch.cuda.synchronize()
    eng.run_queues_device_topk_multi_async([tup], [10], 0, [top0.arg], stream=None, slot=0)
    assert eng.wait(0) is None
    assert np.array_equal(top0.read()[0], want_idx) and np.array_equal(top0.read()[1], want_sc) and top0.guards_untouched()
    del lens


# ------------------------------------------------------------------------------------------------
# 4. a set that fails on the device
def test_a_set_with_an_index_out_of_range_is_minus_one_and_nan_everywhere(eng):
    torch = torch_cuda()
    good, bad = query(60, 65), query(61, 256)
    ids = bad.ids.copy()
    ids[1, 100] = ROWS[1]                                    # one past the table: the input pass clamps it and sets the error word
    qs = [good, bad._replace(ids=ids)]
    ups = [DI.upload(q) for q in qs]
    tops = [Top(10, eng.n_out), Top(256, eng.n_out)]
    torch.cuda.synchronize()
    eng.run_queues_device_topk_multi_async([u[1] for u in ups], [10, 256], 0, [t.arg for t in tops], slot=0)      # returns DRS_OK
    with pytest.raises(N.DrsError) as err:
        eng.wait(0)
    assert err.value.code == N.ERR_INDEX_RANGE, str(err.value)
    for t in tops:                                           # the good query of the set too
        idx, sc = t.read()
        assert (idx == -1).all() and (sc == NAN_BITS).all() and t.guards_untouched()
    check_set(eng, [good, bad], [10, 256])                   # the slot serves the next set


# ------------------------------------------------------------------------------------------------
# 5. refused before launch
class Refusals(object):
    def __init__(self, eng):
        torch = torch_cuda()
        self.qs = [query(70, 65), query(71, 1025)]
        self.ups = [DI.upload(q) for q in self.qs]
        self.tups = [u[1] for u in self.ups]
        self.ks = [10, 1024]
        self.tops = [Top(10, eng.n_out), Top(1024, eng.n_out)]
        self.args = [t.arg for t in self.tops]
        self.pin_f = torch.full((16,), TOP_GUARD).pin_memory()
        self.pin_i = torch.full((16,), IDX_GUARD, dtype=torch.int32).pin_memory()
        torch.cuda.synchronize()

    def untouched(self):
        return (all(t.untouched() for t in self.tops) and (self.pin_i.numpy() == IDX_GUARD).all() and
                (bits(self.pin_f) == np.float32(TOP_GUARD).view(np.uint32)).all())


@pytest.fixture(scope="module")
def refusals(eng):
    return Refusals(eng)


def _tops(c, q, idx=None, top=None):
    a = list(c.args)
    a[q] = (a[q][0] if idx is None else idx, a[q][1] if top is None else top)
    return a


REFUSALS = [
    ("ordered_2", lambda c: dict(ordered=2)),
    ("ordered_minus_1", lambda c: dict(ordered=-1)),
    ("col_n_out", lambda c: dict(col=1)),
    ("col_minus_1", lambda c: dict(col=-1)),
    ("null_k_table", lambda c: dict(null_k=True)),
    ("k_above_bs", lambda c: dict(ks=[66, 10])),
    ("k_minus_1", lambda c: dict(ks=[-1, 10])),
    ("k_1025_of_1025", lambda c: dict(ks=[10, 1025])),
    ("null_output_tables", lambda c: dict(null_tables=True)),
    ("null_idx", lambda c: dict(tops=_tops(c, 0, idx=0))),
    ("null_scores", lambda c: dict(tops=_tops(c, 1, top=0))),
    ("idx_plus_2_bytes", lambda c: dict(tops=_tops(c, 0, idx=c.args[0][0] + 2))),
    ("scores_plus_2_bytes", lambda c: dict(tops=_tops(c, 1, top=c.args[1][1] + 2))),
    ("pinned_idx", lambda c: dict(tops=_tops(c, 0, idx=c.pin_i.data_ptr()))),
    ("pinned_scores", lambda c: dict(tops=_tops(c, 0, top=c.pin_f.data_ptr()))),
    ("the_same_idx_twice", lambda c: dict(tops=_tops(c, 0, idx=c.args[1][0]))),
    ("the_same_scores_twice", lambda c: dict(tops=_tops(c, 0, top=c.args[1][1]))),
    ("idx_inside_the_other_querys_scores", lambda c: dict(tops=_tops(c, 0, idx=c.args[1][1] + 4 * 1000))),
    ("scores_sharing_one_float", lambda c: dict(tops=_tops(c, 0, top=c.args[1][1] + 4 * 1023))),
    # what the device-input call refuses is refused here as well
    ("slot_2_of_2", lambda c: dict(slot=2)),
    ("n_17", lambda c: dict(tups=[c.tups[0]] * 17, ks=[1] * 17, tops=[c.args[0]] * 17)),
]


@pytest.mark.parametrize("name,make", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_a_synchronous_refusal_leaves_the_slot_free_and_writes_nothing(eng, refusals, name, make):
    torch = torch_cuda()
    c = refusals
    kw = make(c)
    with pytest.raises(N.DrsError) as err:
        call_topk(eng, kw.pop("tups", c.tups), kw.pop("ks", c.ks), kw.pop("col", 0), kw.pop("tops", c.args), slot=kw.pop("slot", 0), **kw)
    assert err.value.code == N.ERR_BAD_ARG, str(err.value)
    assert eng.wait(0) is None                     # nothing in flight on the slot
    torch.cuda.synchronize()
    assert c.untouched()


def test_the_arguments_of_the_refusal_cases_are_served_and_touching_outputs_are_legal(eng, refusals):
    torch = torch_cuda()
    c = refusals
    want, _ = io_bits(eng, c.ups, c.qs)
    call_topk(eng, c.tups, c.ks, 0, c.args)
    assert eng.wait(0) is None
    for t, k, w in zip(c.tops, c.ks, want):
        idx, sc = t.read()
        assert np.array_equal(idx, topk_ref(w, 0, k)[0]) and np.array_equal(sc, topk_ref(w, 0, k)[1]) and t.guards_untouched()
    # k 0 with NULL pointers, even a NULL pair of tables when nothing is asked for
    call_topk(eng, c.tups, [0, 5], 0, [(0, 0), c.args[1]])
    assert eng.wait(0) is None
    call_topk(eng, c.tups, [0, 0], 0, [(0, 0), (0, 0)], null_tables=True)
    assert eng.wait(0) is None
    # touching outputs: idx and scores of both queries back to back in one buffer
    buf = torch.zeros((4 * 10,), dtype=torch.int32, device="cuda:0")
    p = buf.data_ptr()
    call_topk(eng, c.tups, [10, 10], 0, [(p, p + 40), (p + 80, p + 120)])
    assert eng.wait(0) is None
    flat = buf.cpu().numpy()
    for i, w in enumerate(want):
        wi, ws = topk_ref(w, 0, 10)
        assert np.array_equal(flat[20 * i:20 * i + 10], wi) and np.array_equal(flat[20 * i + 10:20 * i + 20].view(np.uint32), ws[:, 0])
    for t in c.tops:
        t.ibuf.fill_(IDX_GUARD)
        t.sbuf.fill_(TOP_GUARD)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------
# 6. the wrapper
def test_the_wrapper_returns_the_best_rows_without_a_host_wait(monkeypatch):
    torch = torch_cuda()
    from deeprecsys_amd import dlrm_s_hip as M
    meta, z = H.load_fixture("dlrm_dot_small")
    args = H.args_from(meta["args"], accel_slots=2)
    np.random.seed(args.numpy_rand_seed)
    net, lX, lS_l, lS_i, lT = H.materialize(args)
    w = M.DLRM_Wrapper(args)
    w.create(lX[0], lS_l[0], lS_i[0], lT[0])
    try:
        Lk = int(args.num_indices_per_lookup)
        n = len(lS_l[0][0])
        dev = "cuda:%d" % w.net.engine.device
        dreqs = []
        for j in range(min(len(lS_l), 3)):
            bs = max(1, n - j)
            ids = np.ascontiguousarray(np.stack([np.asarray(i, dtype=np.int64) for i in lS_i[j]])[:, :bs * Lk])
            lengths = np.ascontiguousarray(np.stack([np.asarray(l, dtype=np.int32) for l in lS_l[j]])[:, :bs])
            fc = np.ascontiguousarray(np.asarray(lX[j], dtype=np.float32)[:bs])
            dreqs.append((torch.as_tensor(ids, device=dev), torch.as_tensor(lengths, device=dev), torch.as_tensor(fc, device=dev), bs))
        full = w.run_queues_device_io_multi(dreqs, slot=1)
        w.finish_device(slot=1)
        want = [bits(t).reshape(t.shape) for t in full]
        k = 4

        def no_sync(*a, **kw):
            raise AssertionError("the wrapper synchronised on the host")
        with monkeypatch.context() as m:
            m.setattr(torch.cuda.Stream, "synchronize", no_sync)
            m.setattr(torch.cuda, "synchronize", no_sync)
            got = w.run_queues_device_topk_multi(dreqs, k, slot=1)
        assert len(got) == len(dreqs)
        for (idx, sc), ws, r in zip(got, want, dreqs):
            ki = min(k, r[3])
            assert idx.dtype == torch.int32 and tuple(idx.shape) == (ki,) and sc.dtype == torch.float32 and tuple(sc.shape) == (ki, ws.shape[1])
            wi, wsc = topk_ref(ws, 0, ki)
            # read on torch's current stream BEFORE the set's completion was asked for: the stream is ordered behind the set
            assert np.array_equal(idx.cpu().numpy(), wi) and np.array_equal(bits(sc).reshape(ki, -1), wsc)
            if np.unique(ws[:, 0]).size == ws.shape[0]:
                v, i = torch.topk(torch.from_numpy(ws[:, 0].copy().view(np.float32)), ki)
                assert np.array_equal(i.numpy().astype(np.int32), wi) and np.array_equal(bits(v), wsc[:, 0])
        assert 1 in w.net._device_refs and len(w.net._device_refs[1][0]) == len(dreqs)
        assert w.finish_device(slot=1) is None and 1 not in w.net._device_refs
        # into tensors of the caller's
        mine = [(torch.full((min(k, r[3]),), IDX_GUARD, dtype=torch.int32, device=dev),
                 torch.full((min(k, r[3]), want[0].shape[1]), TOP_GUARD, device=dev)) for r in dreqs]
        back = w.run_queues_device_topk_multi(dreqs, k, out=mine, slot=1)
        assert all(b[0].data_ptr() == m_[0].data_ptr() and b[1].data_ptr() == m_[1].data_ptr() for b, m_ in zip(back, mine))
        w.finish_device(slot=1)
        for (idx, sc), ws, r in zip(mine, want, dreqs):
            wi, wsc = topk_ref(ws, 0, min(k, r[3]))
            assert np.array_equal(idx.cpu().numpy(), wi) and np.array_equal(bits(sc).reshape(wsc.shape), wsc)
        with pytest.raises(ValueError) as err:
            w.run_queues_device_topk_multi(dreqs, k, out=[(a.to(torch.int64), b) for a, b in mine], slot=1)
        assert "idx" in str(err.value)
        # a request with an index far out of range: -1 and NaN everywhere, and finish_device raises
        bad_ids = dreqs[0][0].clone()
        bad_ids[0, 0] = 2 ** 40
        got = w.run_queues_device_topk_multi([(bad_ids,) + dreqs[0][1:], dreqs[1]], k, slot=1)
        with pytest.raises(N.DrsError) as err:
            w.finish_device(slot=1)
        assert err.value.code == N.ERR_INDEX_RANGE and 1 not in w.net._device_refs
        for idx, sc in got:
            assert (idx.cpu().numpy() == -1).all() and (bits(sc) == NAN_BITS).all()
    finally:
        w.net.engine.close()
