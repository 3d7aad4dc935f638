"""Launch sets whose arrays are device arrays (include/drs_device_inputs.h, deeprecsys_amd/csrc/input_pass.hip) against the
yardstick that exists without them: drs_run_queues_multi_async on the same engine with the same arrays on the host.  The
device path must return the same bits -- outputs and interaction rows -- and, where its promises are what the host path
detects, take the same launch forms.  Bad arrays end in the catalogue's code (tests/device_inputs_ref.py) and leave a slot
that serves the next set; nothing here can fault the card: the pass stores only valid rows and clamped prefix sums, and the
pointer check is shown with pinned memory, which the GPU could read."""
import numpy as np
import pytest

from deeprecsys_amd import _native as N
from tests import device_inputs_ref as R
from tests import helpers as H

pytestmark = pytest.mark.gpu

FP16 = 1


def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch


def upload(q, layout="plain"):
    """the query's arrays as device tensors -> (keep-alive tensors, the tuple Engine.run_queues_device_multi_async takes).
    layout "sliced": ids as big[:, 1:1+n] of a wider tensor (an odd 8-byte offset, a row stride != n), lengths a column
    slice, dense contiguous rows that start one float into a flat buffer (4-byte aligned, no more)."""
    torch = torch_cuda()
    dev = "cuda:0"
    n = q.ids.shape[1]
    if layout == "sliced":
        big = torch.full((R.T, n + 4), -7, dtype=torch.int64, device=dev)
        big[:, 1:1 + n] = torch.from_numpy(q.ids).to(dev)
        ids = big[:, 1:1 + n]
        wide = torch.full((R.T, q.bs + 5), -3, dtype=torch.int32, device=dev)
        wide[:, 3:3 + q.bs] = torch.from_numpy(q.lengths).to(dev)
        lengths = wide[:, 3:3 + q.bs]
        # dense: one float into a flat buffer, viewed as [bs, m_den] -- contiguous rows whose first byte is only 4-byte aligned
        m = q.dense.shape[1]
        tall = torch.full((q.bs * m + 2,), float("nan"), device=dev)
        dense = tall[1:1 + q.bs * m].view(q.bs, m)
        dense.copy_(torch.from_numpy(q.dense).to(dev))
        keep = (big, wide, tall)
        assert ids.data_ptr() % 16 == 8 or n == 0
        assert dense.data_ptr() % 16 == 4 or q.bs * m == 0
    else:
        lengths, dense = torch.from_numpy(q.lengths).to(dev), torch.from_numpy(q.dense).to(dev)
        # (torch gives an empty tensor a null data_ptr: no indices at all still come as a pointer into device memory)
        ids = torch.from_numpy(q.ids).to(dev) if n else torch.zeros((R.T, 1), dtype=torch.int64, device=dev)
        keep = (ids, lengths, dense)
    has_dense = q.dense.shape[1] > 0
    tup = (q.bs, dense.data_ptr() if has_dense and q.bs else 0, ids.data_ptr() if q.bs else 0, ids.stride(0), n,
           lengths.data_ptr() if q.bs else 0, lengths.stride(0), q.fixed_len)
    return keep, tup


def collect(eng, qs, slot):
    """wait for the set on `slot` -> (outputs per query, interaction rows per query, dispatch tokens)"""
    total = sum(q.bs for q in qs)
    out = eng.wait(slot, total)
    log = eng.last_dispatch(slot)
    vrows = sum((q.bs + 63) // 64 * 64 for q in qs)
    Rw = eng.fetch_interaction(vrows, slot=slot) if vrows else np.zeros((0, eng.num_int), np.float32)
    outs, rows, o, v = [], [], 0, 0
    for q in qs:
        outs.append(out[o:o + q.bs].copy())
        rows.append(Rw[v:v + q.bs].copy())
        o += q.bs
        v += (q.bs + 63) // 64 * 64
    return outs, rows, log


def poison(eng, n, slot, qs=()):
    """Leave the slot's first n per-query blocks holding nothing of a good query's answer (R.poison_sets), through the host
    path.  The host yardstick writes the very blocks the device pass writes: without this a device run that follows a host
    run of the same arrays would find every index row, offsets row and dense row already in place, and a pass that left a
    store out could not fail."""
    cap = eng.max_batch * eng.max_lookups
    assert all(q.ids.shape[1] != cap - 1 for q in qs)
    for sets in R.poison_sets([int(r) for r in eng._rows], eng.m_den, eng.max_batch, cap, max(n, 1)):
        eng.run_queues_multi_async(sets, slot=slot)
        eng.wait(slot)


def run_host(eng, qs, slot=0):
    eng.run_queues_multi_async(R.host_args(qs), slot=slot)
    return collect(eng, qs, slot)


def run_device(eng, qs, slot=0, layout="plain", scrub=True):
    torch = torch_cuda()
    ups = [upload(q, layout) for q in qs]
    torch.cuda.synchronize()
    if scrub:
        poison(eng, len(qs), slot, qs)
    eng.run_queues_device_multi_async([u[1] for u in ups], slot=slot)
    res = collect(eng, qs, slot)
    del ups
    return res


def same_bits(a, b):
    return all(x.shape == y.shape and np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))


def check_against_host(eng, qs, layout="plain", slot=0):
    """both paths on one engine: the same bits; the same forms behind the pass's own entry when the promises are what the
    host detects, else the comparison runs under "sls_exact" 1 (the host may take a flat form for the equal lengths)"""
    forms = R.same_forms(qs)
    eng.set_option("sls_exact", 0 if forms else 1)
    try:
        ho, hr, hlog = run_host(eng, qs, slot)
        do, dr, dlog = run_device(eng, qs, slot, layout)
    finally:
        eng.set_option("sls_exact", 0)
    assert same_bits(do, ho), "outputs differ from the host path"
    assert same_bits(dr, hr), "interaction rows differ from the host path"
    assert all(np.isfinite(o).all() for o in do)
    if sum(q.bs for q in qs):
        assert dlog[0].startswith("input_pass[") and not any(t.startswith("input_pass") for t in hlog), (dlog, hlog)
        if forms:
            assert dlog[1:] == hlog, (dlog, hlog)
    return do


@pytest.fixture(scope="module")
def eng():
    e = R.make_engine(dispatch_log=1)
    yield e
    e.close()


# ------------------------------------------------------------------------------------------------
# 1. the same bits as the host path
@pytest.mark.parametrize("name", list(R.GOOD))
def test_every_good_set_has_the_bits_of_the_host_path(eng, name):
    check_against_host(eng, R.GOOD[name])


def test_the_first_use_of_the_device_path_needs_no_host_set_before_it():
    """a fresh engine: the device path allocates the HBM blocks alone, the host path adds its pinned half later"""
    e = R.make_engine(dispatch_log=1)
    try:
        qs = R.GOOD["set_of_2"]
        do, dr, _ = run_device(e, qs, scrub=False)          # (no host call before it: freshly allocated blocks)
        ho, hr, _ = run_host(e, qs)
        assert same_bits(do, ho) and same_bits(dr, hr)
        do2, _, _ = run_device(e, qs, slot=1)
        assert same_bits(do2, ho)
    finally:
        e.close()


# ------------------------------------------------------------------------------------------------
# 2. alignment and strides
@pytest.mark.parametrize("name", ["ragged_bs65_n5", "ragged_bs257_n257", "ragged_bs600_n1023", "ragged_bs257_n2049",
                                  "fixed_bs600_L8", "set_of_2"])
def test_slices_of_wider_tensors_have_the_bits_of_contiguous_copies(eng, name):
    torch = torch_cuda()
    qs = R.GOOD[name]
    plain = check_against_host(eng, qs)
    ups = [upload(q, "sliced") for q in qs]
    before = [[t.clone() for t in u[0]] for u in ups]
    torch.cuda.synchronize()
    poison(eng, len(qs), 0, qs)
    eng.run_queues_device_multi_async([u[1] for u in ups], slot=0)
    got, _, _ = collect(eng, qs, 0)
    assert same_bits(got, plain)
    torch.cuda.synchronize()
    for u, b in zip(ups, before):            # read, never written (NaN padding: compare the bytes)
        for t, c in zip(u[0], b):
            assert torch.equal(t.view(torch.uint8), c.view(torch.uint8))


# ------------------------------------------------------------------------------------------------
# 3. sets
def test_every_query_of_a_set_of_16_has_the_bits_it_has_alone(eng):
    qs = R.GOOD["set_of_16"]
    do, dr, _ = run_device(eng, qs)
    for i, q in enumerate(qs):
        o1, r1, _ = run_device(eng, [q], slot=i % 2)
        assert same_bits(o1, [do[i]]) and same_bits(r1, [dr[i]]), i


def test_mixed_promises_take_the_forms_of_the_host_set(eng):
    for name in ("promises_8_8_ragged", "promises_8_8_2"):
        qs = R.GOOD[name]
        assert R.same_forms(qs)
        _, _, hlog = run_host(eng, qs)
        _, _, dlog = run_device(eng, qs)
        assert dlog[1:] == hlog and len(hlog) >= 2, (name, dlog, hlog)


def test_two_slots_in_flight_waited_for_in_reverse_order(eng):
    torch = torch_cuda()
    a, b = R.GOOD["set_of_2"], R.GOOD["promises_8_8_2"]
    ha, _, _ = run_host(eng, a)
    hb, _, _ = run_host(eng, b)
    ua, ub = [upload(q) for q in a], [upload(q) for q in b]
    torch.cuda.synchronize()
    poison(eng, len(a), 0, a)
    poison(eng, len(b), 1, b)
    eng.run_queues_device_multi_async([u[1] for u in ua], slot=0)
    eng.run_queues_device_multi_async([u[1] for u in ub], slot=1)
    gb, _, _ = collect(eng, b, 1)
    ga, _, _ = collect(eng, a, 0)
    assert same_bits(ga, ha) and same_bits(gb, hb)


# ------------------------------------------------------------------------------------------------
# 4. all six models
def model_queries(eng, lX, lS_l, lS_i, L, promise):
    n = len(lS_l[0][0])
    qs = []
    for k in range(min(len(lS_l), 3)):
        bs = max(1, n - 3 * k)
        ids = np.stack([np.asarray(i, dtype=np.int64) for i in lS_i[k]])[:, :bs * L]
        lengths = np.stack([np.asarray(l, dtype=np.int32) for l in lS_l[k]])[:, :bs]
        dense = np.asarray(lX[k], dtype=np.float32)[:bs] if eng.m_den else np.zeros((bs, 0), np.float32)
        q = R.Q(bs, np.ascontiguousarray(ids), np.ascontiguousarray(lengths), np.ascontiguousarray(dense), -1)
        qs.append(q._replace(fixed_len=R.host_uniform(q) if promise else -1))
    return qs


@pytest.mark.parametrize("case", ["dlrm_dot_small", "wnd_mini", "mtwnd_mini", "ncf_mini", "din_mini", "dien_mini"])
def test_one_good_set_on_every_model_kind(case):
    meta, z = H.load_fixture(case)
    args = H.args_from(meta["args"], accel_slots=2)
    net, lX, lS_l, lS_i, lT = H.materialize(args)
    net.create(lX[0], lS_l[0], lS_i[0], lT[0])
    e = net.engine
    try:
        e.set_option("dispatch_log", 1)
        qs = model_queries(e, lX, lS_l, lS_i, int(args.num_indices_per_lookup), promise=True)
        host = [(q.dense if e.m_den else None, q.ids, q.lengths, q.bs) for q in qs]
        e.run_queues_multi_async(host, slot=1)
        ho, hr, hlog = collect_any(e, qs, 1)
        torch = torch_cuda()
        ups = [upload(q) for q in qs]
        torch.cuda.synchronize()
        poison(e, len(qs), 1, qs)
        e.run_queues_device_multi_async([u[1] for u in ups], slot=1)       # (NCF, DIN, DIEN: d_dense NULL)
        do, dr, dlog = collect_any(e, qs, 1)
        assert same_bits(do, ho) and (dr is None or same_bits(dr, hr)), case
        assert dlog[0].startswith("input_pass[") and dlog[1:] == hlog, (dlog, hlog)
        if e.m_den == 0:
            assert all(u[1][1] == 0 for u in ups)
    finally:
        e.close()


def collect_any(e, qs, slot):
    """collect() for any model: W&D / MT-WnD read their dense columns in place, their interaction tensor is not materialised"""
    total = sum(q.bs for q in qs)
    out = e.wait(slot, total)
    log = e.last_dispatch(slot)
    outs, o = [], 0
    for q in qs:
        outs.append(out[o:o + q.bs].copy())
        o += q.bs
    rows = None
    if e.kind not in (N.MODEL_WND, N.MODEL_MTWND):
        vrows = sum((q.bs + 63) // 64 * 64 for q in qs)
        Rw = e.fetch_interaction(vrows, slot=slot)
        rows, v = [], 0
        for q in qs:
            rows.append(Rw[v:v + q.bs].copy())
            v += (q.bs + 63) // 64 * 64
    return outs, rows, log


def test_fp16_tables_have_the_bits_of_the_host_path():
    e = R.make_engine(table_dtype=FP16, dispatch_log=1)
    try:
        check_against_host(e, R.GOOD["set_of_2"])
        check_against_host(e, R.GOOD["fixed_bs600_L8"])
    finally:
        e.close()


# ------------------------------------------------------------------------------------------------
# 5. errors found on the device
@pytest.mark.parametrize("name", list(R.BAD))
def test_a_bad_set_ends_in_its_code_and_the_slot_serves_the_next_set(eng, name):
    torch = torch_cuda()
    qs, code, host_code = R.BAD[name]
    good, other = R.GOOD["set_of_2"], R.GOOD["promises_8_8_ragged"]
    want_good, _, _ = run_host(eng, good)
    want_other, _, _ = run_host(eng, other)
    # the host path, same arrays
    if host_code == N.OK:
        run_host(eng, qs)
    else:
        with pytest.raises(N.DrsError) as err:
            eng.run_queues_multi_async(R.host_args(qs), slot=0)
        assert err.value.code == host_code
    # the device path: accepted, found by the pass, reported by the wait -- with a good set in flight on the other slot
    ub, uo = [upload(q) for q in qs], [upload(q) for q in other]
    torch.cuda.synchronize()
    poison(eng, len(qs), 0)
    poison(eng, len(other), 1, other)
    eng.run_queues_device_multi_async([u[1] for u in ub], slot=0)            # returns DRS_OK
    eng.run_queues_device_multi_async([u[1] for u in uo], slot=1)
    with pytest.raises(N.DrsError) as err:
        eng.wait(0, sum(q.bs for q in qs))
    assert err.value.code == code, str(err.value)
    got_other, _, _ = collect(eng, other, 1)
    assert same_bits(got_other, want_other)
    got_good, _, _ = run_device(eng, good, slot=0)                            # the next set on the slot: its own bits
    assert same_bits(got_good, want_good)


# ------------------------------------------------------------------------------------------------
# 6. refused before launch
# (The "coalesced rows exceed the slot capacity" refusal cannot be reached and has no case: the capacity is DRS_MAX_COALESCE *
#  round_up(max_batch, 64) rows, and a set is at most DRS_MAX_COALESCE queries of at most max_batch samples.)
class Refusals(object):
    """one valid uploaded query (65 bags of 4), its arrays in pinned host memory as well, and what the host path gives a good set"""

    def __init__(self, eng):
        torch = torch_cuda()
        self.good = R.GOOD["set_of_2"]
        self.want, _, _ = run_host(eng, self.good)
        self.q = R.query(500, 65, fixed_len=4)
        self.keep, self.tup = upload(self.q)
        # PINNED host memory for the pointer check: the GPU could read it, so a missing check fails the test and faults nothing
        self.pinned = [torch.from_numpy(x).pin_memory() for x in (self.q.ids, self.q.lengths, self.q.dense)]
        assert all(t.is_pinned() and t.device.type == "cpu" for t in self.pinned)
        torch.cuda.synchronize()


@pytest.fixture(scope="module")
def refusals(eng):
    return Refusals(eng)


def _tup(c, **kw):
    d = dict(zip(("bs", "dp", "ip", "irs", "n", "lp", "lrs", "fl"), c.tup))
    d.update(kw)
    return tuple(d[k] for k in ("bs", "dp", "ip", "irs", "n", "lp", "lrs", "fl"))


REFUSALS = [
    ("slot_2_of_2", N.ERR_BAD_ARG, lambda c: dict(queries=[c.tup], slot=2)),
    ("slot_minus_1", N.ERR_BAD_ARG, lambda c: dict(queries=[c.tup], slot=-1)),
    ("n_17", N.ERR_BAD_ARG, lambda c: dict(queries=[c.tup] * 17)),
    ("n_0", N.ERR_BAD_ARG, lambda c: dict(queries=[])),
    ("null_dense", N.ERR_BAD_ARG, lambda c: dict(queries=[_tup(c, dp=0)])),
    ("null_ids", N.ERR_BAD_ARG, lambda c: dict(queries=[_tup(c, ip=0)])),
    ("null_lengths", N.ERR_BAD_ARG, lambda c: dict(queries=[_tup(c, lp=0)])),
    ("bs_601", N.ERR_BAD_ARG, lambda c: dict(queries=[_tup(c, bs=601, fl=-1)])),
    ("bs_minus_1", N.ERR_BAD_ARG, lambda c: dict(queries=[_tup(c, bs=-1, fl=-1)])),
    ("n_idx_cap_plus_1", N.ERR_BAD_ARG, lambda c: dict(queries=[_tup(c, n=R.CAP + 1, fl=-1)])),
    ("n_idx_minus_1", N.ERR_BAD_ARG, lambda c: dict(queries=[_tup(c, n=-1, fl=-1)])),
    ("fixed_len_minus_2", N.ERR_BAD_ARG, lambda c: dict(queries=[_tup(c, fl=-2)])),
    ("ids_stride_negative", N.ERR_BAD_ARG, lambda c: dict(queries=[_tup(c, irs=-1)])),
    ("lengths_stride_negative", N.ERR_BAD_ARG, lambda c: dict(queries=[_tup(c, lrs=-1)])),
    # 2 * 2^62 elements wrap a 64-bit byte count to a small extent: refused by the arithmetic, not by luck
    ("ids_stride_2p62", N.ERR_BAD_ARG, lambda c: dict(queries=[_tup(c, irs=2 ** 62)])),
    ("lengths_stride_2p61", N.ERR_BAD_ARG, lambda c: dict(queries=[_tup(c, lrs=2 ** 61)])),
    ("promise_contradicts_count", N.ERR_LENGTHS_SUM, lambda c: dict(queries=[_tup(c, fl=3)])),
    ("count_contradicts_promise", N.ERR_LENGTHS_SUM, lambda c: dict(queries=[_tup(c, n=c.tup[4] - 1)])),
    ("promise_contradicts_count_in_a_later_query", N.ERR_LENGTHS_SUM, lambda c: dict(queries=[c.tup, _tup(c, fl=3)])),
    ("null_table", N.ERR_BAD_ARG, lambda c: dict(null_table=True)),
    ("pinned_ids", N.ERR_BAD_ARG, lambda c: dict(queries=[_tup(c, ip=c.pinned[0].data_ptr(), irs=c.pinned[0].stride(0))])),
    ("pinned_lengths", N.ERR_BAD_ARG, lambda c: dict(queries=[_tup(c, lp=c.pinned[1].data_ptr(), lrs=c.pinned[1].stride(0))])),
    ("pinned_dense", N.ERR_BAD_ARG, lambda c: dict(queries=[_tup(c, dp=c.pinned[2].data_ptr())])),
]


@pytest.mark.parametrize("name,code,make", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_a_synchronous_refusal_leaves_the_slot_free(eng, refusals, name, code, make):
    c = refusals
    kw = make(c)
    with pytest.raises(N.DrsError) as err:
        if kw.get("null_table"):
            bs, _, ip, _, n = c.tup[:5]
            null = N.C.POINTER(N.C.c_void_p)()
            one = (N.C.c_void_p * 1)(ip)
            i32, i64 = np.array([bs], np.int32), np.array([n], np.int64)
            eng._check(N.lib().drs_run_queues_device_multi_async(
                eng._h, 0, 1, i32.ctypes.data_as(N._i32p), one, null, i64.ctypes.data_as(N._i64p), i64.ctypes.data_as(N._i64p), one,
                i64.ctypes.data_as(N._i64p), None), "drs_run_queues_device_multi_async")
        else:
            eng.run_queues_device_multi_async(kw["queries"], slot=kw.get("slot", 0))
    assert err.value.code == code, str(err.value)
    assert eng.wait(0) is None                     # nothing in flight on the slot
    got, _, _ = run_device(eng, c.good, slot=0)
    assert same_bits(got, c.want)


def test_the_arrays_of_the_refusal_cases_are_served_and_the_scalar_form_is_the_set_of_one(eng, refusals):
    c = refusals
    want = run_host(eng, [c.q])[0]
    poison(eng, 1, 0, [c.q])
    eng.run_queues_device_multi_async([c.tup], slot=0)
    got, _, _ = collect(eng, [c.q], 0)
    assert same_bits(got, want)
    poison(eng, 1, 0, [c.q])
    eng._check(N.lib().drs_run_queues_device_async(eng._h, 0, *c.tup), "drs_run_queues_device_async")
    assert same_bits(collect(eng, [c.q], 0)[0], want)


# ------------------------------------------------------------------------------------------------
# 7. the wrapper
def test_the_wrapper_equals_run_queues_multi_on_uploaded_requests():
    torch = torch_cuda()
    from deeprecsys_amd import dlrm_s_hip as M
    meta, z = H.load_fixture("dlrm_dot_small")
    args = H.args_from(meta["args"], accel_slots=2)
    np.random.seed(args.numpy_rand_seed)
    net, lX, lS_l, lS_i, lT = H.materialize(args)
    w = M.DLRM_Wrapper(args)
    w.create(lX[0], lS_l[0], lS_i[0], lT[0])
    try:
        L = int(args.num_indices_per_lookup)
        n = len(lS_l[0][0])
        reqs = []
        for k in range(min(len(lS_l), 3)):
            bs = max(1, n - k)
            ids = np.ascontiguousarray(np.stack([np.asarray(i, dtype=np.int64) for i in lS_i[k]])[:, :bs * L])
            lengths = np.ascontiguousarray(np.stack([np.asarray(l, dtype=np.int32) for l in lS_l[k]])[:, :bs])
            reqs.append((ids, lengths, np.ascontiguousarray(np.asarray(lX[k], dtype=np.float32)[:bs]), bs))
        want = w.run_queues_multi(reqs, slot=1)
        dev = "cuda:%d" % w.net.engine.device
        # promised: what the host path finds by looking at the lengths, so both take the same forms
        dreqs = [(torch.as_tensor(i, device=dev), torch.as_tensor(l, device=dev), torch.as_tensor(f, device=dev), bs,
                  int(l[0, 0]) if (l == l[0, 0]).all() else -1) for i, l, f, bs in reqs]
        poison(w.net.engine, len(reqs), 1)
        got = w.run_queues_device_multi(dreqs, slot=1)
        assert len(got) == len(want) and same_bits(got, want)
        assert same_bits([w.net._out], [want[-1]])
        # nothing promised (a request of four): the ragged forms; every form sums alike under the sequential order
        w.net.engine.set_option("sls_exact", 1)
        want = w.run_queues_multi(reqs, slot=0)
        poison(w.net.engine, len(reqs), 0)
        got = w.run_queues_device_multi([r[:4] for r in dreqs], slot=0)
        assert same_bits(got, want)
        with pytest.raises(ValueError):
            w.run_queues_device_multi([(torch.as_tensor(reqs[0][0]), dreqs[0][1], dreqs[0][2], reqs[0][3])])
    finally:
        w.net.engine.close()
