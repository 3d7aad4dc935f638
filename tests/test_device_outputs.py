"""Launch sets whose results stay on the device (include/drs_device_outputs.h, deeprecsys_amd/csrc/output_pass.hip) against
the yardstick that exists without them: drs_run_queues_multi_async + drs_wait on the same engine with the same arrays on the
host.  The device tensors must hold the bits the host receives, and nothing around them may change; a set that failed on the
device holds NaN everywhere; under `ordered` 1 the set runs behind the caller's stream and the caller's stream behind the set,
with no host wait.  Nothing here can fault the card: every index in every state of every tensor is valid or is clamped by
the input pass, and the pointer check is shown with pinned memory, which the GPU could write."""
import time

import numpy as np
import pytest

from deeprecsys_amd import _native as N
from tests import device_inputs_ref as R
from tests import helpers as H
from tests import test_device_inputs as DI

pytestmark = pytest.mark.gpu

SENTINEL = -77.25
NAN_BITS = 0x7FC00000
upload, poison, same_bits, run_host = DI.upload, DI.poison, DI.same_bits, DI.run_host


def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch


def bits(t):
    """a float32 torch tensor (any layout, any device) -> its bits as a numpy uint32 array"""
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


class Out(object):
    """one query's output tensor inside a buffer full of the sentinel.  layout "plain": [bs, n_out] contiguous; "cols": the
    column block big[:, 2:2 + n_out] of a wider tensor (row stride n_out + 5); "offset": contiguous rows that start one float
    into a flat buffer (4-byte aligned, no more).  An empty query gets three rows the pass must not touch."""

    def __init__(self, bs, n_out, layout="plain"):
        torch = torch_cuda()
        rows = bs if bs else 3
        if layout == "cols":
            self.buf = torch.full((rows, n_out + 5), SENTINEL, device="cuda:0")
            self.t = self.buf[:, 2:2 + n_out]
            self.scores = np.zeros((rows, n_out + 5), bool)
            self.scores[:bs, 2:2 + n_out] = True
        elif layout == "offset":
            self.buf = torch.full((rows * n_out + 2,), SENTINEL, device="cuda:0")
            self.t = self.buf[1:1 + rows * n_out].view(rows, n_out)
            self.scores = np.zeros(rows * n_out + 2, bool)
            self.scores[1:1 + bs * n_out] = True
            assert self.t.data_ptr() % 16 == 4
        else:
            self.buf = torch.full((rows, n_out), SENTINEL, device="cuda:0")
            self.t = self.buf
            self.scores = np.zeros((rows, n_out), bool)
            self.scores[:bs] = True
        self.bs = bs
        self.arg = (self.t.data_ptr(), self.t.stride(0))

    def rows(self):
        """the query's [bs, n_out] scores"""
        return self.t[:self.bs].cpu().contiguous().numpy()

    def surroundings_untouched(self):
        """everything of the buffer that is no score of the query still holds the sentinel's bits"""
        return bool((bits(self.buf)[~self.scores] == np.float32(SENTINEL).view(np.uint32)).all())


def call_io(eng, tups, outs, stream=None, slot=0, ordered=None, null_out_table=False, null_stride_table=False):
    """drs_run_queues_device_io_multi_async as the binding calls it, with every argument open to a refusal case"""
    args, keep = eng._device_set(tups)
    n = len(outs)
    op = (N.C.c_void_p * max(n, 1))()
    st = np.empty(max(n, 1), dtype=np.int64)
    for i, (ptr, rs) in enumerate(outs):
        op[i] = ptr or None
        st[i] = rs
    if ordered is None:
        ordered = 0 if stream is None else 1
    eng._check(N.lib().drs_run_queues_device_io_multi_async(
        eng._h, slot, *(args + [N.C.POINTER(N.C.c_void_p)() if null_out_table else op,
                                None if null_stride_table else st.ctypes.data_as(N._i64p), stream or None, ordered])),
        "drs_run_queues_device_io_multi_async")
    del keep


def run_io(eng, qs, slot=0, layout="plain", in_layout="plain", scrub=True, null_empty=False):
    """the set through the io call with `ordered` 0 -> (scores per query read from the device tensors after wait, the host
    floats the same wait returned, the Out objects, the dispatch tokens)"""
    torch = torch_cuda()
    ups = [upload(q, in_layout) for q in qs]
    outs = [Out(q.bs, eng.n_out, layout) for q in qs]
    torch.cuda.synchronize()
    if scrub:
        poison(eng, len(qs), slot, qs)
    eng.run_queues_device_io_multi_async([u[1] for u in ups], [(0, eng.n_out) if null_empty and not q.bs else o.arg
                                                                for q, o in zip(qs, outs)], stream=None, slot=slot)
    total = sum(q.bs for q in qs)
    host = eng.wait(slot, total)
    log = eng.last_dispatch(slot)
    got = [o.rows() for o in outs]
    hosts, k = [], 0
    for q in qs:
        hosts.append(host[k:k + q.bs].copy())
        k += q.bs
    del ups
    return got, hosts, outs, log


def check_against_host(eng, qs, layout="plain", slot=0, **kw):
    forms = R.same_forms(qs)
    eng.set_option("sls_exact", 0 if forms else 1)
    try:
        want, _, hlog = run_host(eng, qs, slot)
        got, hosts, outs, log = run_io(eng, qs, slot, layout, **kw)
    finally:
        eng.set_option("sls_exact", 0)
    assert same_bits(got, want), "the device tensors differ from the host path"
    assert same_bits(hosts, want), "the host floats of the same wait differ from the host path"
    assert all(np.isfinite(o).all() for o in got)
    assert all(o.surroundings_untouched() for o in outs), "something beside the scores was written"
    if sum(q.bs for q in qs):
        assert log[0].startswith("input_pass[") and log[-1].startswith("output_pass[") and log[-1].endswith("x 256]"), log
        assert sum(t.startswith("output_pass") for t in log) == 1 and not any(t.startswith("output_pass") for t in hlog)
        if forms:
            assert log[1:-1] == hlog, (log, hlog)
    else:
        assert not any(t.startswith("output_pass") for t in log)
    return got


@pytest.fixture(scope="module")
def eng():
    e = R.make_engine(dispatch_log=1)
    yield e
    e.close()


# ------------------------------------------------------------------------------------------------
# 1. the same bits as the host results
@pytest.mark.parametrize("name", list(R.GOOD))
def test_every_good_set_leaves_the_bits_of_the_host_path_on_the_device(eng, name):
    check_against_host(eng, R.GOOD[name])


def test_an_empty_query_may_come_without_an_output(eng):
    check_against_host(eng, R.GOOD["empty_first_and_middle"], null_empty=True)


# ------------------------------------------------------------------------------------------------
# 2. strides and alignment
@pytest.mark.parametrize("layout", ["cols", "offset"])
@pytest.mark.parametrize("name", ["set_of_2", "ragged_bs257_n257", "empty_first_and_middle"])
def test_slices_of_wider_tensors_receive_the_same_bits_and_nothing_around_them(eng, name, layout):
    qs = R.GOOD[name]
    check_against_host(eng, qs, layout=layout, in_layout="sliced" if layout == "offset" and all(q.bs for q in qs) else "plain")


# ------------------------------------------------------------------------------------------------
# 3. sets
def test_every_query_of_a_set_of_16_has_the_bits_it_has_alone(eng):
    qs = R.GOOD["set_of_16"]
    got, _, _, _ = run_io(eng, qs)
    for i, q in enumerate(qs):
        alone, _, _, _ = run_io(eng, [q], slot=i % 2)
        assert same_bits(alone, [got[i]]), i


def test_two_slots_in_flight_waited_for_in_reverse_order(eng):
    torch = torch_cuda()
    a, b = R.GOOD["set_of_2"], R.GOOD["promises_8_8_2"]
    ha, _, _ = run_host(eng, a)
    hb, _, _ = run_host(eng, b)
    ua, ub = [upload(q) for q in a], [upload(q) for q in b]
    oa, ob = [Out(q.bs, eng.n_out) for q in a], [Out(q.bs, eng.n_out, "cols") for q in b]
    torch.cuda.synchronize()
    poison(eng, len(a), 0, a)
    poison(eng, len(b), 1, b)
    eng.run_queues_device_io_multi_async([u[1] for u in ua], [o.arg for o in oa], slot=0)
    eng.run_queues_device_io_multi_async([u[1] for u in ub], [o.arg for o in ob], slot=1)
    assert eng.wait(1) is None
    gb = [o.rows() for o in ob]
    assert eng.wait(0) is None
    ga = [o.rows() for o in oa]
    assert same_bits(ga, ha) and same_bits(gb, hb)
    assert all(o.surroundings_untouched() for o in oa + ob)


# ------------------------------------------------------------------------------------------------
# 4. all six model kinds
@pytest.mark.parametrize("case", ["dlrm_dot_small", "wnd_mini", "mtwnd_mini", "ncf_mini", "din_mini", "dien_mini"])
def test_one_good_set_on_every_model_kind(case):
    torch = torch_cuda()
    meta, z = H.load_fixture(case)
    args = H.args_from(meta["args"], accel_slots=2)
    net, lX, lS_l, lS_i, lT = H.materialize(args)
    net.create(lX[0], lS_l[0], lS_i[0], lT[0])
    e = net.engine
    try:
        e.set_option("dispatch_log", 1)
        assert e.n_out > 1 or case != "mtwnd_mini"
        qs = DI.model_queries(e, lX, lS_l, lS_i, int(args.num_indices_per_lookup), promise=True)
        host = [(q.dense if e.m_den else None, q.ids, q.lengths, q.bs) for q in qs]
        e.run_queues_multi_async(host, slot=1)
        ho, _, hlog = DI.collect_any(e, qs, 1)
        ups = [upload(q) for q in qs]
        torch.cuda.synchronize()
        # the device-input call: its log, and no token of the output pass in it
        poison(e, len(qs), 1, qs)
        e.run_queues_device_multi_async([u[1] for u in ups], slot=1)
        do, _, dlog = DI.collect_any(e, qs, 1)
        assert same_bits(do, ho) and not any(t.startswith("output_pass") for t in dlog)
        for layout in ("plain", "cols"):
            outs = [Out(q.bs, e.n_out, layout) for q in qs]
            torch.cuda.synchronize()
            poison(e, len(qs), 1, qs)
            e.run_queues_device_io_multi_async([u[1] for u in ups], [o.arg for o in outs], slot=1)
            assert e.wait(1) is None
            log = e.last_dispatch(1)
            assert same_bits([o.rows() for o in outs], ho), (case, layout)
            assert all(o.surroundings_untouched() for o in outs)
            assert log[:-1] == dlog and log[-1].startswith("output_pass["), (log, dlog)
    finally:
        e.close()


# ------------------------------------------------------------------------------------------------
# 5. ordering on the caller's stream
def sleep_cycles(torch, want_ms):
    """torch.cuda._sleep's argument for a delay of want_ms (inside [50 ms, 1 s]) at the rate one short sleep shows"""
    probe = 2000000
    torch.cuda._sleep(1000)                                       # (the kernel's first launch loads its module)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    torch.cuda._sleep(probe)
    torch.cuda.synchronize()
    per_cycle = (time.perf_counter() - t0) * 1e3 / probe          # (an overestimate: it holds the launch and the sync)
    assert 50.0 <= want_ms <= 1000.0 and per_cycle > 0
    return int(want_ms / per_cycle)


@pytest.mark.parametrize("which", ["side_stream", "default_stream"])
def test_a_set_runs_behind_the_callers_stream_and_the_callers_stream_behind_the_set(eng, which):
    torch = torch_cuda()
    slot = 0
    # two queries of the same shapes, different ids and dense rows, all valid
    A, B = R.query(600, 257, 1025), R.query(601, 257, 1025)
    lengths = A.lengths
    B = B._replace(lengths=lengths)          # (the same lengths: B's ids are valid for them -- 1025 per table either way)
    (wa,), _, _ = run_host(eng, [A], slot)
    (wb,), _, _ = run_host(eng, [B], slot)
    assert not np.array_equal(wa.view(np.uint32), wb.view(np.uint32)), "A and B must differ for the test to show anything"
    keep, tup = upload(A)
    ids, lens, dense = keep
    b_ids, b_dense = torch.from_numpy(B.ids).to("cuda:0"), torch.from_numpy(B.dense).to("cuda:0")
    out = Out(A.bs, eng.n_out)
    poison(eng, 1, slot, [A])
    cycles = sleep_cycles(torch, 150.0)
    S = torch.cuda.Stream() if which == "side_stream" else torch.cuda.default_stream()
    handle = S.cuda_stream
    assert (handle == 0) == (which == "default_stream")
    torch.cuda.synchronize()
    with torch.cuda.stream(S):
        torch.cuda._sleep(cycles)
        ids.copy_(b_ids, non_blocking=True)
        dense.copy_(b_dense, non_blocking=True)
        eng.run_queues_device_io_multi_async([tup], [out.arg], stream=handle, slot=slot)
        got = out.t.clone()
        still_running = not S.query()
    assert still_running, "the call (or the clone behind it) waited on the host for the stream"
    S.synchronize()
    assert np.array_equal(bits(got), wb.view(np.uint32)), \
        "the scores cloned on the stream are not B's: " + ("they are A's -- the input edge is missing"
                                                           if np.array_equal(bits(got), wa.view(np.uint32)) else
                                                           "the clone ran before the output pass, or the set read a torn state")
    assert eng.wait(slot) is None
    assert np.array_equal(bits(out.t), wb.view(np.uint32)) and out.surroundings_untouched()
    del keep, lens


# ------------------------------------------------------------------------------------------------
# 6. errors found on the device
@pytest.mark.parametrize("name", list(R.BAD))
def test_a_bad_set_is_all_nan_on_the_device_and_the_slot_serves_the_next_set(eng, name):
    torch = torch_cuda()
    qs, code, _ = R.BAD[name]
    good, other = R.GOOD["set_of_2"], R.GOOD["promises_8_8_ragged"]
    want_good, _, _ = run_host(eng, good)
    want_other, _, _ = run_host(eng, other)
    ub, uo = [upload(q) for q in qs], [upload(q) for q in other]
    ob, oo = [Out(q.bs, eng.n_out, "cols") for q in qs], [Out(q.bs, eng.n_out) for q in other]
    torch.cuda.synchronize()
    poison(eng, len(qs), 0)
    poison(eng, len(other), 1, other)
    eng.run_queues_device_io_multi_async([u[1] for u in ub], [o.arg for o in ob], slot=0)          # returns DRS_OK
    eng.run_queues_device_io_multi_async([u[1] for u in uo], [o.arg for o in oo], slot=1)
    with pytest.raises(N.DrsError) as err:
        eng.wait(0)
    assert err.value.code == code, str(err.value)
    for o in ob:                                       # every element of every query, the good queries of the set too
        assert (o.rows().view(np.uint32) == NAN_BITS).all()
        assert o.surroundings_untouched()
    assert eng.wait(1) is None
    assert same_bits([o.rows() for o in oo], want_other)
    got_good, _, _, _ = run_io(eng, good, slot=0)                            # the next set on the slot: its own bits
    assert same_bits(got_good, want_good)


# ------------------------------------------------------------------------------------------------
# 7. refused before launch
class Refusals(object):
    """a valid uploaded set of two (65 and 256 rows), good outputs for it, and the outputs the cases need"""

    def __init__(self, eng):
        torch = torch_cuda()
        self.good = R.GOOD["set_of_2"]
        self.want, _, _ = run_host(eng, self.good)
        self.ups = [upload(q) for q in self.good]
        self.tups = [u[1] for u in self.ups]
        self.n_out = eng.n_out
        self.outs = [Out(q.bs, eng.n_out) for q in self.good]
        self.args = [o.arg for o in self.outs]
        # PINNED host memory: the GPU could write it, so a missing check fails the test and faults nothing
        self.pinned = torch.full((65, eng.n_out), SENTINEL).pin_memory()
        assert self.pinned.is_pinned() and self.pinned.device.type == "cpu"
        # two slices of one buffer that share exactly one float
        self.tall = torch.full((65 + 256,), SENTINEL, device="cuda:0")
        self.wide = torch.full((256, eng.n_out + 5), SENTINEL, device="cuda:0")
        torch.cuda.synchronize()

    def untouched(self):
        want = np.float32(SENTINEL).view(np.uint32)
        return all((bits(t) == want).all() for t in [o.buf for o in self.outs] + [self.pinned, self.tall, self.wide])


@pytest.fixture(scope="module")
def refusals(eng):
    return Refusals(eng)


def _outs(c, k, ptr=None, stride=None):
    a = list(c.args)
    a[k] = (a[k][0] if ptr is None else ptr, a[k][1] if stride is None else stride)
    return a


REFUSALS = [
    ("null_output_table", lambda c: dict(null_out_table=True)),
    ("null_stride_table", lambda c: dict(null_stride_table=True)),
    ("null_output_of_a_query_with_rows", lambda c: dict(outs=[c.args[0], (0, c.n_out)])),
    ("pointer_plus_2_bytes", lambda c: dict(outs=_outs(c, 0, ptr=c.args[0][0] + 2))),
    ("stride_n_out_minus_1", lambda c: dict(outs=_outs(c, 1, stride=c.n_out - 1))),
    ("stride_negative", lambda c: dict(outs=_outs(c, 1, stride=-c.n_out))),
    # 255 * 2^62 floats wrap a 64-bit byte count: refused by the arithmetic, not by luck
    ("stride_2p62", lambda c: dict(outs=_outs(c, 1, stride=2 ** 62))),
    ("ordered_2", lambda c: dict(ordered=2)),
    ("ordered_minus_1", lambda c: dict(ordered=-1)),
    ("pinned_output", lambda c: dict(outs=_outs(c, 0, ptr=c.pinned.data_ptr(), stride=c.pinned.stride(0)))),
    ("the_same_tensor_twice", lambda c: dict(outs=[c.args[1], c.args[1]])),
    ("slices_sharing_one_float", lambda c: dict(outs=[(c.tall.data_ptr() + 4 * 255, c.n_out), (c.tall.data_ptr(), c.n_out)])),
    ("interleaved_column_blocks", lambda c: dict(outs=[(c.wide.data_ptr(), c.n_out + 5), (c.wide.data_ptr() + 4 * c.n_out, c.n_out + 5)])),
    # what the device-input call refuses is refused here as well
    ("slot_2_of_2", lambda c: dict(slot=2)),
    ("n_17", lambda c: dict(tups=[c.tups[0]] * 17, outs=[c.args[0]] * 17)),
]


@pytest.mark.parametrize("name,make", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_a_synchronous_refusal_leaves_the_slot_free(eng, refusals, name, make):
    c = refusals
    kw = make(c)
    with pytest.raises(N.DrsError) as err:
        call_io(eng, kw.pop("tups", c.tups), kw.pop("outs", c.args), slot=kw.pop("slot", 0), **kw)
    assert err.value.code == N.ERR_BAD_ARG, str(err.value)
    assert eng.wait(0) is None                     # nothing in flight on the slot
    assert c.untouched()
    got, _, _, _ = run_io(eng, c.good, slot=0)
    assert same_bits(got, c.want)


def test_the_outputs_of_the_refusal_cases_are_served_and_the_scalar_form_is_the_set_of_one(eng, refusals):
    torch = torch_cuda()
    c = refusals
    poison(eng, 2, 0, c.good)
    call_io(eng, c.tups, c.args, slot=0)
    assert eng.wait(0) is None
    assert same_bits([o.rows() for o in c.outs], c.want)
    # touching outputs are legal: two slices of one buffer, the second starting where the first ends
    poison(eng, 2, 0, c.good)
    call_io(eng, c.tups, [(c.tall.data_ptr(), c.n_out), (c.tall.data_ptr() + 4 * 65 * c.n_out, c.n_out)], slot=0)
    assert eng.wait(0) is None
    flat = c.tall.cpu().numpy()
    assert same_bits([flat[:65].reshape(65, 1), flat[65:].reshape(256, 1)], c.want)
    c.tall.fill_(SENTINEL)
    # the scalar form
    q, o = c.good[0], Out(c.good[0].bs, eng.n_out)
    torch.cuda.synchronize()
    poison(eng, 1, 0, [q])
    eng._check(N.lib().drs_run_queues_device_io_async(eng._h, 0, *(c.tups[0] + (o.arg[0], o.arg[1], None, 0))),
               "drs_run_queues_device_io_async")
    assert eng.wait(0) is None
    assert same_bits([o.rows()], c.want[:1]) and o.surroundings_untouched()
    for x in c.outs:
        x.buf.fill_(SENTINEL)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------
# 8. the wrapper
def test_the_wrapper_returns_device_tensors_without_a_host_wait(monkeypatch):
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
        dreqs = [(torch.as_tensor(i, device=dev), torch.as_tensor(l, device=dev), torch.as_tensor(f, device=dev), bs,
                  int(l[0, 0]) if (l == l[0, 0]).all() else -1) for i, l, f, bs in reqs]
        poison(w.net.engine, len(reqs), 1)
        torch.cuda.synchronize()

        def no_sync(*a, **k):
            raise AssertionError("the wrapper synchronised on the host")
        with monkeypatch.context() as m:
            m.setattr(torch.cuda.Stream, "synchronize", no_sync)
            m.setattr(torch.cuda, "synchronize", no_sync)
            got = w.run_queues_device_io_multi(dreqs, slot=1)
        assert len(got) == len(want)
        assert all(isinstance(t, torch.Tensor) and t.device.type == "cuda" and t.dtype == torch.float32 and
                   tuple(t.shape) == x.shape for t, x in zip(got, want))
        # read on torch's current stream, BEFORE the set's completion was asked for: the stream is ordered behind the set
        early = [t.cpu().numpy() for t in got]
        assert same_bits(early, want)
        assert 1 in w.net._device_refs and len(w.net._device_refs[1][0]) == len(dreqs)
        assert w.finish_device(slot=1) is None
        assert 1 not in w.net._device_refs                      # the references are dropped
        # into tensors of the caller's, column blocks of wider ones; a second call on the slot without finish_device is served
        bigs = [torch.full((x.shape[0], x.shape[1] + 3), SENTINEL, device=dev) for x in want]
        first = w.run_queues_device_io_multi(dreqs, out=[b[:, 1:1 + x.shape[1]] for b, x in zip(bigs, want)], slot=1)
        second = w.run_queues_device_io_multi(dreqs[::-1], slot=1)
        assert same_bits([t.cpu().numpy() for t in second], want[::-1])
        assert same_bits([b[:, 1:1 + x.shape[1]].cpu().numpy() for b, x in zip(bigs, want)], want)
        assert all(f.data_ptr() == b[:, 1:].data_ptr() for f, b in zip(first, bigs))
        assert all((bits(b[:, 0]) == np.float32(SENTINEL).view(np.uint32)).all() for b in bigs)
        w.finish_device(slot=1)
        assert not w.net._device_refs
        with pytest.raises(ValueError):
            w.run_queues_device_io_multi(dreqs, out=[torch.zeros_like(t).cpu() for t in got])
        assert w.net.engine.wait(1) is None and not w.net._device_refs
    finally:
        w.net.engine.close()
