"""Per-sample weights on the device-array path (-m gpu): drs_run_queues_device_weighted_multi_async
(include/drs_device_weights.h, deeprecsys_amd/csrc/input_pass.hip's weighted instance).

Two references.  Independent of the code under test: tests/test_sls_weights_cpu.py's `weighted_ref` (and its rowwise twin),
the sequential chain acc = fma(w, x, acc) pinned there to torch's CPU operators, which the pooled columns equal bit for bit
under "sls_exact" 1.  And the route that existed before: the same arrays staged with stage_batch(..., weights=) on the same
engine and served by forward_multi_async in the same set composition -- the same kernels on the same values, so outputs and
interaction rows are compared bitwise, under "sls_exact" 0 and "sls_weighted_flat" 1 too.

Nothing here can fault the card: every index is valid or is clamped by the input pass, every weight pointer handed to an
accepted call lies inside a live tensor with the extent the call reads, and the refused pointers are refused on the host."""
import numpy as np
import pytest

from deeprecsys_amd import _native as N
from tests import helpers as H
from tests.test_half_tables import _load
from tests.test_sls_weights import _engine, _ref, _stored
from tests.test_sls_weights_cpu import same_bits
from tests.test_sls_weights_flat_cpu import expected_form, log_token

pytestmark = pytest.mark.gpu

T, B = 3, 48
ROWS = [1501 + 13 * t for t in range(T)]
NAN_BITS = 0x7FC00000
CHUNK = 4096                                   # csrc/weight_plan.h kInPassWgt


def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch


def cuts(rng, bs, total):
    """bs ragged bag lengths that sum to `total`, with empty bags among them"""
    c = np.sort(rng.randint(0, total + 1, size=bs - 1)) if bs > 1 else np.zeros(0, np.int64)
    if bs > 4:
        c[1] = c[0]                            # (an empty bag at least)
    ln = np.diff(np.concatenate([[0], c, [total]])).astype(np.int32)
    assert ln.sum() == total and (ln >= 0).all()
    return ln


class Q(object):
    """one query on the host: ids [T, n] int64, lengths [T, bs] int32, dense [bs, 8], weights [T, n] fp32 (k / 1024: exact in
    fp16 and bf16 is not needed here, see test 2) or None"""

    def __init__(self, rng, bs, L, rows=ROWS, weighted=True, n_tables=T):
        self.bs, self.L = bs, L
        if L == "ragged":
            n = bs * 9
            self.lengths = np.stack([cuts(rng, bs, n) for _ in range(n_tables)]) if bs else np.zeros((n_tables, 0), np.int32)
        else:
            n = bs * L
            self.lengths = np.full((n_tables, bs), L, np.int32)
        self.n = n
        self.ids = np.stack([rng.randint(0, rows[t], size=n) for t in range(n_tables)]).astype(np.int64).reshape(n_tables, n)
        if n:
            self.ids[:, 0], self.ids[:, -1] = 0, np.asarray(rows) - 1
        self.dense = rng.rand(bs, 8).astype(np.float32)
        self.w = rng.uniform(0, 1, size=(n_tables, n)).astype(np.float32) if weighted else None
        # the promise is what the host finds by looking at the lengths (a "ragged" query of ONE bag per table has equal lengths):
        # the staged route detects it so, and both routes must take the same forms
        same = bs > 0 and bool((self.lengths == self.lengths[0, 0]).all())
        self.fixed_len = int(self.lengths[0, 0]) if same else -1

    def stage(self, eng, b, weights=True):
        eng.stage_batch(b, self.dense, list(self.ids), list(self.lengths),
                        weights=list(self.w) if weights and self.w is not None else None)


class Up(object):
    """a query's arrays as device tensors: .tup is Engine.run_queues_device_multi_async's tuple, .wt its weights entry.
    weights: an array [T, n] of any of the three dtypes (a torch tensor or numpy fp32), default the query's own"""

    def __init__(self, q, weights="own", dev="cuda:0"):
        torch = torch_cuda()
        self.bs = q.bs
        if q.bs == 0:
            self.keep, self.tup, self.wt = (), (0, 0, 0, 0, 0, 0, 0, -1), None
            return
        ids = torch.from_numpy(q.ids).to(dev) if q.n else torch.zeros((q.ids.shape[0], 1), dtype=torch.int64, device=dev)
        lengths, dense = torch.from_numpy(q.lengths).to(dev), torch.from_numpy(q.dense).to(dev)
        w = q.w if isinstance(weights, str) else weights
        if w is not None and not isinstance(w, torch.Tensor):
            w = torch.from_numpy(np.ascontiguousarray(w))
        if w is not None:
            w = w.to(dev)
            if q.n == 0:
                w = torch.zeros((q.ids.shape[0], 1), dtype=w.dtype, device=dev)
        self.keep = (ids, lengths, dense, w)
        self.tup = (q.bs, dense.data_ptr(), ids.data_ptr(), ids.stride(0), q.n, lengths.data_ptr(), lengths.stride(0), q.fixed_len)
        code = None if w is None else {torch.float32: N.WEIGHT_FP32, torch.float16: N.WEIGHT_FP16, torch.bfloat16: N.WEIGHT_BF16}[w.dtype]
        self.wt = None if w is None else (w.data_ptr(), w.stride(0), code)


def split_rows(eng, sizes, slot):
    """the interaction rows of the set on `slot`, per query (64-row blocks per query; the pad rows are not compared)"""
    vrows = sum((n + 63) // 64 * 64 for n in sizes)
    R = eng.fetch_interaction(vrows, slot=slot) if vrows else np.zeros((0, eng.num_int), np.float32)
    rows, v = [], 0
    for n in sizes:
        rows.append(R[v:v + n].copy())
        v += (n + 63) // 64 * 64
    return rows


def split_out(out, sizes):
    outs, o = [], 0
    for n in sizes:
        outs.append(out[o:o + n].copy())
        o += n
    return outs


def run_dev(eng, ups, slot=0, form="host", weights="ups"):
    """the set through the new symbol (weights None: through the old ones) -> (outputs, interaction rows, dispatch tokens).
    form "host": results through wait; "io": the `ordered` 1 device-output form on torch's current stream -- the outputs are
    read from the device tensors (and the host floats of the same wait must equal them)"""
    torch = torch_cuda()
    sizes = [u.bs for u in ups]
    wts = [u.wt for u in ups] if isinstance(weights, str) else weights
    tups = [u.tup for u in ups]
    if form == "host":
        torch.cuda.synchronize()
        eng.run_queues_device_multi_async(tups, slot=slot, weights=wts)
        outs = split_out(eng.wait(slot, sum(sizes)), sizes)
    else:
        dst = [torch.full((max(n, 1), eng.n_out), -77.25, device="cuda:0") for n in sizes]
        stream = torch.cuda.current_stream()
        eng.run_queues_device_io_multi_async(tups, [(d.data_ptr() if n else 0, eng.n_out) for d, n in zip(dst, sizes)],
                                             stream=stream.cuda_stream, slot=slot, weights=wts)
        outs = [d[:n].cpu().numpy() for d, n in zip(dst, sizes)]          # (on the same stream, behind the set: no host wait before it)
        host = split_out(eng.wait(slot, sum(sizes)), sizes)
        assert all(same_bits(a, b) for a, b in zip(outs, host)), "device tensors differ from the host floats of the same wait"
    return outs, split_rows(eng, sizes, slot), eng.last_dispatch(slot)


def run_staged(eng, jobs, slot=1):
    eng.forward_multi_async(slot, [b for b, _ in jobs], [n for _, n in jobs])
    sizes = [n for _, n in jobs]
    outs = split_out(eng.wait(slot, sum(sizes)), sizes)
    return outs, split_rows(eng, sizes, slot), eng.last_dispatch(slot)


def all_same(a, b):
    return len(a) == len(b) and all(same_bits(x, y) for x, y in zip(a, b))


def gather_tokens(log):
    return [t for t in log if t.startswith("sls_")]


# ------------------------------------------------------------------------------------------------------------------------
# 1. weighted device sets against both references
SIZES = (B, 1, 33, 0)


@pytest.mark.parametrize("kind", ["fp32", "fp16", "int8"])
@pytest.mark.parametrize("D", [10, 32, 64])
@pytest.mark.parametrize("L", [1, 2, 20, "ragged"])
def test_weighted_device_sets_against_the_fma_chain_and_the_staged_route(kind, D, L):
    rng = np.random.RandomState(D * 13 + (5 if L == "ragged" else L))
    tables = [rng.uniform(-1, 1, (r, D)).astype(np.float32) for r in ROWS]
    stored = [_stored(kind, W) for W in tables]
    qs = [Q(rng, n, L) for n in SIZES]
    ref = [np.concatenate([_ref(stored[t], q.ids[t], q.lengths[t], q.w[t]) for t in range(T)], axis=1) if q.bs else None for q in qs]
    eng = _engine(ROWS, D, 20 if L == "ragged" else L, B, kind, slots=2, staged=3)
    try:
        _load(eng, 11, tables, D, T)
        eng.set_option("dispatch_log", 1)
        for b in range(3):
            qs[b].stage(eng, b)
        ups = [Up(q) for q in qs]
        singles = [([ups[k]], [(k, SIZES[k])]) for k in range(3)]
        set16 = ([ups[k % 4] for k in range(16)], [((k % 4) % 3, SIZES[k % 4]) for k in range(16)])
        for exact, wflat in ((1, 0), (0, 0), (0, 1)):
            eng.set_option("sls_exact", exact)
            eng.set_option("sls_weighted_flat", wflat)
            for us, jobs in singles + [set16]:
                so, sr, slog = run_staged(eng, jobs)
                for form in ("host", "io"):
                    where = (kind, D, L, exact, wflat, len(us), form)
                    do, dr, dlog = run_dev(eng, us, form=form)
                    assert all_same(do, so) and all_same(dr, sr), where        # the staged route: bit for bit
                    assert dlog[0].startswith("input_pass[") and dlog[0].endswith(",w]"), (where, dlog)
                    assert gather_tokens(dlog) == gather_tokens(slog) and all(",w>" in t or "<w>" in t for t in gather_tokens(dlog)), (where, dlog, slog)
                    if exact:
                        for u, rows, (b, n) in zip(us, dr, jobs):
                            if n:
                                assert same_bits(rows[:, D:], ref[SIZES.index(n)]), where   # the fma chain, bit for bit
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------------------------------
# 2. weight dtypes
@pytest.mark.parametrize("L", [20, "ragged"])
def test_half_weights_are_their_fp32_upcast_and_ones_and_null_are_the_unweighted_call(L):
    torch = torch_cuda()
    D = 32
    rng = np.random.RandomState(77)
    tables = [rng.uniform(-1, 1, (r, D)).astype(np.float32) for r in ROWS]
    qs = [Q(rng, n, L) for n in (B, 33, 1)]
    eng = _engine(ROWS, D, 20, B, "fp32", slots=2, staged=1)
    try:
        _load(eng, 11, tables, D, T)
        eng.set_option("dispatch_log", 1)
        plain = [Up(q, weights=None) for q in qs]
        for exact in (1, 0):
            eng.set_option("sls_exact", exact)
            for dt in (torch.float16, torch.bfloat16):
                half = [torch.from_numpy(q.w).to(dt) for q in qs]
                assert any((h.to(torch.float32).numpy() != q.w).any() for h, q in zip(half, qs))        # (the rounding is visible)
                got = run_dev(eng, [Up(q, h) for q, h in zip(qs, half)])
                want = run_dev(eng, [Up(q, h.to(torch.float32)) for q, h in zip(qs, half)])
                assert all_same(got[0], want[0]) and all_same(got[1], want[1]), (L, exact, dt)
                assert got[2] == want[2]
        # weights of 1.0 in every dtype: the unweighted call's bits (the sequential order: the weighted set takes the ring walk)
        eng.set_option("sls_exact", 1)
        un = run_dev(eng, plain, weights=None)
        assert not any(",w" in t for t in un[2])
        for dt in (torch.float32, torch.float16, torch.bfloat16):
            got = run_dev(eng, [Up(q, torch.ones((T, q.n), dtype=dt)) for q in qs])
            assert all_same(got[0], un[0]) and all_same(got[1], un[1]), (L, dt)
            assert any(",w>" in t for t in got[2])
        # all-NULL weights through the new symbol: the unweighted call -- its bits and its dispatch log, under the defaults too
        for exact in (1, 0):
            eng.set_option("sls_exact", exact)
            for form in ("host", "io"):
                un = run_dev(eng, plain, form=form, weights=None)
                got = run_dev(eng, plain, form=form, weights=[None] * len(plain))
                assert all_same(got[0], un[0]) and all_same(got[1], un[1]) and got[2] == un[2], (L, exact, form, got[2], un[2])
                assert not any(",w" in t for t in got[2])
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------------------------------
# 3. source alignment and chunk edges
@pytest.mark.parametrize("n", [0, 1, 3, 4, 5, CHUNK - 1, CHUNK, CHUNK + 1])
def test_every_source_alignment_at_every_chunk_edge(n):
    """One query of three bags per table, the middle one holding all n indices; cap = 17 x 241 = 4097 floats: odd, so the
    destination rows of the weight block start at every 4-byte misalignment, and just above the weight chunk.  The weights
    are column slices of wider tensors with odd row strides, starting at each of the 4 (fp32) and 8 (fp16) element offsets
    inside a 16-byte line; their values are k / 1024, exact in fp16, so all twelve queries of the set must give the bits of
    ONE reference."""
    torch = torch_cuda()
    D, bs = 32, 3
    rng = np.random.RandomState(n + 1)
    tables = [rng.uniform(-1, 1, (r, D)).astype(np.float32) for r in ROWS]
    eng = _engine(ROWS, D, 241, 17, "fp32", slots=1, staged=1)
    try:
        assert eng.max_batch * eng.max_lookups == CHUNK + 1
        _load(eng, 11, tables, D, T)
        eng.set_option("dispatch_log", 1)
        eng.set_option("sls_exact", 1)
        q = Q(rng, bs, 1)
        q.n, q.fixed_len = n, -1
        q.lengths = np.zeros((T, bs), np.int32)
        q.lengths[:, 1] = n
        q.ids = np.stack([rng.randint(0, ROWS[t], size=n) for t in range(T)]).astype(np.int64).reshape(T, n)
        q.w = (rng.randint(0, 1024, size=(T, n)) / 1024.0).astype(np.float32)
        ref = np.concatenate([_ref(tables[t], q.ids[t], q.lengths[t], q.w[t]) for t in range(T)], axis=1)
        base = Up(q, weights=None)
        width = n + 9 if n % 2 == 0 else n + 10                      # an odd row stride
        assert width % 2 == 1
        ups, keep, wts = [], [], []
        for dt, size, code in ((torch.float32, 4, N.WEIGHT_FP32), (torch.float16, 2, N.WEIGHT_FP16)):
            for off in range(16 // size):
                wide = torch.full((T, width), float("nan"), dtype=dt, device="cuda:0")
                lead = (-(wide.data_ptr() // size) + off) % (16 // size)                       # the slice starts `off` elements into a line
                wide[:, lead:lead + n] = torch.from_numpy(q.w).to(dt).to("cuda:0")
                ptr = wide.data_ptr() + lead * size
                assert ptr % 16 == off * size and lead + n <= width
                keep.append(wide)
                wts.append((ptr, width, code))
                ups.append(base)
        got = run_dev(eng, ups, weights=wts)
        assert got[2][0].endswith(",w]")
        for k, rows in enumerate(got[1]):
            assert same_bits(rows[:, D:], ref), (n, k)
        for form in ("io",):
            again = run_dev(eng, ups, form=form, weights=wts)
            assert all_same(again[1], got[1]) and all_same(again[0], got[0])
        torch.cuda.synchronize()
        for wide in keep:                                             # read, never written: the NaN around the slices is still there
            assert int(torch.isnan(wide.to(torch.float32)).sum()) == T * (width - n)
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------------------------------
# 4. mixed sets
@pytest.mark.parametrize("D,Tn,L", [(64, 3, 20), (64, 3, 1), (32, 4, 10), (10, 3, 5)])
def test_weighted_and_unweighted_queries_alternate_in_one_set(D, Tn, L):
    """Even queries weighted, odd ones unweighted.  The unweighted ones keep the bits they have in an all-unweighted set of
    the same form (tests/test_sls_weights.py's rule) -- under "sls_exact" 1, and under "sls_weighted_flat" 1, where the mixed
    set takes the unweighted set's own form with `w` (tests/gather_shapes.expected_gather_form)."""
    rows = [1501 + 13 * t for t in range(Tn)]
    rng = np.random.RandomState(D + L)
    tables = [rng.uniform(-1, 1, (r, D)).astype(np.float32) for r in rows]
    sizes = (B, 5, 33, 1, 17, B)
    qs = [Q(rng, n, L, rows=rows, n_tables=Tn) for n in sizes]
    eng = _engine(rows, D, L, B, "fp32", slots=2, staged=1)
    try:
        _load(eng, 11, tables, D, Tn)
        eng.set_option("dispatch_log", 1)
        eng.set_option("sls_nt", 0)
        ups = [Up(q, "own" if k % 2 == 0 else None) for k, q in enumerate(qs)]
        plain = [Up(q, None) for q in qs]
        form = expected_form((D, Tn, L, {}), sizes)
        for exact, wflat in ((1, 0), (0, 1)):
            eng.set_option("sls_exact", exact)
            eng.set_option("sls_weighted_flat", wflat)
            un = run_dev(eng, plain, weights=None)
            assert not any(",w" in t or "<w>" in t for t in un[2]), un[2]
            for how in ("host", "io"):
                mixed = run_dev(eng, ups, form=how)
                assert mixed[2][0].endswith(",w]") and all(",w>" in t or "<w>" in t for t in gather_tokens(mixed[2])), mixed[2]
                for k in range(1, len(qs), 2):
                    assert same_bits(mixed[0][k], un[0][k]) and same_bits(mixed[1][k], un[1][k]), (D, L, exact, how, k)
                for k in range(0, len(qs), 2):
                    assert not same_bits(mixed[1][k][:, D:], un[1][k][:, D:]), (D, L, exact, how, k)      # (the weights did something)
                if not exact and form != "any":
                    assert form.split()[0] in ("flatc", "flat", "one"), form
                    want, plain_tok = log_token(form, 0), log_token(form, 0, weighted=False)
                    assert any(t.startswith(want) for t in mixed[2]), (want, mixed[2])
                    assert any(t.startswith(plain_tok) for t in un[2]), (plain_tok, un[2])
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------------------------------
# 5. no stale weights
def test_a_slot_that_served_weights_serves_the_next_unweighted_set_of_every_path_with_fresh_bits():
    D, L = 32, 20
    rng = np.random.RandomState(5)
    tables = [rng.uniform(-1, 1, (r, D)).astype(np.float32) for r in ROWS]
    qs = [Q(rng, n, L) for n in (B, 33, 7)]
    jobs = [(b, q.bs) for b, q in enumerate(qs)]

    def host_set(e):
        e.run_queues_multi_async([(q.dense, q.ids, q.lengths, q.bs) for q in qs], slot=0)
        sizes = [q.bs for q in qs]
        return split_out(e.wait(0, sum(sizes)), sizes), split_rows(e, sizes, 0)

    def build():
        e = _engine(ROWS, D, L, B, "fp32", slots=1, staged=3)
        _load(e, 11, tables, D, T)
        for b, q in enumerate(qs):
            q.stage(e, b, weights=False)
        return e
    fresh = build()
    try:
        want_host = host_set(fresh)
        want_staged = run_staged(fresh, jobs, slot=0)[:2]
        want_dev = run_dev(fresh, [Up(q, None) for q in qs], weights=None)[:2]
    finally:
        fresh.close()
    eng = build()
    try:
        eng.set_option("dispatch_log", 1)
        weighted, plain = [Up(q) for q in qs], [Up(q, None) for q in qs]
        for name, run, want in (("host", lambda: host_set(eng), want_host),
                                ("staged", lambda: run_staged(eng, jobs, slot=0)[:2], want_staged),
                                ("device", lambda: run_dev(eng, plain, weights=None)[:2], want_dev),
                                ("device, all NULL", lambda: run_dev(eng, plain, weights=[None] * 3)[:2], want_dev)):
            w = run_dev(eng, weighted)
            assert w[2][0].endswith(",w]") and not all_same(w[1], want_dev[1])
            got = run()
            assert all_same(got[0], want[0]) and all_same(got[1], want[1]), name
            assert not any(",w" in t or "<w>" in t for t in eng.last_dispatch(0)), (name, eng.last_dispatch(0))
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------------------------------
# 6. refusals
def call_weighted(eng, tups, wp, stride, dtype, outs=None, stream=None, ordered=0, slot=0, null_w=False, null_stride=False):
    """the symbol itself, with every argument open to a refusal case"""
    args, keep = eng._device_set(tups)
    n = len(tups)
    wpa = (N.C.c_void_p * max(n, 1))(*[p or None for p in wp])
    st = np.asarray(stride, dtype=np.int64)
    dt = None if dtype is None else np.asarray(dtype, dtype=np.int32)
    op, ost = None, None
    if outs is not None:
        op = (N.C.c_void_p * max(n, 1))(*[p or None for p, _ in outs])
        ost = np.asarray([s for _, s in outs], dtype=np.int64)
    eng._check(N.lib().drs_run_queues_device_weighted_multi_async(
        eng._h, slot, *(args + [N.C.POINTER(N.C.c_void_p)() if null_w else wpa, None if null_stride else st.ctypes.data_as(N._i64p),
                                None if dt is None else dt.ctypes.data_as(N._i32p), op,
                                None if ost is None else ost.ctypes.data_as(N._i64p), stream, ordered])),
        "drs_run_queues_device_weighted_multi_async")
    del keep


def hip_runtime_path():
    with open("/proc/self/maps") as f:
        paths = sorted({line.split()[-1] for line in f if "libamdhip64" in line})
    assert paths, "the HIP runtime is loaded once the library is"
    return paths[0]


def test_every_refusal_is_synchronous_and_leaves_the_slot_free():
    torch = torch_cuda()
    D, L = 32, 4
    rng = np.random.RandomState(9)
    tables = [rng.uniform(-1, 1, (r, D)).astype(np.float32) for r in ROWS]
    q = Q(rng, 33, L)
    eng = _engine(ROWS, D, L, B, "fp32", slots=2, staged=1)
    try:
        _load(eng, 11, tables, D, T)
        u = Up(q)
        want = run_dev(eng, [u])
        w = u.keep[3]
        ptr, stride, _ = u.wt
        n = q.n
        pinned = torch.from_numpy(q.w).pin_memory()
        assert pinned.is_pinned() and pinned.device.type == "cpu"
        empty = Up(Q(rng, 0, L))
        cases = [
            ("null weight table", N.ERR_BAD_ARG, dict(null_w=True)),
            ("null stride table", N.ERR_BAD_ARG, dict(null_stride=True)),
            ("dtype 3", N.ERR_BAD_ARG, dict(dtype=[3])),
            ("dtype -1", N.ERR_BAD_ARG, dict(dtype=[-1])),
            ("dtype 8", N.ERR_BAD_ARG, dict(dtype=[8])),
            ("negative stride", N.ERR_BAD_ARG, dict(stride=[-1])),
            ("stride 2^62", N.ERR_BAD_ARG, dict(stride=[2 ** 62])),
            ("fp32 pointer 2 bytes in", N.ERR_BAD_ARG, dict(wp=[ptr + 2])),
            ("fp16 pointer 1 byte in", N.ERR_BAD_ARG, dict(wp=[ptr + 1], dtype=[1])),
            ("pinned host memory", N.ERR_BAD_ARG, dict(wp=[pinned.data_ptr()])),
            ("extent past the allocation's end: the stride", N.ERR_BAD_ARG, dict(stride=[1 << 40])),
            ("ordered 1 without d_out", N.ERR_BAD_ARG, dict(ordered=1)),
            ("ordered 2 with d_out", N.ERR_BAD_ARG, dict(ordered=2, outs=True)),
        ]
        out = torch.zeros((q.bs, eng.n_out), device="cuda:0")
        for name, code, kw in cases:
            kw = dict(dict(wp=[ptr], stride=[stride], dtype=[0]), **kw)
            if kw.get("outs") is True:
                kw["outs"] = [(out.data_ptr(), eng.n_out)]
            with pytest.raises(N.DrsError) as err:
                call_weighted(eng, [u.tup], **kw)
            assert err.value.code == code, (name, str(err.value))
            assert eng.wait(0) is None, name                                  # nothing in flight on the slot
        # an empty query's weight pointer is checked too
        with pytest.raises(N.DrsError) as err:
            call_weighted(eng, [empty.tup], [pinned.data_ptr()], [0], [0])
        assert err.value.code == N.ERR_BAD_ARG
        # managed memory, and another device where there is one
        managed = N.C.c_void_p()
        hip = N.C.CDLL(hip_runtime_path())                                    # (the runtime the process has loaded already)
        assert hip.hipMallocManaged(N.C.byref(managed), N.C.c_size_t(4 * T * n), 1) == 0 and managed.value
        try:
            with pytest.raises(N.DrsError) as err:
                call_weighted(eng, [u.tup], [managed.value], [n], [0])
            assert err.value.code == N.ERR_BAD_ARG and "managed" in str(err.value), str(err.value)
        finally:
            hip.hipFree(managed)
        if torch.cuda.device_count() > 1:
            other = torch.from_numpy(q.w).to("cuda:1")
            with pytest.raises(N.DrsError) as err:
                call_weighted(eng, [u.tup], [other.data_ptr()], [n], [0])
            assert err.value.code == N.ERR_BAD_ARG
        assert eng.wait(0) is None
        # nothing changed: the same set, the same bits; a NULL wgt_dtype table means fp32
        call_weighted(eng, [u.tup], [ptr], [stride], None)
        got = split_out(eng.wait(0, q.bs), [q.bs])
        assert all_same(got, want[0])
        # "sls_pool" 1: there is no weighted mean; unweighted entries through the new symbol are still served
        eng.set_option("sls_pool", 1)
        with pytest.raises(N.DrsError) as err:
            run_dev(eng, [u])
        assert err.value.code == N.ERR_UNSUPPORTED and "sls_pool" in str(err.value)
        assert eng.wait(0) is None
        run_dev(eng, [Up(q, None)], weights=[None])
        eng.set_option("sls_pool", 0)
        again = run_dev(eng, [u])
        assert all_same(again[0], want[0]) and all_same(again[1], want[1])
        del w
    finally:
        eng.close()


@pytest.mark.parametrize("case", ["din_mini", "dien_mini"])
def test_din_and_dien_refuse_device_weights_and_keep_serving_the_same_bits(case):
    torch = torch_cuda()
    from tests import test_device_inputs as DI
    meta, z = H.load_fixture(case)
    args = H.args_from(meta["args"], accel_slots=2)
    net, lX, lS_l, lS_i, lT = H.materialize(args)
    net.create(lX[0], lS_l[0], lS_i[0], lT[0])
    e = net.engine
    try:
        qs = DI.model_queries(e, lX, lS_l, lS_i, int(args.num_indices_per_lookup), promise=True)
        ups = [DI.upload(q) for q in qs]
        torch.cuda.synchronize()
        e.run_queues_device_multi_async([u[1] for u in ups], slot=1)
        before = e.wait(1, sum(q.bs for q in qs))
        ones = [torch.ones(q.ids.shape, device="cuda:0") for q in qs]
        torch.cuda.synchronize()
        with pytest.raises(N.DrsError) as err:
            e.run_queues_device_multi_async([u[1] for u in ups], slot=1, weights=[(w.data_ptr(), w.stride(0), 0) for w in ones])
        assert err.value.code == N.ERR_UNSUPPORTED and "plain sum" in str(err.value)
        assert e.wait(1) is None
        e.run_queues_device_multi_async([u[1] for u in ups], slot=1, weights=[None] * len(ups))     # no weights: served
        assert same_bits(e.wait(1, sum(q.bs for q in qs)), before)
    finally:
        e.close()


# ------------------------------------------------------------------------------------------------------------------------
# 7. bad indices in a weighted set
def test_a_weighted_set_with_a_bad_index_reports_it_answers_nan_and_the_slot_serves_the_next_set():
    torch = torch_cuda()
    D, L = 32, 4
    rng = np.random.RandomState(3)
    tables = [rng.uniform(-1, 1, (r, D)).astype(np.float32) for r in ROWS]
    good = [Q(rng, n, L) for n in (33, 5)]
    bad = Q(rng, 33, L)
    bad.ids = bad.ids.copy()
    bad.ids[1, 7] = ROWS[1]                                          # one past the last row of table 1
    eng = _engine(ROWS, D, L, B, "fp32", slots=1, staged=1)
    try:
        _load(eng, 11, tables, D, T)
        gu = [Up(q) for q in good]
        want = run_dev(eng, gu)
        us = [gu[0], Up(bad), gu[1]]
        sizes = [u.bs for u in us]
        dst = [torch.full((n, eng.n_out), -77.25, device="cuda:0") for n in sizes]
        eng.run_queues_device_io_multi_async([u.tup for u in us], [(d.data_ptr(), eng.n_out) for d in dst],
                                             stream=torch.cuda.current_stream().cuda_stream, slot=0, weights=[u.wt for u in us])
        seen = [d.cpu().numpy() for d in dst]
        with pytest.raises(N.DrsError) as err:
            eng.wait(0, sum(sizes))
        assert err.value.code == N.ERR_INDEX_RANGE, str(err.value)
        assert all((s.view(np.uint32) == NAN_BITS).all() for s in seen)
        # the same through the host-output form: the wait reports it
        torch.cuda.synchronize()
        eng.run_queues_device_multi_async([u.tup for u in us], slot=0, weights=[u.wt for u in us])
        with pytest.raises(N.DrsError) as err:
            eng.wait(0, sum(sizes))
        assert err.value.code == N.ERR_INDEX_RANGE
        for form in ("io", "host"):
            again = run_dev(eng, gu, form=form)
            assert all_same(again[0], want[0]) and all_same(again[1], want[1]), form
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------------------------------
# 8. the wrapper, on the four model kinds that take weights
@pytest.mark.parametrize("case", ["dlrm_dot_small", "wnd_mini", "ncf_mini", "mtwnd_mini"])
def test_the_wrapper_serves_weighted_requests_with_the_scores_of_the_staged_route(case):
    torch = torch_cuda()
    from deeprecsys_amd import dlrm_s_hip as M
    meta, z = H.load_fixture(case)
    args = H.args_from(meta["args"], accel_slots=2)
    np.random.seed(args.numpy_rand_seed)
    net, lX, lS_l, lS_i, lT = H.materialize(args)
    w = [cls for cls in M.WRAPPERS.values() if cls.net_cls is type(net)][0](args)
    w.create(lX[0], lS_l[0], lS_i[0], lT[0])
    e = w.net.engine
    try:
        L = int(args.num_indices_per_lookup)
        nb = min(len(lS_l), 3)
        n = len(lS_l[0][0])
        rs = np.random.RandomState(1)
        wts = [[rs.uniform(0, 1, size=len(i)).astype(np.float32) for i in lS_i[k]] for k in range(nb)]
        w.net.stage_batches(lX, lS_l[:nb], lS_i[:nb], lS_w=wts)
        sizes = [max(1, n - 2 * k) for k in range(nb)]
        for exact in (1, 0):
            e.set_option("sls_exact", exact)
            e.forward_multi_async(1, list(range(nb)), sizes)
            want = split_out(e.wait(1, sum(sizes)), sizes)
            dev = "cuda:%d" % e.device
            reqs = []
            for k, bs in enumerate(sizes):
                ids = np.ascontiguousarray(np.stack([np.asarray(i, dtype=np.int64) for i in lS_i[k]])[:, :bs * L])
                lengths = np.ascontiguousarray(np.stack([np.asarray(l, dtype=np.int32) for l in lS_l[k]])[:, :bs])
                assert int(lengths.sum(axis=1).max()) == bs * L == int(lengths.sum(axis=1).min())
                fc = None if lX is None or not e.m_den else torch.as_tensor(np.ascontiguousarray(np.asarray(lX[k], dtype=np.float32)[:bs]), device=dev)
                fl = int(lengths[0, 0]) if (lengths == lengths[0, 0]).all() else -1
                wide = torch.zeros((e.T, bs * L + 3), device=dev)
                wide[:, 1:1 + bs * L] = torch.as_tensor(np.stack(wts[k])[:, :bs * L], device=dev)
                reqs.append((torch.as_tensor(ids, device=dev), torch.as_tensor(lengths, device=dev), fc, bs, fl, wide[:, 1:1 + bs * L]))
            got = w.run_queues_device_multi(reqs, slot=0)
            assert all_same(got, want), (case, exact)
            outs = w.run_queues_device_io_multi(reqs, slot=0)
            w.finish_device(slot=0)
            assert all_same([o.cpu().numpy() for o in outs], want), (case, exact)
            # half weights go down as they are: the scores of their upcast
            half = [r[:5] + (r[5].to(torch.float16),) for r in reqs]
            up = [r[:5] + (r[5].to(torch.float16).to(torch.float32),) for r in reqs]
            assert all_same(w.run_queues_device_multi(half, slot=0), w.run_queues_device_multi(up, slot=0)), (case, exact)
    finally:
        e.close()
