"""Launch sets whose arrays are device arrays (include/drs_device_inputs.h): the catalogue of sets the CPU and GPU tests
share, the base engine they run on, and a numpy restatement of the device input pass (deeprecsys_amd/csrc/input_pass.hip).

A query is a Q: bs, ids [T, n] int64, lengths [T, bs] int32, dense [bs, M_DEN] float32, fixed_len (the promise handed to the
device path; the host path takes no promise, it looks at the lengths).  GOOD: name -> list of Q, every one valid.  BAD: name ->
(list of Q, code the device path ends in, code the host path gives the same arrays).  Each bad set carries exactly one kind of
error, so the device path's precedence (lengths before indices) never decides."""
import collections

import numpy as np

from deeprecsys_amd import _native as N

ROWS = [50, 1000, 7]
T, D, M_DEN = 3, 16, 8
LN_BOT, LN_TOP = [M_DEN, D], [D + T * D, 4, 1]
MAX_BATCH, MAX_LOOKUPS, SLOTS = 600, 8, 2
CAP = MAX_BATCH * MAX_LOOKUPS

Q = collections.namedtuple("Q", "bs ids lengths dense fixed_len")


def make_engine(table_dtype=0, **options):
    """the base engine: DLRM cat, T 3, rows [50, 1000, 7], D 16, bottom [8, 16], top [64, 4, 1], max_batch 600, max_lookups
    8, 2 slots -- with whatever library deeprecsys_amd._native has bound"""
    rng = np.random.RandomState(11)
    eng = N.Engine(N.MODEL_DLRM, ROWS, D, LN_BOT, LN_TOP, N.INTERACT_CAT, sigmoid_top=2, max_batch=MAX_BATCH,
                   max_lookups=MAX_LOOKUPS, num_staged_batches=1, num_slots=SLOTS)
    try:
        if table_dtype:
            eng.set_option("table_dtype", table_dtype)
        for k, v in options.items():
            eng.set_option(k, v)
        for t, r in enumerate(ROWS):
            eng.set_table(t, rng.uniform(-1, 1, (r, D)).astype(np.float32))
        for which, ln in ((N.MLP_BOT, LN_BOT), (N.MLP_TOP, LN_TOP)):
            for l in range(len(ln) - 1):
                eng.set_fc(which, l, rng.normal(0, 1.0 / np.sqrt(ln[l]), (ln[l + 1], ln[l])).astype(np.float32),
                           rng.normal(0, 0.1, ln[l + 1]).astype(np.float32))
    except Exception:
        eng.close()
        raise
    return eng


def ragged(rng, bs, total):
    """bs bag lengths summing to `total`: zeros among them, an empty first and last bag where there is room"""
    p = rng.uniform(0, 1, bs) * (rng.uniform(0, 1, bs) < 0.7)
    if bs >= 3:
        p[0] = p[-1] = 0.0
    if p.sum() == 0:
        p[bs // 2] = 1.0
    return rng.multinomial(total, p / p.sum()).astype(np.int32)


def query(seed, bs, total=None, fixed_len=-1):
    """a valid query: `total` indices per table in ragged bags, or fixed_len >= 0: every bag that long (and promised)"""
    rng = np.random.RandomState(seed)
    if fixed_len >= 0:
        total = bs * fixed_len
        lengths = np.full((T, bs), fixed_len, np.int32)
    else:
        lengths = np.stack([ragged(rng, bs, total) for _ in range(T)]) if bs else np.zeros((T, 0), np.int32)
    ids = np.stack([rng.randint(0, ROWS[t], size=total).astype(np.int64) for t in range(T)])
    return Q(bs, ids, lengths, rng.uniform(-1, 1, (bs, M_DEN)).astype(np.float32), fixed_len)


def host_uniform(q):
    """what the host path finds by looking at the lengths: the one length every bag of every table has, else -1"""
    if q.bs == 0 or not np.all(q.lengths == q.lengths[0, 0]):
        return -1
    return int(q.lengths[0, 0])


def same_forms(qs):
    """the device path's promises are what the host path detects: both choose the same launch forms (else compare under
    "sls_exact" 1, where every form sums in the sequential order)"""
    return all(q.bs == 0 or q.fixed_len == host_uniform(q) for q in qs)


# bs: the scan crosses a wave (63 / 64 / 65), a workgroup chunk (255 / 256 / 257), ends ragged (600 = 2 * 256 + 88).
# per-table totals: two int64 per 16-byte load (0, 1, 3, 4, 5), the workgroup's last load round (255 / 256 / 257 pairs and
# indices), one narrowing workgroup's 2048 indices and the next (1023 / 1024 / 1025 are inside one; CAP = 4800 needs three)
SINGLES = [(1, 0), (1, 1), (63, 3), (64, 4), (65, 5), (255, 255), (256, 256), (257, 257), (600, 1023), (63, 1024), (65, 1025),
           (256, 2047), (257, 2049), (600, CAP), (255, CAP)]
FIXED = [(65, 1), (257, 2), (600, 8), (64, 8), (1, 8)]


def _good():
    g = collections.OrderedDict()
    for k, (bs, total) in enumerate(SINGLES):
        g["ragged_bs%d_n%d" % (bs, total)] = [query(100 + k, bs, total)]
    for k, (bs, L) in enumerate(FIXED):
        g["fixed_bs%d_L%d" % (bs, L)] = [query(200 + k, bs, fixed_len=L)]
        g["unpromised_bs%d_L%d" % (bs, L)] = [query(200 + k, bs, fixed_len=L)._replace(fixed_len=-1)]
    g["set_of_2"] = [query(300, 65, 257), query(301, 256, 1025)]
    g["set_of_16"] = [query(310 + i, (1, 63, 64, 65, 255, 256, 257, 600)[i % 8], (5, 255, 256, 257, 1023, 1024, 1025, CAP)[i % 8])
                      for i in range(16)]
    g["empty_first_and_middle"] = [query(330, 0, 0), query(331, 65, 257), query(332, 0, 0), query(333, 64, 256)]
    # rule 6 of DESIGN 3.2: one ragged query makes the set ragged; fixed lengths that differ keep the fixed forms
    g["promises_8_8_ragged"] = [query(340, 64, fixed_len=8), query(341, 65, fixed_len=8), query(342, 63, 255)]
    g["promises_8_8_2"] = [query(343, 64, fixed_len=8), query(344, 65, fixed_len=8), query(345, 257, fixed_len=2)]
    return g


def _bad():
    b = collections.OrderedDict()

    def with_id(q, t, pos, v):
        ids = q.ids.copy()
        ids[t, pos] = v
        return q._replace(ids=ids)

    def with_len(q, t, changes):
        lengths = q.lengths.copy()
        for bag, d in changes:
            lengths[t, bag] += d
        return q._replace(lengths=lengths)

    base = query(400, 65, fixed_len=4)._replace(fixed_len=-1)        # 260 indices per table, every bag 4 long, nothing promised
    b["index_eq_rows"] = ([with_id(base, 1, 200, ROWS[1])], N.ERR_INDEX_RANGE, N.ERR_INDEX_RANGE)
    b["index_minus_one"] = ([with_id(base, 0, 0, -1)], N.ERR_INDEX_RANGE, N.ERR_INDEX_RANGE)
    b["index_2p32_plus_3"] = ([with_id(base, 2, 259, 2 ** 32 + 3)], N.ERR_INDEX_RANGE, N.ERR_INDEX_RANGE)     # narrows to row 3
    b["negative_length"] = ([with_len(base, 1, [(10, -6), (11, +6)])], N.ERR_LENGTHS_SUM, N.ERR_LENGTHS_SUM)  # 4 - 6 = -2; sum right
    b["sum_one_short"] = ([with_len(base, 2, [(64, -1)])], N.ERR_LENGTHS_SUM, N.ERR_LENGTHS_SUM)
    b["sum_one_over"] = ([with_len(base, 0, [(0, +1)])], N.ERR_LENGTHS_SUM, N.ERR_LENGTHS_SUM)
    # the sum is right, the promise is not: the host path takes no promise and serves these arrays
    b["promise_broken"] = ([with_len(base, 1, [(3, -1), (40, +1)])._replace(fixed_len=4)], N.ERR_LENGTHS_SUM, N.OK)
    b["bad_query_in_the_middle"] = ([query(410, 64, 256), with_id(base, 1, 7, 1000), query(411, 257, 1025)],
                                    N.ERR_INDEX_RANGE, N.ERR_INDEX_RANGE)
    return b


GOOD = _good()
BAD = _bad()


def poison_sets(rows, m_den, max_batch, cap, n):
    """Two host-path sets of n queries that leave every per-query block of a slot holding none of a good query's answer, so
    that a device run after them must store everything it is compared on: index rows full of each table's LAST row up to the
    staging capacity, every offset from entry 1 on equal to cap - 1 (all indices in bag 0 of max_batch bags, so the bags are
    ragged and the host path copies the offsets; a good query's tail holds its own count, which is never cap - 1 here), and
    dense rows of 77.0.  The first set (cap indices) covers the last index position, the second (cap - 1) sets the offsets."""
    assert max_batch >= 2 and cap >= 2
    out = []
    for n_p in (cap, cap - 1):
        ids = np.stack([np.full(n_p, r - 1, np.int64) for r in rows])
        lengths = np.zeros((len(rows), max_batch), np.int32)
        lengths[:, 0] = n_p
        dense = np.full((max_batch, m_den), 77.0, np.float32) if m_den else None
        out.append([(dense, ids, lengths, max_batch)] * n)
    return out


def host_args(qs):
    """the set as Engine.run_queues_multi_async takes it"""
    return [(q.dense, q.ids, q.lengths, q.bs) for q in qs]


def input_pass(ids, lengths, rows, fixed_len, max_batch=MAX_BATCH):
    """The device input pass on one query, restated: -> (int32 index rows [T, n], offsets rows [T, max_batch + 1], code).
    A bad index is stored as row 0; a negative length counts as 0; every prefix sum is clamped to n; entries bs + 1 ..
    max_batch hold the (clamped) total.  code: ERR_LENGTHS_SUM (a negative length, a sum != n, a length != a promised
    fixed_len) before ERR_INDEX_RANGE (an index outside [0, rows_t), judged on the 64-bit value), else OK."""
    ids, lengths = np.asarray(ids, np.int64), np.asarray(lengths, np.int32)
    Tn, n = ids.shape
    bs = lengths.shape[1]
    idx32 = np.zeros((Tn, n), np.int32)
    off = np.zeros((Tn, max_batch + 1), np.int32)
    bad_len = bad_idx = False
    for t in range(Tn):
        u = ids[t].view(np.uint64)
        out = u >= np.uint64(rows[t])
        bad_idx = bad_idx or bool(out.any())
        idx32[t] = np.where(out, 0, u & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.int32)
        run = 0
        for b in range(bs):
            l = int(lengths[t, b])
            if l < 0 or (fixed_len >= 0 and l != fixed_len):
                bad_len = True
            run += max(l, 0)
            if run > n:
                bad_len = True
            off[t, b + 1] = min(run, n)
        if run != n:
            bad_len = True
        off[t, bs + 1:] = min(run, n)
    return idx32, off, (N.ERR_LENGTHS_SUM if bad_len else N.ERR_INDEX_RANGE if bad_idx else N.OK)
