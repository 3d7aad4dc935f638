"""CPU side of inf and NaN table rows in DIN's and DIEN's own kernels (tests/test_din_dien_nonfinite.py runs the layout below
on the GPU).

csrc/din.hip, csrc/dien.hip and csrc/din_any.hip use the gather's tricks in code tests/test_sls_nonfinite*.py never run:
slots past a bag's end load the zero page, a lane group without a unit in a round runs unit 0's weights over the sample's
candidate ad and a select drops the result, non-live samples of the last workgroup are sample 0 again, the MFMA recurrence
clamps the unused columns of its 16-sample tile to the last sample and prefetches four steps ahead with a clamped step,
its fused top MLP multiplies LDS pad columns by zero weights.  Each is correct by a select or a zero-page load; a multiply
by a 0 / 1 mask would pass every finite test and fail on +-inf (0 * inf = NaN).

What is pinned here, without a GPU:
  1. `din_ref64` / `dien_ref64`, float64 references in plain numpy (bags by class_ref; units Concat(u, ad, u + ad) -> FC ->
     ReLU -> FC -> ReLU -> Sum; the recurrence through the Reshape, h = tanh((G h + g) + (W x + w)), two layers; ReLU as
     where(v > 0, v, 0), which maps NaN to 0 as the oracle's `v > 0 ? v : 0` does).  Their class map (0 finite, 1 +inf, 2 -inf,
     3 NaN) of the top MLP's input row and of the outputs is the C oracle's at every case.

     Why the class of an element does not depend on the order of any sum behind it -- the k-ordered chain of the oracle, the
     in-lane dot4 + butterfly of the fused DIN forms, the MFMA chains, numpy's pairwise sums: every sum here is a sum of
     products weight * value with FINITE weights, none of them zero (`assert_weights`), so a product is non-finite exactly
     when its value is, and never 0 * inf.  A sum of terms is NaN iff a term is NaN or +inf and -inf both occur, +inf (-inf)
     iff only that infinity occurs, else finite -- PROVIDED no finite partial sum overflows.  The largest finite table
     element is 1e5, a bag holds at most 5 rows, a unit's input at most 2e5 + 10; xavier weights are bounded by sqrt(3) (by
     1 on the wide layers), so no finite partial sum exceeds 256 * 2e6 << 3.4e38 in any order, nor does a float64 one.  ReLU
     and tanh map classes to classes (NaN -> 0 | NaN, +-inf -> +inf, 0 | +-1), so the argument carries through the layers.
  2. The consequences the GPU test relies on: a NaN in a unit's bag leaves the attention block finite; +-inf in a sequence
     step gives layer-1 states of exactly +-1 and finite states afterwards (tanhf(+-inf) = +-1 in the oracle; csrc/rnn_dev.h's
     tanh_rnn reaches the same value by v_exp_f32 -> inf -> v_rcp_f32 -> 0); a NaN step makes every later state of that sample
     NaN, and the outputs are then the biases-only path of the top MLP.
  3. The conditions that keep the GPU test from passing vacuously, per case.
  4. The bar for the finite elements of hot samples: tests/test_gather_boundaries.py's for the same block (imported, not
     restated), its floor taken per SAMPLE ROW over that row's finite reference elements: a 1e5 element widens nobody
     else's floor.  The C oracle against float64 stays within it at every case.
"""
import collections
import functools
import json
import os
import zlib

import numpy as np
import pytest

from tests import gather_shapes as S
from tests.test_gather_boundaries import DIEN_OUT, DIEN_ROW, DIN_OUT, DIN_OUT_EXACT, DIN_ROW
from tests.test_sls_nonfinite_cpu import N_POISON, RECIPES, class_ref, classes, close_finite, poison_rows, seq_bits_ref

DIN_CASES = ["din_32_h1", "din_64_h2", "din_32_h4", "din_s4_75", "din_s2_77", "din_L_1_2_3", "din_ragged", "din_h2_L4", "din_L_3_ragged",
             "din_T257", "din_32_U33", "din_64_U17", "din_32_h3", "din_32_h65", "din_30"]
DIEN_CASES = ["wg_16", "wg_17", "wg_shared", "wg_ragged", "dien_64_16", "dien_16_64", "dien_32_32_split0", "wg_valu_5", "wg_shared_valu",
              "dien_32_48", "dien_12_16", "top_off", "top_256", "top_28", "seq_1", "seq_2", "seq_5", "seq_3_valu"]
NAMES = DIN_CASES + DIEN_CASES
# (cases of one engine key side by side: the GPU module keeps one pair of engines per key)
ORDER = sorted(NAMES, key=lambda n: (repr(S.engine_key(S.BY_NAME[n])), NAMES.index(n)))

# the unweighted recipes of tests/test_sls_nonfinite_cpu.RECIPES (first row or None, last row), the telling ones first: a query
# of five samples holds two marked bags.  +inf and -inf in one column; a NaN element; a whole row of +inf; +inf last in the
# bag; -inf and +inf in different columns; 1e5; -inf last; +inf in the last column
_UNWEIGHTED = [(r0, r1) for r0, w0, r1, w1 in RECIPES if w0 is None and w1 is None]
UNWEIGHTED = [_UNWEIGHTED[i] for i in (3, 2, 4, 0, 6, 5, 1, 7)]
assert sorted(UNWEIGHTED, key=repr) == sorted(set(_UNWEIGHTED), key=repr) and len(UNWEIGHTED) == 8
EMPTY_AT = (2, 5, 14)            # ragged batches: these samples' bags are empty in every table (but a marked one)

Mark = collections.namedtuple("Mark", "s t role recipe k")


def report(**kw):
    path = os.environ.get("DRS_DIN_DIEN_NONFINITE_REPORT")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(kw) + "\n")


# ---- the layout -------------------------------------------------------------------------------------------------------------------
class PTables(object):
    """The tables of one engine key (what tests/test_gather_boundaries.make_engine takes): the uniform(-1, 1) rows of
    S.Tables(key), rows 0 .. 7 as drawn (`clean`) or set by poison_rows (`poisoned`: row 0 all NaN)."""

    def __init__(self, rows, W):
        self.rows, self.W = rows, W

    def table_rows(self):
        return [W.shape[0] for W in self.W]


@functools.lru_cache(maxsize=2)
def tables_of(key):
    """-> (clean, poisoned)"""
    tab = S.Tables(key)
    clean = [np.ascontiguousarray(W[:r]) for W, r in zip(tab.W, tab.rows)]
    poisoned = [poison_rows(W.copy()) for W in clean]
    for W in clean + poisoned:
        W.setflags(write=False)
    return PTables(tab.rows, clean), PTables(tab.rows, poisoned)


def lane_groups(case):
    """lane groups per workgroup of the fused DIN forms (4 waves x 64 / G lanes), None for every other form"""
    return 4 * 64 // (case.D // 4) if case.kind == "din" and S.din_class(case) == "fused" else None


def roles_of(case):
    """role -> table, in the order the marked bags rotate over; tables that coincide (U = 1; the second unit of lane group 0
    is the last one) are listed once"""
    T, U = case.T, case.T - 3
    if case.kind == "din":
        order = [("first unit", 1), ("candidate ad", T - 2), ("profile", 0), ("last unit", U), ("context", T - 1)]
        ngb = lane_groups(case)
        if ngb is not None and U > ngb:
            order.append(("second unit of a lane group", 1 + ngb))
    else:
        order = [("last unit", U), ("first unit", 1), ("candidate ad", T - 2), ("profile", 0), ("context", T - 1)]
    out = collections.OrderedDict()
    for role, t in order:
        if t not in out.values():
            out[role] = t
    return out


class Layout(object):
    """The staged batches of one case.  Batch b holds S.B_MAX samples of bag length case.L[b]; ordinary indices come from
    [8, rows); every bag beyond the largest query that reads the batch names row 0; samples b % 3, b % 3 + 3, ... are MARKED:
    one bag of each names poison rows by a recipe (its table rotates over roles_of), the two samples behind it name ordinary
    rows only.  `plain` is the same batch with every marked bag pointed back at the ordinary rows it was drawn with."""

    def __init__(self, case):
        self.case = case
        self.key = S.engine_key(case)
        self.clean, self.poisoned = tables_of(self.key)
        rows = self.clean.rows
        T = case.T
        rng = np.random.RandomState(zlib.crc32(("nonfinite " + case.name).encode()) % (1 << 31))
        self.nb = min(len(case.sizes), S.N_BATCH)
        self.jobs = [(i % self.nb, n) for i, n in enumerate(case.sizes)]
        self.need = {}
        for b, n in self.jobs:
            self.need[b] = max(self.need.get(b, 0), n)
        self.roles = roles_of(case)
        role_list = list(self.roles.items())
        self.lens, self.idx, self.plain, self.marks = [], [], [], []
        k_next = 0
        for b in range(self.nb):
            L = case.L[b]
            marks = []
            for s in range(b % 3, S.B_MAX, 3):
                k = k_next                                 # (the rotation runs on from batch to batch)
                k_next += 1 if s < self.need[b] else 0
                role, t = role_list[k % len(role_list)]
                marks.append(Mark(s, t, role, (k + k // 24) % len(UNWEIGHTED), k))
            lens = []
            for t in range(T):
                if L == S.RAGGED:
                    l = rng.randint(0, S.RAGGED_MAX + 1, S.B_MAX).astype(np.int32)
                    l[list(EMPTY_AT)] = 0
                else:
                    l = np.full(S.B_MAX, L, np.int32)
                lens.append(l)
            if L == S.RAGGED:
                for m in marks:                            # a marked bag is not empty: 2 .. 5 rows at least (5: add_tail's round)
                    lens[m.t][m.s] = max(int(lens[m.t][m.s]), 2 + m.k % 4)
            idx, plain = [], []
            n = self.need[b]
            for t in range(T):
                off = np.concatenate([[0], np.cumsum(lens[t])]).astype(np.int64)
                i_t = rng.randint(N_POISON, rows[t], int(off[-1])).astype(np.int64)
                i_t[off[n]:] = 0                           # bags beyond the query: the all-NaN row
                p_t = i_t.copy()
                for m in marks:
                    if m.t != t or m.s >= n:
                        continue
                    r0, r1 = UNWEIGHTED[m.recipe]
                    first, last = off[m.s], off[m.s + 1] - 1
                    if r0 is not None and last > first:
                        i_t[first] = r0
                    i_t[last] = r1
                idx.append(i_t)
                plain.append(p_t)
            self.lens.append(lens)
            self.idx.append(idx)
            self.plain.append(plain)
            self.marks.append([m for m in marks if m.s < n])

    def query(self, b, n, plain=False):
        """-> (idx, lens) of the first n samples of batch b"""
        src = self.plain[b] if plain else self.idx[b]
        return ([src[t][:int(self.lens[b][t][:n].sum())] for t in range(self.case.T)], [l[:n] for l in self.lens[b]])

    def named(self, b, n):
        """bool [T, n]: the bags of the query that name a poison row"""
        out = np.zeros((self.case.T, n), bool)
        for m in self.marks[b]:
            if m.s < n:
                out[m.t, m.s] = True
        return out

    # -- the hot sets, from the layout alone ------------------------------------------------------------------------------
    def hot(self, b, n):
        """-> dict of bool [n]: "passthrough" [3, n] (profile, candidate ad, context), "block" (DIN's attention block /
        DIEN's recurrent state), "out" (the union), "own" (samples whose OWN bags name a poison row)"""
        T, U = self.case.T, self.case.T - 3
        named = self.named(b, n)
        passthrough = named[[0, T - 2, T - 1]]
        if self.case.kind == "din":
            block = named[1:1 + U].any(axis=0) | named[T - 2]
        else:
            # the Reshape: step t of sample b' is embedding n' % U of sample n' // U, n' = t * n + b': the marked bag of
            # (sample s, unit u) is flat element s * U + u, which is a step of sample (s * U + u) % n
            block = np.zeros(n, bool)
            for u, s in zip(*np.nonzero(named[1:1 + U])):
                block[(s * U + u) % n] = True
        return dict(passthrough=passthrough, block=block, out=block | passthrough.any(axis=0), own=named.any(axis=0))


@functools.lru_cache(maxsize=4)
def layout(name):
    return Layout(S.BY_NAME[name])


# ---- the float64 references -------------------------------------------------------------------------------------------------------
def relu(v):
    return np.where(v > 0, v, 0.0)


def fc64(x, W, b):
    """x [n, K] . W [N, K] + b, every product formed (no library shortcut around a zero operand), float64"""
    with np.errstate(all="ignore"):
        return (x[:, None, :] * np.asarray(W, np.float64)[None]).sum(axis=2) + np.asarray(b, np.float64)


def mlp64(x, layers):
    """create_mlp with sigmoid_layer -1: every layer FC + ReLU; -> (output, the first layer's activations)"""
    first = None
    for W, b in layers:
        x = relu(fc64(x, W, b))
        first = x if first is None else first
    return x, first


def pooled64(tables, idx, lens):
    return [class_ref(W, i, l, None) for W, i, l in zip(tables, idx, lens)]


def din_ref64(w, E):
    """E: T float64 [n, D] pooled tensors -> the top MLP's input row [n, 4 D]"""
    T = len(E)
    ad = E[T - 2]
    att = np.zeros_like(ad)
    with np.errstate(all="ignore"):
        for i, unit in enumerate(w.att):
            x = np.concatenate([E[1 + i], ad, E[1 + i] + ad], axis=1)
            att = att + mlp64(x, unit)[0]
    return np.concatenate([E[0], att, ad, E[T - 1]], axis=1)


def dien_ref64(w, E, trace=None):
    """E -> the top MLP's input row [n, H + 3 D]; trace: a list that takes (layer-1 state, layer-2 state) of every step"""
    T, n = len(E), E[0].shape[0]
    U, Hh = T - 3, w.ln_bot[1]
    seq = np.stack(E[1:1 + U], axis=1).reshape(n * U, -1).reshape(U, n, -1)      # the Reshape: row-major reinterpretation
    (Wi0, bi0), (Wg0, bg0) = w.rnn[0]
    (Wi1, bi1), (Wg1, bg1) = w.rnn[1]
    h0, h1 = np.zeros((n, Hh)), np.zeros((n, Hh))
    with np.errstate(all="ignore"):
        for t in range(U):
            h0 = np.tanh(fc64(h0, Wg0, bg0) + fc64(seq[t], Wi0, bi0))
            h1 = np.tanh(fc64(h1, Wg1, bg1) + fc64(h0, Wi1, bi1))
            if trace is not None:
                trace.append((h0, h1))
    return np.concatenate([h1, E[0], E[T - 2], E[T - 1]], axis=1)


def block_columns(case):
    """the columns of the attention block / the recurrent state in the top MLP's input row"""
    return (case.D, 2 * case.D) if case.kind == "din" else (0, case.H[0])


def passthrough_columns(case):
    """(table, first column) of the profile, candidate-ad and context blocks"""
    D, T = case.D, case.T
    if case.kind == "din":
        return [(0, 0), (T - 2, 2 * D), (T - 1, 3 * D)]
    Hh = case.H[0]
    return [(0, Hh), (T - 2, Hh + D), (T - 1, Hh + 2 * D)]


def assert_weights(w):
    """finite, none zero, bounded by sqrt(3): what the docstring's order argument stands on"""
    mats = [W for W, _ in w.top]
    mats += [W for unit in (w.att or []) for W, _ in unit]
    mats += [W for layer in (w.rnn or []) for W, _ in layer]
    for W in mats:
        assert np.all(np.isfinite(W)) and np.all(W != 0) and np.abs(W).max() <= np.sqrt(3.0) + 1e-6
    for _, b in w.top:
        assert np.all(np.isfinite(b))


# ---- the bar ---------------------------------------------------------------------------------------------------------------------
def bar_fraction(got, ref, rtol, atol=0.0, atol_scale=0.0):
    """tests/helpers.close per SAMPLE ROW on the elements whose reference is finite: -> [n] the largest |got - ref| of the
    row as a fraction of atol + atol_scale max|ref_row| + rtol |ref| (0 for a row without a finite element; <= 1: inside)"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    fin = np.isfinite(ref)
    mag = np.where(fin, np.abs(ref), 0.0)
    allowed = atol + atol_scale * mag.max(axis=1, keepdims=True) + rtol * mag
    with np.errstate(all="ignore"):
        err = np.where(fin, np.abs(got - ref), 0.0)
        frac = np.where(err == 0, 0.0, err / allowed)
    frac[fin & ~np.isfinite(got)] = np.inf
    return frac.max(axis=1) if frac.shape[1] else np.zeros(len(frac))


def row_bar(case):
    return DIN_ROW if case.kind == "din" else DIEN_ROW


def out_bar(case, exact=False):
    if case.kind == "dien":
        return DIEN_OUT
    return DIN_OUT_EXACT if exact else DIN_OUT


# ---- the references of a case, computed once ---------------------------------------------------------------------------------------
_models = {}


def models_of(key):
    """-> (weights, oracle model on the clean tables, oracle model on the poisoned ones) of an engine key"""
    if key not in _models:
        _models.clear()
        clean, poisoned = tables_of(key)
        w = S.Weights(key)
        if key[0] == "din":
            # unit 0's first layer weighs columns 1 and D - 1 of the candidate ad and of the Sum positively (the magnitudes stay
            # as drawn): a lane group without a unit in the last round applies unit 0 to (0, ad, ad), and with +inf in one of
            # those columns of the ad the result it drops is +inf, not NaN
            D = key[1]
            W1 = w.att[0][0][0]
            for c in (D + 1, 2 * D - 1, 2 * D + 1, 3 * D - 1):
                W1[:, c] = np.abs(W1[:, c])
        _models[key] = (w, w.oracle_model(clean.W), w.oracle_model(poisoned.W))
    return _models[key]


@functools.lru_cache(maxsize=4)
def references(name):
    """{(batch, n): dict} for every query of the case: R64 / out64 (float64, poisoned tables), R64_clean / out64_clean,
    R_orc / out_orc, R_orc_clean / out_orc_clean (the C oracle), seq [3] (the sequential chain's bits of the pass-through
    bags), E64 (the pooled tensors), hot (the hot sets)"""
    lay = layout(name)
    case = lay.case
    w, om_c, om_p = models_of(lay.key)
    ref64 = din_ref64 if case.kind == "din" else dien_ref64
    out = {}
    for b, n in sorted(set(lay.jobs)):
        if n == 0:
            continue
        idx, lens = lay.query(b, n)
        r = dict(hot=lay.hot(b, n))
        for tag, tabs, om in (("", lay.poisoned, om_p), ("_clean", lay.clean, om_c)):
            E = pooled64(tabs.W, idx, lens)
            R64 = ref64(w, E)
            r["R64" + tag], r["out64" + tag] = R64, mlp64(R64, w.top)[0]
            r["out_orc" + tag], r["R_orc" + tag] = om.forward(None, idx, lens, bs=n, want_R=True)
            if not tag:
                r["E64"] = E
        r["seq"] = [seq_bits_ref(lay.poisoned.W[t], idx[t], lens[t], None) for t, _ in passthrough_columns(case)]
        for a in r.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        out[(b, n)] = r
    return out


def set_numbering(lay):
    """the launch set's samples in the kernels' numbering (the live queries back to back): -> [(query, sample)]"""
    return [(i, s) for i, (b, n) in enumerate(lay.jobs) for s in range(n)]


def mixed_groups(lay, group, which="out"):
    """the groups of `group` consecutive samples of the launch set that hold both a hot and a clean sample"""
    hot = [lay.hot(b, n)[which] for b, n in lay.jobs if n]
    live = [i for i, (b, n) in enumerate(lay.jobs) if n]
    flat = np.concatenate(hot)
    assert flat.size == len(set_numbering(lay)) and len(live) == len(hot)
    return [g for g in range(0, flat.size, group) if flat[g:g + group].any() and not flat[g:g + group].all()]


# ---- 1. the references ----------------------------------------------------------------------------------------------------------------
def test_the_case_list_is_the_catalogues():
    assert len(set(NAMES)) == len(NAMES) == 33 and all(n in S.BY_NAME for n in NAMES)
    assert all(max(S.BY_NAME[n].sizes) <= 160 for n in NAMES)
    assert len(UNWEIGHTED) == 8
    # every kernel name of the second half is expected by a case of the list
    pats = [p for n in NAMES for p in S.BY_NAME[n].expect]
    for k in S.SECOND_TOKENS:
        assert any(p.startswith((k + "<", k + "[")) for p in pats), k
    by_form = {n: S.BY_NAME[n].form for n in NAMES}
    assert "C4" in by_form["din_ragged"] and "C4" in by_form["din_h2_L4"] and "din_pipe" in by_form["din_T257"]
    assert by_form["din_32_h3"].endswith("din_two") and by_form["din_32_h65"].endswith("din_any") and by_form["din_30"] == "any + din_any"


def test_relu_and_tanh_rules_the_expectations_rest_on():
    v = np.array([np.nan, np.inf, -np.inf, -1.0, 0.0, 2.0])
    assert np.array_equal(relu(v), [0.0, np.inf, 0.0, 0.0, 0.0, 2.0])
    # C's fmaxf(v, 0) (the fused DIN forms) has the same classes: a NaN operand yields the other one
    assert np.array_equal(np.fmax(v, 0.0), relu(v))
    assert np.tanh(np.float32(np.inf)) == 1 and np.tanh(np.float32(-np.inf)) == -1 and np.isnan(np.tanh(np.float32(np.nan)))
    # tanh_rnn's large branch, 1 - 2 / (e^{2|x|} + 1), at +-inf and where e^{2|x|} overflows: exactly 1
    with np.errstate(all="ignore"):
        for x in (np.float32(np.inf), np.float32(1e5), np.float32(89.0)):
            e = np.exp2(np.float32(x) * np.float32(2.8853900817779268))
            assert np.isinf(e) and np.float32(1) - np.float32(2) * (np.float32(1) / (e + np.float32(1))) == 1
    # 0 * inf: the reason a mask by multiplication cannot stand in for a select
    with np.errstate(all="ignore"):
        assert np.isnan(np.float32(0) * np.float32(np.inf)) and np.float32(0) * np.float32(1e5) == 0


@pytest.mark.parametrize("name", ORDER)
def test_references_agree_and_the_layout_cannot_pass_vacuously(name):
    lay = layout(name)
    case = lay.case
    T, U, D = case.T, case.T - 3, case.D
    w, om_c, om_p = models_of(lay.key)
    assert_weights(w)
    refs = references(name)
    lo, hi = block_columns(case)
    rec = dict(test="cpu", case=name, kind=case.kind, queries=[], worst_row=0.0, worst_out=0.0)

    # ---- the tables and the staged bags
    for Wc, Wp in zip(lay.clean.W, lay.poisoned.W):
        assert np.all(np.isnan(Wp[0])) and np.all(np.isfinite(Wc)) and np.array_equal(Wc[N_POISON:], Wp[N_POISON:])
        assert np.abs(Wc).max() <= 1 and np.abs(np.where(np.isfinite(Wp), Wp, 0)).max() == 1e5
    seen_recipes, seen_roles = set(), set()
    for b in range(lay.nb):
        n = lay.need[b]
        named = lay.named(b, n)
        for t in range(T):
            off = np.concatenate([[0], np.cumsum(lay.lens[b][t])]).astype(np.int64)
            i_t = lay.idx[b][t]
            assert np.all(i_t[off[n]:] == 0) and not np.any(i_t[:off[n]] == 0), "row 0: every bag beyond the query, none inside"
            is_named = np.array([np.any(i_t[off[s]:off[s + 1]] < N_POISON) for s in range(n)])
            assert np.array_equal(is_named, named[t]), (b, t)
            assert np.all(lay.plain[b][t][:off[n]] >= N_POISON)
        for m in lay.marks[b]:
            assert m.s % 3 == b % 3 and named[:, m.s].sum() == 1
            for nxt in (m.s + 1, m.s + 2):                               # the two samples behind a marked one: ordinary rows only
                assert nxt >= n or not named[:, nxt].any()
    for b, n in lay.jobs:
        for m in lay.marks[b]:
            if m.s < n:
                seen_recipes.add(m.recipe)
                seen_roles.add(m.role)
    # every recipe and every table role occurs inside a query -- as far as the set's marked bags go round (a set of five
    # samples holds two)
    n_marked = len({m.k for b, n in lay.jobs for m in lay.marks[b] if m.s < n})       # (the rotation's distinct places)
    assert len(seen_recipes) == min(len(UNWEIGHTED), n_marked), (sorted(seen_recipes), n_marked)
    assert len(seen_roles) == min(len(lay.roles), n_marked), (sorted(seen_roles), n_marked)
    assert n_marked >= 2
    if case.kind == "dien":
        assert {"first unit", "last unit"} <= seen_roles or U == 1
    else:
        assert {"first unit", "candidate ad"} <= seen_roles
    ragged = [b for b in range(lay.nb) if case.L[b] == S.RAGGED]
    for b in ragged:
        n = lay.need[b]
        marked_lens = [int(lay.lens[b][m.t][m.s]) for m in lay.marks[b]]
        assert all(l >= 2 for l in marked_lens) and (S.RAGGED_MAX in marked_lens or n < 12), "a poison row in add_tail's round"
        assert all(lay.lens[b][t][s] == 0 or lay.named(b, n)[t, s] for t in range(T) for s in EMPTY_AT if s < n)
    if any(L == S.RAGGED or L < 3 for L in case.L) and case.kind == "din" and lay.need[0] >= 1:
        # slots past a bag's end read index slot 0 of the table's block: in batch 0 that slot names a poison row
        t0 = lay.marks[0][0].t
        assert lay.marks[0][0].s == 0 and lay.idx[0][t0][0] < N_POISON

    # ---- per query: the references
    some_mixed, n_differ = False, 0
    for (b, n), r in sorted(refs.items()):
        hot = r["hot"]
        R64, out64, R_orc, out_orc = r["R64"], r["out64"], r["R_orc"], r["out_orc"]
        # on `clean` no element of any reference is non-finite
        for k in ("R64_clean", "out64_clean", "R_orc_clean", "out_orc_clean"):
            assert np.all(np.isfinite(r[k])), (b, n, k)
        # the class maps agree: float64 and the C oracle, input row and outputs
        assert np.array_equal(classes(R64), classes(R_orc)), (b, n, np.argwhere(classes(R64) != classes(R_orc))[:8].tolist())
        assert np.array_equal(classes(out64), classes(out_orc)), (b, n, np.argwhere(classes(out64) != classes(out_orc))[:8].tolist())
        # poison stays inside the hot sets: there the oracle on `poisoned` is the oracle on `clean`, bit for bit
        cold_cols = np.ones(R_orc.shape, bool)
        cold_cols[hot["block"], lo:hi] = False
        for (t, c0), h in zip(passthrough_columns(case), hot["passthrough"]):
            cold_cols[h, c0:c0 + D] = False
        bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)
        assert np.array_equal(bits(R_orc)[cold_cols], bits(r["R_orc_clean"])[cold_cols]), (b, n)
        assert np.array_equal(bits(out_orc)[~hot["out"]], bits(r["out_orc_clean"])[~hot["out"]]), (b, n)
        assert not np.any(classes(R64)[cold_cols]) and not np.any(classes(out64)[~hot["out"]])
        # (a hot row MAY equal the clean one: a unit whose bag holds a NaN contributes ReLU(b2), and so does one whose hidden
        #  value is negative.  Some row of the case differs: asserted below.)
        n_differ += sum(1 for s in np.nonzero(hot["block"])[0] if not np.array_equal(bits(R_orc)[s, lo:hi], bits(r["R_orc_clean"])[s, lo:hi]))
        # the pass-through bags: class_ref's classes are the sequential chain's
        for (t, c0), seq in zip(passthrough_columns(case), r["seq"]):
            assert np.array_equal(classes(seq), classes(R64[:, c0:c0 + D])) and np.array_equal(bits(seq), bits(R_orc[:, c0:c0 + D]))
        # the bar: the oracle against float64, per sample row, on the finite elements
        f_row = bar_fraction(R_orc[:, lo:hi], R64[:, lo:hi], **row_bar(case))
        f_out = bar_fraction(out_orc, out64, **out_bar(case))
        f_out_exact = bar_fraction(out_orc, out64, **out_bar(case, exact=True))
        rec["worst_row"] = max(rec["worst_row"], float(f_row.max()))
        rec["worst_out"] = max(rec["worst_out"], float(f_out_exact.max()))
        assert f_row.max() <= 1, (b, n, "block: the oracle is outside the bar of float64", int(f_row.argmax()), float(f_row.max()))
        assert f_out.max() <= 1, (b, n, "outputs: the oracle is outside the bar of float64", int(f_out.argmax()), float(f_out.max()))
        assert f_out_exact.max() <= 1, (b, n, "outputs, sls_exact's bar", int(f_out_exact.argmax()), float(f_out_exact.max()))
        # the network is alive
        assert np.count_nonzero(r["R64_clean"][:, lo:hi]) * 4 >= r["R64_clean"][:, lo:hi].size
        cls = classes(R64)
        rec["queries"].append(dict(batch=b, n=n, hot=int(hot["out"].sum()), clean=int((~hot["out"]).sum()),
                                   block_hot=int(hot["block"].sum()), classes=sorted(int(c) for c in np.unique(cls[:, lo:hi]))))
        some_mixed |= 2 * int((~hot["out"]).sum()) >= n and hot["out"].any()

        # ---- 2. the consequences
        named = lay.named(b, n)
        if case.kind == "din":
            E = r["E64"]
            for s in range(n):
                unit_cls = [classes(E[t][s]).max() for t in range(1, 1 + U)]
                if classes(E[T - 2][s]).max() == 0 and set(unit_cls) <= {0, 3} and 3 in unit_cls:
                    # a NaN in a unit's bag (the other units and the ad finite): ReLU maps it to 0, the block stays finite
                    assert not np.any(cls[s, lo:hi]), (b, n, s)
                    rec["nan_unit_finite"] = rec.get("nan_unit_finite", 0) + 1
            assert not np.any(np.isin(cls[:, lo:hi], (2, 3))), "the attention block is a sum of ReLUs: finite or +inf"
        else:
            trace = []
            dien_ref64(w, r["E64"], trace)
            seq = np.stack(r["E64"][1:1 + U], axis=1).reshape(n * U, -1).reshape(U, n, -1)
            for s in range(n):
                step_cls = [classes(seq[t][s]) for t in range(U)]
                nan_from = next((t for t in range(U) if classes(trace[t][0][s]).max() == 3), None)
                for t in range(U):
                    x_inf = np.isin(step_cls[t], (1, 2)).sum()
                    if x_inf == 1 and not np.any(step_cls[t] == 3) and (nan_from is None or t < nan_from):
                        # one +-inf element in the step: every layer-1 state exactly +-1, the layer-2 state finite
                        assert np.all(np.abs(trace[t][0][s]) == 1.0) and np.all(np.isfinite(trace[t][1][s])), (b, n, s, t)
                        if t + 1 < U and not np.any(step_cls[t + 1]):
                            assert np.all(np.isfinite(trace[t + 1][0][s])) and np.all(np.abs(trace[t + 1][0][s]) < 1)
                        rec["inf_step"] = rec.get("inf_step", 0) + 1
                if nan_from is not None:
                    assert all(np.all(np.isnan(trace[t][0][s])) for t in range(nan_from, U)), (b, n, s)
                    assert all(np.all(np.isnan(trace[t][1][s])) for t in range(nan_from, U)), (b, n, s)
                    if not hot["passthrough"][:, s].any():
                        # the outputs: the top MLP's first layer is all NaN -> 0, the rest is the biases-only path
                        zero_first = np.zeros((1, w.top[0][0].shape[0]))
                        assert np.array_equal(out64[s], mlp64(zero_first, w.top[1:])[0][0]), (b, n, s)
                        rec["nan_state_bias_path"] = rec.get("nan_state_bias_path", 0) + 1
            assert not np.any(np.isin(cls[:, lo:hi], (1, 2))), "a state is a tanh: finite or NaN"
            assert hot["block"].sum() == len({(s * U + u) % n for u, s in zip(*np.nonzero(named[1:1 + U]))})

    # ---- 3. not vacuous
    rec["hot_block_rows_that_differ_from_clean"] = n_differ
    assert n_differ >= 1, "every hot block row equals the clean one"
    assert some_mixed, "no query with hot samples and at least half of its samples outside every hot set"
    if case.kind == "din":
        own_S = int(case.form.split(",S")[1][0]) if S.din_class(case) == "fused" else 1
        for grp in sorted({own_S, 2, 4} - {1}):
            assert mixed_groups(lay, grp, "block"), (grp, "no DIN workgroup holds both a hot and a clean sample")
        rec["mixed_groups"] = {str(g): len(mixed_groups(lay, g, "block")) for g in (2, 4)}
    else:
        for grp in (16, 4):
            assert mixed_groups(lay, grp, "block"), (grp, "no DIEN tile holds both a hot and a clean sample")
        rec["mixed_groups"] = {str(g): len(mixed_groups(lay, g, "block")) for g in (16, 4)}
        via = sum(int((r["hot"]["block"] & ~r["hot"]["own"]).sum()) for r in refs.values())
        rec["hot_through_reshape_only"] = via
        assert via >= 1 or U == 1, "no sample is hot through the Reshape alone"
    all_cls = set()
    for r in refs.values():
        all_cls |= set(np.unique(classes(r["R64"])).tolist())
    assert (3 in all_cls and all_cls & {1, 2}) or n_marked < 4, all_cls            # an infinity and a NaN reach the input rows
    print("%s: oracle against float64 at %.3f (block) and %.3f (outputs, the exact bar) of the bar" % (name, rec["worst_row"], rec["worst_out"]))
    report(**rec)


def test_the_lane_group_without_a_unit_sees_an_infinite_candidate_ad():
    """din_pipe_kernel / din_fused_kernel: in the last round a lane group without a unit applies unit 0's weights to
    (0, ad, ad) and a select drops the result.  The cases din_32_U33 and din_64_U17 each hold a sample whose candidate ad makes
    that dropped result +inf in some column: multiplied by 0 instead of selected away it would be NaN."""
    for name in ("din_32_U33", "din_64_U17"):
        lay = layout(name)
        case = lay.case
        U = case.T - 3
        assert U % lane_groups(case) == 1                               # one lane group holds a unit more than the others
        w = models_of(lay.key)[0]
        found = 0
        for (b, n), r in references(name).items():
            ad = r["E64"][case.T - 2]
            x = np.concatenate([np.zeros_like(ad), ad, ad], axis=1)
            dropped = mlp64(x, w.att[0])[0]
            found += int(np.sum(np.isposinf(dropped).any(axis=1) & r["hot"]["passthrough"][1]))
        assert found >= 1, name


def test_close_finite_is_the_floor_the_row_bar_generalises():
    """bar_fraction on one row is tests/test_sls_nonfinite_cpu.close_finite"""
    rng = np.random.RandomState(3)
    ref = rng.uniform(-1, 1, (1, 64))
    ref[0, 5], ref[0, 9] = np.inf, np.nan
    for scale in (1e-7, 3e-6):
        got = ref + scale * rng.uniform(-1, 1, ref.shape)
        got[0, 5], got[0, 9] = np.inf, np.nan
        assert close_finite(got, ref) == bool(bar_fraction(got, ref, rtol=1e-5, atol_scale=2e-6).max() <= 1)
    # a 1e5 element widens its own row's floor and nobody else's
    two = np.array([[1.0, 1e5], [1.0, 0.5]])
    off = two + np.array([[0.1, 0.0], [0.1, 0.0]])
    f = bar_fraction(off, two, rtol=1e-5, atol_scale=2e-6)
    assert f[0] <= 1 < f[1]
