"""The gather, DIN and DIEN launch choosers' boundary catalogue (a plain module: no tests in it).

csrc/sls.hip (plan_sls / lanes_per_row), csrc/din.hip (fused_shape / din_fused_applicable / din_pipe_lds /
launch_din_fused), csrc/dien.hip (dien_applicable / dien_top_fusable / launch_dien_rnn) and their callers in
csrc/engine_dispatch.hip (launch_gather / mlp_din / mlp_dien) pick the first half of every launch set.  CASES holds one small
launch set on each side of every rule (DESIGN.md 3.2 lists the rules and names the cases).  The rule numbers:

   gather   1  width classes: G = lanes per row (2 | 4 | 8 | 16 | 32 | 64 at D <= 8 | 16 | 32 | 64 | 128 | more); D % 4 != 0 or
               D > 256 -> sls_any_kernel; the flat forms exist for G in {8, 16, 32} only
            2  fixed bags of ONE row at D in {16, 32, 64, 128} -> the copy form; L >= 2 -> a flat form
            3  loads per lane: need = ceil(bpw L / (64 / G)) -> NL 5 | 10 | 20, beyond 20 the ring walk
            4  automatic bags per wave: the first c in (4, 2) with T % c == 0 and c L <= 5 (64 / G), else 1
            5  forced "sls_bpw": 2 / 4 need bpw | T and NL <= 10, else the ring walk; "sls_flat" 0 | 1 | 2
            6  the queries of a set must agree: one fixed L >= 2 for the flat forms, every L == 1 for the copy form;
               every L fixed and <= sls_short_bag = 2048 / D -> the sequential ring walk, else the split one
            7  the copy form's samples per wave: 16 while T ceil(n / 64) < 1024, else 64 ("sls_one" 16 | 64 force one)
            8  "sls_exact" 1: sequential order whatever the flat options say (any / copy / sequential ring walk)
   DIN      9  din_fused_applicable: D in {32, 64} and h in {1, 2, 4}; drs_create's din_any rule (more than one hidden
               layer, h > 64, (T - 3) h > 4096, D % 4 != 0, D > 256)
           10  samples per workgroup S = 1 | 2 | 4 below 512 | below 1024 | from 1024 samples on ("din_s" forces one)
           11  bag class: every query's L fixed and <= 3 -> C3 (and, at h == 1, din_pipe_kernel), else C4 for every query
           12  din_pipe_kernel's staging loop (256 tables per round) and its LDS gate T (8 + 12 S) <= 48 KB
           13  units per lane group K = ceil(U / NGB) against the pipeline depth 2 (NGB = 4 waves x 64 / G lane groups)
   DIEN    14  dien_applicable: D in {16, 32, 64} x H in {8, 16, 32, 64}; H % 16 != 0 has no matrix-core form
           15  dien_top_fusable: <= 4 top layers, every input width % 4 == 0 and <= 256 (the 60 KB LDS test is shadowed)
           16  workgroup edges: 16 samples per workgroup (4 under "dien_mfma" 0), 1 ... 5 behaviour tables

Every case writes the form it stands for BY HAND (`form`, in the shorthand of render()); expected_gather_form /
expected_din_form / expected_dien_form restate the rules in plain Python from DESIGN.md 3 and docs/OPTIONS.md, and
tests/test_gather_boundaries_cpu.py holds the two against each other -- nothing here calls the engine.  `expect` (dispatch-log
tokens the set must show) is render(form); `exclude` strings must be part of no token.

A case is ONE launch set: query i has sizes[i] samples of bag length L[i] (RAGGED = -1: lengths drawn from 0 ... 5).
"""
import collections
import zlib

import numpy as np

from oracle import oracle as orc

Case = collections.namedtuple("Case", "name kind D T H top L sizes opts rule thr side form expect exclude alone note")

RAGGED = -1
RAGGED_MAX = 5
B_MAX = 160
N_BATCH = 4                      # staged batches per engine: query i reads batch i % min(len(sizes), N_BATCH)

# what every case sets first (the defaults of docs/OPTIONS.md, but for the non-temporal hints, which the engine picks per
# model: 0 here, so that no token carries ",nt")
BASE_OPTS = (("sls_exact", 0), ("sls_flat", 1), ("sls_bpw", 0), ("sls_one", 1), ("sls_nt", 0), ("din_fused", 1), ("din_pipe", 1),
             ("din_s", 0), ("din_nt", 0), ("dien_mfma", 2), ("dien_fuse_top", 1))

CASES = []


# ---- the rules, restated ------------------------------------------------------------------------------------------------------
def lanes_per_row(D):
    for lim, g in ((8, 2), (16, 4), (32, 8), (64, 16), (128, 32)):
        if D <= lim:
            return g
    return 64


def options(case):
    o = collections.OrderedDict(BASE_OPTS)
    o.update(case.opts)
    return o


def live_queries(case, only=None):
    """(L, size) of the queries that take rows: a query of size 0 is no part of the set"""
    qs = [(L, n) for L, n in zip(case.L, case.sizes) if n > 0]
    return qs if only is None else [(case.L[only], case.sizes[only])]


def expected_gather_form(case, only=None):
    """-> the gather launch's form in render()'s shorthand; only = i: query i served alone"""
    o = options(case)
    D, T = case.D, case.T
    qs = live_queries(case, only)
    n = sum(s for _, s in qs)
    if D % 4 or D > 256:
        return "any"
    G = lanes_per_row(D)
    NG = 64 // G
    L0 = qs[0][0]
    exact = bool(o["sls_exact"])
    flat = (not exact) and o["sls_flat"] != 0 and L0 >= 2 and G in (8, 16, 32) and all(L == L0 for L, _ in qs)
    bpw = 1
    if flat and o["sls_bpw"]:
        bpw = o["sls_bpw"]
        flat = T % bpw == 0
    elif flat:
        for c in (4, 2):
            if T % c == 0 and c * L0 <= 5 * NG:
                bpw = c
                break
    need = -(-bpw * L0 // NG)
    nl = 5 if need <= 5 else 10 if need <= 10 else 20 if need <= 20 else 0
    if flat and nl and (bpw == 1 or nl <= 10):
        if bpw == 1 and o["sls_flat"] == 1:
            return "flatc %d,%d" % (G, nl)
        return "flat %d,%d,bpw%d" % (G, nl, bpw)
    short = all(0 <= L <= 2048 // D for L, _ in qs)
    exact = exact or short
    if exact and o["sls_one"] and D in (16, 32, 64, 128) and all(L == 1 for L, _ in qs):
        bw = o["sls_one"] if o["sls_one"] in (16, 64) else (16 if T * -(-n // 64) < 1024 else 64)
        return "one %d,%d" % (D // 4, bw)
    return "ring %d,%s" % (G, "sequential" if exact else "split")


def din_class(case):
    """any | two (gather + din_attention_kernel) | fused"""
    h, U = case.H, case.T - 3
    if len(h) != 1 or h[0] > 64 or U * h[0] > 4096 or case.D % 4 or case.D > 256:
        return "any"
    o = options(case)
    if o["sls_exact"] or not o["din_fused"] or case.D not in (32, 64) or h[0] not in (1, 2, 4):
        return "two"
    return "fused"


def expected_din_form(case, only=None):
    cls = din_class(case)
    if cls == "any":
        return expected_gather_form(case, only) + " + din_any"
    if cls == "two":
        return expected_gather_form(case, only) + " + din_two"
    o = options(case)
    qs = live_queries(case, only)
    n = sum(s for _, s in qs)
    S = o["din_s"] or (4 if n >= 1024 else 2 if n >= 512 else 1)
    C = 3 if all(0 <= L <= 3 for L, _ in qs) else 4
    G, h = case.D // 4, case.H[0]
    if o["din_pipe"] and h == 1 and C == 3 and case.T * (8 + 12 * S) <= 48 * 1024:
        return "din_pipe %d,S%d" % (G, S)
    return "din_fused %d,S%d,h%d,C%d" % (G, S, h, C)


def dien_top_fused(case):
    o = options(case)
    H, D = case.H[0], case.D
    ln = (H + 3 * D,) + tuple(case.top)
    applicable = D in (16, 32, 64) and H in (8, 16, 32, 64)
    mfma_form = applicable and o["dien_mfma"] in (1, 2) and H % 16 == 0
    nt = len(ln) - 1
    return bool(o["dien_fuse_top"] and mfma_form and 1 <= nt <= 4 and all(0 < k <= 256 and k % 4 == 0 for k in ln[:-1]))


def expected_dien_form(case, only=None):
    o = options(case)
    H, D = case.H[0], case.D
    g = expected_gather_form(case, only)
    if not (D in (16, 32, 64) and H in (8, 16, 32, 64)) or o["dien_mfma"] == 3:
        return g + " + dien_any %d,%d" % (D, H)
    if o["dien_mfma"] and H % 16 == 0:
        return g + " + dien_mfma %d,%d%s" % (D, H, ",top" if dien_top_fused(case) else "")
    return g + " + dien_valu %d,%d" % (D, H)


EXPECTED = {"sls": expected_gather_form, "din": expected_din_form, "dien": expected_dien_form}


def render(form, tag=""):
    """shorthand -> the dispatch-log patterns (token prefixes) of the launches; tag: the table dtype's token ("f16")"""
    t = ("," + tag) if tag else ""
    out = []
    for part in form.split(" + "):
        k, _, a = part.partition(" ")
        if k == "any":
            out.append("sls_any_kernel<%s>[" % tag if tag else "sls_any_kernel[")
        elif k == "flatc":
            out.append("sls_flatc_kernel<%s%s>[" % (a, t))
        elif k == "flat":
            out.append("sls_flat_kernel<%s%s>[" % (a, t))
        elif k == "one":
            out.append("sls_one_kernel<%s%s>[" % (a, t))
        elif k == "ring":
            out.append("sls_kernel<%s%s>[" % (a, t))
        elif k == "din_any":
            out.append("din_attention_any_kernel[")
        elif k == "din_two":
            out.append("din_attention_kernel[")
        elif k == "din_pipe":
            out.append("din_pipe_kernel<%s,P2>[" % a)
        elif k == "din_fused":
            out.append("din_fused_kernel<%s>[" % a)
        elif k == "dien_any":
            out.append("dien_rnn_any_kernel<%s>[" % a)
        elif k == "dien_mfma":
            out.append("dien_rnn_mfma_kernel<%s>[" % a)
        elif k == "dien_valu":
            out.append("dien_rnn_kernel<%s>[" % a)
        else:
            raise ValueError(form)
    return tuple(out)


GATHER_TOKENS = ("sls_any_kernel", "sls_flatc_kernel", "sls_flat_kernel", "sls_one_kernel", "sls_kernel")
SECOND_TOKENS = ("din_attention_any_kernel", "din_attention_kernel", "din_pipe_kernel", "din_fused_kernel", "dien_rnn_any_kernel",
                 "dien_rnn_mfma_kernel", "dien_rnn_kernel")
MLP_TOKENS = ("stream4_kernel", "stream_kernel", "chain_kernel", "fc_kernel", "gemm_kernel", "gemm32_kernel")


def check_dispatch(case, log, form=None, tag=""):
    """-> list of complaints (empty: the set took exactly the forms the case stands for).  Every gather / DIN / DIEN token of
    the log must be one of the expected ones: a set that took another form fails."""
    form = case.form if form is None else form
    expect = render(form, tag)
    bad = []
    for pat in expect:
        if not any(t.startswith(pat) for t in log):
            bad.append("missing %r" % pat)
    for t in log:
        if t.startswith(GATHER_TOKENS + SECOND_TOKENS) and not t.startswith(expect):
            bad.append("unexpected %r" % t)
    for pat in case.exclude:
        if any(pat in t for t in log if not t.startswith("set[")):
            bad.append("excluded %r" % pat)
    if case.kind == "dien":
        # the top MLP: inside the recurrence's launch (",top") or a launch of its own -- one of the two, never both
        sep = sum(1 for t in log if t.startswith(MLP_TOKENS))
        top = any(",top>" in t for t in log)
        if top == bool(sep):
            bad.append("top MLP: %s and %d MLP launches" % ("fused" if top else "not fused", sep))
    return bad


def _case(name, kind, D, T, L, sizes, rule, side, form, thr="", H=(), top=(), exclude=(), alone=None, note="", **opts):
    """side: at | beyond (the two sides of the rule's threshold `thr`) or "shadowed"; alone: the form query i takes when it is
    served alone, where that differs from the set's -- None: the same form, same bits.  "tile" / "S" (samples per wave or per
    workgroup) and "copy" (the copy form against the sequential walk) change the launch, not the order of any sum: the same
    bits are still promised (BITS_PROMISED); "flat" / "sequential" / "C" change the order or the kernel: tolerance only"""
    if isinstance(L, int):
        L = (L,) * len(sizes)
    assert len(L) == len(sizes)
    nb = min(len(sizes), N_BATCH)
    assert all(L[i] == L[i % nb] for i in range(len(L))), name
    CASES.append(Case(name, kind, D, T, tuple(H), tuple(top), tuple(L), tuple(sizes), tuple(sorted(opts.items())), rule, thr, side, form,
                      render(form), tuple(exclude), alone, note))


BITS_PROMISED = (None, "tile", "S", "copy")
TWO = (70, 5)          # the usual set: two queries of the same bag length (two 64-row blocks and a short one)


def sls(name, D, T, L, rule, side, form, thr="", sizes=TWO, **kw):
    _case(name, "sls", D, T, L, sizes, rule, side, form, thr=thr, **kw)


# ---- rule 1: width classes (T = 3: no bags share a wave; L = 20) ----------------------------------------------------------------------
# 2048 / D >= 20 up to D = 102: the ring walk of the narrow widths is the sequential one; w_8_long / w_16_long reach the split one
for _D, _side, _form in ((4, "at", "ring 2,sequential"), (8, "at", "ring 2,sequential"), (12, "beyond", "ring 4,sequential"),
                         (16, "at", "ring 4,sequential"), (20, "beyond", "flatc 8,5"), (32, "at", "flatc 8,5"), (36, "beyond", "flatc 16,5"),
                         (64, "at", "flatc 16,5"), (68, "beyond", "flatc 32,10"), (128, "at", "flatc 32,10"), (132, "beyond", "ring 64,split"),
                         (252, "at", "ring 64,split"), (256, "at", "ring 64,split"), (260, "beyond", "any"), (30, "beyond", "any")):
    sls("w_%d" % _D, _D, 3, 20, 1, _side, _form, thr={30: "D%4", 252: "D<=256", 256: "D<=256", 260: "D<=256"}.get(_D, "G"))
sls("w_28", 28, 3, 20, 1, "at", "flatc 8,5", thr="D%4")
sls("w_8_long", 8, 3, 257, 1, "at", "ring 2,split", thr="G")
sls("w_16_long", 16, 3, 129, 1, "at", "ring 4,split", thr="G")

# ---- rule 2: one row per bag | two (T = 3) ------------------------------------------------------------------------------------------
for _D, _two in ((16, "ring 4,sequential"), (32, "flatc 8,5"), (64, "flatc 16,5"), (128, "flatc 32,5")):
    sls("one_%d_L1" % _D, _D, 3, 1, 2, "at", "one %d,16" % (_D // 4), thr="D%d" % _D)
    sls("one_%d_L2" % _D, _D, 3, 2, 2, "beyond", _two, thr="D%d" % _D, exclude=["sls_one_kernel"])
sls("one_48_L1", 48, 3, 1, 2, "beyond", "ring 16,sequential", thr="width", exclude=["sls_one_kernel"])
sls("one_64_L1_w", 64, 4, 1, 2, "at", "one 16,16", thr="width")

# ---- rule 3: loads per lane under "sls_bpw" 1 (T = 4) ----------------------------------------------------------------------------------
RUNGS = {32: (40, 80, 160), 64: (20, 40, 80), 128: (10, 20, 40), 36: (None, 40, None), 68: (None, 20, None)}
for _D, _ls in sorted(RUNGS.items()):
    _G = lanes_per_row(_D)
    for _nl, _nxt, _L in zip((5, 10, 20), (10, 20, 0), _ls):
        if _L is None:
            continue
        sls("rung_%d_L%d" % (_D, _L), _D, 4, _L, 3, "at", "flatc %d,%d" % (_G, _nl), thr="D%d nl%d" % (_D, _nl), sls_bpw=1)
        sls("rung_%d_L%d" % (_D, _L + 1), _D, 4, _L + 1, 3, "beyond", "flatc %d,%d" % (_G, _nxt) if _nxt else "ring %d,split" % _G,
            thr="D%d nl%d" % (_D, _nl), sls_bpw=1)

# ---- rule 4: automatic bags per wave ------------------------------------------------------------------------------------------------
for _D, _G, (_a, _b) in ((32, 8, (10, 20)), (64, 16, (5, 10)), (128, 32, (2, 5))):
    sls("bpw_%d_L%d" % (_D, _a), _D, 4, _a, 4, "at", "flat %d,5,bpw4" % _G, thr="D%d c4" % _D)
    sls("bpw_%d_L%d" % (_D, _a + 1), _D, 4, _a + 1, 4, "beyond", "flat %d,5,bpw2" % _G, thr="D%d c4" % _D)
    sls("bpw_%d_L%d" % (_D, _b), _D, 4, _b, 4, "at", "flat %d,5,bpw2" % _G, thr="D%d c2" % _D)
    sls("bpw_%d_L%d" % (_D, _b + 1), _D, 4, _b + 1, 4, "beyond", "flatc %d,5" % _G, thr="D%d c2" % _D)
sls("bpw_T6", 32, 6, 10, 4, "beyond", "flat 8,5,bpw2", thr="T%4")           # (T = 4: bpw_32_L10)
sls("bpw_T8", 32, 8, 10, 4, "at", "flat 8,5,bpw4", thr="T%4")
sls("bpw_T5", 32, 5, 10, 4, "beyond", "flatc 8,5", thr="T%2")
sls("bpw_T6_c2", 32, 6, 20, 4, "at", "flat 8,5,bpw2", thr="T%2")

# ---- rule 5: forced "sls_bpw", "sls_flat" ------------------------------------------------------------------------------------------
sls("force_bpw2_fits", 64, 4, 10, 5, "at", "flat 16,5,bpw2", thr="nl<=10", sls_bpw=2)
sls("force_bpw4_nl10", 64, 4, 10, 5, "at", "flat 16,10,bpw4", thr="nl<=10", sls_bpw=4)
sls("force_bpw4_nl20_short", 64, 4, 20, 5, "beyond", "ring 16,sequential", thr="nl<=10", sls_bpw=4)      # need = 20; 20 <= 2048 / 64
sls("force_bpw2_nl20", 64, 4, 40, 5, "beyond", "ring 16,split", thr="nl<=10", sls_bpw=2)                 # need = 20; 40 > 32
sls("force_bpw2_T4", 32, 4, 35, 5, "at", "flat 8,10,bpw2", thr="bpw|T", sls_bpw=2)
sls("flat2_nl20", 32, 4, 100, 5, "at", "flat 8,20,bpw1", thr="sls_flat", sls_bpw=1, sls_flat=2, note="the 20-load rung exists for one bag per wave only")
sls("force_bpw2_T5", 32, 5, 70, 5, "beyond", "ring 8,split", thr="bpw|T", sls_bpw=2)
sls("force_bpw4_T6", 32, 6, 10, 5, "beyond", "ring 8,sequential", thr="bpw|T", sls_bpw=4)
sls("force_bpw2_T6", 32, 6, 10, 5, "at", "flat 8,5,bpw2", thr="bpw|T", sls_bpw=2)
sls("flat0", 32, 4, 70, 5, "beyond", "ring 8,split", thr="sls_flat", sls_bpw=1, sls_flat=0)
sls("flat1", 32, 4, 70, 5, "at", "flatc 8,10", thr="sls_flat", sls_bpw=1, sls_flat=1)
sls("flat2", 32, 4, 69, 5, "at", "flat 8,10,bpw1", thr="sls_flat", sls_bpw=1, sls_flat=2)
sls("flat2_auto", 32, 4, 20, 5, "at", "flat 8,5,bpw2", thr="sls_flat", sls_flat=2)

# ---- rule 6: sets whose queries disagree (three queries) ---------------------------------------------------------------------------------
THREE = (70, 5, 33)
sls("mix_20_20_10", 32, 4, (20, 20, 10), 6, "beyond", "ring 8,sequential", thr="same L", sizes=THREE, alone="flat")
sls("mix_20_20_10_wide", 128, 4, (20, 20, 10), 6, "beyond", "ring 32,split", thr="same L", sizes=THREE, alone="flat")
sls("mix_20_20_20", 128, 4, (20, 20, 20), 6, "at", "flatc 32,10", thr="same L", sizes=THREE)
sls("mix_20_ragged_20", 32, 4, (20, RAGGED, 20), 6, "beyond", "ring 8,split", thr="ragged", sizes=THREE, alone="flat")
sls("mix_20_20_20_narrow", 32, 4, (20, 20, 20), 6, "at", "flat 8,5,bpw2", thr="ragged", sizes=THREE)
sls("mix_ragged_only", 32, 4, (RAGGED,), 6, "beyond", "ring 8,split", thr="ragged", sizes=(77,))
sls("mix_1_1_2", 32, 4, (1, 1, 2), 6, "beyond", "ring 8,sequential", thr="all L=1", sizes=THREE, exclude=["sls_one_kernel"], alone="copy")
sls("mix_2_1_1", 32, 4, (2, 1, 1), 6, "beyond", "ring 8,sequential", thr="all L=1", sizes=THREE, exclude=["sls_one_kernel"], alone="copy")
sls("mix_1_1_1", 32, 4, (1, 1, 1), 6, "at", "one 8,16", thr="all L=1", sizes=THREE)
sls("short_32_32", 64, 4, (32, 32), 6, "at", "ring 16,sequential", thr="short bag", sls_flat=0)
sls("short_32_33", 64, 4, (32, 33), 6, "beyond", "ring 16,split", thr="short bag", sls_flat=0, alone="sequential")
sls("mix_empty_middle", 32, 4, (20, 10, 20), 6, "at", "flat 8,5,bpw2", thr="empty", sizes=(70, 0, 5),
    note="the empty query's L = 10 does not count: the set is flat")
sls("mix_nonempty_middle", 32, 4, (20, 10, 20), 6, "beyond", "ring 8,sequential", thr="empty", sizes=(70, 3, 5), alone="flat")
sls("mix_empty_first", 32, 4, (10, 20, 20), 6, "at", "flat 8,5,bpw2", thr="empty", sizes=(0, 70, 5))

# ---- rule 7: the copy form's samples per wave --------------------------------------------------------------------------------------------
sls("tile_1023", 16, 341, 1, 7, "at", "one 4,16", thr="waves", sizes=(100, 30), note="341 x ceil(130 / 64) = 1023 waves")
sls("tile_768", 16, 256, 1, 7, "at", "one 4,16", thr="waves", sizes=(160, 32), note="256 x ceil(192 / 64) = 768")
sls("tile_1024", 16, 256, 1, 7, "beyond", "one 4,64", thr="waves", sizes=(160, 33), alone="tile", note="256 x ceil(193 / 64) = 1024; ragged last tile")
sls("tile_force16", 16, 256, 1, 7, "at", "one 4,16", thr="sls_one", sizes=(160, 33), sls_one=16)
sls("tile_force64", 32, 3, 1, 7, "beyond", "one 8,64", thr="sls_one", sizes=(77, 5), sls_one=64)
sls("tile_ragged16", 32, 3, 1, 7, "at", "one 8,16", thr="sls_one", sizes=(77,), note="77 = 4 x 16 + 13")
sls("tile_off", 32, 3, 1, 7, "beyond", "ring 8,sequential", thr="sls_one", sizes=(77, 5), sls_one=0, exclude=["sls_one_kernel"])
sls("tile_n1", 64, 3, 1, 7, "at", "one 16,16", thr="sls_one", sizes=(1,))
sls("tile_n1_64", 64, 3, 1, 7, "at", "one 16,64", thr="sls_one", sizes=(1,), sls_one=64)

# ---- rule 8: "sls_exact" 1 at one case of each group -----------------------------------------------------------------------------------
sls("exact_w_36", 36, 3, 20, 8, "at", "ring 16,sequential", thr="exact", sls_exact=1)
sls("exact_w_260", 260, 3, 20, 8, "at", "any", thr="exact", sls_exact=1)
sls("exact_one_64", 64, 3, 1, 8, "at", "one 16,16", thr="exact", sls_exact=1)
sls("exact_L2_128", 128, 3, 2, 8, "at", "ring 32,sequential", thr="exact", sls_exact=1)
sls("exact_rung", 64, 4, 81, 8, "at", "ring 16,sequential", thr="exact", sls_exact=1, sls_bpw=1)
sls("exact_bpw_auto", 32, 4, 10, 8, "at", "ring 8,sequential", thr="exact", sls_exact=1)
sls("exact_bpw", 32, 4, 20, 8, "at", "ring 8,sequential", thr="exact", sls_exact=1, sls_flat=2, sls_bpw=2)
sls("exact_mix", 32, 4, (20, RAGGED, 20), 8, "at", "ring 8,sequential", thr="exact", sizes=THREE, sls_exact=1)
sls("exact_tile", 16, 256, 1, 8, "at", "one 4,64", thr="exact", sizes=(160, 33), sls_exact=1, alone="tile")
sls("exact_bpw_off", 32, 4, 20, 8, "beyond", "flat 8,5,bpw2", thr="exact", sls_flat=2, sls_bpw=2)


# ---- DIN ----------------------------------------------------------------------------------------------------------------------
def din(name, D, U, h, L, rule, side, form, thr="", sizes=TWO, **kw):
    _case(name, "din", D, U + 3, L, sizes, rule, side, form, thr=thr, H=h if isinstance(h, tuple) else (h,), top=(24, 2), **kw)


S511, S512, S1023, S1024 = (160, 160, 160, 31), (160, 160, 160, 32), (160,) * 6 + (63,), (160,) * 6 + (64,)

# rule 9: the fused launch's instances (U = 5, L = 3)
for _D in (32, 64):
    din("din_%d_h1" % _D, _D, 5, 1, 3, 9, "at", "din_pipe %d,S1" % (_D // 4), thr="fused")
    for _h in (2, 4):
        din("din_%d_h%d" % (_D, _h), _D, 5, _h, 3, 9, "at", "din_fused %d,S1,h%d,C3" % (_D // 4, _h), thr="fused")
din("din_16_h1", 16, 5, 1, 3, 9, "beyond", "ring 4,sequential + din_two", thr="fused")
din("din_128_h1", 128, 5, 1, 3, 9, "beyond", "flat 32,5,bpw2 + din_two", thr="fused")
din("din_32_h3", 32, 5, 3, 3, 9, "beyond", "flat 8,5,bpw4 + din_two", thr="fused")
din("din_32_h64", 32, 5, 64, 3, 9, "at", "flat 8,5,bpw4 + din_two", thr="h<=64")
din("din_32_h65", 32, 5, 65, 3, 9, "beyond", "flat 8,5,bpw4 + din_any", thr="h<=64")
din("din_32_two_layers", 32, 5, (8, 4), 3, 9, "beyond", "flat 8,5,bpw4 + din_any", thr="one hidden layer")
din("din_32_one_layer", 32, 5, 8, 3, 9, "at", "flat 8,5,bpw4 + din_two", thr="one hidden layer")
din("din_30", 30, 5, 1, 3, 9, "beyond", "any + din_any", thr="D%4")
din("din_28", 28, 5, 1, 3, 9, "at", "flat 8,5,bpw4 + din_two", thr="D%4")
din("din_256", 256, 5, 1, 3, 9, "at", "ring 64,sequential + din_two", thr="D<=256")
din("din_260", 260, 5, 1, 3, 9, "beyond", "any + din_any", thr="D<=256")
din("din_lds_4096", 32, 64, 64, 3, 9, "at", "flatc 8,5 + din_two", thr="(T-3)h", note="64 units x 64 hidden values x 4 samples = 64 KB")
din("din_lds_4160", 32, 65, 64, 3, 9, "beyond", "flat 8,5,bpw4 + din_any", thr="(T-3)h")
# rule 10: samples per workgroup by launch size (U = 5)
din("din_s_511", 32, 5, 1, 3, 10, "at", "din_pipe 8,S1", thr="512", sizes=S511)
din("din_s_512", 32, 5, 1, 3, 10, "beyond", "din_pipe 8,S2", thr="512", sizes=S512, alone="S")
din("din_s_1023", 32, 5, 1, 3, 10, "at", "din_pipe 8,S2", thr="1024", sizes=S1023, alone="S")
din("din_s_1024", 32, 5, 1, 3, 10, "beyond", "din_pipe 8,S4", thr="1024", sizes=S1024, alone="S")
din("din_s_1024_h2", 64, 5, 2, RAGGED, 10, "beyond", "din_fused 16,S4,h2,C4", thr="1024", sizes=S1024, alone="S")
din("din_s_1023_h2", 64, 5, 2, RAGGED, 10, "at", "din_fused 16,S2,h2,C4", thr="1024", sizes=S1023, alone="S")
din("din_s4_75", 32, 5, 1, 3, 10, "beyond", "din_pipe 8,S4", thr="n%S", sizes=(70, 5), din_s=4, note="75 = 18 x 4 + 3")
din("din_s4_76", 32, 5, 1, 3, 10, "at", "din_pipe 8,S4", thr="n%S", sizes=(70, 6), din_s=4)
din("din_s2_77", 32, 5, 4, 3, 10, "beyond", "din_fused 8,S2,h4,C3", thr="n%S", sizes=(77,), din_s=2)
din("din_s4_one_sample", 32, 5, 1, 3, 10, "beyond", "din_pipe 8,S4", thr="n%S", sizes=(1,), din_s=4)
din("din_one_sample", 64, 5, 1, 3, 10, "at", "din_pipe 16,S1", thr="n%S", sizes=(1,))
# rule 11: the bag class
for _L in (1, 2):
    din("din_L%d" % _L, 32, 6, 1, _L, 11, "at", "din_pipe 8,S1", thr="L<=3")
din("din_L3", 32, 6, 1, 3, 11, "at", "din_pipe 8,S1", thr="L<=3")
din("din_L4", 32, 6, 1, 4, 11, "beyond", "din_fused 8,S1,h1,C4", thr="L<=3")
din("din_ragged", 32, 6, 1, RAGGED, 11, "beyond", "din_fused 8,S1,h1,C4", thr="L<=3")
din("din_h2_L3", 32, 6, 2, 3, 11, "at", "din_fused 8,S1,h2,C3", thr="h2 L<=3")
din("din_h2_L4", 32, 6, 2, 4, 11, "beyond", "din_fused 8,S1,h2,C4", thr="h2 L<=3")
din("din_L_1_2_3", 32, 6, 1, (1, 2, 3), 11, "at", "din_pipe 8,S1", thr="set", sizes=THREE)
din("din_L_3_4", 32, 6, 1, (3, 4), 11, "beyond", "din_fused 8,S1,h1,C4", thr="set", alone="C")
din("din_L_3_ragged", 64, 6, 1, (3, RAGGED), 11, "beyond", "din_fused 16,S1,h1,C4", thr="set", alone="C")
# rule 12: the pipe form's staging loop and LDS gate (T counts every table)
din("din_T256", 32, 253, 1, (2, 1), 12, "at", "din_pipe 8,S1", thr="staging")
din("din_T257", 32, 254, 1, (2, 1), 12, "beyond", "din_pipe 8,S1", thr="staging", note="the staging loop goes round twice")
din("din_T257_L3", 32, 254, 1, (3, 1, 2), 12, "beyond", "din_pipe 8,S1", thr="staging", sizes=THREE)
din("din_T877_s4", 32, 874, 1, 3, 12, "at", "din_pipe 8,S4", thr="gate S4", sizes=S1024, alone="S", note="877 x 56 = 49 112 <= 49 152")
din("din_T878_s4", 32, 875, 1, 3, 12, "beyond", "din_fused 8,S4,h1,C3", thr="gate S4", sizes=S1024, alone="S", note="878 x 56 = 49 168")
din("din_T1536_s2", 32, 1533, 1, 3, 12, "at", "din_pipe 8,S2", thr="gate S2", sizes=S512, alone="S", note="1536 x 32 = 49 152")
din("din_T1537_s2", 32, 1534, 1, 3, 12, "beyond", "din_fused 8,S2,h1,C3", thr="gate S2", sizes=S512, alone="S")
# rule 13: units per lane group against the pipeline depth 2
for _D, _ngb, _ks in ((32, 32, (1, 2, 3, 4)), (64, 16, (1, 2, 3))):
    for _k in _ks:
        din("din_%d_U%d" % (_D, _k * _ngb), _D, _k * _ngb, 1, 3, 13, "at", "din_pipe %d,S1" % (_D // 4), thr="D%d K%d" % (_D, _k))
        din("din_%d_U%d" % (_D, _k * _ngb + 1), _D, _k * _ngb + 1, 1, 3, 13, "beyond", "din_pipe %d,S1" % (_D // 4), thr="D%d K%d" % (_D, _k),
            note="U = %d: one lane group holds %d units" % (_k * _ngb + 1, _k + 1))


# ---- DIEN ---------------------------------------------------------------------------------------------------------------------
def dien(name, D, H, U, rule, side, form, thr="", sizes=(33, 2), L=1, top=(24, 2), **kw):
    _case(name, "dien", D, U + 3, L, sizes, rule, side, form, thr=thr, H=(H,), top=top, **kw)


# rule 14: the corners of dien.hip's instances, and one step outside each
dien("dien_16_16", 16, 16, 5, 14, "at", "one 4,16 + dien_mfma 16,16,top", thr="D")
dien("dien_16_64", 16, 64, 5, 14, "at", "one 4,16 + dien_mfma 16,64,top", thr="H")
dien("dien_64_16", 64, 16, 5, 14, "at", "one 16,16 + dien_mfma 64,16,top", thr="H%16")
dien("dien_64_64", 64, 64, 5, 14, "at", "one 16,16 + dien_mfma 64,64,top", thr="H")
dien("dien_32_32_split0", 32, 32, 5, 14, "at", "one 8,16 + dien_mfma 32,32,top", thr="D", dien_mfma=1)
dien("dien_12_16", 12, 16, 5, 14, "beyond", "ring 4,sequential + dien_any 12,16", thr="D")
dien("dien_128_16", 128, 16, 5, 14, "beyond", "one 32,16 + dien_any 128,16", thr="D")
dien("dien_32_128", 32, 128, 5, 14, "beyond", "one 8,16 + dien_any 32,128", thr="H")
dien("dien_32_4", 32, 4, 5, 14, "beyond", "one 8,16 + dien_any 32,4", thr="H")
dien("dien_32_48", 32, 48, 5, 14, "beyond", "one 8,16 + dien_any 32,48", thr="H")
for _m in (0, 1, 2):
    dien("dien_16_8_mfma%d" % _m, 16, 8, 5, 14, "beyond", "one 4,16 + dien_valu 16,8", thr="H%16", dien_mfma=_m)
dien("dien_64_8", 64, 8, 5, 14, "beyond", "one 16,16 + dien_valu 64,8", thr="H%16")
dien("dien_32_16_mfma3", 32, 16, 5, 14, "beyond", "one 8,16 + dien_any 32,16", thr="dien_mfma", dien_mfma=3)
dien("dien_32_16_mfma0", 32, 16, 5, 14, "beyond", "one 8,16 + dien_valu 32,16", thr="dien_mfma", dien_mfma=0)
dien("dien_32_16_mfma2", 32, 16, 5, 14, "at", "one 8,16 + dien_mfma 32,16,top", thr="dien_mfma")
# rule 15: the top MLP inside the recurrence's launch
dien("top_4_layers", 32, 32, 5, 15, "at", "one 8,16 + dien_mfma 32,32,top", thr="layers", top=(24, 16, 8, 2))
dien("top_5_layers", 32, 32, 5, 15, "beyond", "one 8,16 + dien_mfma 32,32", thr="layers", top=(24, 16, 8, 8, 2))
dien("top_256", 32, 32, 5, 15, "at", "one 8,16 + dien_mfma 32,32,top", thr="width", top=(256, 2))
dien("top_260", 32, 32, 5, 15, "beyond", "one 8,16 + dien_mfma 32,32", thr="width", top=(260, 2))
dien("top_in_256", 64, 64, 5, 15, "at", "one 16,16 + dien_mfma 64,64,top", thr="width", top=(256, 256, 2),
     note="first layer 64 + 3 x 64 = 256 wide; 2 x 16 x 256 + 4 x 16 x 64 floats = 48 KB: the 60 KB LDS test is shadowed")
dien("top_30", 32, 32, 5, 15, "beyond", "one 8,16 + dien_mfma 32,32", thr="width%4", top=(30, 2))
dien("top_28", 32, 32, 5, 15, "at", "one 8,16 + dien_mfma 32,32,top", thr="width%4", top=(28, 2))
dien("top_off", 32, 32, 5, 15, "beyond", "one 8,16 + dien_mfma 32,32", thr="dien_fuse_top", dien_fuse_top=0)
dien("top_valu", 32, 8, 5, 15, "beyond", "one 8,16 + dien_valu 32,8", thr="dien_fuse_top")
dien("top_on", 32, 32, 5, 15, "at", "one 8,16 + dien_mfma 32,32,top", thr="dien_fuse_top")
# rule 16: workgroup edges
for _n, _side in ((15, "at"), (16, "at"), (17, "beyond")):
    dien("wg_%d" % _n, 32, 64, 5, 16, _side, "one 8,16 + dien_mfma 32,64,top", thr="16 samples", sizes=(_n,))
for _n, _side in ((3, "at"), (4, "at"), (5, "beyond")):
    dien("wg_valu_%d" % _n, 32, 64, 5, 16, _side, "one 8,16 + dien_valu 32,64", thr="4 samples", sizes=(_n,), dien_mfma=0)
dien("wg_shared", 32, 64, 5, 16, "beyond", "one 8,16 + dien_mfma 32,64,top", thr="shared", sizes=(5, 7, 9))
dien("wg_shared_valu", 32, 16, 5, 16, "beyond", "one 8,16 + dien_valu 32,16", thr="shared", sizes=(5, 1, 9), dien_mfma=0)
dien("wg_ragged", 32, 64, 5, 16, "at", "ring 8,split + dien_mfma 32,64,top", thr="shared", sizes=(21, 12), L=RAGGED)
for _u, _side in ((1, "at"), (2, "at"), (4, "at"), (5, "beyond")):
    dien("seq_%d" % _u, 32, 32, _u, 16, _side, "one 8,16 + dien_mfma 32,32,top", thr="prefetch", sizes=(19, 2))
dien("seq_3_valu", 32, 32, 3, 16, "at", "one 8,16 + dien_valu 32,32", thr="prefetch", sizes=(19, 2), dien_mfma=0)

BY_NAME = {c.name: c for c in CASES}
NAMES = [c.name for c in CASES]
RULES = {"sls": range(1, 9), "din": range(9, 14), "dien": range(14, 17)}
SHADOWED = {15: "dien_top_fusable's LDS test (two 16-row activation buffers + four 16 x H state buffers <= 60 KB) cannot fail "
                "while every width <= 256 and H <= 64: 32 KB + 16 KB",
            12: "the S = 1 gate (T = 2457 | 2458) has no case: two engines of ~2 460 tables and units for one pair"}

# every kernel form launch_sls_e / launch_din_fused / mlp_din / mlp_dien can log in the product build, as token prefixes
# (fp32 tables, no non-temporal hint); the catalogue must show each one, or list it in NOT_SHOWN with the reason
PRODUCT_FORMS = (["sls_any_kernel["] +
                 ["sls_flatc_kernel<%d,%d>[" % (g, nl) for g in (8, 16, 32) for nl in (5, 10, 20)] +
                 ["sls_flat_kernel<%d,%d,bpw%d>[" % (g, nl, b) for g in (8, 16, 32) for nl in (5, 10, 20) for b in (1, 2, 4) if b == 1 or nl <= 10] +
                 ["sls_one_kernel<%d,%d>[" % (g, bw) for g in (4, 8, 16, 32) for bw in (16, 64)] +
                 ["sls_kernel<%d,%s>[" % (g, o) for g in (2, 4, 8, 16, 32, 64) for o in ("sequential", "split")] +
                 ["din_attention_any_kernel[", "din_attention_kernel["] +
                 ["din_pipe_kernel<%d,S%d,P2>[" % (g, s) for g in (8, 16) for s in (1, 2, 4)] +
                 ["din_fused_kernel<%d,S%d,h%d,C%d>[" % (g, s, h, c) for g in (8, 16) for s in (1, 2, 4) for h in (1, 2, 4) for c in (3, 4)] +
                 ["dien_rnn_any_kernel<", "dien_rnn_kernel<"] +
                 ["dien_rnn_mfma_kernel<%d,%d%s>[" % (d, h, t) for d in (16, 32, 64) for h in (16, 32, 64) for t in ("", ",top")])
KERNEL_NAMES = GATHER_TOKENS + SECOND_TOKENS


def sweeps(case):
    """the option sweeps the GPU test runs on top of a case's own options (every one must give the case's own bits)"""
    if case.kind == "dien":
        return [dict(dien_mfma=m, dien_fuse_top=f) for m, f in ((1, 1), (2, 0), (2, 1), (1, 0), (0, 1), (0, 0), (3, 1), (3, 0))]
    if case.kind == "din" and din_class(case) == "fused":
        return [dict(din_s=s, din_pipe=p) for s in (0, 1, 2, 4) for p in (1, 0)]
    return []


def predicted_tokens():
    """every token prefix the rules say a run of the catalogue shows: each case's own options, its sweeps, its queries alone"""
    out = set()
    for c in CASES:
        variants = [c] + [c._replace(opts=tuple(sorted(dict(options(c), **o).items()))) for o in sweeps(c)]
        for v in variants:
            out.update(render(EXPECTED[c.kind](v)))
        if sum(1 for n in c.sizes if n) >= 2:
            for i, n in enumerate(c.sizes):
                if n:
                    out.update(render(EXPECTED[c.kind](c, only=i)))
    return out


# The template-argument combinations of PRODUCT_FORMS that a run of the catalogue does NOT show (own options, sweeps, queries
# alone), pinned: the closing GPU test asserts that the run's list is exactly this one, the CPU hygiene test that the rules
# predict it.  All of them are instances of kernels whose other instances run; what each would need:
NOT_SHOWN = (
    # the phased flat form with one bag per wave ("sls_flat" 2) beyond D = 32, and the 10-load rung with shared waves at
    # G = 8 / 32 (forced "sls_bpw" with longer bags): flat2 / flat2_nl20 / force_bpw4_nl10 show the same code at other G
    "sls_flat_kernel<8,5,bpw1>[", "sls_flat_kernel<8,10,bpw4>[", "sls_flat_kernel<16,5,bpw1>[", "sls_flat_kernel<16,10,bpw1>[",
    "sls_flat_kernel<16,10,bpw2>[", "sls_flat_kernel<16,20,bpw1>[", "sls_flat_kernel<32,5,bpw1>[", "sls_flat_kernel<32,10,bpw1>[",
    "sls_flat_kernel<32,10,bpw2>[", "sls_flat_kernel<32,10,bpw4>[", "sls_flat_kernel<32,20,bpw1>[",
    "sls_one_kernel<32,64>[",                                        # D = 128 with 64 samples per wave
    # hidden width 4 with bags of 4 rows or ragged ones (h2 and h1 show C4, h4 shows C3)
    "din_fused_kernel<8,S1,h4,C4>[", "din_fused_kernel<8,S2,h4,C4>[", "din_fused_kernel<8,S4,h4,C4>[",
    "din_fused_kernel<16,S1,h4,C4>[", "din_fused_kernel<16,S2,h4,C4>[", "din_fused_kernel<16,S4,h4,C4>[",
    # H = 32 away from D = 32 (the corners and D = 32 are shown)
    "dien_rnn_mfma_kernel<16,32>[", "dien_rnn_mfma_kernel<16,32,top>[", "dien_rnn_mfma_kernel<64,32>[", "dien_rnn_mfma_kernel<64,32,top>[",
)


def not_shown():
    """the template-argument combinations the product can launch that no case's own form names (the closing GPU test
    lists them; every kernel NAME is shown)"""
    named = [p for c in CASES for p in c.expect]
    return [f for f in PRODUCT_FORMS if not any(p.startswith(f) for p in named)]


# ---- building a case -------------------------------------------------------------------------------------------------------------
def engine_key(c):
    return (c.kind, c.D, c.T, c.H, c.top)


def max_lookups(key):
    return max(max(RAGGED_MAX if L == RAGGED else L for L in c.L) for c in CASES if engine_key(c) == key)


class Tables(object):
    """The tables of one engine: per table r rows uniform(-1, 1), then r rows of small integers (|v| <= 8: every summation
    order is exact in fp32, and in fp16), then ONE row of NaN that no valid bag names."""

    def __init__(self, key):
        kind, D, T, H, top = key
        rng = np.random.RandomState(zlib.crc32(repr(key).encode()) % (1 << 31))
        small = T > 16
        self.rows = [(37 if small else 203) + (t % 5) * 7 for t in range(T)]
        self.W = []
        for r in self.rows:
            W = np.empty((2 * r + 1, D), np.float32)
            W[:r] = rng.uniform(-1, 1, (r, D))
            W[r:2 * r] = rng.randint(-8, 9, (r, D))
            W[2 * r] = np.nan
            self.W.append(W)

    def table_rows(self):
        return [W.shape[0] for W in self.W]


class Staged(object):
    """The staged batches of one case: batch b holds B_MAX samples of bag length L[b]; stage(b, n, integer) points every bag
    beyond sample n at the NaN row, and -- integer pass -- every other bag at the integer rows."""

    def __init__(self, case, tables):
        self.case, self.tables = case, tables
        rng = np.random.RandomState(zlib.crc32(case.name.encode()) % (1 << 31))
        self.nb = min(len(case.sizes), N_BATCH)
        self.lens, self.idx = [], []
        for b in range(self.nb):
            L = case.L[b]
            lens, idx = [], []
            for t in range(case.T):
                l = rng.randint(0, RAGGED_MAX + 1, B_MAX).astype(np.int32) if L == RAGGED else np.full(B_MAX, L, np.int32)
                if L == RAGGED and t == 1:
                    l[:3] = 0                       # empty bags at the front of a query
                i = rng.randint(0, tables.rows[t], int(l.sum())).astype(np.int64)
                if i.size:
                    i[0], i[-1] = 0, tables.rows[t] - 1       # first and last row of every table
                lens.append(l)
                idx.append(i)
            self.lens.append(lens)
            self.idx.append(idx)

    def jobs(self):
        """(batch, size) per query of the set"""
        return [(i % self.nb, n) for i, n in enumerate(self.case.sizes)]

    def need(self):
        """batch -> the largest prefix a query of the set reads"""
        need = {}
        for b, n in self.jobs():
            need[b] = max(need.get(b, 0), n)
        return need

    def stage(self, b, n, integer=False):
        """-> (idx, lens) of batch b with every bag beyond sample n naming the NaN row"""
        out = []
        for t in range(self.case.T):
            i = self.idx[b][t] + (self.tables.rows[t] if integer else 0)
            i[int(self.lens[b][t][:n].sum()):] = 2 * self.tables.rows[t]
            out.append(i)
        return out, self.lens[b]

    def query(self, b, n, integer=False):
        """-> (idx, lens) of the query's own bags"""
        idx = [self.idx[b][t][:int(self.lens[b][t][:n].sum())] + (self.tables.rows[t] if integer else 0) for t in range(self.case.T)]
        return idx, [l[:n] for l in self.lens[b]]


def sls64(W, idx, lens):
    """float64 pooled rows, and the sum of the magnitudes"""
    W = np.asarray(W, np.float64)
    bag = np.repeat(np.arange(len(lens)), lens)
    out = np.zeros((len(lens), W.shape[1]))
    mag = np.zeros_like(out)
    np.add.at(out, bag, W[idx])
    np.add.at(mag, bag, np.abs(W[idx]))
    return out, mag


class Weights(object):
    """The model around the gather: xavier weights (uniform(+-sqrt(3 / fan_in)), the scale at which test_gpu_parity.py's bars
    for the DIN / DIEN rows hold), small biases.  DIN / DIEN: the top MLP's LAST layer has non-negative weights and biases of
    0.5, so that every output is a sum of non-negative terms and >= 0.5 -- the outputs are held to a purely RELATIVE bar
    (rtol 1e-4, no floor: test_din_fused_and_two_launch_forms_match_oracle's), which says nothing about an output that is
    the small difference of large terms."""

    def __init__(self, key):
        kind, D, T, H, top = key
        rng = np.random.RandomState(zlib.crc32(("w" + repr(key)).encode()) % (1 << 31))

        def mlp(ln):
            return [(rng.uniform(-np.sqrt(3.0 / ln[l]), np.sqrt(3.0 / ln[l]), (ln[l + 1], ln[l])).astype(np.float32),
                     rng.normal(0, 0.05, ln[l + 1]).astype(np.float32)) for l in range(len(ln) - 1)]
        def positive_last(layers):
            W, bias = layers[-1]
            return layers[:-1] + [(np.abs(W), np.full_like(bias, 0.5))]
        self.kind, self.D, self.T = kind, D, T
        self.att = self.rnn = None
        if kind == "sls":
            self.ln_bot, self.ln_top = [8, D], [D * (T + 1), 4, 1]
            self.bot, self.top = mlp(self.ln_bot), mlp(self.ln_top)
            self.dense = rng.uniform(-1, 1, (B_MAX, 8)).astype(np.float32)
        elif kind == "din":
            self.ln_bot = [3 * D] + list(H) + [D]
            self.ln_top = [4 * D] + list(top)
            self.att = [mlp(self.ln_bot) for _ in range(T - 3)]
            self.top = positive_last(mlp(self.ln_top))
        else:
            Hh = H[0]
            self.ln_bot = [D, Hh]
            self.ln_top = [Hh + 3 * D] + list(top)
            z = np.zeros(Hh, np.float32)
            xav = lambda n, k: rng.uniform(-np.sqrt(3.0 / k), np.sqrt(3.0 / k), (n, k)).astype(np.float32)
            self.rnn = [[(xav(Hh, din), z), (xav(Hh, Hh), z)] for din in (D, Hh)]          # per layer: i2h, gates_t
            self.top = positive_last(mlp(self.ln_top))

    def oracle_model(self, tables):
        if self.kind == "din":
            return orc.Model(orc.MODEL_DIN, tables, [0], [], self.ln_top, self.top, ln_att=self.ln_bot, att=self.att)
        if self.kind == "dien":
            rnn = [a for layer in self.rnn for a in (layer[0][0], layer[0][1], layer[1][0], layer[1][1])]
            return orc.Model(orc.MODEL_DIEN, tables, [0], [], self.ln_top, self.top, rnn=rnn)
        return orc.Model(orc.MODEL_DLRM, tables, self.ln_bot, self.bot, self.ln_top, self.top, interaction_op=orc.INTERACT_CAT, sigmoid_top=2)
