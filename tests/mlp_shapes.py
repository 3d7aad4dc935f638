"""The MLP launch planner's boundary catalogue (a plain module: no tests in it).

csrc/mlp_plan.hip (plan_chains / plan_layer / stream_plan / chain_plan / pick_kc), csrc/gemm.hip (gemm_plan) and
csrc/engine_dispatch.hip (run_mlp / dlrm_one_launch / mlp_ncf / mlp_dense) pick the kernel form of every MLP launch from about a
dozen thresholds.  CASES holds one small model on each side of every one of them (DESIGN.md 3.1 lists the thresholds and
names the cases).  The rule numbers:

   1  a chain holds <= DRS_MAX_CHAIN = 6 layers, a fused launch <= 12
   2  stream4_kernel's step table holds DRS_MAX_STREAM_TILES = 96 steps; stream_kernel's 128-column tile table 96 tiles
   3  stream4_kernel needs every N <= 4080 and every K <= 4096
   4  the LDS layout must fit kLdsBudget = 156 KB (stream_plan, then chain_plan / pick_kc, else the layer alone)
   5  the stream forms need every layer input width (and d_out) to be a multiple of 4
   6  tiles per wave 1 / 2 / 4 at N <= 64 / <= 128 / > 128, a second pass above 256 columns (hidden layers: out_pad)
   7  the column-split form: first top layer 128 ... 1024 wide in 64s, slice width in {64, 128, 256}
   8  mlp_rows32: 32 rows per workgroup when the slabs fit the budget, else 16; Q in X0's space (q_in_x0)
   9  K N >= mlp_wide_kn = 262 144: the layer runs alone, as a GEMM form if K >= 64 and N >= 64, else fc_kernel
  10  fc_kernel / chain_kernel <vec | scalar> by K % 4
  11  the summed input (NCF's join), task heads: the zero pad must fall in an existing pass

`expect` / `absent` are literal strings written from those rules, by hand; nothing here restates the planner.  An `expect`
string is "fragment .. fragment ..": ONE token of drs_last_dispatch must start with the first fragment and hold the others
behind it in that order.  An `absent` string must be part of no token.  `launches`: how many MLP launches (stream4 / stream /
chain / fc / gemm tokens) a single query takes.

The step counts quoted in the comments: a layer K -> N whose outputs are padded to P columns in the slab (hidden layers:
P = N rounded up to 64; a chain's last layer: P = N) has etl = ceil(P / 16) column tiles; tiles per wave tpw = 1 / 2 / 4 for
etl <= 4 / <= 8 / more; a pass covers 4 tpw tiles; steps = ceil(etl / (4 tpw)) * ceil(K / 64).  The 128-column tile count of
stream_kernel: ceil(N / 128) * ceil(K / 64).  The budget is 159 744 B = 39 936 floats.

build: Built(case) makes the model's weights, tables and inputs from the case's own seed; the CPU test (oracle against
float64) and the GPU test (engine against oracle) share it.

poison: Built(case, poison=True) and poisoned(net, bs), at the end of this file, put NaN, +-inf and +-3e38 INSIDE valid rows
(tests/test_mlp_nonfinite_cpu.py, tests/test_mlp_nonfinite.py).
"""
import collections
import copy
import re
import zlib

import numpy as np

from deeprecsys_amd import _native as N
from oracle import oracle as orc

Case = collections.namedtuple("Case", "name kind D T L bot top task num_tasks fin rows opts rule thr side expect absent launches")

ROWS_ALL = (1, 15, 16, 17, 31, 32, 33, 100)
ROWS_FEW = (1, 17, 100)
ROWS_32 = (1, 31, 32, 33, 63, 64, 65, 100)
B_MAX = 100

# what every case sets first, so that no expectation depends on what drs_create chose for the model's class
BASE_OPTS = (("mlp_stream", 4), ("mlp_stream_2cu", 0), ("mlp_rows32", 0), ("mlp_nsplit", 0), ("mlp_nsplit_rows", 512),
             ("mlp_gemm_tile", 0), ("mlp_fuse", 1), ("mlp_split", 1), ("mlp_wide_kn", 262144))

CASES = []


def _case(name, kind, D, T, bot, top, rule, side, expect, absent=(), launches=None, rows=ROWS_FEW, L=2, task="",
          num_tasks=0, fin=0, thr="", **opts):
    """thr: which of a rule's thresholds the case stands on, where the rule bundles several (each needs both sides);
    side: at | below | beyond, or "shadowed" (the threshold cannot be reached: the case counts for no side)"""
    ln = lambda s: tuple(int(w) for w in s.split("-")) if s else ()
    CASES.append(Case(name, kind, D, T, L, ln(bot), ln(top), ln(task), num_tasks, fin, tuple(rows), tuple(sorted(opts.items())),
                      rule, thr, side, tuple(expect), tuple(absent), launches))


S4 = "stream4_kernel["          # the plain instance: no <...>

# ---- rule 1: chain depth ---------------------------------------------------------------------------------------------
# 6 + 6 layers: ONE fused launch of 12 (every layer K <= 64, N <= 64: 12 steps)
_case("depth_6_6_fused", "dlrm_cat", 16, 2, "16-32-32-32-32-32-16", "48-32-32-32-32-32-1", 1, "at",
      [S4 + " .. , 12 layers"], ["chain_kernel", ", 6 layers"], launches=1, rows=ROWS_ALL)
# ... with the dot interaction between the chains (F = 8: 16 + 28 = 44 columns)
_case("depth_6_6_fused_dot", "dlrm_dot", 16, 7, "16-32-32-32-32-32-16", "44-32-32-32-32-32-1", 1, "at",
      [S4 + " .. , 12 layers, dot"], ["chain_kernel", "interact_dot_kernel"], launches=1)
# 6 + 7: dlrm_one_launch refuses (nt > 6); bottom chain of 6, top as a run of 6 and the 7th layer alone
_case("depth_6_7_unfused", "dlrm_cat", 16, 2, "16-32-32-32-32-32-16", "48-32-32-32-32-32-32-1", 1, "beyond",
      [S4 + " .. , 6 layers", S4 + " .. , 1 layers"], ["12 layers", "13 layers", ", 7 layers"], launches=3, rows=ROWS_ALL)
# 7-layer bottom MLP: runs of 6 and 1 (through s.H), then the 2-layer top chain
_case("depth_bot_7", "dlrm_cat", 16, 2, "16-32-32-32-32-32-32-16", "48-32-1", 1, "beyond",
      [S4 + " .. , 6 layers", S4 + " .. , 1 layers", S4 + " .. , 2 layers"], [", 7 layers", ", 9 layers"], launches=3)
# 7-layer top MLP behind a 2-layer bottom
_case("depth_top_7", "dlrm_cat", 16, 2, "16-32-16", "48-32-32-32-32-32-32-1", 1, "beyond",
      [S4 + " .. , 2 layers", S4 + " .. , 6 layers", S4 + " .. , 1 layers"], [", 7 layers", ", 9 layers"], launches=3)
# 13-layer W&D top: runs of 6, 6 and 1 -- the second run reads s.H and must write s.Hb
_case("depth_wnd_top_13", "wnd", 16, 3, "16", "64-48-48-48-48-48-48-48-48-48-48-48-48-1", 1, "beyond",
      ["copy_rows_multi_kernel", S4 + " .. , 6 layers", S4 + " .. , 1 layers"], ["13 layers", "12 layers"], launches=3,
      rows=ROWS_ALL, L=1)
# MT-WnD: 2-layer shared top, two heads of 7 layers each (6 + 1, through s.H)
_case("depth_mtwnd_head_7", "mtwnd", 16, 3, "16", "64-48-32", 1, "beyond",
      ["stream_kernel<packed,2cu>[ .. , 2 layers", "stream_kernel<packed,2cu>[ .. , 6 layers", "stream_kernel<packed,2cu>[ .. , 1 layers"],
      [", 7 layers", "stream4_kernel"], launches=5, L=1, task="32-24-24-24-24-24-24-2", num_tasks=2, mlp_stream=2, mlp_stream_2cu=1)

# ---- rule 2: the step table / the tile table hold 96 entries -----------------------------------------------------------
# stream4 steps.  bottom 64-1024-64-1024-64-320-64: 4 + 16 + 4 + 16 + 2 + 5 = 47 (64 -> 1024: etl 64, 4 passes x 1 chunk;
# 1024 -> 64: 1 pass x 16 chunks; 64 -> 320: etl 20, 2 passes; 320 -> 64: 5 chunks); top 512-64-1024-64-1024-64-1:
# 8 + 4 + 16 + 4 + 16 + 1 = 49.  47 + 49 = 96 steps
_case("steps_96", "dlrm_cat", 64, 7, "64-1024-64-1024-64-320-64", "512-64-1024-64-1024-64-1", 2, "at",
      [S4 + " .. , 12 layers"], ["stream_kernel"], launches=1, L=1, thr="steps")
# ... 64 -> 384 (2 passes) and 384 -> 64 (6 chunks): 48 + 49 = 97 steps: stream_kernel on the packed twins; its own
# 128-column tiles number 57 + 57 = 114 > 96: the iterator form (n_table 0)
_case("steps_97", "dlrm_cat", 64, 7, "64-1024-64-1024-64-384-64", "512-64-1024-64-1024-64-1", 2, "beyond",
      ["stream_kernel<packed>[ .. , 12 layers"], ["stream4_kernel"], launches=1, L=1, thr="steps")
# stream_kernel's tile table ("mlp_stream" 2; the <packed,2cu> instance needs the table).  bottom 64-1024-64-1024-64-128-64:
# 8 + 16 + 8 + 16 + 1 + 2 = 51; top 512-64-1024-64-512-64-1: 8 + 8 + 16 + 4 + 8 + 1 = 45.  96 tiles
_case("tiles_96", "dlrm_cat", 64, 7, "64-1024-64-1024-64-128-64", "512-64-1024-64-512-64-1", 2, "at",
      ["stream_kernel<packed,2cu>[ .. , 12 layers"], ["stream4_kernel", "stream_kernel<packed>["], launches=1, L=1,
      thr="tiles", mlp_stream=2, mlp_stream_2cu=1)
# ... bottom 64-1024-64-1024-64-64-64: 50; top 512-64-1024-64-576-64-1: 8 + 8 + 16 + 5 + 9 + 1 = 47.  97 tiles: no table
_case("tiles_97", "dlrm_cat", 64, 7, "64-1024-64-1024-64-64-64", "512-64-1024-64-576-64-1", 2, "beyond",
      ["stream_kernel<packed>[ .. , 12 layers"], ["stream4_kernel", "packed,2cu"], launches=1, L=1, thr="tiles", mlp_stream=2, mlp_stream_2cu=1)

# ---- rule 3: stream4_kernel's N <= 4080 (255 column tiles in 8 bits of a step), K <= 4096 --------------------------------
# (a chain's LAST layer keeps no output slab, so N = 4080 fits LDS; 60 x 4080 = 244 800 < mlp_wide_kn)
_case("n_4080_last", "dlrm_cat", 16, 2, "16-16", "48-60-4080", 3, "at", [S4 + " .. , 3 layers"], ["stream_kernel"], launches=1, thr="n")
_case("n_4081_last", "dlrm_cat", 16, 2, "16-16", "48-60-4081", 3, "beyond", ["stream_kernel<packed>[ .. , 3 layers"],
      ["stream4_kernel"], launches=1, thr="n")
# K = 4096 / 4100 as W&D's first top layer: a 16-row input slab of 4 096 columns is 262 KB -- rule 4 refuses the stream forms
# long before the K limit is reached (the limit is shadowed: DESIGN.md 3.1); chain_kernel, K chunks of 64 double-buffered
# (kc 128: 152 064 B of staging + 8 192 B of slabs > 159 744).  Side "shadowed": they count for neither side of rule 3
_case("k_4096_first_top", "wnd", 16, 4, "4032", "4096-60-1", 3, "shadowed", ["copy_rows_multi_kernel", "chain_kernel<vec,64>[ .. , 2 layers"],
      ["stream"], launches=1, L=1, thr="k")
_case("k_4100_first_top", "wnd", 16, 4, "4036", "4100-60-1", 3, "shadowed", ["copy_rows_multi_kernel", "chain_kernel<vec,64>[ .. , 2 layers"],
      ["stream"], launches=1, L=1, thr="k")

# ---- rule 4: the LDS budget ---------------------------------------------------------------------------------------------
# 4000 -> 60 as DLRM's first top layer (8 features of 500): the 16 x 4 040 slab does not fit; both chains in ONE chain_kernel
_case("lds_4000_to_60", "dlrm_cat", 500, 7, "16-500", "4000-60-1", 4, "beyond", ["chain_kernel<vec,64>[ .. , 3 layers"], ["stream"],
      launches=1, L=1)
# 60 -> 4000 -> 1: the 4 000-wide hidden slab fits neither the stream forms nor chain_kernel (2 x 16 x 4 004 floats): the
# fused launch and the 2-layer chain are refused; 60 -> 4000 alone is a stream4 launch (last layer: no slab), 4000 -> 1 alone
# a chain_kernel (kc 128: 152 064 + 1 024 B fit, 32 rounds)
_case("lds_60_to_4000", "dlrm_cat", 12, 4, "16-12", "60-4000-1", 4, "beyond",
      [S4 + " .. , 1 layers", "chain_kernel<vec,128>[ .. , 1 layers"], [", 2 layers", ", 3 layers"], launches=3, L=1)
# the same depth with slabs that fit: one fused launch
_case("lds_fits", "dlrm_cat", 12, 4, "16-12", "60-400-1", 4, "at", [S4 + " .. , 3 layers"], ["chain_kernel"], launches=1, L=1)

# chain_kernel's K chunk: the fewest rounds that fit beside the slabs, the smaller chunk on a tie; one round is single-buffered.
# 250-30-1 (scalar: 250 % 4 != 0): slabs 2 x 16 x 36 floats = 4 608 B; kc 256 is ONE round, single buffer: 4 x 144 x 260 =
# 149 760 B, together 154 368 <= 159 744; kc 192 would need two rounds.  The rungs 192, 128 and 64 are pinned by hidden_129
# (one round of 192: 112 896 + 17 408 B; 256 does not fit beside the slabs), hidden_65 (one round each of 256 / 192 / 128:
# the smallest) and hidden_257 (only 64 double-buffered fits beside 33 792 B of slabs)
_case("kc_256_single_buffer", "wnd", 16, 1, "234", "250-30-1", 4, "beyond", ["copy_rows_multi_kernel", "chain_kernel<scalar,256>[ .. , 2 layers"],
      ["stream"], launches=1, L=1)

# ---- rule 5: input widths that are not multiples of 4 -------------------------------------------------------------------
for _w in (30, 6):
    # cat: the fused pair of chains as ONE chain_kernel<scalar>
    _case("odd_%d_cat" % _w, "dlrm_cat", 16, 3, "16-%d-16" % _w, "64-%d-1" % _w, 5, "beyond",
          ["chain_kernel<scalar .. , 4 layers"], ["stream"], launches=1, rows=ROWS_ALL)
    # dot: chain_kernel has no interaction: bottom chain, interact_dot_kernel, top chain
    _case("odd_%d_dot" % _w, "dlrm_dot", 16, 7, "16-%d-16" % _w, "44-%d-1" % _w, 5, "beyond",
          ["chain_kernel<scalar .. , 2 layers", "interact_dot_kernel"], ["stream", ", 4 layers"], launches=2, rows=ROWS_ALL)
_case("even_32_dot", "dlrm_dot", 16, 7, "16-32-16", "44-32-1", 5, "at", [S4 + " .. , 4 layers, dot"],
      ["chain_kernel", "interact_dot_kernel"], launches=1, rows=ROWS_ALL)

# ---- rule 6: tiles per wave / passes of a HIDDEN layer (padded to 64 columns in the slab) ------------------------------------
# (65 / 129 / 257 are not multiples of 4: rule 5 sends them to chain_kernel<scalar>, so they say nothing about tpw3 / out_pad --
#  80 / 144 / 272 do that work; the odd ones pin chain_kernel's kc rungs instead, see rule 4)
HIDDEN = {64: ("at", [S4 + " .. , 5 layers"], ["chain_kernel"]),
          65: ("beyond", ["chain_kernel<scalar,128>[ .. , 5 layers"], ["stream"]),
          80: ("beyond", [S4 + " .. , 5 layers"], ["chain_kernel"]),
          128: ("at", [S4 + " .. , 5 layers"], ["chain_kernel"]),
          129: ("beyond", ["chain_kernel<scalar,192>[ .. , 5 layers"], ["stream"]),
          144: ("beyond", [S4 + " .. , 5 layers"], ["chain_kernel"]),
          256: ("at", [S4 + " .. , 5 layers"], ["chain_kernel"]),
          257: ("beyond", ["chain_kernel<scalar,64>[ .. , 5 layers"], ["stream"]),
          272: ("beyond", [S4 + " .. , 5 layers"], ["chain_kernel"])}
for _w, (_side, _expect, _absent) in sorted(HIDDEN.items()):
    _case("hidden_%d" % _w, "dlrm_cat", 16, 3, "16-%d-16" % _w, "64-%d-%d-1" % (_w, _w), 6, _side, _expect, _absent, launches=1,
          rows=ROWS_ALL)

# ---- rule 7: the column-split form ----------------------------------------------------------------------------------------
# slices of width / S for S = 4 (when asked for), then 2; a slice must be 64, 128 or 256 columns wide
NSPLIT_FORM = {(128, 2): ("at", "stream4_kernel<nsplit2>[", ["chain_kernel"]),                    # 2 x 64
               (128, 4): ("at", "stream4_kernel<nsplit2>[", ["chain_kernel"]),
               (192, 2): ("beyond", S4, ["chain_kernel", "nsplit"]),                             # 96, 48: no slice width
               (192, 4): ("beyond", S4, ["chain_kernel", "nsplit"]),
               (256, 2): ("at", "stream4_kernel<nsplit2>[", ["chain_kernel"]),                    # 2 x 128
               (256, 4): ("at", "stream4_kernel<nsplit4>[", ["chain_kernel"]),                    # 4 x 64
               (384, 2): ("beyond", S4, ["chain_kernel", "nsplit"]),                             # 192, 96
               (384, 4): ("beyond", S4, ["chain_kernel", "nsplit"]),
               (512, 2): ("at", "stream4_kernel<nsplit2>[", ["chain_kernel"]),                    # 2 x 256
               (512, 4): ("at", "stream4_kernel<nsplit4>[", ["chain_kernel"]),                    # 4 x 128
               (768, 2): ("beyond", S4, ["chain_kernel", "nsplit"]),                             # 384, 192
               (768, 4): ("beyond", S4, ["chain_kernel", "nsplit"]),
               (1024, 2): ("beyond", S4, ["chain_kernel", "nsplit"]),                            # 512: none
               (1024, 4): ("at", "stream4_kernel<nsplit4>[", ["chain_kernel"])}                   # 4 x 256
for (_w, _s), (_side, _form, _absent) in sorted(NSPLIT_FORM.items()):
    _case("nsplit%d_%d" % (_s, _w), "dlrm_cat", 16, 3, "16-16", "64-%d-16-1" % _w, 7, _side, [_form + " .. , 4 layers"], _absent,
          launches=1, mlp_nsplit=_s)
_case("nsplit4_rows32", "dlrm_cat", 16, 3, "16-16", "64-256-16-1", 7, "at", ["stream4_kernel<rows32,nsplit4>[ .. , 4 layers"], [],
      launches=1, rows=ROWS_32, mlp_nsplit=4, mlp_rows32=1)
_case("nsplit2_rows32", "dlrm_cat", 16, 3, "16-16", "64-256-16-1", 7, "at", ["stream4_kernel<rows32,nsplit2>[ .. , 4 layers"], [],
      launches=1, rows=ROWS_32, mlp_nsplit=2, mlp_rows32=1)

# ---- rule 8: 32 rows per workgroup --------------------------------------------------------------------------------------
# single chain 1024-128-64-1: X0 32 x 1 032 + P 32 x 136 floats, Q (64 wide) in X0's space, 196 of biases, the step table 384
# and the layer table 12 x 22: 38 220 floats = 152 880 B (a Q slab of its own, 32 x 72 more, would not fit 39 936 floats)
_case("rows32_q_in_x0", "wnd", 16, 4, "960", "1024-128-64-1", 8, "at", ["stream4_kernel<rows32>[ .. , 3 layers, 152880 B lds]"], [], launches=1,
      rows=ROWS_32, L=1, mlp_rows32=1)
# single chain 64-64-128-1: Q (128 wide) is wider than X0 (64): a slab of its own: 32 x (72 + 72 + 136) + 196 + 384 + 264 =
# 9 804 floats = 39 216 B (in X0's space it would be 32 x 136 floats less)
_case("rows32_q_own_slab", "wnd", 16, 3, "16", "64-64-128-1", 8, "at", ["stream4_kernel<rows32>[ .. , 3 layers, 39216 B lds]"], [], launches=1,
      rows=ROWS_32, L=1, mlp_rows32=1)
_case("rows32_fused", "dlrm_cat", 16, 3, "16-32-16", "64-32-1", 8, "at", ["stream4_kernel<rows32>[ .. , 4 layers"], [], launches=1,
      rows=ROWS_32, mlp_rows32=1)
# single chain 1280-192-64-1: X0 alone is 32 x 1 288 = 41 216 floats > 39 936: 16 rows (20 608 + 3 200 + 1 152 fit)
_case("rows32_budget_single", "wnd", 16, 4, "1216", "1280-192-64-1", 8, "beyond", [S4 + " .. , 3 layers"], ["rows32"], launches=1,
      rows=ROWS_32, L=1, mlp_rows32=1)
# fused 16-64 | 512-448-256-1: 32 x (72 + 520 + 456 + 264) = 41 984 floats > 39 936: 16 rows
_case("rows32_budget_fused", "dlrm_cat", 64, 7, "16-64", "512-448-256-1", 8, "beyond", [S4 + " .. , 4 layers"], ["rows32"], launches=1,
      rows=ROWS_32, L=1, mlp_rows32=1)

# ---- rule 9: wide layers run alone -----------------------------------------------------------------------------------------
# 512 x 512 = 262 144 exactly: a GEMM launch between two chains; 512 x 508 and 513 x 511 = 262 143 stay in the chain
_case("wide_512x512", "dlrm_cat", 128, 3, "16-128", "512-512-64-1", 9, "at",
      [S4 + " .. , 1 layers", "gemm_kernel< .. 512x512]", S4 + " .. , 2 layers"], [", 4 layers", "fc_kernel"], launches=3,
      rows=ROWS_ALL, L=1)
_case("wide_512x508", "dlrm_cat", 128, 3, "16-128", "512-508-64-1", 9, "below", [S4 + " .. , 4 layers"], ["gemm", "fc_kernel"],
      launches=1, rows=ROWS_ALL, L=1)
_case("wide_513x511", "wnd", 16, 1, "497", "513-511-1", 9, "below", ["chain_kernel<scalar .. , 2 layers"], ["gemm", "fc_kernel", "stream"],
      launches=1, L=1)
# a wide layer without a GEMM form: N < 64 (8192 -> 32) and K < 64 (32 -> 8192, with the former right behind it)
_case("wide_8192x32", "wnd", 16, 4, "8128", "8192-32-1", 9, "at",
      ["copy_rows_multi_kernel", "fc_kernel<vec,128>[ .. 8192x32]", S4 + " .. , 1 layers"], ["gemm", "chain_kernel"], launches=2, L=1)
_case("wide_32x8192x32", "wnd", 16, 1, "16", "32-8192-32-1", 9, "at",
      ["fc_kernel<vec .. 32x8192]", "fc_kernel<vec .. 8192x32]", S4 + " .. , 1 layers"], ["gemm", "chain_kernel"], launches=3, L=1)
# three launches in a row through s.H / s.Hb, the middle one a GEMM of 30 x 32 workgroups in a 12-query set (more than the
# chip holds at once: a GEMM that wrote where it reads would hand late workgroups overwritten inputs -- a stream or chain
# launch reads its 16 rows before it writes them and would not notice)
_case("wide_after_wide", "wnd", 16, 1, "16", "32-8192-2048-1", 9, "at",
      ["fc_kernel<vec .. 32x8192]", "gemm_kernel<1,1>[ .. 8192x2048]", S4 + " .. , 1 layers"], ["chain_kernel"], launches=3, L=1,
      mlp_gemm_tile=11)
# ... in the middle of the bottom MLP, and as the model's last layer (it carries the completion hand-off)
_case("wide_mid_bottom", "dlrm_cat", 64, 1, "16-512-512-64", "128-32-1", 9, "at",
      [S4 + " .. , 1 layers", "gemm_kernel< .. 512x512]", S4 + " .. , 2 layers"], ["fc_kernel", "chain_kernel"], launches=4, L=1)
_case("wide_last_layer", "dlrm_cat", 64, 1, "16-64", "128-512-512", 9, "at", [S4 + " .. , 1 layers", "gemm_kernel< .. 512x512]"],
      ["fc_kernel", "chain_kernel", ", 2 layers"], launches=3, L=1)
# the other GEMM forms, by "mlp_gemm_tile": two workgroups per CU; the 32x32x2 kernel with scalar-base requests (K % 32 == 0),
# without (528 % 32 != 0), and reading W&D's dense columns in place (448 = 14 x 32 dense columns: no copy launch)
_case("wide_gemm_2cu", "dlrm_cat", 128, 3, "16-128", "512-512-64-1", 9, "at", ["gemm_kernel<2,1,2cu>[ .. 512x512]"], ["fc_kernel"],
      launches=3, L=1, mlp_gemm_tile=214)
_case("wide_gemm32_sbase", "dlrm_cat", 128, 3, "16-128", "512-512-64-1", 9, "at", ["gemm32_kernel<2,2,sbase>[ .. 512x512]"],
      ["fc_kernel", "split"], launches=3, L=1, mlp_gemm_tile=322)
_case("wide_gemm32_plain", "wnd", 16, 4, "464", "528-512-64-1", 9, "at", ["copy_rows_multi_kernel", "gemm32_kernel<2,2>[ .. 528x512]"],
      ["fc_kernel", "sbase"], launches=2, L=1, mlp_gemm_tile=322)
_case("wide_gemm32_split", "wnd", 16, 4, "448", "512-512-64-1", 9, "at", ["gemm32_kernel<2,2,sbase,split448>[ .. 512x512]"],
      ["fc_kernel", "copy_rows_multi_kernel"], launches=2, L=1, mlp_gemm_tile=322)

# ---- rule 10: K % 4 --------------------------------------------------------------------------------------------------------
_case("k_640", "wnd", 16, 1, "624", "640-32-1", 10, "at", [S4 + " .. , 2 layers"], ["chain_kernel"], launches=1, rows=ROWS_ALL, L=1)
_case("k_642", "wnd", 16, 1, "626", "642-32-1", 10, "beyond", ["chain_kernel<scalar .. , 2 layers"], ["stream"], launches=1,
      rows=ROWS_ALL, L=1)
_case("wide_8193x32", "wnd", 16, 4, "8129", "8193-32-1", 10, "beyond", ["fc_kernel<scalar,128>[ .. 8193x32]", S4 + " .. , 1 layers"],
      ["gemm", "fc_kernel<vec"], launches=2, L=1)

# ---- rule 11: the summed input, the task heads ----------------------------------------------------------------------------------
# NCF (D = 4): predictor input [4 summed | 128] -> 132 columns, padded to 192: stream4_kernel<sum> zero-fills 188 columns behind
# the summed block in the last branch layer's own pass (etl 12, one pass)
_case("ncf_sum_stream4", "ncf", 4, 4, "", "8-32-128", 11, "at", ["stream4_kernel<sum>[ .. , 3 layers"], ["add_rows_kernel"], launches=1,
      rows=ROWS_ALL, L=1, fin=5)
# stream_kernel: the pad (192 - 4 = 188) must fall in the passes of the 128 outputs (one pass of 128): refused -> add_rows_kernel,
# the branch and the predictor as launches of their own; 124 outputs: 128 - 4 = 124 <= 128 fits
_case("ncf_sum_packed_124", "ncf", 4, 4, "", "8-32-124", 11, "at", ["stream_kernel<packed>[ .. , 3 layers"], ["add_rows_kernel", "stream4"],
      launches=1, rows=ROWS_ALL, L=1, fin=5, mlp_stream=2)
_case("ncf_sum_packed_128", "ncf", 4, 4, "", "8-32-128", 11, "beyond",
      ["add_rows_kernel", "stream_kernel<packed>[ .. , 2 layers", "stream_kernel<packed>[ .. , 1 layers"], [", 3 layers", "stream4"],
      launches=2, rows=ROWS_ALL, L=1, fin=5, mlp_stream=2)
# MT-WnD: three heads 48-20-3 side by side in the output row behind a shared 64-80-48 top
_case("mtwnd_heads", "mtwnd", 16, 3, "16", "64-80-48", 11, "at", ["stream_kernel<packed>[ .. , 2 layers"], ["chain_kernel", "stream4"],
      launches=4, rows=ROWS_ALL, L=1, task="48-20-3", num_tasks=3, mlp_stream=2)
# ... and the instance with two workgroups per CU of stream4_kernel
_case("stream4_2cu", "dlrm_cat", 16, 3, "16-32-16", "64-32-1", 11, "at", ["stream4_kernel<2cu>[ .. , 4 layers"], ["chain_kernel"], launches=1,
      rows=ROWS_ALL, mlp_stream_2cu=1)

BY_NAME = {c.name: c for c in CASES}
NAMES = [c.name for c in CASES]
SIDES = {"at": "at", "below": "other", "beyond": "other", "shadowed": None}     # (None: counts for no side)

# every MLP form of the product build named in launch_plan's table (mlp.hip), as `expect`-style strings
PRODUCT_FORMS = [S4, "stream4_kernel<sum>[", "stream4_kernel<2cu>[", "stream4_kernel<rows32>[", "stream4_kernel<nsplit2>[",
                 "stream4_kernel<nsplit4>[", "stream4_kernel<rows32,nsplit2>[", "stream4_kernel<rows32,nsplit4>[",
                 "stream_kernel<packed>[", "stream_kernel<packed,2cu>[", "chain_kernel<vec", "chain_kernel<scalar", "fc_kernel<vec",
                 "fc_kernel<scalar", "gemm_kernel<", "gemm32_kernel<2,2>[", "gemm32_kernel<2,2,sbase>[", "gemm32_kernel<2,2,sbase,split"]
LAB_FORMS = ["stream_kernel<lds>["]          # reachable with the lab build's "mlp_stream" 1 only
UNREACHABLE = {}                             # form -> reason (none: every product form is reached by a case above)
MLP_TOKENS = ("stream4_kernel", "stream_kernel", "chain_kernel", "fc_kernel", "gemm_kernel", "gemm32_kernel", "gemm_bf16_kernel")


def matches(token, pattern):
    """does the dispatch-log token start with the pattern's first fragment and hold the others behind it, in order?"""
    return re.match(".*".join(re.escape(f) for f in pattern.split(" .. ")), token) is not None


def check_dispatch(case, log):
    """-> list of complaints (empty: the launch set took exactly the forms the case stands for)"""
    bad = []
    for pat in case.expect:
        if not any(matches(t, pat) for t in log):
            bad.append("missing %r" % pat)
    for pat in case.absent:
        if any(pat in t for t in log if not t.startswith("set[")):
            bad.append("unexpected %r" % pat)
    if case.launches is not None:
        n = sum(1 for t in log if t.startswith(MLP_TOKENS))
        if n != case.launches:
            bad.append("%d MLP launches, expected %d" % (n, case.launches))
    return bad


def options(case):
    opts = collections.OrderedDict(BASE_OPTS)
    opts.update(case.opts)
    return opts


# ------------------------------------------------------------------------------------------------------------------------------
KIND = {"dlrm_cat": N.MODEL_DLRM, "dlrm_dot": N.MODEL_DLRM, "wnd": N.MODEL_WND, "mtwnd": N.MODEL_MTWND, "ncf": N.MODEL_NCF}


class Built(object):
    """One catalogue model: weights normal(0, 1 / sqrt(K)), biases normal(0, 0.1), tables and dense inputs uniform(-1, 1).
    Every table carries one extra LAST row of NaN that no valid bag names: stage(bs) points the bags beyond bs at it.
    poison=True: the tables of poison_tables() carry the POISON_ROWS in front of that NaN row (no valid bag names them
    either; poisoned(net, bs) points bags of its hot samples at them).  Everything else is drawn as without."""

    def __init__(self, case, seed=None, poison=False):
        self.case = c = case
        self.kind = KIND[c.kind]
        self.dot = c.kind == "dlrm_dot"
        rng = np.random.RandomState(zlib.crc32(c.name.encode()) % (1 << 31) if seed is None else seed)
        self.rows = [41 + 7 * t for t in range(c.T)] if c.D > 256 else [301 + 17 * t for t in range(c.T)]
        self.tables = []
        for r in self.rows:
            W = rng.uniform(-1, 1, (r + 1, c.D)).astype(np.float32)
            W[r] = np.nan
            self.tables.append(W)
        self.nan_row = list(self.rows)           # per table: the index of its all-NaN row
        self.poison_row = {}                     # table -> the index of its first poison row
        self.w = {}

        def mlp(which, ln):
            for l in range(len(ln) - 1):
                self.w[(which, l)] = (rng.normal(0, 1.0 / np.sqrt(ln[l]), (ln[l + 1], ln[l])).astype(np.float32),
                                      rng.normal(0, 0.1, ln[l + 1]).astype(np.float32))
        if self.kind == N.MODEL_DLRM:
            mlp(N.MLP_BOT, c.bot)
        mlp(N.MLP_TOP, c.top)
        for k in range(c.num_tasks):
            mlp(N.MLP_TASK0 + k, c.task)
        if self.kind == N.MODEL_NCF:
            mlp(N.MLP_FINAL, (c.D + c.top[-1], c.fin))
        self.m_den = c.bot[0] if self.kind != N.MODEL_NCF else 0
        self.dense = rng.uniform(-1, 1, (B_MAX, self.m_den)).astype(np.float32) if self.m_den else None
        self.idx = [rng.randint(0, self.rows[t], size=B_MAX * c.L).astype(np.int64) for t in range(c.T)]
        self.lens = [np.full(B_MAX, c.L, np.int32) for _ in range(c.T)]
        # the sigmoid sits on the last layer of a narrow output (DLRM / W&D: the top MLP's, MT-WnD: every head's); NCF has none
        last = c.task if self.kind == N.MODEL_MTWND else c.top
        self.sigmoid_top = len(last) - 1 if (self.kind != N.MODEL_NCF and last[-1] < 8) else -1
        self.ln_bot = list(c.bot) if self.kind != N.MODEL_NCF else [1]
        if poison:
            # (a stream of its own, after everything else is drawn: the clean model is the one the boundary tests build)
            prng = np.random.RandomState(zlib.crc32(("poison " + c.name).encode()) % (1 << 31))
            for t in self.poison_tables():
                P = poison_rows(prng, c.D)
                self.poison_row[t] = self.rows[t]
                self.nan_row[t] = self.rows[t] + len(P)
                self.tables[t] = np.ascontiguousarray(np.concatenate([self.tables[t][:-1], P, self.tables[t][-1:]]))

    # -- the engine's view ---------------------------------------------------------------------------------------------------
    def table_rows(self):
        return [int(W.shape[0]) for W in self.tables]

    def poison_tables(self):
        """the tables that carry poison rows, in the order the hot samples take them: NCF one of the concatenated pair (the MLP
        branch's input: its 5th hot sample, `huge`, can overflow there -- K = 2 D) and one of the summed pair (rule 11's join);
        every other model its last table (DLRM-dot: the last pairs of the interaction)"""
        return (2, 0) if self.kind == N.MODEL_NCF else (self.case.T - 1,)

    def stage(self, bs):
        """(dense, idx, lens) of the whole staged batch with everything beyond row bs poisoned: NaN dense rows, bags of the NaN row"""
        c = self.case
        dense = None
        if self.dense is not None:
            dense = self.dense.copy()
            dense[bs:] = np.nan
        idx = []
        for t in range(c.T):
            i = self.idx[t].copy()
            i[bs * c.L:] = self.nan_row[t]
            idx.append(i)
        return dense, idx, self.lens

    def act(self, which, l):
        if which == N.MLP_BOT or self.kind == N.MODEL_NCF:
            return N.ACT_RELU
        if self.kind == N.MODEL_MTWND and which == N.MLP_TOP:
            return N.ACT_RELU
        return N.ACT_SIGMOID if l + 1 == self.sigmoid_top else N.ACT_RELU

    def layers(self, which):
        c = self.case
        if which == N.MLP_BOT:
            return c.bot if self.kind == N.MODEL_DLRM else ()
        if which == N.MLP_TOP:
            return c.top
        if which == N.MLP_FINAL:
            return (c.D + c.top[-1], c.fin)
        return c.task

    def oracle_model(self):
        c = self.case
        ws = lambda which, ln: [self.w[(which, l)] for l in range(len(ln) - 1)]
        if self.kind == N.MODEL_NCF:
            return orc.Model(orc.MODEL_NCF, self.tables, [0], [], list(c.top), ws(N.MLP_TOP, c.top), final=self.w[(N.MLP_FINAL, 0)])
        if self.kind == N.MODEL_MTWND:
            return orc.Model(orc.MODEL_MTWND, self.tables, list(c.bot), [], list(c.top), ws(N.MLP_TOP, c.top),
                             sigmoid_top=self.sigmoid_top, ln_task=list(c.task),
                             tasks=[ws(N.MLP_TASK0 + k, c.task) for k in range(c.num_tasks)])
        if self.kind == N.MODEL_WND:
            return orc.Model(orc.MODEL_WND, self.tables, list(c.bot), [], list(c.top), ws(N.MLP_TOP, c.top), sigmoid_top=self.sigmoid_top)
        return orc.Model(orc.MODEL_DLRM, self.tables, list(c.bot), ws(N.MLP_BOT, c.bot), list(c.top), ws(N.MLP_TOP, c.top),
                         interaction_op=orc.INTERACT_DOT if self.dot else orc.INTERACT_CAT, sigmoid_top=self.sigmoid_top)

    def oracle_forward(self, om, bs):
        return om.forward(self.dense, self.idx, self.lens, bs=bs, nthreads=0, want_R=True)

    # -- the forward, composed from operators ------------------------------------------------------------------------------------
    def compose(self, ops, bs):
        """The model's forward from `ops` (.sls(W, idx, lens), .fc(x, W, b, act), .dot(T3), .cat(list), .add(a, b)) ->
        (outputs, interaction tensor, record): the record lists every operator call with its inputs and its output, and
        record["last_in"] the inputs of the layers that produce the model's outputs."""
        c = self.case
        rec = {"fc": [], "sls": [], "dot": [], "last_in": []}

        def run(which, x, out_layer=False):
            ln = self.layers(which)
            for l in range(len(ln) - 1):
                W, b = self.w[(which, l)]
                if out_layer and l == len(ln) - 2:
                    rec["last_in"].append(x)
                y = ops.fc(x, W, b, self.act(which, l))
                rec["fc"].append((which, l, self.act(which, l), x, W, b, y))
                x = y
            return x
        pooled = []
        for t in range(c.T):
            idx, lens = self.idx[t][:bs * c.L], self.lens[t][:bs]
            y = ops.sls(self.tables[t], idx, lens)
            rec["sls"].append((t, idx, lens, y))
            pooled.append(y)
        if self.kind == N.MODEL_NCF:
            h = run(N.MLP_TOP, ops.cat([pooled[2], pooled[3]]))
            R = ops.cat([ops.add(pooled[0], pooled[1]), h])
            return run(N.MLP_FINAL, R, True), R, rec
        dense = self.dense[:bs]
        if self.kind == N.MODEL_DLRM:
            x = run(N.MLP_BOT, dense)
            R = ops.cat([x] + pooled)
            if self.dot:
                T3 = R.reshape(bs, c.T + 1, c.D)
                R = ops.dot(T3)
                rec["dot"].append((T3, R))
            return run(N.MLP_TOP, R, True), R, rec
        R = ops.cat([dense] + pooled)
        if self.kind == N.MODEL_WND:
            return run(N.MLP_TOP, R, True), R, rec
        h = run(N.MLP_TOP, R)
        return ops.cat([run(N.MLP_TASK0 + k, h, True) for k in range(c.num_tasks)]), R, rec


class OracleOps(object):
    """the CPU oracle's operators (fp32, the kernels' summation order)"""
    sls = staticmethod(lambda W, idx, lens: orc.sls(W, idx, lens))
    fc = staticmethod(lambda x, W, b, act: orc.fc(x, W, b, act))
    dot = staticmethod(lambda T3: orc.interact_dot(T3, False))
    cat = staticmethod(lambda xs: np.ascontiguousarray(np.concatenate(xs, axis=1)))
    add = staticmethod(lambda a, b: a + b)


def act64(s, act):
    if act == N.ACT_RELU:
        return np.maximum(s, 0.0)
    if act == N.ACT_SIGMOID:
        return 1.0 / (1.0 + np.exp(-s))
    return s


def pair_index(F):
    """(i, j) of the interaction's pairs in the order the reference gathers them: the strict lower triangle, row by row"""
    li = [i for i in range(F) for j in range(i)]
    lj = [j for i in range(F) for j in range(i)]
    return np.array(li), np.array(lj)


def sls64(W, idx, lens):
    W = np.asarray(W, np.float64)
    out = np.zeros((len(lens), W.shape[1]))
    o = 0
    for b, n in enumerate(lens):
        out[b] = W[idx[o:o + n]].sum(axis=0)
        o += n
    return out


def dot64(T3):
    T3 = np.asarray(T3, np.float64)
    Z = np.einsum("bik,bjk->bij", T3, T3)
    li, lj = pair_index(T3.shape[1])
    return np.concatenate([T3[:, 0, :], Z[:, li, lj]], axis=1)


class Float64Ops(object):
    """plain numpy in float64 from end to end: shares nothing with the oracle"""
    sls = staticmethod(sls64)
    fc = staticmethod(lambda x, W, b, act: act64(np.asarray(x, np.float64) @ np.asarray(W, np.float64).T + np.asarray(b, np.float64), act))
    dot = staticmethod(dot64)
    cat = staticmethod(lambda xs: np.concatenate([np.asarray(x, np.float64) for x in xs], axis=1))
    add = staticmethod(lambda a, b: np.asarray(a, np.float64) + np.asarray(b, np.float64))


# ---- the poison layout (tests/test_mlp_nonfinite_cpu.py, tests/test_mlp_nonfinite.py) ------------------------------------------
HOT = (0, 15, 16, 31, 32, 63, 64)            # ... and bs - 1: both sides of every 16-, 32- and 64-row tile edge
KINDS = ("nan", "pinf", "ninf", "both", "huge")
HUGE = 3e38                                  # finite in fp32 (max 3.4028e38); a sum of two of one sign is not
# the poison rows of a table, in this order: (kind, variant); variant 0 plants a single element in column 0, variant 1 in the
# last column; "both": +inf in column 0 and -inf in the last column (variant 0) or the other way round (variant 1)
POISON_ROWS = (("nan", 0), ("nan", 1), ("pinf", 0), ("pinf", 1), ("ninf", 0), ("ninf", 1), ("both", 0), ("both", 1), ("huge", 0))


def plant(row, kind, variant, rng):
    """plant `kind` into the carrier `row` (a dense row, a table row), in place"""
    at = 0 if variant == 0 else row.size - 1
    if kind == "nan":
        row[at] = np.nan
    elif kind == "pinf":
        row[at] = np.inf
    elif kind == "ninf":
        row[at] = -np.inf
    elif kind == "both":
        assert row.size >= 2
        row[at], row[row.size - 1 - at] = np.inf, -np.inf
    else:
        row[:] = np.where(rng.randint(0, 2, row.size) > 0, HUGE, -HUGE).astype(np.float32)


def poison_rows(rng, D):
    P = rng.uniform(-1, 1, (len(POISON_ROWS), D)).astype(np.float32)
    for j, (kind, variant) in enumerate(POISON_ROWS):
        plant(P[j], kind, variant, rng)
    return P


def hot_samples(bs):
    return sorted({s for s in HOT + (bs - 1,) if s < bs})


def poisoned(net, bs):
    """-> a copy of `net` (a Built(case, poison=True)) whose staged inputs (.dense, .idx, .lens: what stage_batch, compose and
    oracle_forward read) hold the poison layout of a query of bs samples, with
        .hot   bool[bs]: the poisoned samples -- hot_samples(bs)
        .hot_kind  per sample its kind (None: clean), .hot_route "dense" | "table" | None
    The hot samples, numbered 1, 2, ... in order, take KINDS in turn.  A model with a dense input carries the poison of the
    odd-numbered ones (the 1st, 3rd, ...: nan, ninf, huge, pinf) in that sample's dense row, single elements alternately in
    column 0 and in the last column; every even-numbered one, and every hot sample of NCF, names a poison row (POISON_ROWS)
    in the last place of one bag: the model's poisoned table, for NCF alternately table 2 (concatenated with table 3) and table 0
    (summed with table 1).  Rows beyond bs are as Built.stage leaves them."""
    c = net.case
    assert net.poison_row, "Built(case, poison=True)"
    rng = np.random.RandomState(zlib.crc32(("hot %d " % bs + c.name).encode()) % (1 << 31))
    out = copy.copy(net)
    out.dense, out.idx, out.lens = net.stage(bs)
    out.hot = np.zeros(bs, bool)
    out.hot_kind, out.hot_route = [None] * bs, [None] * bs
    tabs = net.poison_tables()
    n_dense = n_table = 0
    for p, s in enumerate(hot_samples(bs)):
        kind = KINDS[p % len(KINDS)]
        out.hot[s], out.hot_kind[s] = True, kind
        if net.m_den and p % 2 == 0:
            out.hot_route[s] = "dense"
            plant(out.dense[s], kind, n_dense % 2, rng)
            n_dense += kind != "huge"
        else:
            out.hot_route[s] = "table"
            t = tabs[n_table % len(tabs)]
            variant = 0 if kind == "huge" else (n_table // len(tabs)) % 2
            out.idx[t][s * c.L + c.L - 1] = net.poison_row[t] + POISON_ROWS.index((kind, variant))
            n_table += 1
    return out
