#!/usr/bin/env python3
"""row_update_cost.py [--rows 1000000] [--dim 64] [--reps 5]: what refreshing rows of a loaded table costs.

One RMC1-shaped table (1 M rows x 64) per stored type ("table_dtype" 0 | 1 | 2 | 4 | 8 | 9, the rowwise types also
line-packed): Engine.update_rows of n in {1, 1 000, 100 000} random distinct rows, Engine.get_rows of the same rows, and
Engine.set_table of the whole table -- the only way to change a row before update_rows existed -- for comparison.  Every call
is synchronous (it drains the engine and returns when the rows are stored), so wall-clock time around the call is the cost
a caller sees; the median of --reps calls after one warm-up call is reported.  Prints one JSON line per stored type
(profiles/r25_row_updates.md)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deeprecsys_amd import _native as N  # noqa: E402

ARMS = [("fp32", 0, None), ("fp16", 1, None), ("bf16", 2, None), ("fp8_e4m3", 4, None), ("int8", 8, None),
        ("int8 lines", 8, "table_int8_lines"), ("int4", 9, None), ("int4 lines", 9, "table_int4_lines")]


def median_ms(fn, reps):
    fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return round(float(np.median(t)), 3)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n", type=int, nargs="+", default=[1, 1_000, 100_000])
    opt = ap.parse_args()
    rows, D = opt.rows, opt.dim
    rng = np.random.RandomState(0)
    W = rng.uniform(-0.05, 0.05, (rows, D)).astype(np.float32)
    for name, dtype, lines_key in ARMS:
        eng = N.Engine(N.MODEL_DLRM, [rows], D, [8, D], [2 * D, 4, 1], N.INTERACT_CAT, sigmoid_top=2, max_batch=1, max_lookups=1)
        try:
            if lines_key:
                eng.set_option(lines_key, 1)
            if dtype:
                eng.set_option("table_dtype", dtype)
            rec = {"table_dtype": name, "rows": rows, "D": D, "set_table_ms": median_ms(lambda: eng.set_table(0, W), max(opt.reps // 2, 1))}
            for n in opt.n:
                ids = rng.permutation(rows)[:n].astype(np.int64)
                V = W[ids[::-1]].copy()                      # (values of the table's own range: an fp8 table keeps its scale)
                rec["update_%d_ms" % n] = median_ms(lambda: eng.update_rows(0, ids, V), opt.reps)
                rec["get_%d_ms" % n] = median_ms(lambda: eng.get_rows(0, ids), opt.reps)
                rec["set_table_over_update_%d" % n] = round(rec["set_table_ms"] / rec["update_%d_ms" % n], 1)
            print(json.dumps(rec), flush=True)
        finally:
            eng.close()


if __name__ == "__main__":
    main()
