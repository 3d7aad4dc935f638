#!/usr/bin/env python3
"""device_rows_cost.py [--rows 1000000] [--dim 64] [--reps 5]: what refreshing table rows costs when the rows are ON the GPU.

tools/row_update_cost.py's setup -- one RMC1-shaped table (1 M rows x 64) per stored type ("table_dtype" 0 | 1 | 2 | 4 | 8 | 9,
the rowwise types also line-packed) -- with the ids (int64, unsorted, a tenth of them repeats) and the fp32 rows held in
torch tensors on the engine's GPU, n in {1, 1 000, 100 000}:

  arm A  today's route from device data: synchronise, ids.cpu(), values.cpu(), then Engine.update_rows
  arm B  Engine.update_rows_device with `ordered` 1 on torch's current stream: nothing crosses the bus

Both arms return when the rows are stored, so wall-clock time around the call is what a caller sees.  The arms alternate,
A B A B A B: three runs each, a run being the median of --reps calls after one warm-up call.  Prints one JSON line per stored
type and n with every run, the two means, their run-to-run spread ((max - min) / mean) and A / B
(profiles/r29_device_rows.md)."""
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
    return float(np.median(t))


def summary(runs):
    mean = float(np.mean(runs))
    return round(mean, 3), round((max(runs) - min(runs)) / mean, 3)


def main():
    import torch
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--n", type=int, nargs="+", default=[1, 1_000, 100_000])
    opt = ap.parse_args()
    rows, D = opt.rows, opt.dim
    rng = np.random.RandomState(0)
    W = rng.uniform(-0.05, 0.05, (rows, D)).astype(np.float32)
    stream = torch.cuda.current_stream(0)
    for name, dtype, lines_key in ARMS:
        eng = N.Engine(N.MODEL_DLRM, [rows], D, [8, D], [2 * D, 4, 1], N.INTERACT_CAT, sigmoid_top=2, max_batch=1, max_lookups=1)
        try:
            if lines_key:
                eng.set_option(lines_key, 1)
            if dtype:
                eng.set_option("table_dtype", dtype)
            eng.set_table(0, W)
            for n in opt.n:
                ids = rng.randint(0, rows, size=n).astype(np.int64)
                if n >= 10:
                    ids[-(n // 10):] = ids[:n // 10]             # unsorted, a tenth of the positions repeat an id
                V = W[ids[::-1]].copy()                          # (values of the table's own range: an fp8 table keeps its scale)
                ids_t, V_t = torch.from_numpy(ids).to("cuda:0"), torch.from_numpy(V).to("cuda:0")

                def host_route():
                    stream.synchronize()
                    eng.update_rows(0, ids_t.cpu().numpy(), V_t.cpu().numpy())

                def device_route():
                    eng.update_rows_device(0, ids_t.data_ptr(), n, V_t.data_ptr(), D, N.TABLE_FP32, stream=stream.cuda_stream)

                a, b = [], []
                for _ in range(opt.runs):
                    a.append(median_ms(host_route, opt.reps))
                    b.append(median_ms(device_route, opt.reps))
                (ma, sa), (mb, sb) = summary(a), summary(b)
                print(json.dumps({"table_dtype": name, "rows": rows, "D": D, "n": n, "repeats": int(n - np.unique(ids).size),
                                  "host_route_ms": [round(x, 3) for x in a], "device_route_ms": [round(x, 3) for x in b],
                                  "host_route_mean_ms": ma, "host_route_spread": sa, "device_route_mean_ms": mb, "device_route_spread": sb,
                                  "host_over_device": round(ma / mb, 2)}), flush=True)
        finally:
            eng.close()


if __name__ == "__main__":
    main()
