#!/usr/bin/env python3
"""What per-sample weights cost the gather launch at RMC1's shape (8 tables x D 64, fixed L 80, 256 samples per query).

Four arms on one engine, same tables and indices, the launch timed by the kernels' own clock stamps (drs_kernel_time,
DRS_KERNEL_SLS_CLOCK), alternating `--rounds` times:
  flatc     the unweighted default (sls_flatc_kernel<16,20,nt>)
  ring      the unweighted ring walk, forced with "sls_flat" 0 (sls_kernel<16,split,nt>)
  ring,w    the weighted ring walk (sls_kernel<16,split,nt,w>): the batches carry uniform [0, 1) weights
  flatc,w   the same weighted batches under "sls_weighted_flat" 1: the form of the unweighted default with weights
            (sls_flatc_kernel<16,20,nt,w>)
for single queries and for launch sets of `--coalesce` queries.  The byte model allows a weighted launch
(row bytes + 8) / (row bytes + 4) over its unweighted twin: a looked-up row moves its bytes, a 4-byte index and now a
4-byte weight.  With `--lookups 1 --dim 32` the arms are the one-lookup copy form and the sequential walk (the arm names
stay; the `form` of every run is in the output), with `--table_dtype 8` or `9` the rowwise instances of the same forms.  Prints one JSON line.  Needs a GPU.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deeprecsys_amd import _native as N  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--tables", type=int, default=8)
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--lookups", type=int, default=80)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--coalesce", type=int, default=12)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--table_dtype", type=int, default=0, choices=(0, 1, 2, 4, 8, 9),
                    help='the engine\'s "table_dtype": 0 fp32, 1 fp16, 2 bf16, 4 fp8 e4m3, 8 int8 rowwise, 9 int4 rowwise')
    a = ap.parse_args()
    T, D, L, B = a.tables, a.dim, a.lookups, a.batch
    rng = np.random.RandomState(1)
    eng = N.Engine(N.MODEL_DLRM, [a.rows] * T, D, [128, 64, D], [D * (T + 1), 256, 64, 1], N.INTERACT_CAT, sigmoid_top=2,
                   max_batch=B, max_lookups=L, num_staged_batches=2, num_slots=2)
    if a.table_dtype:
        eng.set_option("table_dtype", a.table_dtype)   # (before the fill: the rows are written in their stored type)
    for t in range(T):
        eng.fill_table_uniform(t, -0.01, 0.01, 7)
    for mlp, ln in ((N.MLP_BOT, [128, 64, D]), (N.MLP_TOP, [D * (T + 1), 256, 64, 1])):
        for i in range(len(ln) - 1):
            eng.set_fc(mlp, i, (rng.randn(ln[i + 1], ln[i]) * 0.05).astype(np.float32), np.zeros(ln[i + 1], np.float32))
    sets = []
    for _ in range(2):
        ix = [rng.randint(0, a.rows, size=B * L).astype(np.int64) for _ in range(T)]
        ln = [np.full(B, L, np.int32) for _ in range(T)]
        wt = [rng.uniform(0, 1, size=B * L).astype(np.float32) for _ in range(T)]
        sets.append((rng.rand(B, 128).astype(np.float32), ix, ln, wt))
    eng.set_option("dispatch_log", 1)
    eng.set_profiling(1)

    def stage(weighted):
        for b, (X, ix, ln, wt) in enumerate(sets):
            eng.stage_batch(b, X, ix, ln, weights=wt if weighted else None)

    def timed(n_q):
        def once(i):
            if n_q == 1:
                eng.forward(i % 2, B)
            else:
                eng.forward_multi_async(1, [(i + k) % 2 for k in range(n_q)], [B] * n_q)
                eng.wait(1)
        for i in range(20):
            once(i)
        eng.reset_kernel_time()
        for i in range(a.iters):
            once(i)
        ms, n = eng.kernel_time(N.KERNEL_SLS_CLOCK)
        form = [tok for tok in eng.last_dispatch(0 if n_q == 1 else 1) if tok.startswith("sls_")][0]
        return 1e3 * ms / max(n, 1), eng.kernel_bytes(N.KERNEL_SLS_CLOCK) / max(n, 1), form

    # (name, "sls_flat" / "sls_one", weights staged, "sls_weighted_flat")
    arms = [("flatc", 1, False, 0), ("ring", 0, False, 0), ("ring,w", 1, True, 0), ("flatc,w", 1, True, 1)]
    out = {"shape": dict(tables=T, rows=a.rows, D=D, L=L, batch=B, table_dtype=a.table_dtype), "iters": a.iters, "runs": []}
    for r in range(a.rounds):
        for name, flat, weighted, wflat in arms:
            stage(weighted)
            eng.set_option("sls_flat", flat)
            eng.set_option("sls_one", flat)
            eng.set_option("sls_weighted_flat", wflat)
            for n_q in (1, a.coalesce):
                us, nbytes, form = timed(n_q)
                out["runs"].append(dict(round=r, arm=name, queries=n_q, us_per_launch=round(us, 2), bytes_per_launch=int(nbytes),
                                        gbs=round(nbytes / us / 1e3, 1), form=form))
    eng.set_option("sls_flat", 1)
    eng.set_option("sls_one", 1)
    eng.set_option("sls_weighted_flat", 0)
    row_bytes = {0: D * 4, 1: D * 2, 2: D * 2, 4: D, 8: (D + 7) // 8 * 8 + 8, 9: (D // 2 + 3) // 4 * 4 + 4}[a.table_dtype]
    out["byte_model_ring_w_over_ring"] = round((row_bytes + 8) / (row_bytes + 4), 4)
    out["byte_model_flatc_w_over_flatc"] = out["byte_model_ring_w_over_ring"]
    for n_q in (1, a.coalesce):
        med = {name: float(np.median([x["us_per_launch"] for x in out["runs"] if x["arm"] == name and x["queries"] == n_q]))
               for name, _, _, _ in arms}
        out["median_us_%dq" % n_q] = med
        out["ring_w_over_ring_%dq" % n_q] = round(med["ring,w"] / med["ring"], 4)
        out["ring_w_over_flatc_%dq" % n_q] = round(med["ring,w"] / med["flatc"], 4)
        out["flatc_w_over_flatc_%dq" % n_q] = round(med["flatc,w"] / med["flatc"], 4)
        out["flatc_w_over_ring_w_%dq" % n_q] = round(med["flatc,w"] / med["ring,w"], 4)
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
