#!/usr/bin/env python3
"""device_weights_cost.py [--sets 300] [--runs 3] [--only weighted|unweighted|staged] [--in_flight 4] [--wgt_dtype fp32|fp16|bf16]: what per-sample weights cost on the device-array path.

RMC1's shape (8 tables x 1 M rows x 64, 80 lookups per bag, 256 samples per query; bottom 128-64-64, top 576-256-64-1), the
arrays of four queries uploaded once as torch tensors, every slot of the engine in flight, three arms:
  weighted     Engine.run_queues_device_multi_async(..., weights=): one launch of the weighted input pass per set
               (include/drs_device_weights.h), then the weighted gather
  unweighted   the same call without weights: the unweighted pass, the unweighted gather
  staged       the only route the same weights had before: download them (torch .cpu()), stage_batch + stage_batch_weights
               per query, then forward_multi_async by batch id
Sets of 1 and of 12 queries; --runs alternating runs per arm in one process, each reported, so the spread is visible.  --only
runs one arm alone, for a kernel trace of the input pass taken from outside; --in_flight 1 keeps ONE set in flight, so that
the trace shows the pass with the chip to itself.  Prints one JSON line per measurement (profiles/r28_device_weights.md)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402,F401  (before the library: torch bundles its own HIP runtime)
from deeprecsys_amd import _native as N  # noqa: E402

T, ROWS, D, L, BS, M_DEN, SLOTS = 8, 1_000_000, 64, 80, 256, 128, 4
LN_BOT, LN_TOP = [M_DEN, 64, D], [D + T * D, 256, 64, 1]
STAGED = 12                     # staged batches: one per query of the largest set


def make_engine():
    rng = np.random.RandomState(0)
    eng = N.Engine(N.MODEL_DLRM, [ROWS] * T, D, LN_BOT, LN_TOP, N.INTERACT_CAT, sigmoid_top=3, max_batch=BS, max_lookups=L,
                   num_staged_batches=STAGED, num_slots=SLOTS)
    for t in range(T):
        eng.fill_table_uniform(t, -0.001, 0.001, 7)
    for which, ln in ((N.MLP_BOT, LN_BOT), (N.MLP_TOP, LN_TOP)):
        for l in range(len(ln) - 1):
            eng.set_fc(which, l, rng.normal(0, 1.0 / np.sqrt(ln[l]), (ln[l + 1], ln[l])).astype(np.float32),
                       rng.normal(0, 0.1, ln[l + 1]).astype(np.float32))
    return eng


def rate(submit, eng, n_sets, co, in_flight=SLOTS):
    """queries/s of n_sets sets of co queries, in_flight slots in flight"""
    busy = [False] * SLOTS
    t0 = time.perf_counter()
    for i in range(n_sets):
        s = i % in_flight
        if busy[s]:
            eng.wait(s, BS * co)
        submit(i, s)
        busy[s] = True
    for s in range(SLOTS):
        if busy[s]:
            eng.wait(s, BS * co)
    return n_sets * co / (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--sets", type=int, default=300)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--only", choices=["weighted", "unweighted", "staged"], default=None)
    ap.add_argument("--in_flight", type=int, default=SLOTS, choices=range(1, SLOTS + 1))
    ap.add_argument("--wgt_dtype", choices=["fp32", "fp16", "bf16"], default="fp32")
    opt = ap.parse_args()
    tdt, code = {"fp32": (torch.float32, N.WEIGHT_FP32), "fp16": (torch.float16, N.WEIGHT_FP16),
                 "bf16": (torch.bfloat16, N.WEIGHT_BF16)}[opt.wgt_dtype]
    rng = np.random.RandomState(1)
    host = [(rng.uniform(-1, 1, (BS, M_DEN)).astype(np.float32), rng.randint(0, ROWS, size=(T, BS * L)).astype(np.int64),
             np.full((T, BS), L, np.int32), rng.uniform(0, 1, (T, BS * L)).astype(np.float32)) for _ in range(4)]
    dev = [(torch.from_numpy(x).cuda(), torch.from_numpy(i).cuda(), torch.from_numpy(l).cuda(), torch.from_numpy(w).cuda().to(tdt))
           for x, i, l, w in host]
    dq = [(BS, x.data_ptr(), i.data_ptr(), i.stride(0), i.shape[1], l.data_ptr(), l.stride(0), L) for x, i, l, _ in dev]
    dw = [(w.data_ptr(), w.stride(0), code) for _, _, _, w in dev]
    torch.cuda.synchronize()
    eng = make_engine()

    def staged(i, s, co):
        # the weights live on the device: they come down, the batches are staged, the weights attached, the set is served by id.
        # (drs_stage_batch waits for every slot in flight: the route cannot overlap its sets)
        for k in range(co):
            x, ids, ln, _ = host[(i + k) % 4]
            w = dev[(i + k) % 4][3].to(torch.float32).cpu().numpy()
            eng.stage_batch(k, x, ids, ln, weights=list(w))
        eng.forward_multi_async(s, list(range(co)), [BS] * co)

    try:
        for co in (1, 12):
            arms = {
                "weighted": lambda i, s, co=co: eng.run_queues_device_multi_async([dq[(i + k) % 4] for k in range(co)], slot=s,
                                                                                  weights=[dw[(i + k) % 4] for k in range(co)]),
                "unweighted": lambda i, s, co=co: eng.run_queues_device_multi_async([dq[(i + k) % 4] for k in range(co)], slot=s),
                "staged": lambda i, s, co=co: staged(i, s, co),
            }
            if opt.only:
                arms = {opt.only: arms[opt.only]}
            n_sets = max(opt.sets // (1 if co == 1 else 4), 8)
            sets_of = {k: max(n_sets // 8, 8) if k == "staged" else n_sets for k in arms}     # (the staged route is ~100x slower per set)
            got = {k: [] for k in arms}
            for k, f in arms.items():
                rate(f, eng, max(sets_of[k] // 10, SLOTS), co, opt.in_flight)        # warm-up (first use allocates the blocks)
            for _ in range(opt.runs):
                for k, f in arms.items():                             # alternating
                    got[k].append(round(rate(f, eng, sets_of[k], co, opt.in_flight), 1))
            rec = {"queries_per_set": co, "sets_per_run": sets_of, "in_flight": opt.in_flight, "wgt_dtype": opt.wgt_dtype}
            for k, v in got.items():
                rec[k + "_queries_per_s"] = v
                rec[k + "_median"] = float(np.median(v))
            if "weighted" in got and "unweighted" in got:
                rec["weighted_over_unweighted"] = round(rec["weighted_median"] / rec["unweighted_median"], 3)
            if "weighted" in got and "staged" in got:
                rec["weighted_over_staged"] = round(rec["weighted_median"] / rec["staged_median"], 2)
            if opt.only != "staged":
                eng.set_option("dispatch_log", 1)
                list(arms.values())[0](0, 0)
                eng.wait(0, BS * co)
                rec["dispatch"] = [t for t in eng.last_dispatch(0) if t.startswith(("input_pass", "sls_"))]
                eng.set_option("dispatch_log", 0)
            print(json.dumps(rec), flush=True)
    finally:
        eng.close()


if __name__ == "__main__":
    main()
