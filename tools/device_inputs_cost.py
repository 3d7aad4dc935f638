#!/usr/bin/env python3
"""device_inputs_cost.py [--sets 300] [--runs 3] [--only host|device] [--in_flight 4]: what handing a launch set over as DEVICE arrays costs.

RMC1's shape (8 tables x 1 M rows x 64, 80 lookups per bag, 256 samples per query; bottom 128-64-64, top 576-256-64-1): the
same four queries' arrays go through Engine.run_queues_multi_async (host arrays: narrowed and checked on the CPU, one DMA copy
per set -- the path that exists without the device form) and, uploaded once as torch tensors, through
Engine.run_queues_device_multi_async (one input-pass launch per set, include/drs_device_inputs.h), with every slot of the
engine in flight.  Sets of 1 and of 12 queries; --runs alternating runs per arm in one process, each reported, so the spread is
visible.  Also: the host cost of the pointer check (three hipPointerGetAttributes + hipMemGetAddressRange per query), as the
difference between sets of 12 EMPTY queries (bs 0: nothing is launched) with and without pointers.  --only device runs that arm
alone, for a kernel trace of the input pass taken from outside; --in_flight 1 keeps ONE set in flight, so that the trace shows
the pass with the chip to itself.  Prints one JSON line per measurement
(profiles/r26_device_inputs.md)."""
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


def make_engine():
    rng = np.random.RandomState(0)
    eng = N.Engine(N.MODEL_DLRM, [ROWS] * T, D, LN_BOT, LN_TOP, N.INTERACT_CAT, sigmoid_top=3, max_batch=BS, max_lookups=L,
                   num_staged_batches=1, num_slots=SLOTS)
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
    ap.add_argument("--only", choices=["host", "device"], default=None)
    ap.add_argument("--in_flight", type=int, default=SLOTS, choices=range(1, SLOTS + 1))
    opt = ap.parse_args()
    rng = np.random.RandomState(1)
    host = [(rng.uniform(-1, 1, (BS, M_DEN)).astype(np.float32), rng.randint(0, ROWS, size=(T, BS * L)).astype(np.int64),
             np.full((T, BS), L, np.int32)) for _ in range(4)]
    dev = [(torch.from_numpy(x).cuda(), torch.from_numpy(i).cuda(), torch.from_numpy(l).cuda()) for x, i, l in host]
    dq = [(BS, x.data_ptr(), i.data_ptr(), i.stride(0), i.shape[1], l.data_ptr(), l.stride(0), L) for x, i, l in dev]
    torch.cuda.synchronize()
    eng = make_engine()
    try:
        for co in (1, 12):
            arms = {
                "host": lambda i, s, co=co: eng.run_queues_multi_async([(host[(i + k) % 4][0], host[(i + k) % 4][1], host[(i + k) % 4][2], BS)
                                                                        for k in range(co)], slot=s),
                "device": lambda i, s, co=co: eng.run_queues_device_multi_async([dq[(i + k) % 4] for k in range(co)], slot=s),
            }
            if opt.only:
                arms = {opt.only: arms[opt.only]}
            n_sets = max(opt.sets // (1 if co == 1 else 4), 8)
            got = {k: [] for k in arms}
            for k, f in arms.items():
                rate(f, eng, max(n_sets // 10, SLOTS), co, opt.in_flight)            # warm-up (first use allocates the blocks)
            for _ in range(opt.runs):
                for k, f in arms.items():                             # alternating
                    got[k].append(round(rate(f, eng, n_sets, co, opt.in_flight), 1))
            rec = {"queries_per_set": co, "sets_per_run": n_sets, "in_flight": opt.in_flight}
            for k, v in got.items():
                rec[k + "_queries_per_s"] = v
                rec[k + "_median"] = float(np.median(v))
            if len(got) == 2:
                rec["device_over_host"] = round(rec["device_median"] / rec["host_median"], 3)
            print(json.dumps(rec), flush=True)
        # the pointer check on the host: sets of 12 empty queries (nothing is enqueued), with and without pointers
        empty_ptr = [(0, x.data_ptr(), i.data_ptr(), i.stride(0), 0, l.data_ptr(), l.stride(0), -1) for x, i, l in dev] * 3
        empty_null = [(0, 0, 0, 0, 0, 0, 0, -1)] * 12
        per = {}
        for name, qs in (("with_pointers", empty_ptr), ("null_pointers", empty_null)):
            runs = []
            for _ in range(opt.runs + 1):
                t0 = time.perf_counter()
                for _ in range(2000):
                    eng.run_queues_device_multi_async(qs, slot=0)
                runs.append((time.perf_counter() - t0) / 2000 * 1e6)
            per[name] = [round(v, 2) for v in runs[1:]]
        diff = float(np.median(per["with_pointers"]) - np.median(per["null_pointers"]))
        print(json.dumps({"pointer_check": per, "us_per_call_of_12_queries": round(diff, 2),
                          "us_per_query_3_pointers": round(diff / 12, 3)}), flush=True)
    finally:
        eng.close()


if __name__ == "__main__":
    main()
