#!/usr/bin/env python3
"""device_topk_cost.py [--sets 300] [--runs 3] [--k 10] [--skip_mtwnd]: what one top-k launch per set is worth to a ranker in a torch pipeline.

Two ways to hand a ranker, whose next step runs on the GPU, the k best samples of every query of a launch set (here the
consumer is trivial: acc += the winners' scores):
  A  run_queued_device_io_multi, then on the caller's stream one torch.topk per query over the ranking column, and one row
     gather per query where the rows carry more than one score (n_out > 1) -- the way INTEGRATION.md shows without the call;
  B  run_queued_device_topk_multi -- ONE kernel launch per set ranks every query (include/drs_device_topk.h) and writes the
     winners' row numbers and score rows.
Both are ordered on the caller's stream at both ends; finish_device only when the slot comes round again.  RMC1's shape with
sets of 1 and of 12 queries, MT-WnD's shape with its full sets of 16 queries (device_outputs_cost.py's shapes).  --runs
alternating runs per arm in one process, each reported, so that the spread is visible.  Also, with the chip to itself and one
set in flight: what the top-k pass adds to a set (the top-k call minus the device-input call, each followed by wait; the
same difference for the device-output call beside it), and the time per launch of the pass alone on one query's array
(drs_topk_rows back to back on one stream, between two events).
Prints one JSON line per measurement (profiles/r30_device_topk.md)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402,F401  (before the library: torch bundles its own HIP runtime)
import device_outputs_cost as DOC  # noqa: E402  (the shapes and the engines)
from deeprecsys_amd import dlrm_s_hip as M  # noqa: E402

BS, SLOTS, SHAPES, make_net = DOC.BS, DOC.SLOTS, DOC.SHAPES, DOC.make_net


def arm_a(net, reqs, co, n_sets, outs, acc, k, col):
    """queries/s of n_sets sets: device outputs, then torch.topk (and the row gather) per query"""
    busy = [False] * SLOTS
    n_out = outs[0].shape[1]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(n_sets):
        s = i % SLOTS
        if busy[s]:
            net.finish_device(s)
        got = net.run_queued_device_io_multi([reqs[(i + j) % len(reqs)] for j in range(co)],
                                             out=[outs[s][j * BS:(j + 1) * BS] for j in range(co)], slot=s)
        busy[s] = True
        for o in got:
            top = torch.topk(o[:, col], k)
            acc.add_(top.values.sum() if n_out == 1 else o.index_select(0, top.indices).sum())
    for s in range(SLOTS):
        if busy[s]:
            net.finish_device(s)
    torch.cuda.synchronize()
    return n_sets * co / (time.perf_counter() - t0)


def arm_b(net, reqs, co, n_sets, tops, acc, k, col):
    """queries/s of n_sets sets with the one-call form: tops[s] is slot s's list of (idx, scores) pairs"""
    busy = [False] * SLOTS
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(n_sets):
        s = i % SLOTS
        if busy[s]:
            net.finish_device(s)
        got = net.run_queued_device_topk_multi([reqs[(i + j) % len(reqs)] for j in range(co)], k, col=col, out=tops[s], slot=s)
        busy[s] = True
        for _, sc in got:
            acc.add_(sc.sum())
    for s in range(SLOTS):
        if busy[s]:
            net.finish_device(s)
    torch.cuda.synchronize()
    return n_sets * co / (time.perf_counter() - t0)


def pass_alone(eng, reqs, co, out, tops, k, col, reps=300):
    """microseconds one set takes from call to wait, one in flight: the device-input call, the io call, the top-k call"""
    qs = [M.device_request(reqs[j % len(reqs)], eng.T, eng.m_den, eng.device, j) for j in range(co)]
    od = [M.device_out(out[j * BS:(j + 1) * BS], BS, eng.n_out, eng.device, j) for j in range(co)]
    td = [M.device_top(tops[j], k, eng.n_out, eng.device, j) for j in range(co)]
    res = {}
    for name, call in (("device_inputs", lambda: eng.run_queues_device_multi_async(qs, slot=0)),
                       ("device_io", lambda: eng.run_queues_device_io_multi_async(qs, od, stream=None, slot=0)),
                       ("device_topk", lambda: eng.run_queues_device_topk_multi_async(qs, [k] * co, col, td, stream=None, slot=0))):
        runs = []
        for _ in range(4):
            t0 = time.perf_counter()
            for _ in range(reps):
                call()
                eng.wait(0)
            runs.append((time.perf_counter() - t0) / reps * 1e6)
        res[name] = [round(v, 2) for v in runs[1:]]
    res["us_added_per_set_output_pass"] = round(float(np.median(res["device_io"]) - np.median(res["device_inputs"])), 2)
    res["us_added_per_set_topk_pass"] = round(float(np.median(res["device_topk"]) - np.median(res["device_inputs"])), 2)
    # the pass alone on one query's array: launches back to back on one stream between two events
    idx, sc = tops[0]
    src = out[:BS]
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    stream = torch.cuda.current_stream().cuda_stream
    per = []
    for _ in range(4):
        torch.cuda.synchronize()
        a.record()
        for _ in range(reps):
            eng.topk_rows(src.data_ptr(), BS, eng.n_out, eng.n_out, col, k, idx.data_ptr(), sc.data_ptr(), stream=stream)
        b.record()
        b.synchronize()
        per.append(round(a.elapsed_time(b) / reps * 1e3, 2))
    res["us_per_topk_rows_launch_back_to_back"] = per[1:]
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--sets", type=int, default=300)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--skip_mtwnd", action="store_true")
    opt = ap.parse_args()
    k = opt.k
    for name, w in SHAPES.items():
        if name == "mtwnd" and opt.skip_mtwnd:
            continue
        rng = np.random.RandomState(1)
        T, L = len(w["rows"]), w["L"]
        eng, net = make_net(w)
        try:
            eng.set_option("dispatch_log", 1)
            col = eng.n_out - 1
            reqs = [(torch.from_numpy(np.stack([rng.randint(0, r, size=BS * L) for r in w["rows"]]).astype(np.int64)).cuda(),
                     torch.full((T, BS), L, dtype=torch.int32).cuda(),
                     torch.from_numpy(rng.uniform(-1, 1, (BS, eng.m_den)).astype(np.float32)).cuda(), BS, L) for _ in range(4)]
            acc = torch.zeros((), device="cuda")
            for co in w["sets"]:
                outs = [torch.empty((co * BS, eng.n_out), device="cuda") for _ in range(SLOTS)]
                tops = [[(torch.empty((k,), dtype=torch.int32, device="cuda"), torch.empty((k, eng.n_out), device="cuda"))
                         for _ in range(co)] for _ in range(SLOTS)]
                n_sets = max(opt.sets // (1 if co == 1 else 4), 8)
                arms = {"A_io_then_torch_topk": lambda n, co=co: arm_a(net, reqs, co, n, outs, acc, k, col),
                        "B_device_topk": lambda n, co=co: arm_b(net, reqs, co, n, tops, acc, k, col)}
                got = {a: [] for a in arms}
                for f in arms.values():
                    f(max(n_sets // 10, SLOTS))                            # warm-up (first use allocates the blocks)
                log = eng.last_dispatch(0)
                for _ in range(opt.runs):
                    for a, f in arms.items():                              # alternating
                        got[a].append(round(f(n_sets), 1))
                rec = {"shape": name, "queries_per_set": co, "sets_per_run": n_sets, "k": k, "n_out": eng.n_out, "col": col,
                       "last_token": log[-1] if log else None}
                for a, v in got.items():
                    rec[a + "_queries_per_s"] = v
                    rec[a + "_mean"] = round(float(np.mean(v)), 1)
                    rec[a + "_spread"] = round((max(v) - min(v)) / float(np.mean(v)), 4)
                rec["B_over_A"] = round(rec["B_device_topk_mean"] / rec["A_io_then_torch_topk_mean"], 3)
                print(json.dumps(rec), flush=True)
                print(json.dumps({"shape": name, "queries_per_set": co,
                                  "topk_pass_alone": pass_alone(eng, reqs, co, outs[0], tops[0], k, col)}), flush=True)
            assert bool(torch.isfinite(acc))
        finally:
            eng.close()


if __name__ == "__main__":
    main()
