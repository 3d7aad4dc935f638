#!/usr/bin/env python3
"""device_outputs_cost.py [--sets 300] [--runs 3] [--skip_mtwnd]: what leaving a launch set's results on the GPU is worth to a caller in a torch pipeline.

Two ways to serve a caller whose features live in HBM and whose next step consumes the scores on the GPU (here a trivial
consumer kernel on the caller's stream: acc += scores.sum()):
  A  run_queued_device_multi -- the way that exists without device outputs: one host synchronisation of torch's stream per
     set, the scores back as host floats (drs_wait), uploaded again into a device tensor for the consumer;
  B  run_queued_device_io_multi -- the scores stay in the caller's device tensor, the set is ordered on the caller's stream at
     both ends (include/drs_device_outputs.h), finish_device only when the slot comes round again.
RMC1's shape (8 tables x 1 M rows x 64, 80 lookups per bag, 256 samples per query; bottom 128-64-64, top 576-256-64-1) with
sets of 1 and of 12 queries, and MT-WnD's shape (43 tables x 32, one lookup, shared top 1888-1024-512, one head 512-256-128) with
its full sets of 16 queries, whose outputs are 2 MB a set.  --runs alternating runs per arm in one process, each reported, so
that the spread is visible.  Also: what the output pass adds to ONE set with the chip to itself (its launch, its event and its
run), as the difference between the io call and the device-input call, each followed by wait, one set in flight.
Prints one JSON line per measurement (profiles/r27_device_outputs.md)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402,F401  (before the library: torch bundles its own HIP runtime)
from deeprecsys_amd import _native as N  # noqa: E402
from deeprecsys_amd import dlrm_s_hip as M  # noqa: E402

BS, SLOTS = 256, 4
SHAPES = {
    "rmc1": dict(kind=N.MODEL_DLRM, rows=[1_000_000] * 8, D=64, L=80, ln_bot=[128, 64, 64], ln_top=[64 + 8 * 64, 256, 64, 1],
                 sigmoid_top=3, sets=(1, 12)),
    "mtwnd": dict(kind=N.MODEL_MTWND, rows=[500_000] * 41 + [5_000_000] * 2, D=32, L=1, ln_bot=[512], ln_top=[43 * 32 + 512, 1024, 512],
                  sigmoid_top=2, ln_task=[512, 256, 128], num_tasks=1, sets=(16,)),
}


def make_net(w):
    """an engine of the shape, and a net object around it for the two wrapper-level calls (they use nothing but .engine)"""
    rng = np.random.RandomState(0)
    eng = N.Engine(w["kind"], w["rows"], w["D"], w["ln_bot"], w["ln_top"], N.INTERACT_CAT, sigmoid_top=w["sigmoid_top"],
                   max_batch=BS, max_lookups=w["L"], num_staged_batches=1, num_slots=SLOTS, ln_task=w.get("ln_task"),
                   num_tasks=w.get("num_tasks", 0))
    for t in range(len(w["rows"])):
        eng.fill_table_uniform(t, -0.001, 0.001, 7)
    mlps = [(N.MLP_TOP, w["ln_top"])]
    if w["kind"] == N.MODEL_DLRM:
        mlps.append((N.MLP_BOT, w["ln_bot"]))
    for k in range(w.get("num_tasks", 0)):
        mlps.append((N.MLP_TASK0 + k, w["ln_task"]))
    for which, ln in mlps:
        for l in range(len(ln) - 1):
            eng.set_fc(which, l, rng.normal(0, 1.0 / np.sqrt(ln[l]), (ln[l + 1], ln[l])).astype(np.float32),
                       rng.normal(0, 0.1, ln[l + 1]).astype(np.float32))
    net = object.__new__(M._HipNet)
    net.engine = eng
    return eng, net


def arm_a(net, reqs, co, n_sets, scores, acc):
    """queries/s of n_sets sets the parent's way: host sync, host floats, upload, consumer"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(n_sets):
        outs = net.run_queued_device_multi([reqs[(i + k) % len(reqs)] for k in range(co)], slot=i % SLOTS)
        scores.copy_(torch.from_numpy(np.concatenate(outs)), non_blocking=True)
        acc.add_(scores.sum())
    torch.cuda.synchronize()
    return n_sets * co / (time.perf_counter() - t0)


def arm_b(net, reqs, co, n_sets, outs, acc):
    """queries/s of n_sets sets with device outputs: outs[s] is slot s's [co * BS, n_out] tensor, a row block per query"""
    busy = [False] * SLOTS
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(n_sets):
        s = i % SLOTS
        if busy[s]:
            net.finish_device(s)
        net.run_queued_device_io_multi([reqs[(i + k) % len(reqs)] for k in range(co)],
                                       out=[outs[s][k * BS:(k + 1) * BS] for k in range(co)], slot=s)
        busy[s] = True
        acc.add_(outs[s].sum())
    for s in range(SLOTS):
        if busy[s]:
            net.finish_device(s)
    torch.cuda.synchronize()
    return n_sets * co / (time.perf_counter() - t0)


def pass_alone(eng, reqs, co, out, reps=300):
    """microseconds one set takes from call to wait, one in flight: the device-input call, the io call, the difference"""
    qs = [M.device_request(reqs[k % len(reqs)], eng.T, eng.m_den, eng.device, k) for k in range(co)]
    od = [M.device_out(out[k * BS:(k + 1) * BS], BS, eng.n_out, eng.device, k) for k in range(co)]
    res = {}
    for name, call in (("device_inputs", lambda: eng.run_queues_device_multi_async(qs, slot=0)),
                       ("device_io", lambda: eng.run_queues_device_io_multi_async(qs, od, stream=None, slot=0))):
        runs = []
        for _ in range(4):
            t0 = time.perf_counter()
            for _ in range(reps):
                call()
                eng.wait(0)
            runs.append((time.perf_counter() - t0) / reps * 1e6)
        res[name] = [round(v, 2) for v in runs[1:]]
    res["us_added_per_set"] = round(float(np.median(res["device_io"]) - np.median(res["device_inputs"])), 2)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--sets", type=int, default=300)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--skip_mtwnd", action="store_true")
    opt = ap.parse_args()
    for name, w in SHAPES.items():
        if name == "mtwnd" and opt.skip_mtwnd:
            continue
        rng = np.random.RandomState(1)
        T, L = len(w["rows"]), w["L"]
        eng, net = make_net(w)
        try:
            reqs = [(torch.from_numpy(np.stack([rng.randint(0, r, size=BS * L) for r in w["rows"]]).astype(np.int64)).cuda(),
                     torch.full((T, BS), L, dtype=torch.int32).cuda(),
                     torch.from_numpy(rng.uniform(-1, 1, (BS, eng.m_den)).astype(np.float32)).cuda(), BS, L) for _ in range(4)]
            acc = torch.zeros((), device="cuda")
            for co in w["sets"]:
                scores = torch.empty((co * BS, eng.n_out), device="cuda")
                outs = [torch.empty((co * BS, eng.n_out), device="cuda") for _ in range(SLOTS)]
                n_sets = max(opt.sets // (1 if co == 1 else 4), 8)
                arms = {"A_host_floats": lambda n, co=co: arm_a(net, reqs, co, n, scores, acc),
                        "B_device_outputs": lambda n, co=co: arm_b(net, reqs, co, n, outs, acc)}
                got = {k: [] for k in arms}
                for f in arms.values():
                    f(max(n_sets // 10, SLOTS))                            # warm-up (first use allocates the blocks)
                for _ in range(opt.runs):
                    for k, f in arms.items():                              # alternating
                        got[k].append(round(f(n_sets), 1))
                rec = {"shape": name, "queries_per_set": co, "sets_per_run": n_sets, "output_bytes_per_set": co * BS * eng.n_out * 4}
                for k, v in got.items():
                    rec[k + "_queries_per_s"] = v
                    rec[k + "_mean"] = round(float(np.mean(v)), 1)
                    rec[k + "_spread"] = round((max(v) - min(v)) / float(np.mean(v)), 4)
                rec["B_over_A"] = round(rec["B_device_outputs_mean"] / rec["A_host_floats_mean"], 3)
                print(json.dumps(rec), flush=True)
                print(json.dumps({"shape": name, "queries_per_set": co, "output_pass_alone": pass_alone(eng, reqs, co, outs[0])}), flush=True)
            assert bool(torch.isfinite(acc))
        finally:
            eng.close()


if __name__ == "__main__":
    main()
