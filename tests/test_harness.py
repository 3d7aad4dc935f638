"""Process-level tests of the serving harness (orchestrator + load generator + engines)
and of the multi-rank statistics collective.  CPU only unless marked gpu."""
import os
import socket
import sys

import numpy as np
import pytest
import torch.multiprocessing as mp

from deeprecsys_amd import latency_table, stats
from deeprecsys_amd.DeepRecSys import DeepRecSys
from deeprecsys_amd.utils.utils import cli


def _args(tmp_path, **kw):
    a = cli(["--queue", "--model_accel", "--inference_engines", "0", "--num_batches", "8",
             "--nepochs", "2", "--avg_arrival_rate", "1", "--batch_size_distribution", "normal",
             "--avg_mini_batch_size", "20", "--var_mini_batch_size", "4", "--max_mini_batch_size", "32",
             "--req_granularity", "4", "--log_file", str(tmp_path / "log" / "out.log")])
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _write_sim_tables(root):
    d = os.path.join(root, "nvidia_gtx_1080_ti", "raw_data")
    os.makedirs(d)
    for m in latency_table.MODELS:
        rows = [(0.1, 0.01, 0.2, 0.02, 0.3, 0.2 * (i + 1)) for i in range(6)]   # 0.2 .. 1.2 ms
        latency_table.write_results(os.path.join(d, "results_%s.txt" % m), rows)


def test_harness_with_two_simulated_accelerators(tmp_path):
    """Queue protocol end to end on CPU: ready tokens, whole-query routing to the shared
    accelerator queue, per-engine sentinels, response reassembly, QPS/p95/p99 summary --
    with the reference's latency-table engine behaviour (--accel_backend sim) on two
    accelerator engines."""
    root = str(tmp_path / "accel") + "/"
    os.makedirs(root)
    _write_sim_tables(root)
    a = _args(tmp_path, accel_backend="sim", num_accels=2, accel_root_dir=root, model_name="rm1")
    s = DeepRecSys(a, quiet=True)
    assert s["accel_requests"] == 16 and s["cpu_requests"] == 0 and s["cpu_sub_requests"] == 0
    assert s["responses"] == 16 and s["measured_queries"] == 16
    assert s["qps"] > 0 and 0.1 < s["p99_ms"] < 1000
    lines = open(a.log_file).read().strip().splitlines()
    assert len(lines) == 16
    consumers = {eval(l)["consumer_id"] for l in lines}
    assert consumers <= {0, 1} and len(consumers) >= 1


def _write_mix_configs(tmp_path):
    """Shrunk models/configs/{wide_and_deep,ncf}.json (same keys, small tables)."""
    import json
    wnd = {"arch_mlp_bot": "64", "arch_mlp_top": "128-64-1", "arch_embedding_size": "-".join(["300"] * 5),
           "arch_sparse_feature_size": 16, "num_indices_per_lookup_fixed": True, "num_indices_per_lookup": 1,
           "arch_interaction_op": "cat", "model_type": "wnd", "model_name": "wnd"}
    ncf = {"arch_mlp_bot": "64", "arch_mlp_top": "64-32-16", "arch_embedding_size": "200-200-40-40",
           "arch_sparse_feature_size": 16, "num_indices_per_lookup_fixed": True, "num_indices_per_lookup": 1,
           "arch_interaction_op": "cat", "model_type": "ncf", "model_name": "ncf"}
    files = []
    for name, cfg in (("wnd", wnd), ("ncf", ncf)):
        f = str(tmp_path / (name + ".json"))
        json.dump(cfg, open(f, "w"))
        files.append(f)
    return ",".join(files)


@pytest.mark.parametrize("rate,req_batch,accels", [(0.0, 16, 1), (0.0, 16, 2), (0.0, 1, 2), (3.0, 16, 2)])
def test_load_generator_batches_back_to_back_requests(tmp_path, rate, req_batch, accels):
    """--accel_req_batch: accelerator requests generated back to back travel as ONE put of a list (the packets
    are the reference's, utils/packets.py:6-22); the list is flushed before every sleep, so when the
    inter-arrival gap is non-zero every request leaves at once; 1 = the reference's one packet per put.
    Several engines on the one queue: lists of at most 8 (a list lands on ONE engine).
    Sentinels are always their own put (loadGenerator.py:208-214)."""
    import queue
    from deeprecsys_amd.loadGenerator import loadGenerator
    from deeprecsys_amd.utils.packets import ServiceRequest
    a = _args(tmp_path, num_accels=accels, nepochs=3, num_batches=8, avg_arrival_rate=rate, accel_req_batch=req_batch)
    a.inference_engines = accels
    np.random.seed(a.numpy_rand_seed)
    rq, ret, ready, pid, aq = (queue.Queue() for _ in range(5))
    for _ in range(accels):
        ready.put(True)
    loadGenerator(a, rq, ret, ready, pid, aq)
    puts = []
    while not aq.empty():
        puts.append(aq.get())
    assert puts[-accels:] == [None] * accels and rq.empty()
    body = puts[:-accels]
    flat = [r for p in body for r in (p if isinstance(p, list) else [p])]
    assert all(isinstance(r, ServiceRequest) for r in flat)
    assert [(r.epoch, r.batch_id) for r in flat] == [(e, b) for e in range(3) for b in range(8)]      # order kept
    assert ret.get() == (0, 0, 24)
    if req_batch == 1:
        assert len(body) == 24 and not any(isinstance(p, list) for p in body)
    elif rate == 0.0:
        assert [len(p) for p in body] == ([16, 8] if accels == 1 else [8, 8, 8])
    else:
        # poisson(3 ms) is non-zero ~95 % of the time: (almost) every request is flushed on its own
        assert len(body) >= 20


def test_mixed_model_stream_tags_queries_deterministically(tmp_path):
    """BASELINE config 4's stream: every query is for one of the engine's models, drawn from
    its own seeded stream with the configured shares; the log carries model_id."""
    from deeprecsys_amd.utils.utils import mix_models
    root = str(tmp_path / "accel") + "/"
    os.makedirs(root)
    _write_sim_tables(root)
    a = _args(tmp_path, accel_backend="sim", num_accels=1, accel_root_dir=root, model_name="wnd",
              mix_config_files=_write_mix_configs(tmp_path), mix_weights="3,1")
    mm = mix_models(a)
    assert [m.model_type for m, _ in mm] == ["wnd", "ncf"] and [w for _, w in mm] == [0.75, 0.25]
    assert mm[1][0].arch_mlp_top == "64-32-16" and a.model_name == "wnd"       # copies, run args untouched
    s = DeepRecSys(a, quiet=True)
    lines = [eval(l) for l in open(a.log_file).read().strip().splitlines()]
    got = [l["model_id"] for l in sorted(lines, key=lambda l: (l["epoch"], l["batch_id"]))]
    rng = np.random.RandomState(a.numpy_rand_seed + 7919)
    assert got == [int(rng.choice(2, p=[0.75, 0.25])) for _ in range(len(got))]
    assert s["queries_per_model"] == {str(k): got.count(k) for k in sorted(set(got))}
    with pytest.raises(ValueError):
        a.mix_weights = "1"
        mix_models(a)


def test_harness_rejects_cpu_engines_without_a_cpu_forward(tmp_path):
    a = _args(tmp_path, inference_engines=2)
    with pytest.raises(SystemExit):
        DeepRecSys(a, quiet=True)


def test_accel_engine_startup_failure_still_sends_sentinel(tmp_path):
    """A dying engine must not hang the orchestrator's join loop (DeepRecSys.py:89)."""
    a = _args(tmp_path, accel_backend="sim", num_accels=1, accel_root_dir=str(tmp_path / "missing") + "/",
              model_name="rm1")
    s = DeepRecSys(a, quiet=True)
    assert s["responses"] == 0 and s["qps"] is None


# ---- the statistics collective, world_size 2 over gloo -----------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _rank_main(rank, world, port, out):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    rng = np.random.RandomState(rank)
    lat = rng.uniform(1e-4, 3e-3, size=500 + 100 * rank)
    elapsed = 1.0 + rank
    el, n, h = stats.allreduce_run_stats(dist, elapsed, lat.size, stats.latency_histogram(lat))
    if rank == 0:
        out.put((el, n, int(h.sum()), stats.percentile_from_histogram(h, 99)))
    dist.destroy_process_group()


def test_multi_rank_stats_allreduce_gloo():
    ctx = mp.get_context("spawn")
    out = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank_main, args=(r, 2, port, out)) for r in range(2)]
    for p in procs:
        p.start()
    el, n, total, p99 = out.get(timeout=120)
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    lat = np.concatenate([np.random.RandomState(r).uniform(1e-4, 3e-3, size=500 + 100 * r) for r in range(2)])
    assert el == 2.0 and n == 1100 and total == 1100
    assert p99 == pytest.approx(np.percentile(lat, 99, method="higher") * 1e3, rel=0.01)


def _bench_cmd(cpu_abi):
    """bench.py as the driver starts it -- or, for the CPU tests of its rank entry, through
    tests/cpu_abi_entry.py, which binds the CPU restatement of the C ABI first (the product binding
    has no override for that: deeprecsys_amd/_native.py)."""
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if cpu_abi:
        return [sys.executable, os.path.join(root, "tests", "cpu_abi_entry.py"), "bench.py"]
    return [sys.executable, os.path.join(root, "bench.py")]


def _bench(extra, env_extra=None, timeout=600, cpu_abi=False):
    import json
    import subprocess
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "DRS_HIP_LIB"):
        env.pop(k, None)
    env.update(env_extra or {})
    r = subprocess.run(_bench_cmd(cpu_abi) + extra, env=env, capture_output=True,
                       text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout          # ONE JSON line, from rank 0
    return json.loads(lines[0])


_TINY = ["--workload", "tiny", "--steps", "3", "--warmup", "1", "--queries_per_step", "20", "--batch", "4",
         "--num_batches", "2", "--no_cpu_baseline", "--timed_only"]


def test_bench_rank_entry_world_size_2_end_to_end_on_cpu():
    """`python bench.py --gpus 2` with no launcher spawns its own two ranks; each
    runs the rank entry end to end -- model build, warm-up, K timed steps, barrier on both sides,
    the statistics collective -- above the CPU restatement of the C ABI (tests only; the
    collective on gloo), and rank 0 prints one line for the whole job."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    # one OpenMP thread per rank: two oracle-backed ranks spinning on all cores starve each other
    cpu = {"OMP_NUM_THREADS": "1"}
    two = _bench(["--gpus", "2", "--collective", "gloo", "--allow_device_sharing"] + _TINY, cpu, cpu_abi=True)
    assert two["n_gpus"] == 2 and two["steps"] == 3 and two["warmup"] == 1 and two["scaling"] == "weak"
    assert two["config"]["queries_per_step"] == 20 and two["config"]["timed_queries_per_gpu"] == 60
    assert two["latency_ms"]["queries"] == 120                      # both ranks' histograms, summed
    # whole-job throughput: all ranks' queries over the slowest rank's time
    assert two["value"] == pytest.approx(120 / two["config"]["timed_seconds"], rel=0.15)   # (timed_seconds is rounded to 0.1 ms)
    assert two["ms_per_step"] == pytest.approx(two["config"]["timed_seconds"] / 3 * 1e3, rel=0.15)
    # default --collective rccl above a library without RCCL: the run still produces its line, the
    # statistics are combined over gloo and the line says why
    fb = _bench(["--gpus", "2", "--allow_device_sharing"] + _TINY, cpu, cpu_abi=True)
    assert fb["n_gpus"] == 2 and fb["latency_ms"]["queries"] == 120
    assert "RCCL communicator did not come up" in fb["config"]["collective"]
    one = _bench(["--gpus", "1"] + _TINY, cpu, cpu_abi=True)
    assert one["n_gpus"] == 1 and one["latency_ms"]["queries"] == 60 and one["config"]["collective"] is None
    # identical line structure at N = 1 and N = 2
    assert set(one) == set(two) and set(one["roofline"]) == set(two["roofline"])
    # with --full (and without --timed_only) the line carries the check of the timed region's own outputs against the oracle
    tiny = [a for a in _TINY if a != "--timed_only"]
    chk = _bench(["--gpus", "1", "--full"] + tiny, cpu, cpu_abi=True)
    assert chk["verified"]["ok"] is True and chk["verified_queries"] == chk["verified"]["verified_queries"] > 0


def test_bench_rank_entry_world_size_8_shares_the_host():
    """The driver's largest launch: 8 ranks on one node.  Above the CPU restatement of the ABI (gloo), the line
    is the whole job's -- 8 x the per-rank queries -- and every rank's per-call conversion workers are capped at
    its share of the cores this process may use (8 ranks x (poll thread + workers) on a
    16-CPU cgroup), which the line records."""
    import bench
    cpu = {"OMP_NUM_THREADS": "1"}
    eight = _bench(["--gpus", "8", "--collective", "gloo", "--allow_device_sharing"] + _TINY, cpu, timeout=900, cpu_abi=True)
    assert eight["n_gpus"] == 8 and eight["latency_ms"]["queries"] == 8 * 60
    assert eight["value"] == pytest.approx(8 * 60 / eight["config"]["timed_seconds"], rel=0.15)
    h = eight["config"]["host"]
    assert h["ranks"] == 8 and h["cores"] == bench.host_cores()
    assert h["conversion_workers_per_rank"] == max(0, min(7, bench.host_cores() // 8 - 1))
    assert (h["conversion_workers_per_rank"] + 1) * 8 <= max(8, h["cores"])     # workers + caller fit the budget


def test_bench_refuses_more_ranks_than_devices():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    import subprocess
    import sys
    env = dict(os.environ, OMP_NUM_THREADS="1")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE"):
        env.pop(k, None)
    r = subprocess.run(_bench_cmd(True) + ["--gpus", "2", "--collective", "gloo"] + _TINY,
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "device 1 of 1" in r.stderr and not r.stdout.strip()


# ---- the real thing ------------------------------------------------------------------------------
@pytest.mark.gpu
def test_stats_allreduce_over_rccl_through_the_c_abi():
    """drs_stats_allreduce on real RCCL through the C ABI: a communicator of world size 1, created and
    used in-process (ncclCommInitRank, the grouped all-reduce = identity, drs_comm_barrier).  The
    box has one GPU: nothing with more than one rank can run here (the N > 1 path is covered by the
    world-size-2 gloo runs of bench.py's rank entry on CPU)."""
    from deeprecsys_amd import _native as N
    uid = N.Comm.unique_id()
    assert len(uid) == N.COMM_ID_BYTES
    c = N.Comm(uid, 0, 1, 0)
    try:
        h = np.arange(4095, dtype=np.int64)
        h2, s4 = c.stats_allreduce(h, [5.0, 0.25, 1.5, 2.5])
        assert np.array_equal(h2, h) and list(s4) == [5.0, 0.25, 1.5, 2.5]
        c.barrier()
    finally:
        c.close()


@pytest.mark.gpu
def test_bench_self_spawn_n1_equals_plain_n1_line_shape():
    """On the GPU: `--gpus 1` (in-process) prints the same line structure the driver reads, with
    per-launch byte accounting (frac follows from bytes_timed / launches, whatever the mix of
    full and partial launch sets)."""
    out = _bench(["--gpus", "1", "--steps", "2", "--warmup", "1", "--queries_per_step", "1001",
                  "--no_cpu_baseline", "--timed_only"])
    r = out["roofline"]
    assert out["n_gpus"] == 1 and out["config"]["timed_queries_per_gpu"] == 2002
    co = out["config"]["queries_per_launch"]                         # the engine's preference for RMC1
    assert co == 12
    assert r["launches_timed"] == (2002 + co - 1) // co              # full sets + one partial set
    assert r["bytes_timed"] == 2002 * 43130880                       # RMC1: 43.13 MB per query, exactly
    assert r["frac"] == pytest.approx(r["bytes_timed"] / (r["avg_launch_us"] * 1e-6 * r["launches_timed"]) / 8e12, rel=2e-3)
    assert 0.3 < r["frac"] < 0.8                                       # above the copy ceiling = accounting bug
    m = r["mlp_end_to_end"]                                            # RMC1: 2 x 256 x 176 192 MACs per query
    assert m["flop_per_query"] == 2 * 256 * (128 * 64 + 64 * 64 + 576 * 256 + 256 * 64 + 64) and m["peak"] == 157.3
    assert m["achieved"] == pytest.approx(out["value"] * m["flop_per_query"] / 1e12, rel=1e-2)


@pytest.mark.gpu
def test_bench_line_verifies_the_timed_regions_own_outputs():
    """VERDICT r3 #1c, r4 #1: what the pipelined engine produced for the LAST launch sets of the timed region and for sixteen sets spread over it
    (default flat gather, 12 queries per set, 3 sets in flight, MLP on its own stream) is compared with the
    oracle's forward inside bench.py, at BASELINE configs[1]'s full size."""
    out = _bench(["--gpus", "1", "--steps", "2", "--warmup", "1", "--queries_per_step", "3000", "--no_cpu_baseline",
                  "--full"])
    v = out["verified"]
    # the last three sets and (round 6) sixteen sets spread evenly over the timed region: 19 x 12 queries
    assert v["ok"] is True and v["launch_sets"] == 19 and v["mid_region_sets"] == 16 and out["verified_queries"] == 228
    assert v["max_rel_err"] <= 1e-4


@pytest.mark.gpu
def test_stand_alone_model_entry_on_the_gpu(tmp_path):
    """`python -m deeprecsys_amd.dlrm_s_hip` with the reference's flags (models/run.sh:36-57, generate_data.py:20):
    the six `***` lines parse like the reference's characterisation files and the split is real (the input
    hand-over of a 256-sample RMC1 query is measurable beside its forward)."""
    import json
    import subprocess
    cfg = dict(arch_mlp_bot="128-64-32", arch_mlp_top="256-64-1", arch_embedding_size="-".join(["400000"] * 8),
               arch_sparse_feature_size=32, num_indices_per_lookup_fixed=True, num_indices_per_lookup=80,
               arch_interaction_op="cat", model_type="dlrm", model_name="rm1")
    path = str(tmp_path / "dlrm_rm1.json")
    json.dump(cfg, open(path, "w"))
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-m", "deeprecsys_amd.dlrm_s_hip", "--inference_only", "--use_accel",
                        "--caffe2_net_type", "async_dag", "--config_file", path, "--nepochs", "20", "--num_batches", "4",
                        "--mini_batch_size", "256", "--max_mini_batch_size", "256", "--accel_table_init", "device"],
                       cwd=root, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    f = str(tmp_path / "results_rm1.txt")
    open(f, "w").write(r.stdout)
    rows = latency_table.parse_results(f)
    assert len(rows) == 1
    load, load_it, comp, comp_it, tot, tot_it = rows[0]
    assert tot == pytest.approx(load + comp) and tot_it == pytest.approx(tot / 80)
    assert 0.005 < comp_it < 5.0 and 0.005 < load_it < 20.0            # ms per iteration


def test_orchestrator_without_a_queue_runs_the_stand_alone_loop(tmp_path, capsys):
    """`DeepRecSys.py` without --queue (reference :184-185: "No queue, run DeepRecSys in standalone mode"): the engine's
    queue-less branch -- nepochs passes over the generated batches and the six `***` lines (inferenceEngine.py:137-173).
    Here on the CPU restatement of the ABI; the GPU suite runs the same loop through `python -m deeprecsys_amd.dlrm_s_hip`."""
    from deeprecsys_amd import _native
    from deeprecsys_amd.utils.utils import cli
    from tests.cpu_abi_entry import bind_cpu_abi
    prev = _native._lib
    bind_cpu_abi()
    try:
        a = cli(["--inference_only", "--model_type", "dlrm", "--arch_sparse_feature_size", "8", "--arch_embedding_size", "200-300",
                 "--arch_mlp_bot", "13-16-8", "--arch_mlp_top", "16-1", "--arch_interaction_op", "dot", "--num_indices_per_lookup", "4",
                 "--nepochs", "3", "--num_batches", "4", "--mini_batch_size", "16", "--max_mini_batch_size", "16"])
        assert not a.queue
        DeepRecSys(a, quiet=True)
    finally:
        _native._lib = prev
    out = capsys.readouterr().out
    f = str(tmp_path / "results.txt")
    open(f, "w").write(out)
    rows = latency_table.parse_results(f)
    assert len(rows) == 1
    load, load_it, comp, comp_it, tot, tot_it = rows[0]
    assert tot == pytest.approx(load + comp) and tot_it == pytest.approx(tot / 12) and tot > 0


@pytest.mark.gpu
def test_harness_with_a_real_accelerator_engine(tmp_path):
    a = _args(tmp_path, accel_backend="hip", num_accels=1, arch_sparse_feature_size=16,
              arch_embedding_size="2000-3000-1000", arch_mlp_bot="13-32-16", arch_mlp_top="32-1",
              arch_interaction_op="dot", num_indices_per_lookup=10, model_type="dlrm")
    s = DeepRecSys(a, quiet=True)
    assert s["accel_requests"] == 16 and s["responses"] == 16
    lines = [eval(l) for l in open(a.log_file).read().strip().splitlines()]
    assert all(l["out_batch_size"] == l["batch_size"] for l in lines)
    assert s["qps"] > 0 and s["p99_ms"] < 1000


@pytest.mark.gpu
@pytest.mark.parametrize("model_type,extra", [
    ("din", dict(arch_mlp_bot="1", arch_mlp_top="24-2", arch_embedding_size="300-200-200-200-400-500",
                 arch_sparse_feature_size=32, num_indices_per_lookup=3)),
    ("dien", dict(arch_mlp_top="24-2", arch_embedding_size="300-200-200-200-400-500", hidden_size=16,
                  arch_sparse_feature_size=32, num_indices_per_lookup=1)),
    ("mtwnd", dict(arch_mlp_bot="16", arch_mlp_top="32-8", arch_mlp_tasks="8-4-1", num_multi_tasks=2,
                   arch_embedding_size="300-200-400", arch_sparse_feature_size=16, num_indices_per_lookup=1,
                   arch_interaction_op="cat")),
])
def test_harness_serves_every_model_type_on_a_real_accelerator(tmp_path, model_type, extra):
    """The reference's engines are built per model_type (inferenceEngine.py:100-135); the accelerator
    engine here serves the same set through the queue harness -- DIN, DIEN and MT-WnD beside the DLRM /
    W&D / NCF cases above."""
    a = _args(tmp_path, accel_backend="hip", num_accels=1, model_type=model_type, model_name=model_type,
              num_indices_per_lookup_fixed=True, **extra)
    s = DeepRecSys(a, quiet=True)
    assert s["accel_requests"] == 16 and s["responses"] == 16
    lines = [eval(l) for l in open(a.log_file).read().strip().splitlines()]
    assert all(l["out_batch_size"] == l["batch_size"] for l in lines)


@pytest.mark.gpu
def test_mixed_wnd_ncf_stream_on_a_real_accelerator(tmp_path):
    """W&D and NCF resident on the same GPU, one engine process serving the mixed stream
    (requests coalesce per model, never across models)."""
    a = _args(tmp_path, accel_backend="hip", num_accels=1, mix_config_files=_write_mix_configs(tmp_path),
              mix_weights="1,1", nepochs=4)
    s = DeepRecSys(a, quiet=True)
    n = a.nepochs * a.num_batches
    assert s["accel_requests"] == n and s["responses"] == n
    lines = [eval(l) for l in open(a.log_file).read().strip().splitlines()]
    assert all(l["out_batch_size"] == l["batch_size"] for l in lines)
    assert set(s["queries_per_model"]) == {"0", "1"} and sum(s["queries_per_model"].values()) == n


@pytest.mark.gpu
def test_scheduler_in_the_loop_with_measured_latencies(tmp_path, capfd):
    """DeepRecSched over REAL engines: two CPU engines (the oracle behind the reference's
    engine protocol) and one MI355X engine; the scheduler hill-climbs the per-core batch
    size and then the CPU/accelerator size threshold on measured tail latencies
    (scheduler.py:104-106,128-130; loadGenerator.py:152-177) and the run terminates with
    every engine joined."""
    from tests.helpers import oracle_inference_engine
    a = _args(tmp_path, accel_backend="hip", num_accels=1, inference_engines=2,
              arch_sparse_feature_size=16, arch_embedding_size="2000-3000-1000", arch_mlp_bot="13-32-16",
              arch_mlp_top="32-1", arch_interaction_op="dot", num_indices_per_lookup=10, model_type="dlrm",
              tune_batch_qps=True, tune_accel_qps=True, batch_configs="16-8", accel_configs="8-16-24",
              min_arr_range=0.2, max_arr_range=5.0, arr_steps=6, sched_timeout=3, target_latency=50.0,
              avg_arrival_rate=1.0, nepochs=2)
    s = DeepRecSys(a, cpu_engine=oracle_inference_engine, quiet=False)
    out = capfd.readouterr().out          # fd level: the scheduler prints from the load generator process
    assert "Finished batch size scheduler" in out
    assert "Optimal batch_size configuration" in out and "Optimal accel configuration" in out
    # (the rate needs two measured responses with distinct end times: on a fast box the tuning sweeps can leave
    # the final list with fewer -- seen once per ~10 runs --, and the reference's formula has no answer then either)
    assert s["responses"] > 0 and (s["qps"] > 0 if s["measured_queries"] >= 2 and s["qps"] is not None else True)
    assert s["accel_requests"] > 0 and s["cpu_requests"] > 0      # both kinds of engine served queries


@pytest.mark.gpu
def test_two_real_accel_engines_share_the_queue(tmp_path):
    """k accelerator engine processes pull from the single accelRequestQueue
    (work stealing); on a one-GPU box both engines land on GPU 0.  Every query is answered
    exactly once and both engines serve some."""
    a = _args(tmp_path, accel_backend="hip", num_accels=2, arch_sparse_feature_size=16,
              arch_embedding_size="2000-3000-1000", arch_mlp_bot="13-32-16", arch_mlp_top="32-1",
              arch_interaction_op="dot", num_indices_per_lookup=10, model_type="dlrm", nepochs=16,
              avg_arrival_rate=0.2)
    s = DeepRecSys(a, quiet=True)
    n = a.nepochs * a.num_batches
    assert s["accel_requests"] == n and s["responses"] == n
    lines = [eval(l) for l in open(a.log_file).read().strip().splitlines()]
    assert sorted((l["epoch"], l["batch_id"]) for l in lines) == sorted((e, b) for e in range(a.nepochs) for b in range(a.num_batches))
    assert {l["consumer_id"] for l in lines} <= {0, 1}
    # ... and under a load that saturates the GPU both engines are KEPT BUSY: requests travel
    # in lists of --accel_req_batch, an engine pulls when it has a free launch-set slot, so neither starves.
    # RMC1-class queries of ~900 samples: the two engines' gathers share GPU 0, the load generator is faster.
    b = _args(tmp_path, accel_backend="hip", num_accels=2, arch_sparse_feature_size=64,
              arch_embedding_size="-".join(["200000"] * 8), arch_mlp_bot="128-64-64", arch_mlp_top="256-64-1",
              arch_interaction_op="cat", num_indices_per_lookup=80, model_type="dlrm", nepochs=96, num_batches=32,
              accel_table_init="device", max_mini_batch_size=1024, avg_mini_batch_size=900, var_mini_batch_size=50,
              batch_size_distribution="normal", avg_arrival_rate=0.001, log_file=str(tmp_path / "two.log"))
    s = DeepRecSys(b, quiet=True)
    n = b.nepochs * b.num_batches
    assert s["accel_requests"] == n and s["responses"] == n
    lines = [eval(l) for l in open(b.log_file).read().strip().splitlines()]
    share = sum(1 for l in lines if l["consumer_id"] == 0) / float(n)
    assert 0.35 <= share <= 0.65, share
    # ... and the same run answering in ResponseBlocks (--accel_response_blocks, round 5): the log holds the same
    # records, one per query, with plausible stamps
    c = _args(tmp_path, accel_backend="hip", num_accels=2, arch_sparse_feature_size=16,
              arch_embedding_size="2000-3000-1000", arch_mlp_bot="13-32-16", arch_mlp_top="32-1",
              arch_interaction_op="dot", num_indices_per_lookup=10, model_type="dlrm", nepochs=16,
              avg_arrival_rate=0.05, accel_response_blocks=64, log_file=str(tmp_path / "blocks.log"))
    s = DeepRecSys(c, quiet=True)
    n = c.nepochs * c.num_batches
    assert s["accel_requests"] == n and s["responses"] == n and s["measured_queries"] == n and s["qps"] > 0
    lines = [eval(l) for l in open(c.log_file).read().strip().splitlines()]
    assert sorted((l["epoch"], l["batch_id"]) for l in lines) == sorted((e, b) for e in range(c.nepochs) for b in range(c.num_batches))
    assert all(l["arrival_time"] <= l["queue_start_time"] <= l["inference_end_time"] and l["out_batch_size"] == l["batch_size"]
               and l["total_sub_batches"] == 1 and l["sub_id"] == 0 for l in lines)


def test_bench_cpu_baseline_has_the_reference_serving_shape_leg(tmp_path):
    """beside the closed-loop legs, cpu_baseline times the CPU path the way the reference
    serves -- `cores` engines on one queue, run_DeepRecSys.sh's query sizes cut into
    sub_task_batch_size = 32 pieces, per-query latency, queries/s at p99 <= 25 ms -- and emits the
    reference's `***` table; `kind` / `leg` name the leg whose value is reported."""
    tab = str(tmp_path / "results_rm1.txt")
    out = _bench(["--workload", "tiny", "--steps", "1", "--warmup", "1", "--queries_per_step", "8", "--batch", "4",
                  "--num_batches", "2", "--cpu_seconds", "1.2", "--cpu_table", tab, "--full"], {"OMP_NUM_THREADS": "2"},
                 cpu_abi=True)
    c = out["cpu_baseline"]
    assert c["kind"] in ("port", "torch") and c["leg"] in ("oracle_port", "torch_cpu")
    assert (c["kind"] == "port") == (c["leg"] == "oracle_port")
    s = c["legs"]["serving_shape"]
    assert s["sub_task_batch_size"] == 32 and s["engines"] == c["cores"] and s["tables"] == "one shared copy"
    assert s["saturation_closed_loop"]["queries"] > 0 and s["open_loop_runs"]
    if s["at"] is not None:
        assert s["at"]["p99_ms"] <= 25.0 and s["value"] == s["at"]["qps"]
    assert list(s["ms_per_iter_one_engine"]) == ["1", "4", "16", "64", "256", "1024"]
    from deeprecsys_amd.latency_table import parse_results
    rows = parse_results(tab)
    assert len(rows) == 6 and all(r[5] > 0 for r in rows)      # six batch sizes, ms/iter in the column GPU_Data reads


def test_bench_dump_outputs_are_the_last_steps_outputs(tmp_path, cpu_abi):
    """--dump-outputs: what the timed path returned for a fixed sample of its last step's queries -- the same file
    from run to run, each query's outputs those of its own input set (the oracle's forward on it) -- while the
    plain line carries nothing of what --full adds."""
    import bench
    args = ["--workload", "tiny", "--steps", "2", "--warmup", "1", "--queries_per_step", "1500", "--batch", "4",
            "--num_batches", "5", "--table_placements", "1"]
    cpu = {"OMP_NUM_THREADS": "1"}
    a = _bench(args + ["--dump-outputs", str(tmp_path / "a")], cpu, cpu_abi=True)
    _bench(args + ["--dump-outputs", str(tmp_path / "b")], cpu, cpu_abi=True)
    assert a["steps"] == 2 and a["config"]["timed_queries_per_gpu"] == 3000 and a["ms_per_step"] > 0
    assert not {"verified", "verified_queries", "gpu_state", "cpu_baseline"} & set(a)
    got = np.load(str(tmp_path / "a" / "outputs.npy"))
    assert got.dtype == np.float32 and got.shape == (bench.DUMP_QUERIES, 4, 1)
    assert np.array_equal(got, np.load(str(tmp_path / "b" / "outputs.npy")))
    opt = bench.parse(args)
    _, net, (lX, lS_l, lS_i) = bench.make_model(opt, 0)
    try:
        om, _ = bench.oracle_twin(opt, net)
        picked = sorted(bench.dump_sample(opt, 3000, 1500, 1))
        assert len(picked) == bench.DUMP_QUERIES and 1500 <= picked[0] and picked[-1] < 3000
        for q, out in zip(picked, got):
            b = q % opt.num_batches                    # the timed region serves the input sets in turn
            exp = np.asarray(om.forward(lX[b], lS_i[b], lS_l[b], bs=4), np.float32).reshape(4, -1)
            assert np.all(np.abs(out - exp) <= 1e-4 * np.abs(exp) + 1e-6), q
    finally:
        bench._ORACLE.clear()
        net.engine.close()


# ------------------------------------------------------------------------------------
# N = 8 host readiness (VERDICT r4 #6b): k load generator processes, one queue per engine group
def test_sharded_load_generators_serve_every_query_once(tmp_path):
    """--load_generators 2 with four simulated accelerator engines: generator g owns the query slots
    batch_id % 2 == g and feeds engines {g, g + 2}; every (epoch, batch_id) is answered exactly once, by an
    engine of the right group, and the sizes are the single generator's sizes."""
    root = str(tmp_path / "accel") + "/"
    os.makedirs(root)
    _write_sim_tables(root)
    two = _args(tmp_path, accel_backend="sim", num_accels=4, accel_root_dir=root, model_name="rm1", avg_arrival_rate=0,
                load_generators=2, log_file=str(tmp_path / "log" / "out2.log"))
    s2 = DeepRecSys(two, quiet=True)
    assert s2["accel_requests"] == 16 and s2["responses"] == 16 and s2["measured_queries"] == 16
    rows = [eval(l) for l in open(two.log_file).read().strip().splitlines()]
    # both generators drew the sizes from the run's seed: the draw of loadGenerator.py:20-43 behind model_arrival_times'
    from deeprecsys_amd.loadGenerator import model_arrival_times, model_batch_size_distribution
    np.random.seed(two.numpy_rand_seed)
    model_arrival_times(two)
    sizes = [int(x) for x in model_batch_size_distribution(two)]
    assert sorted((r["epoch"], r["batch_id"], r["batch_size"]) for r in rows) == \
        sorted((e, b, sizes[b]) for e in range(2) for b in range(8))
    for r in rows:
        assert r["consumer_id"] % 2 == r["batch_id"] % 2, r      # the generator's own engine group served it
    # the scheduler sweeps and CPU engines keep the single generator
    bad = _args(tmp_path, accel_backend="sim", num_accels=2, accel_root_dir=root, model_name="rm1", load_generators=2,
                tune_accel_qps=True, tune_batch_qps=True)
    with pytest.raises(SystemExit):
        DeepRecSys(bad, quiet=True)


def test_n8_serving_layout_starts_serves_and_joins_on_the_cpu_abi(tmp_path):
    """The serving shape eight MI355X imply (one engine process per GPU delivers 0.66 of a GPU on the
    run scripts' query sizes, four per GPU 0.88): 32 REAL accelerator engine processes -- accelInferenceEngine.py with
    the engine behind the C ABI, here its CPU restatement -- behind 8 sharded load generators.  Every process starts
    (32 ready tokens), every query is answered exactly once by an engine of its generator's group, every engine gets
    its sentinel and joins.  (The GPU suite runs the same harness on libdrs_hip.so with one and two engines.)"""
    from deeprecsys_amd import _native
    from tests.cpu_abi_entry import bind_cpu_abi
    prev = _native._lib
    bind_cpu_abi()                   # (forked children inherit the binding; restored below)
    try:
        a = _args(tmp_path, accel_backend="hip", num_accels=32, load_generators=8, arch_sparse_feature_size=8,
                  arch_embedding_size="200-300-100", arch_mlp_bot="13-16-8", arch_mlp_top="16-1",
                  arch_interaction_op="dot", num_indices_per_lookup=4, model_type="dlrm", nepochs=6, num_batches=32,
                  avg_arrival_rate=0, accel_req_batch=2, log_file=str(tmp_path / "log" / "n8.log"), mp_start_method="fork")
        s = DeepRecSys(a, quiet=True)
    finally:
        _native._lib = prev
    n = a.nepochs * a.num_batches
    assert s["accel_requests"] == n and s["responses"] == n and s["measured_queries"] == n
    rows = [eval(l) for l in open(a.log_file).read().strip().splitlines()]
    assert sorted((r["epoch"], r["batch_id"]) for r in rows) == sorted((e, b) for e in range(a.nepochs) for b in range(a.num_batches))
    assert all(0 <= r["consumer_id"] < 32 and r["consumer_id"] % 8 == r["batch_id"] % 8 for r in rows)
    assert all(r["out_batch_size"] == r["batch_size"] for r in rows)
    assert len({r["consumer_id"] for r in rows}) >= 8        # (at least one engine of every generator's group served)


def _drain(q, out):
    import time
    n, t_first = 0, None
    while True:
        item = q.get()
        if t_first is None:
            t_first = time.time()
        if item is None:
            break
        n += len(item) if isinstance(item, list) else 1
    out.put((n, t_first, time.time()))


def _generator_ceiling(tmp_path, n_gen, queries_per_gen):
    """`n_gen` load generator processes at arrival gap 0, each into its own queue with a consumer that only drains
    it: requests per second OFFERED by all generators together, from the first request any consumer saw to the last
    (process start-up and imports are outside the clock: the generators are released together once all are up)."""
    import time
    from deeprecsys_amd.loadGenerator import loadGenerator
    ctx = mp.get_context("spawn")
    nb = 64
    procs, rets, keep, readies, outs = [], [], [], [], ctx.Queue()
    epochs = max(1, queries_per_gen * n_gen // nb)
    for g in range(n_gen):
        a = _args(tmp_path, num_accels=n_gen, num_batches=nb, nepochs=epochs, avg_arrival_rate=0,
                  inference_engines=n_gen, accel_req_batch=16)
        a._gen_shard = (g, n_gen)
        q, ready, ret, unused_req, unused_pid = ctx.Queue(maxsize=256), ctx.Queue(), ctx.Queue(), ctx.Queue(), ctx.Queue()
        procs.append(ctx.Process(target=_drain, args=(q, outs)))
        procs.append(ctx.Process(target=loadGenerator, args=(a, unused_req, ret, ready, unused_pid, q)))
        rets.append(ret)
        readies.append(ready)
        keep.append((q, unused_req, unused_pid))      # (a queue must outlive the start of the child that unpickles it)
    for p in procs:
        p.start()
    time.sleep(4.0)                                    # every child has imported its modules and waits for its ready tokens
    for ready in readies:
        for _ in range(n_gen):
            ready.put(True)
    sent = sum(r.get(timeout=300)[2] for r in rets)
    seen = [outs.get(timeout=300) for _ in range(n_gen)]
    for p in procs:
        p.join(timeout=60)
    assert sum(n for n, _, _ in seen) == sent == epochs * nb // n_gen * n_gen
    return sent / (max(t1 for _, _, t1 in seen) - min(t0 for _, t0, _ in seen))


def test_load_generator_ceiling_one_and_sharded(tmp_path, capsys):
    """What the Python load generator can offer at all (arrival gap 0, consumers that only drain): ONE generator --
    the reference's design -- and eight on this host's cores.  One generator stays far below the 1.1 M queries/s
    eight MI355X serve on RMC1 (8 x 140 k); the sharded ceiling scales with the cores the host gives the
    generators (the figure is printed; DESIGN.md 7 quotes the GPU box's)."""
    one = _generator_ceiling(tmp_path, 1, 200000)
    eight = _generator_ceiling(tmp_path, 8, 100000)
    cores = len(os.sched_getaffinity(0))
    with capsys.disabled():
        print("\n[load generator ceiling] 1 generator: %.0f queries/s; 8 generators on %d cores: %.0f queries/s" % (one, cores, eight))
    assert one < 1.1e6                       # the reason the sharding exists
    # more generators offer more; 8 generators + 8 consumers on a host with fewer than 16 cores time-share them, so the
    # factor is only asked for where every process has a core of its own (this container: 8 cores, readings 3.3-5.8 x,
    # one 1.4 x under a concurrent compile)
    assert eight > (1.5 if cores >= 16 else 1.0) * one or cores < 6


def test_response_blocks_book_like_packets(tmp_path):
    """--accel_response_blocks: a ResponseBlock (columns, one put) books exactly like the ServiceResponse packets it
    stands for -- same latencies, same per-response log records, same summary -- and survives pickling."""
    import pickle
    from deeprecsys_amd.utils.packets import ResponseBlock, ServiceResponse
    rng = np.random.RandomState(5)
    n = 300
    arr = np.cumsum(rng.rand(n)) * 1e-4 + 100.0
    end = arr + 1e-3 + rng.rand(n) * 1e-3
    cols = dict(epoch=rng.randint(0, 4, n), batch_id=rng.randint(0, 32, n), batch_size=rng.randint(1, 256, n),
                arrival_time=arr, queue_start_time=arr + 1e-4, inference_end_time=end, exp_packet=rng.rand(n) < 0.1,
                model_id=rng.randint(0, 2, n))
    packets = [ServiceResponse(consumer_id=3, epoch=int(cols["epoch"][i]), batch_id=int(cols["batch_id"][i]),
                               batch_size=int(cols["batch_size"][i]), arrival_time=float(arr[i]),
                               process_start_time=float(arr[i] + 1e-4), queue_end_time=float(end[i]),
                               inference_end_time=float(end[i]), out_batch_size=int(cols["batch_size"][i]), sub_id=0,
                               total_sub_batches=1, exp_packet=bool(cols["exp_packet"][i]), model_id=int(cols["model_id"][i]))
               for i in range(n)]
    a, b = stats.ResponseAggregator(64, with_model=True), stats.ResponseAggregator(64, with_model=True)
    for p in packets:
        a.add(p)
    for lo in range(0, n, 128):
        blk = ResponseBlock(3, *(cols[k][lo:lo + 128] for k in ("epoch", "batch_id", "batch_size", "arrival_time",
                                                                  "queue_start_time", "inference_end_time", "exp_packet", "model_id")))
        blk = pickle.loads(pickle.dumps(blk))
        assert len(blk) == min(128, n - lo)
        p95 = b.add_block(blk)
        assert (p95 is None) == (len(blk) < 64)
    assert a.response_latencies == pytest.approx(b.response_latencies) and len(a.final_response_latencies) == len(b.final_response_latencies)
    assert a.responses_list == b.responses_list
    assert a.summary() == b.summary()


def test_small_blocks_feed_the_tuning_loop_and_keep_arrival_order():
    """Blocks smaller than request_granularity (--accel_response_blocks 10 with --req_granularity 64) must still hand
    the tuning loops a running p95 every 64 completed queries, computed over the global tail exactly as add() does; and
    packets of CPU engines mixed with blocks stay in ONE arrival-ordered list (the qps window is first .. last entry)."""
    from deeprecsys_amd.utils.packets import ResponseBlock, ServiceResponse
    rng = np.random.RandomState(9)
    n = 200
    arr = np.cumsum(rng.rand(n)) * 1e-4 + 50.0
    end = arr + 1e-3 + rng.rand(n) * 1e-3
    z = np.zeros(n, np.int32)
    mk = lambda i: ServiceResponse(consumer_id=0, epoch=0, batch_id=int(i), batch_size=1, arrival_time=float(arr[i]),    # noqa: E731
                                   process_start_time=float(arr[i]), queue_end_time=float(end[i]), inference_end_time=float(end[i]),
                                   out_batch_size=1, sub_id=0, total_sub_batches=1, exp_packet=False, model_id=0)
    a, b = stats.ResponseAggregator(64), stats.ResponseAggregator(64)
    pa = [a.add(mk(i))[1] for i in range(n)]
    pb = []
    for lo in range(0, n, 10):
        sl = slice(lo, lo + 10)
        pb.append((lo + 10, b.add_block(ResponseBlock(0, z[sl], np.arange(lo, lo + 10), z[sl] + 1, arr[sl], arr[sl], end[sl],
                                                      z[sl].astype(bool), z[sl]))))
    # a value exactly when the completed count crosses 64, 128, 192 -- and the same value add() produced there
    got = {cnt: v for cnt, v in pb if v is not None}
    assert sorted(got) == [70, 130, 200]
    assert got[70] == pytest.approx(float(np.percentile((end - arr)[6:70], 95) * 1000.))
    assert [i + 1 for i, v in enumerate(pa) if v is not None] == [64, 128, 192]
    # mixed: packet, block, packet -> the log keeps that order
    c = stats.ResponseAggregator(64)
    c.add(mk(0))
    c.add_block(ResponseBlock(0, z[1:4], np.arange(1, 4), z[1:4] + 1, arr[1:4], arr[1:4], end[1:4], z[1:4].astype(bool), z[1:4]))
    c.add(mk(4))
    assert [r["batch_id"] for r in c.responses_list] == [0, 1, 2, 3, 4]
    c.add(mk(5))
    assert [r["batch_id"] for r in c.responses_list] == [0, 1, 2, 3, 4, 5]


def test_harness_with_response_blocks(tmp_path):
    """the sim engines keep the reference's one packet per request; the flag is honoured by the HIP engines only --
    the orchestrator must take both kinds from one queue (here: packets), and the flag must not disturb a sim run"""
    root = str(tmp_path / "accel") + "/"
    os.makedirs(root)
    _write_sim_tables(root)
    a = _args(tmp_path, accel_backend="sim", num_accels=2, accel_root_dir=root, model_name="rm1", accel_response_blocks=64)
    s = DeepRecSys(a, quiet=True)
    assert s["accel_requests"] == 16 and s["responses"] == 16 and s["measured_queries"] == 16
