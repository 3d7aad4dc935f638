"""GPU parity suite (-m gpu): the HIP path through the C ABI (include/drs.h) against
the CPU oracle on the same seeded inputs, and against the golden fixtures.

Bars: bit-exact for everything integer/ordering (pooling with the sequential
variant, concat layout, tril order) and for the k-ordered fp32 MFMA chains against
the oracle's fmaf chains; 1e-4 relative (BASELINE.json north_star) for fp32 MLP
outputs against the fp64-accumulated golden values.
"""
import os

import numpy as np
import pytest

from deeprecsys_amd import _native as N
from oracle import oracle as orc
from tests import helpers as H

pytestmark = pytest.mark.gpu


def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch


@pytest.fixture(scope="module")
def op_engine():
    """A tiny engine only used as the handle for operator-level entry points."""
    e = N.Engine(N.MODEL_DLRM, [16, 16], 8, [4, 8], [24, 4, 1], N.INTERACT_CAT, sigmoid_top=2,
                 max_batch=4, max_lookups=2, num_staged_batches=1, num_slots=1)
    yield e
    e.close()


# ------------------------------------------------------------------------------------
# whole forward, every golden model case
@pytest.mark.parametrize("case", H.MODEL_CASES)
def test_forward_matches_oracle_and_golden(case):
    meta, z = H.load_fixture(case)
    args = H.args_from(meta["args"])
    net, lX, lS_l, lS_i, lT = H.materialize(args)
    om = H.oracle_model(net)
    net.create(lX[0], lS_l[0], lS_i[0], lT[0])
    try:
        net.stage_batches(None if args.model_type in H.NO_DENSE else lX, lS_l, lS_i)
        n = len(lS_l[0][0])
        for exact in (1, 0):
            net.engine.set_option("sls_exact", exact)
            for bid in range(len(lS_l)):
                for bs in sorted({n, 1, max(1, n // 2)}):
                    got = net.run_staged(bid, bs)
                    R = net.engine.fetch_interaction(bs)
                    dense = None if args.model_type in H.NO_DENSE else lX[bid]
                    exp, R_exp = om.forward(dense, lS_i[bid], lS_l[bid], bs=bs, want_R=True)
                    if args.model_type == "dien":
                        # tanhf: libm vs the device's differ by an ulp, and the fixture's randn
                        # recurrent weights amplify it over the steps -> tolerance on the states,
                        # bitwise on the pass-through features (sequential gather)
                        Hs = args.hidden_size
                        if exact:
                            assert np.array_equal(R[:, Hs:], R_exp[:, Hs:]), (case, bid, bs)
                        assert H.close(R, R_exp, rtol=1e-4, atol=1e-5), (case, bid, bs, np.abs(R - R_exp).max())
                        assert H.close(got, exp, rtol=H.RTOL_OUT, atol=1e-5), np.abs(got - exp).max()
                    elif exact:
                        # pooled embeddings + concat layout + (dot) tril order + bottom MLP: bitwise;
                        # outputs: identical fma chains up to the last expf -> a few ulp
                        assert np.array_equal(R, R_exp), (case, bid, bs, np.abs(R - R_exp).max())
                        assert H.close(got, exp, rtol=1e-6, atol=1e-7), np.abs(got - exp).max()
                    else:
                        # wave-split pooling: same rows, different fp32 summation order
                        assert H.close(R, R_exp, rtol=1e-5, atol_scale=2e-6), (case, bid, bs)
                        assert H.close(got, exp, rtol=H.RTOL_OUT)
        full = net.run_staged(0, n)
        assert H.close(full, H.golden_output(meta, z), rtol=H.RTOL_OUT, atol=1e-5 if args.model_type == "dien" else 0.0)
        # non-staged inputs (run_queues signature) give the same bits as the staged path
        again = net.run_queued(lS_i[0], lS_l[0], None if args.model_type in H.NO_DENSE else lX[0], n)
        assert np.array_equal(full, again)
    finally:
        net.engine.close()


@pytest.mark.parametrize("case", ["dlrm_cat_queue_small", "dlrm_dot_queue_small"])
def test_queue_requests_from_reference_engine(case):
    """Inputs are exactly what the reference engine enqueued per request."""
    meta, z = H.load_fixture(case)
    args = H.args_from(meta["args"])
    net, lX, lS_l, lS_i, lT = H.materialize(args)
    w = H.M.DLRM_Wrapper.__new__(H.M.DLRM_Wrapper)
    w.args, w.dlrm = args, net
    w.create(lX[0], lS_l[0], lS_i[0], lT[0])
    try:
        T = len(net.emb_w)
        for r, (bid, bs) in enumerate(meta["queue_requests"]):
            ids = np.stack([z["req/%d/id_inputs_%d" % (r, t)] for t in range(T)])
            lens = np.stack([z["req/%d/len_inputs_%d" % (r, t)] for t in range(T)])
            out = w.run_queues(ids, lens, z["req/%d/fc_inputs" % r], bs)
            assert out.shape == (bs, 1)
            assert H.close(out, z["req/%d/expected/prob_click" % r], rtol=H.RTOL_OUT)
            # per-call inputs read in place from pinned host memory (default) == copied to HBM
            # however the converted inputs reach the kernels (per-array copies, read in place over
            # PCIe, one DMA copy of the packed block; default: by size): the same bits
            for mode in ((0, 1, 2) if H.LAB else (1, 2)):
                net.engine.set_option("zero_copy_inputs", mode)
                assert np.array_equal(out, w.run_queues(ids, lens, z["req/%d/fc_inputs" % r], bs)), mode
            net.engine.set_option("zero_copy_inputs", 1)
    finally:
        net.engine.close()


# ------------------------------------------------------------------------------------
# operator level
@pytest.mark.parametrize("D", [4, 8, 16, 32, 48, 64, 128, 256])
@pytest.mark.parametrize("L", [1, 20, 80, 300])
def test_sls_exact_is_bitwise_and_split_is_close(op_engine, D, L):
    torch = torch_cuda()
    rng = np.random.RandomState(D + L)
    rows, bags = 5003, 257
    W = rng.uniform(-1, 1, (rows, D)).astype(np.float32)
    lengths = rng.randint(0, L + 1, size=bags).astype(np.int32)
    lengths[::3] = L
    lengths[5] = 0
    idx = rng.randint(0, rows, size=int(lengths.sum())).astype(np.int32)
    exp = orc.sls(W, idx, lengths)
    dW, di, dl = (torch.from_numpy(a).cuda() for a in (W, idx, lengths))
    out = torch.full((bags, D), float("nan"), device="cuda")
    out.fill_(float("nan"))
    torch.cuda.synchronize()   # inputs/outputs were produced on torch's stream, the op runs on the engine's
    op_engine.sls(dW.data_ptr(), rows, D, di.data_ptr(), dl.data_ptr(), bags, idx.size,
                  out.data_ptr(), exact_order=True)
    assert np.array_equal(out.cpu().numpy(), exp), (D, L)
    out.fill_(float("nan"))
    torch.cuda.synchronize()   # inputs/outputs were produced on torch's stream, the op runs on the engine's
    op_engine.sls(dW.data_ptr(), rows, D, di.data_ptr(), dl.data_ptr(), bags, idx.size,
                  out.data_ptr(), exact_order=False)
    assert H.close(out.cpu().numpy(), exp, rtol=1e-5, atol_scale=1e-6), (D, L)


def test_sls_enforces_like_caffe2(op_engine):
    torch = torch_cuda()
    W = torch.ones(10, 8, device="cuda")
    out = torch.zeros(2, 8, device="cuda")
    idx = torch.tensor([1, 10, 2], dtype=torch.int32, device="cuda")
    ln = torch.tensor([2, 1], dtype=torch.int32, device="cuda")
    with pytest.raises(N.DrsError) as e:
        torch.cuda.synchronize()   # inputs/outputs were produced on torch's stream, the op runs on the engine's
        op_engine.sls(W.data_ptr(), 10, 8, idx.data_ptr(), ln.data_ptr(), 2, 3, out.data_ptr())
    assert e.value.code == N.ERR_INDEX_RANGE
    idx = torch.tensor([1, -1, 2], dtype=torch.int32, device="cuda")
    with pytest.raises(N.DrsError) as e:
        torch.cuda.synchronize()   # inputs/outputs were produced on torch's stream, the op runs on the engine's
        op_engine.sls(W.data_ptr(), 10, 8, idx.data_ptr(), ln.data_ptr(), 2, 3, out.data_ptr())
    assert e.value.code == N.ERR_INDEX_RANGE
    ln = torch.tensor([2, 2], dtype=torch.int32, device="cuda")
    with pytest.raises(N.DrsError) as e:
        torch.cuda.synchronize()   # inputs/outputs were produced on torch's stream, the op runs on the engine's
        op_engine.sls(W.data_ptr(), 10, 8, idx.data_ptr(), ln.data_ptr(), 2, 3, out.data_ptr())
    assert e.value.code == N.ERR_LENGTHS_SUM
    # all-empty bags -> zeros
    ln = torch.zeros(2, dtype=torch.int32, device="cuda")
    out.fill_(7.0)
    torch.cuda.synchronize()   # inputs/outputs were produced on torch's stream, the op runs on the engine's
    op_engine.sls(W.data_ptr(), 10, 8, idx.data_ptr(), ln.data_ptr(), 2, 0, out.data_ptr())
    assert float(out.abs().sum()) == 0.0


@pytest.mark.parametrize("M,K,N_", [(1, 3, 1), (5, 6, 12), (16, 128, 64), (33, 576, 256), (256, 100, 64),
                                    (7, 14, 16), (300, 2560, 1024), (64, 64, 1)])
@pytest.mark.parametrize("act", [N.ACT_NONE, N.ACT_RELU, N.ACT_SIGMOID])
def test_fc_matches_oracle_chain(op_engine, M, K, N_, act):
    torch = torch_cuda()
    rng = np.random.RandomState(M + K + N_)
    x = rng.uniform(-1, 1, (M, K)).astype(np.float32)
    W = rng.normal(0, 0.1, (N_, K)).astype(np.float32)
    b = rng.normal(0, 0.1, N_).astype(np.float32)
    exp = orc.fc(x, W, b, act)
    dx, dW, db = (torch.from_numpy(a).cuda() for a in (x, W, b))
    y = torch.full((M, N_), float("nan"), device="cuda")
    torch.cuda.synchronize()   # inputs/outputs were produced on torch's stream, the op runs on the engine's
    op_engine.fc(dx.data_ptr(), M, K, dW.data_ptr(), db.data_ptr(), N_, act, y.data_ptr())
    got = y.cpu().numpy()
    if act == N.ACT_SIGMOID:
        assert H.close(got, exp, rtol=1e-6, atol=1e-7)
    else:
        assert np.array_equal(got, exp)   # MFMA == k-ordered fmaf chain, bit for bit


@pytest.mark.parametrize("tile", [22, 12, 21, 11, 214, 322, 321, 312, 311, 0])   # 214: the 2 x 1 shape compiled for two workgroups per CU; 3xy: the v_mfma_f32_32x32x2_f32 forms (x * 64 rows, y * 64 columns per workgroup)
@pytest.mark.parametrize("M,K,N_", [(300, 896, 1024), (65, 68, 130), (2048, 1024, 512), (31, 132, 64), (129, 64, 200), (257, 1376, 96)])
def test_gemm_kernel_every_tile_shape_is_bitwise(op_engine, tile, M, K, N_):
    """gemm.hip: each per-wave tile shape (2x2, 1x2, 2x1, 1x1 MFMA tiles; 0 = chosen by block
    count) on shapes with row, column and K tails -- one k-ordered chain per output, bit for bit
    the oracle's."""
    torch = torch_cuda()
    rng = np.random.RandomState(M * 7 + K + N_)
    x = rng.uniform(-1, 1, (M, K)).astype(np.float32)
    W = rng.normal(0, 0.1, (N_, K)).astype(np.float32)
    b = rng.normal(0, 0.1, N_).astype(np.float32)
    exp = orc.fc(x, W, b, N.ACT_RELU)
    dx, dW, db = (torch.from_numpy(a).cuda() for a in (x, W, b))
    y = torch.full((M, N_), float("nan"), device="cuda")
    op_engine.set_option("mlp_gemm_tile", tile)
    try:
        torch.cuda.synchronize()   # inputs/outputs were produced on torch's stream, the op runs on the engine's
        op_engine.fc(dx.data_ptr(), M, K, dW.data_ptr(), db.data_ptr(), N_, N.ACT_RELU, y.data_ptr())
    finally:
        op_engine.set_option("mlp_gemm_tile", 0)
    assert np.array_equal(y.cpu().numpy(), exp)
    # and the kernel it replaces agrees (fc_kernel; "mlp_gemm" 0 is a lab option: narrow layers reach it by themselves)
    if H.LAB:
        op_engine.set_option("mlp_gemm", 0)
        try:
            y2 = torch.full((M, N_), float("nan"), device="cuda")
            torch.cuda.synchronize()   # inputs/outputs were produced on torch's stream, the op runs on the engine's
            op_engine.fc(dx.data_ptr(), M, K, dW.data_ptr(), db.data_ptr(), N_, N.ACT_RELU, y2.data_ptr())
        finally:
            op_engine.set_option("mlp_gemm", 1)
        assert np.array_equal(y2.cpu().numpy(), exp)


@pytest.mark.parametrize("F,D,itself", [(4, 8, False), (4, 8, True), (9, 32, False), (9, 64, True),
                                        (33, 64, False), (11, 32, False), (17, 16, False)])
def test_interact_dot_is_bitwise(op_engine, F, D, itself):
    torch = torch_cuda()
    rng = np.random.RandomState(F * D)
    B = 37
    T = rng.uniform(-1, 1, (B, F, D)).astype(np.float32)
    exp = orc.interact_dot(T, itself)
    dT = torch.from_numpy(T).cuda()
    R = torch.full(exp.shape, float("nan"), device="cuda")
    torch.cuda.synchronize()   # inputs/outputs were produced on torch's stream, the op runs on the engine's
    op_engine.interact_dot(dT.data_ptr(), B, F, D, itself, R.data_ptr())
    assert np.array_equal(R.cpu().numpy(), exp)


# ------------------------------------------------------------------------------------
# BASELINE.json sizes: device-filled tables, oracle on the same counter-based fill
def _big_case(rows, D, T, L, bot, top, B, nb=2, seed=99, op="cat"):
    from deeprecsys_amd.data_generator.dlrm_data import generate_fast_input_data
    args = H.args_from({}, arch_sparse_feature_size=D, arch_embedding_size="-".join([str(rows)] * T),
                       arch_mlp_bot=bot, arch_mlp_top=top, arch_interaction_op=op,
                       num_indices_per_lookup=L, num_batches=nb, max_mini_batch_size=B,
                       mini_batch_size=B, numpy_rand_seed=seed, accel_table_init="device",
                       model_type="dlrm", accel_slots=3)
    np.random.seed(seed)
    net = H.M.DLRM_Net(args)
    m_den = int(bot.split("-")[0])
    nb, lX, lS_l, lS_i = generate_fast_input_data(nb, B, m_den, [rows] * T, L, seed)
    return args, net, lX, lS_l, lS_i


def test_full_size_rmc1_baseline_shape_matches_oracle():
    """BASELINE.json config 2: DLRM-RMC1 8 tables x 1M rows x 64, L=80, batch 256."""
    rows, D, T, L, B = 1_000_000, 64, 8, 80, 256
    args, net, lX, lS_l, lS_i = _big_case(rows, D, T, L, "128-64-64", "256-64-1", B)
    net.create(lX[0], lS_l[0], lS_i[0], None)
    try:
        net.stage_batches(lX, lS_l, lS_i)
        net.engine.set_option("sls_exact", 1)
        lo, hi = -float(np.sqrt(1 / rows)), float(np.sqrt(1 / rows))
        tables = [orc.fill_table_uniform(rows, D, t, lo, hi, args.numpy_rand_seed, nthreads=0)
                  for t in range(T)]
        net.emb_w = tables
        om = H.oracle_model(net)
        for bid in (0, 1):
            for bs in (256, 165, 1):
                got = net.run_staged(bid, bs)
                R = net.engine.fetch_interaction(bs)
                exp, R_exp = om.forward(lX[bid], lS_i[bid], lS_l[bid], bs=bs, want_R=True, nthreads=0)
                assert np.array_equal(R, R_exp)
                assert H.close(got, exp, rtol=1e-6, atol=1e-7)
        # size-independent properties: pooling count is exact (sum over a bag of an all-ones
        # column would be L); slots are independent and deterministic
        eng = net.engine
        for s in range(3):
            eng.forward_async(s, s % 2, 256 - s)
        outs = [eng.wait(s, 256 - s) for s in range(3)]
        for s in range(3):
            assert np.array_equal(outs[s], eng.forward(s % 2, 256 - s))
        assert eng.gather_bytes(0, 256) == 256 * T * (L * D * 4 + L * 4 + 4 + D * 4)
        # ---- exactly what bench.py times (VERDICT r3 #1a): the DEFAULT gather (sls_flatc_kernel), launch
        # sets of 12 and 16 queries, pipelined over the gather stream and the MLP stream with 3 sets in
        # flight -- every query of every set against the oracle: R within the flat-gather tolerance
        # (same rows, different fp32 summation order), outputs within north_star's 1e-4
        eng.set_option("sls_exact", 0)
        assert eng.get_option("shared_stream") == 2 and eng.get_option("preferred_coalesce") == 12
        ref = {}

        def oracle(bid, bs):
            if (bid, bs) not in ref:
                ref[(bid, bs)] = om.forward(lX[bid], lS_i[bid], lS_l[bid], bs=bs, want_R=True, nthreads=0)
            return ref[(bid, bs)]
        for per_set in (12, 16):
            sets = [[((s + k) % 2, 256 if (s + k) % 5 else 165) for k in range(per_set)] for s in range(3)]
            for rnd in range(3):                       # slots are reused while the others are still in flight
                for s in range(3):
                    eng.forward_multi_async(s, [b for b, _ in sets[s]], [n for _, n in sets[s]])
                outs = [eng.wait(s, sum(n for _, n in sets[s])) for s in range(3)]
            for s in range(3):
                Rv = eng.fetch_interaction(256 * per_set, slot=s)   # virtual rows: a query starts at the next multiple of 64
                o = v = 0
                for k, (bid, n) in enumerate(sets[s]):
                    exp, R_exp = oracle(bid, n)
                    assert H.close(Rv[v:v + n], R_exp, rtol=1e-5, atol_scale=2e-6), (per_set, s, k)
                    assert np.array_equal(Rv[v:v + n, :D], R_exp[:, :D])     # bottom MLP: bitwise
                    assert H.close(outs[s][o:o + n], exp, rtol=H.RTOL_OUT, atol=1e-7), (per_set, s, k)
                    o += n
                    v += (n + 63) // 64 * 64
    finally:
        net.engine.close()


FULL_SIZE = {
    # reference models/configs/wide_and_deep.json (BASELINE config 4): 27 x 1M x 32, one lookup per
    # table, 512 dense features, top MLP 896-1024-512-256-1 (two GEMM launches + a chain)
    "wnd": dict(kind="wnd", rows=[1_000_000] * 27, D=32, L=1, bot="512", top="1024-512-256-1"),
    # reference models/configs/ncf.json (BASELINE config 4)
    "ncf": dict(kind="ncf", rows=[140_000, 140_000, 28_000, 28_000], D=64, L=1, bot="512", top="256-256-128-64-64"),
    # reference models/configs/dlrm_rm2.json (BASELINE config 5): 32 x 500k x 64, 120 lookups per
    # bag, top input 2112 wide (too wide for an LDS slab: the per-layer chain kernel)
    "rm2": dict(kind="dlrm", rows=[500_000] * 32, D=64, L=120, bot="256-128-64", top="128-64-1"),
    # reference models/configs/din.json as utils/utils.py:132-149 expands it: 254 tables (profile 1M,
    # 251 behaviour x 100k, ad 10M, context 10M) x 32, 3 lookups, 251 attention units 96-1-32,
    # top MLP 128-200-80-2
    "din": dict(kind="din", rows=[1_000_000] + [100_000] * 251 + [10_000_000] * 2, D=32, L=3, bot="1",
                top="200-80-2"),
    # reference models/configs/dien.json: 43 tables (41 x 500k, 2 x 5M) x 32, one lookup, 40 steps of
    # two BasicRNN layers 32 -> 64 -> 64, top MLP 160-200-80-2 (tanhf differs by an ulp between
    # libm and the device: the top MLP's input row is compared with a tolerance, not bitwise)
    "dien": dict(kind="dien", rows=[500_000] * 41 + [5_000_000] * 2, D=32, L=1, bot="512", top="200-80-2"),
    # reference models/configs/dlrm_rm1.json -- SURVEY 8d's "parity run": 8 x 4M x 32, 80 lookups (the
    # D = 32 instance of the one-bag-per-wave flat gather on 4 M-row tables; the fused launch on 288-wide rows)
    "rmc1_ref": dict(kind="dlrm", rows=[4_000_000] * 8, D=32, L=80, bot="128-64-32", top="256-64-1"),
    # reference models/configs/dlrm_rm3.json: 10 x 2M x 32, 20 lookups, bottom 2560-1024-256-32 (two GEMM
    # launches + a chain), top 352-512-256-1, two bags per wave in the gather
    "rmc3_ref": dict(kind="dlrm", rows=[2_000_000] * 10, D=32, L=20, bot="2560-1024-256-32", top="512-256-1"),
    # reference models/configs/mtwnd.json: 43 tables (41 x 500k, 2 x 5M) x 32, one lookup, shared top
    # 1888-1024-512 (all ReLU, two GEMM launches), task heads 512-256-128 -- one head (num_multi_tasks
    # default) and two heads (the last head's launch carries the hand-off)
    "mtwnd": dict(kind="mtwnd", rows=[500_000] * 41 + [5_000_000] * 2, D=32, L=1, bot="512", top="1024-512",
                  tasks="512-256-128", num_tasks=1),
    "mtwnd_2_heads": dict(kind="mtwnd", rows=[500_000] * 41 + [5_000_000] * 2, D=32, L=1, bot="512", top="1024-512",
                          tasks="512-256-128", num_tasks=2),
}


@pytest.mark.parametrize("name", ["wnd", "mtwnd"])
def test_first_top_layer_reads_the_dense_rows_in_place(name):
    """W&D / MT-WnD (models/wide_and_deep.py:271-281: Concat(dense, pooled embeddings) -> top MLP) at full size, launch
    sets of 16 queries: the first top layer goes to a scalar-base gemm32_kernel that reads the dense columns from the
    queries' own arrays ("gemm_split" 1, the default -- no copy_rows_multi_kernel launch, the dispatch log says so).
    Same bits as with the dense rows copied in front of the embeddings first ("gemm_split" 0), every query against
    the oracle; a set of mixed query sizes (the 64-row padding between queries) as well; the interaction tensor is
    only materialised in the copy form, and drs_fetch_interaction says so."""
    from deeprecsys_amd.data_generator.dlrm_data import generate_fast_input_data
    w = FULL_SIZE[name]
    B, seed, nb = 256, 78, 4
    rows, D, L, T = w["rows"], w["D"], w["L"], len(w["rows"])
    args = H.args_from({}, arch_sparse_feature_size=D, arch_embedding_size="-".join(map(str, rows)),
                       arch_mlp_bot=w["bot"], arch_mlp_top=w["top"], arch_interaction_op="cat",
                       num_indices_per_lookup=L, num_batches=nb, max_mini_batch_size=B, mini_batch_size=B,
                       numpy_rand_seed=seed, accel_table_init="device", model_type=w["kind"], accel_slots=2)
    if "tasks" in w:
        args.arch_mlp_tasks, args.num_multi_tasks = w["tasks"], w["num_tasks"]
    np.random.seed(seed)
    net = H.NET_CLS[w["kind"]](args)
    m_den = int(w["bot"].split("-")[0])
    _, lX, lS_l, lS_i = generate_fast_input_data(nb, B, m_den, rows, L, seed)
    net.create(lX[0], lS_l[0], lS_i[0], None)
    eng = net.engine
    try:
        net.stage_batches(lX, lS_l, lS_i)
        net.emb_w = [orc.fill_table_uniform(rows[t], D, t, -float(np.sqrt(1 / rows[t])), float(np.sqrt(1 / rows[t])),
                                            seed, nthreads=0) for t in range(T)]
        om = H.oracle_model(net)
        full = [(k % nb, B) for k in range(16)]
        mixed = [(k % nb, (B, 165, 200, 256, 77, 256, 1, 250)[k % 8]) for k in range(16)]
        outs = {}
        for split in (1, 0):
            eng.set_option("gemm_split", split)
            for tag, jobs in (("full", full), ("mixed", mixed)):
                outs[(split, tag)] = net.run_staged_multi([b for b, _ in jobs], [n for _, n in jobs])
                disp = " ".join(eng.last_dispatch(0))
                if tag == "full":
                    assert ("split%d" % m_den in disp) == bool(split), disp
                    assert ("copy_rows_multi_kernel" in disp) == (not split), disp
                    if split:
                        with pytest.raises(N.DrsError) as ei:
                            eng.fetch_interaction(B)
                        assert ei.value.code == N.ERR_STATE
                    else:
                        R = eng.fetch_interaction(B)
                        _, R_exp = om.forward(lX[0], lS_i[0], lS_l[0], bs=B, want_R=True, nthreads=0)
                        assert np.array_equal(R, R_exp)
        for tag, jobs in (("full", full), ("mixed", mixed)):
            for k, (b, n) in enumerate(jobs):
                assert np.array_equal(outs[(1, tag)][k], outs[(0, tag)][k]), (name, tag, k)
                if k < 6:
                    exp = om.forward(lX[b], lS_i[b], lS_l[b], bs=n, nthreads=0)
                    assert H.close(outs[(1, tag)][k], exp, rtol=1e-6, atol=1e-7), (name, tag, k)
    finally:
        eng.close()


@pytest.mark.parametrize("name", sorted(FULL_SIZE))
def test_full_size_reference_shapes_match_oracle(name):
    """The shapes BASELINE configs 4 and 5 serve, at FULL size and batch 256, against the oracle
    on the same counter-based table fill: interaction tensor bitwise and outputs to 1e-6 with the
    sequential-order gather, the default gather within its tolerance, 8 coalesced queries equal
    to the same queries served alone, and the launch-structure options bit-identical."""
    from deeprecsys_amd.data_generator.dlrm_data import generate_fast_input_data
    w = FULL_SIZE[name]
    B, seed, nb = 256, 77, 2
    rows, D, L, T = w["rows"], w["D"], w["L"], len(w["rows"])
    args = H.args_from({}, arch_sparse_feature_size=D, arch_embedding_size="-".join(map(str, rows)),
                       arch_mlp_bot=w["bot"], arch_mlp_top=w["top"], arch_interaction_op="cat",
                       num_indices_per_lookup=L, num_batches=nb, max_mini_batch_size=B, mini_batch_size=B,
                       numpy_rand_seed=seed, accel_table_init="device", model_type=w["kind"], accel_slots=2)
    if "tasks" in w:
        args.arch_mlp_tasks, args.num_multi_tasks = w["tasks"], w["num_tasks"]
    np.random.seed(seed)
    net = H.NET_CLS[w["kind"]](args)
    ncf = w["kind"] in H.NO_DENSE
    m_den = int(w["bot"].split("-")[0])
    _, lX, lS_l, lS_i = generate_fast_input_data(nb, B, m_den, rows, L, seed)
    dense = (lambda b: None) if ncf else (lambda b: lX[b])
    net.create(None if ncf else lX[0], lS_l[0], lS_i[0], None)
    eng = net.engine
    try:
        net.stage_batches(None if ncf else lX, lS_l, lS_i)
        net.emb_w = [orc.fill_table_uniform(rows[t], D, t, -float(np.sqrt(1 / rows[t])), float(np.sqrt(1 / rows[t])),
                                            seed, nthreads=0) for t in range(T)]
        om = H.oracle_model(net)
        ref = {}
        # (launch sets in flight the engine asks for: 6 for the MLP-bound class -- streams per slot --, 3 for the gather-bound)
        assert eng.get_option("preferred_slots") == (3 if eng.get_option("gather_bound") else 4 if w["kind"] in ("dien", "mtwnd", "wnd") else 6)
        eng.set_option("sls_exact", 1)
        for bid in (0, 1):
            for bs in (B, 165, 1):
                got = net.run_staged(bid, bs)
                R = eng.fetch_interaction(bs)
                exp, R_exp = om.forward(dense(bid), lS_i[bid], lS_l[bid], bs=bs, want_R=True, nthreads=0)
                if name == "dien":
                    assert np.array_equal(R[:, 64:], R_exp[:, 64:]), (name, bid, bs)      # pooled rows: bitwise
                    assert H.close(R, R_exp, rtol=2e-5, atol=2e-6), (name, bid, bs, np.abs(R - R_exp).max())
                    assert H.close(got, exp, rtol=H.RTOL_OUT, atol=1e-6), (name, bid, bs, np.abs(got - exp).max())
                else:
                    assert np.array_equal(R, R_exp), (name, bid, bs)
                    assert H.close(got, exp, rtol=1e-6, atol=1e-7), (name, bid, bs, np.abs(got - exp).max())
                ref[(bid, bs)] = got
        # 8 coalesced queries (one gather launch, one MLP pass) == the same queries served alone
        jobs = [(0, B), (1, 165), (0, 1), (1, B), (0, 165), (1, 1), (0, B), (1, B)]
        outs = net.run_staged_multi([b for b, _ in jobs], [n for _, n in jobs])
        for (bid, bs), o in zip(jobs, outs):
            assert np.array_equal(o, ref[(bid, bs)]), (name, bid, bs)
        # ... and 16 (DRS_MAX_COALESCE: 4 096 rows give the 16-row MLP workgroups all 256 CUs)
        jobs16 = jobs + jobs[::-1]
        outs = net.run_staged_multi([b for b, _ in jobs16], [n for _, n in jobs16])
        for (bid, bs), o in zip(jobs16, outs):
            assert np.array_equal(o, ref[(bid, bs)]), (name, "16 coalesced", bid, bs)
        # other launch structures of the same arithmetic: bit-identical
        defaults = {k: eng.get_option(k) for k in ("mlp_stream", "mlp_stream_2cu", "mlp_fuse", "shared_stream", "out_dma") +
                    (("mlp_gemm", "mlp_gemm_2cu") if H.LAB else ())}
        for opts in (dict(mlp_stream=0), dict(mlp_stream=1), dict(mlp_stream=2), dict(mlp_stream=4, mlp_stream_2cu=0),
                     dict(mlp_stream=4, mlp_stream_2cu=1), dict(mlp_gemm=0), dict(mlp_gemm_2cu=0), dict(mlp_gemm_2cu=1),
                     dict(mlp_fuse=0), dict(shared_stream=1), dict(out_dma=1)):
            if not H.runs_here(opts):
                continue                                    # (a lab option: DRS_TEST_LAB=1 runs it)
            for key, val in opts.items():
                eng.set_option(key, val)
            assert np.array_equal(net.run_staged(1, B), ref[(1, B)]), (name, opts)
            if "out_dma" in opts:
                # outputs by copy engine + stream-ordered flag write (what sets with megabytes of outputs take):
                # 16 coalesced queries, several sets in flight on the slots
                for rep in range(3):
                    outs = net.run_staged_multi([b for b, _ in jobs16], [n for _, n in jobs16])
                    for (bid, bs), o in zip(jobs16, outs):
                        assert np.array_equal(o, ref[(bid, bs)]), (name, "out_dma", rep, bid, bs)
            for key in opts:
                eng.set_option(key, defaults[key])
        # the tables in another place of HBM ("table_placement": one more copy, switch between them, free the others)
        if name in ("ncf", "rm2", "wnd"):
            assert eng.get_option("table_placements") == 1 and eng.get_option("table_placement") == 0
            eng.set_option("table_placement", -1)
            assert eng.get_option("table_placements") == 2 and eng.get_option("table_placement") == 1
            assert np.array_equal(net.run_staged(1, B), ref[(1, B)]), (name, "second placement")
            eng.set_option("table_placement", 0)
            assert np.array_equal(net.run_staged(1, B), ref[(1, B)]), (name, "first placement again")
            eng.set_option("table_placement", 1)
            eng.set_option("table_placement", -2)
            assert eng.get_option("table_placements") == 1 and eng.get_option("table_placement") == 0
            assert np.array_equal(net.run_staged(1, B), ref[(1, B)]), (name, "after freeing the others")
            with pytest.raises(Exception):
                eng.set_option("table_placement", 3)
            # the other ways to build an arena (round 5): the virtual-memory API in 1 GiB handles, best-effort contiguous
            # memory, and a spacer of untouched memory in front of a candidate -- same tables, same bits
            for alloc in (1, 2):
                eng.set_option("table_alloc", alloc)
                eng.set_option("table_spacer", 1 << 30)
                eng.set_option("table_placement", -1)
                assert eng.get_option("table_placements") == 2 and eng.get_option("table_placement") == 1
                assert np.array_equal(net.run_staged(1, B), ref[(1, B)]), (name, "table_alloc", alloc)
                assert np.array_equal(net.run_staged(0, 165), ref[(0, 165)]), (name, "table_alloc", alloc)
                eng.set_option("table_placement", 0)
                eng.set_option("table_placement", -2)
                assert eng.get_option("table_placements") == 1
            eng.set_option("table_alloc", 0)
            tuned = net.tune_table_placement(3, sets=16)      # (gather-bound DLRM only: rm2 here)
            assert (tuned is None) == (name != "rm2"), (name, tuned)
            if tuned is not None:      # up to three arenas x two load policies timed, the best kept, every other arena released
                assert 1 <= len(tuned["gather_us"]) <= 3 and all(len(t) == 2 for t in tuned["gather_us"])
                assert tuned["losers"] == "freed" and eng.get_option("table_placements") == 1 and eng.get_option("table_placement") == 0
                assert eng.get_option("sls_nt") == tuned["sls_nt"] and eng.get_option("table_alloc") == 0
            assert np.array_equal(net.run_staged(1, B), ref[(1, B)]), (name, "after tuning")
        # default gather (flat / wave-split / lane-group-per-bag by shape): the pooling tolerance
        eng.set_option("sls_exact", 0)
        got = net.run_staged(0, B)
        R = eng.fetch_interaction(B)
        _, R_exp = om.forward(dense(0), lS_i[0], lS_l[0], bs=B, want_R=True, nthreads=0)
        assert H.close(R, R_exp, rtol=2e-5 if name == "dien" else 1e-5, atol_scale=2e-6)
        assert H.close(got, ref[(0, B)], rtol=H.RTOL_OUT, atol=1e-6 if name == "dien" else 0.0)
        assert eng.gather_bytes(0, B) == B * T * (L * D * 4 + L * 4 + 4 + D * 4)
    finally:
        eng.close()


# ------------------------------------------------------------------------------------
# The engine as the reference's run scripts build it: max_mini_batch_size 1024
# (run_DeepRecSys.sh:32-36, experiments/scheduling/run_Scheduler.sh:38-44), queries = prefixes of
# 1024-sample batches (inferenceEngine.py:200-206).  A slot then holds 16 x 1024 virtual rows and
# launch sets pick their kernel forms by row count at sizes the batch-256 tests never reach.
RUN_SCRIPT_SHAPES = {
    "rmc1": dict(kind="dlrm", rows=[1_000_000] * 8, D=64, L=80, bot="128-64-64", top="256-64-1"),     # BASELINE config 2's tables
    "rm2": FULL_SIZE["rm2"],       # run_DeepRecSys.sh's own model (dlrm_rm2.json)
    "wnd": FULL_SIZE["wnd"],
}
# first token of a launch set's dispatch: the gather kernel the shape takes by default / with sls_exact
GATHER_FORM = {"rmc1": ("sls_flatc_kernel<16,20,nt>", "sls_kernel<16,sequential>"),
               "rm2": ("sls_kernel<16,split,nt>", "sls_kernel<16,sequential>"),
               "wnd": ("sls_one_kernel<8,", "sls_one_kernel<8,")}      # one lookup per bag: the copy form in either mode


@pytest.mark.parametrize("name", sorted(RUN_SCRIPT_SHAPES))
def test_engine_built_as_the_run_scripts_build_it(name):
    """max_batch 1024, two staged 1024-sample batches: single queries of 257 .. 1024 samples (sequential gather:
    R bitwise, outputs 1e-6; default gather: its tolerance, outputs north_star's 1e-4), then pipelined launch sets
    of 12 and 16 mixed-size queries drawn like the run scripts draw them -- normal(165, 16) and
    lognormal(5.1, 0.2), clamped to [1, 1024] -- three sets in flight, EVERY query against the oracle.  The
    kernel forms each row count selected are read back (drs_last_dispatch) and written to
    gpurun_out/dispatch_1024_<name>.json."""
    import json
    from deeprecsys_amd.data_generator.dlrm_data import generate_fast_input_data
    from deeprecsys_amd.loadGenerator import model_batch_size_distribution
    w = RUN_SCRIPT_SHAPES[name]
    B, seed, nb = 1024, 31, 2
    rows, D, L, T = w["rows"], w["D"], w["L"], len(w["rows"])
    args = H.args_from({}, arch_sparse_feature_size=D, arch_embedding_size="-".join(map(str, rows)),
                       arch_mlp_bot=w["bot"], arch_mlp_top=w["top"], arch_interaction_op="cat",
                       num_indices_per_lookup=L, num_batches=nb, max_mini_batch_size=B, mini_batch_size=B,
                       numpy_rand_seed=seed, accel_table_init="device", model_type=w["kind"], accel_slots=3)
    np.random.seed(seed)
    net = H.NET_CLS[w["kind"]](args)
    m_den = int(w["bot"].split("-")[0])
    _, lX, lS_l, lS_i = generate_fast_input_data(nb, B, m_den, rows, L, seed)
    net.create(lX[0], lS_l[0], lS_i[0], None)
    eng = net.engine
    forms = {}
    try:
        net.stage_batches(lX, lS_l, lS_i)
        net.emb_w = [orc.fill_table_uniform(rows[t], D, t, -float(np.sqrt(1 / rows[t])), float(np.sqrt(1 / rows[t])),
                                            seed, nthreads=0) for t in range(T)]
        om = H.oracle_model(net)
        ref = {}

        def oracle(bid, bs):
            if (bid, bs) not in ref:
                ref[(bid, bs)] = om.forward(lX[bid], lS_i[bid], lS_l[bid], bs=bs, want_R=True, nthreads=0)
            return ref[(bid, bs)]
        singles = (257, 320, 512, 1000, 1024)
        eng.set_option("sls_exact", 1)
        for bs in singles:
            bid = bs % 2
            got = net.run_staged(bid, bs)
            R = eng.fetch_interaction(bs)
            exp, R_exp = oracle(bid, bs)
            assert np.array_equal(R, R_exp), (name, "sequential gather", bs)
            assert H.close(got, exp, rtol=1e-6, atol=1e-7), (name, bs, np.abs(got - exp).max())
            forms["single %d, sls_exact" % bs] = eng.last_dispatch()
            if L == 1:          # 64 samples of one table per wave; 16 while that leaves the launch under 1 024 waves
                bw = 16 if T * -(-bs // 64) < 1024 else 64
                assert forms["single %d, sls_exact" % bs][1] == "%s%d>[%d wg]" % (GATHER_FORM[name][1], bw, T * -(-bs // bw)), forms
            else:
                assert forms["single %d, sls_exact" % bs][1] == "%s[%d wg]" % (GATHER_FORM[name][1], -(-bs * T // (64 // (16 if D == 64 else 8)))), forms
        eng.set_option("sls_exact", 0)
        for bs in singles:
            bid = (bs + 1) % 2
            got = net.run_staged(bid, bs)
            R = eng.fetch_interaction(bs)
            exp, R_exp = oracle(bid, bs)
            assert H.close(R, R_exp, rtol=1e-5, atol_scale=2e-6), (name, "default gather", bs)
            assert H.close(got, exp, rtol=H.RTOL_OUT, atol=1e-7), (name, bs, np.abs(got - exp).max())
            forms["single %d" % bs] = eng.last_dispatch()
            assert forms["single %d" % bs][1].startswith(GATHER_FORM[name][0]), forms
        assert eng.get_option("shared_stream") == 2
        for dist, avg, var in (("normal", 165, 16), ("lognormal", 5.1, 0.2)):
            da = H.args_from({}, batch_size_distribution=dist, avg_mini_batch_size=avg, var_mini_batch_size=var,
                             max_mini_batch_size=B, num_batches=3 * 16)
            np.random.seed(123)                                   # utils/utils.py:110, loadGenerator.py:20-43
            sizes = [int(x) for x in model_batch_size_distribution(da)]
            # the tails the clamps exist for: one query at each end of [1, 1024] in every draw
            sizes[5], sizes[21] = 1, B
            for per_set in (12, 16):
                sets = [[((s + k) % 2, sizes[s * 16 + k]) for k in range(per_set)] for s in range(3)]
                for rnd in range(3):                              # slots are reused while the others are still in flight
                    for s in range(3):
                        eng.forward_multi_async(s, [b for b, _ in sets[s]], [n for _, n in sets[s]])
                    outs = [eng.wait(s, sum(n for _, n in sets[s])) for s in range(3)]
                for s in range(3):
                    vrows = sum((n + 63) // 64 * 64 for _, n in sets[s])
                    forms["%s, %d queries, %d rows" % (dist, per_set, vrows)] = eng.last_dispatch(s)
                    if any("gemm32_kernel" in d and ",split" in d for d in eng.last_dispatch(s)):
                        # W&D from 3 072 rows on: the first top layer read the dense columns from the queries' own arrays,
                        # the interaction tensor was never whole -- the fetch says so; the same set with "gemm_split" 0
                        # (same bits out) materialises it
                        with pytest.raises(N.DrsError) as ei:
                            eng.fetch_interaction(vrows, slot=s)
                        assert ei.value.code == N.ERR_STATE
                        eng.set_option("gemm_split", 0)
                        eng.forward_multi_async(s, [b for b, _ in sets[s]], [n for _, n in sets[s]])
                        assert np.array_equal(eng.wait(s, sum(n for _, n in sets[s])), outs[s])
                        Rv = eng.fetch_interaction(vrows, slot=s)
                        eng.set_option("gemm_split", 1)
                    else:
                        Rv = eng.fetch_interaction(vrows, slot=s)
                    o = v = 0
                    for k, (bid, n) in enumerate(sets[s]):
                        exp, R_exp = oracle(bid, n)
                        assert H.close(Rv[v:v + n], R_exp, rtol=1e-5, atol_scale=2e-6), (name, dist, per_set, s, k, n)
                        assert H.close(outs[s][o:o + n], exp, rtol=H.RTOL_OUT, atol=1e-7), (name, dist, per_set, s, k, n)
                        o += n
                        v += (n + 63) // 64 * 64
        # a set of 16 full 1024-sample queries: the slot's whole capacity (16 384 virtual rows)
        full = [(k % 2, B) for k in range(16)]
        outs = net.run_staged_multi([b for b, _ in full], [n for _, n in full])
        forms["16 x 1024"] = eng.last_dispatch(0)
        for (bid, n), o in zip(full, outs):
            assert H.close(o, oracle(bid, n)[0], rtol=H.RTOL_OUT, atol=1e-7), (name, "16 x 1024", bid)
    finally:
        eng.close()
        os.makedirs(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpurun_out"), exist_ok=True)
        with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpurun_out",
                               "dispatch_1024_%s.json" % name), "w") as f:
            json.dump(forms, f, indent=1)


def test_split_variant_within_tolerance_full_size():
    rows, D, T, L, B = 200_000, 32, 8, 80, 128
    args, net, lX, lS_l, lS_i = _big_case(rows, D, T, L, "128-64-32", "256-64-1", B, nb=1)
    net.create(lX[0], lS_l[0], lS_i[0], None)
    try:
        net.stage_batches(lX, lS_l, lS_i)
        net.engine.set_option("sls_exact", 1)
        exact = net.run_staged(0, B)
        R_exact = net.engine.fetch_interaction(B)
        net.engine.set_option("sls_exact", 0)
        split = net.run_staged(0, B)
        R_split = net.engine.fetch_interaction(B)
        assert H.close(R_split, R_exact, rtol=1e-5, atol_scale=2e-6)
        assert H.close(split, exact, rtol=H.RTOL_OUT)
    finally:
        net.engine.close()


def test_engine_ragged_bags_and_device_error_path():
    """Variable bag lengths (incl. empty bags) through the staged path (prefix-sum
    offsets), for both gather variants; and Caffe2's ENFORCEs at the ABI."""
    rng = np.random.RandomState(5)
    rows, D, T, B, Lmax = [300, 200, 100], 16, 3, 37, 9
    args = H.args_from({}, arch_sparse_feature_size=D, arch_embedding_size="-".join(map(str, rows)),
                       arch_mlp_bot="12-16", arch_mlp_top="8-1", arch_interaction_op="dot",
                       num_indices_per_lookup=Lmax, num_batches=1, max_mini_batch_size=B,
                       mini_batch_size=B, numpy_rand_seed=3, model_type="dlrm")
    np.random.seed(3)
    net = H.M.DLRM_Net(args)
    om = H.oracle_model(net)
    lens = [rng.randint(0, Lmax + 1, size=B).astype(np.int32) for _ in range(T)]
    lens[0][:4] = 0
    idx = [rng.randint(0, rows[t], size=int(lens[t].sum())).astype(np.int64) for t in range(T)]
    X = rng.rand(B, 12).astype(np.float32)
    net.create(X, lens, idx, None)
    try:
        net.engine.stage_batch(0, X, idx, lens)
        for exact in (1, 0):
            net.engine.set_option("sls_exact", exact)
            for bs in (B, 20, 1):
                got = net.run_staged(0, bs)
                R = net.engine.fetch_interaction(bs)
                exp, R_exp = om.forward(X, idx, lens, bs=bs, want_R=True)
                if exact:
                    assert np.array_equal(R, R_exp)
                else:
                    assert H.close(R, R_exp, rtol=1e-5, atol_scale=2e-6)
                assert H.close(got, exp, rtol=H.RTOL_OUT)
        before = net.run_staged(0, B).copy()
        bytes_before = net.engine.gather_bytes(0, B)
        bad = [i.copy() for i in idx]
        bad[1][3] = rows[1]
        with pytest.raises(N.DrsError) as e:
            net.engine.stage_batch(0, X, bad, lens)
        assert e.value.code == N.ERR_INDEX_RANGE
        # a staging call that fails validation part-way (table 1 of 3) leaves the batch that was
        # staged before exactly as it was: device data AND the host-side offsets
        assert np.array_equal(net.run_staged(0, B), before) and net.engine.gather_bytes(0, B) == bytes_before
        with pytest.raises(N.DrsError) as e:
            net.engine.stage_batch(0, X, [i[:-1] for i in idx], lens)
        assert e.value.code == N.ERR_LENGTHS_SUM
        with pytest.raises(N.DrsError) as e:
            net.engine.forward(0, B + 1)
        assert e.value.code == N.ERR_BAD_ARG
        # engine still healthy afterwards
        net.engine.stage_batch(0, X, idx, lens)
        assert net.run_staged(0, B).shape == (B, 1)
    finally:
        net.engine.close()


@pytest.mark.parametrize("D,h,U,ragged", [(32, 1, 6, False), (32, 1, 70, True), (64, 2, 9, True), (32, 4, 130, False),
                                          (16, 1, 5, False), (32, 3, 5, True), (32, 1, 251, False), (64, 1, 70, False),
                                          (32, 1, 33, False)])
def test_din_fused_and_two_launch_forms_match_oracle(D, h, U, ragged):
    """DIN's default launch fuses gather, attention units and Concat (din.hip); "sls_exact" 1 and
    "din_fused" 0 take the two-launch form.  Both against the oracle: two-launch + sequential
    gather bitwise on the top MLP's input row, the fused form within the default-mode tolerance
    -- over ragged bags (incl. empty ones and samples past a workgroup's last), hidden widths
    with and without a fused instance (3: falls back), D without one (16), more units than one
    round of lane groups, and 8 coalesced queries whose samples share workgroups.  Hidden width 1 with
    fixed-length bags of <= 3 rows takes the PIPELINED fused form (din_pipe_kernel: indices staged in
    LDS, units in flight per lane group): the dispatch log says so, and its bits equal the chained
    form's ("din_pipe" 0) at every samples-per-workgroup setting."""
    rng = np.random.RandomState(D + h + U)
    rows = [500] + [300] * U + [700, 400]
    T, B, Lmax = len(rows), 150, 5
    args = H.args_from({}, arch_sparse_feature_size=D, arch_embedding_size="-".join(map(str, rows)),
                       arch_mlp_bot=str(h), arch_mlp_top="24-2", arch_interaction_op="cat",
                       num_indices_per_lookup=Lmax, num_batches=2, max_mini_batch_size=B,
                       mini_batch_size=B, numpy_rand_seed=3, model_type="din", accel_slots=2)
    np.random.seed(3)
    net = H.M.DIN_Net(args)
    om = H.oracle_model(net)
    sets = []
    for b in range(2):
        if ragged:
            lens = [rng.randint(0, Lmax + 1, size=B).astype(np.int32) for _ in range(T)]
            lens[T - 2][:3] = 0
            lens[1][5:9] = 0
        else:
            lens = [np.full(B, 3, dtype=np.int32) for _ in range(T)]
        idx = [rng.randint(0, rows[t], size=int(lens[t].sum())).astype(np.int64) for t in range(T)]
        sets.append((idx, lens))
    net.create(None, sets[0][1], sets[0][0], None)
    eng = net.engine
    try:
        for b, (idx, lens) in enumerate(sets):
            eng.stage_batch(b, None, idx, lens)
        ref = {}
        fused_instance = D in (32, 64) and h in (1, 2, 4)
        for mode, opts in (("exact", {"sls_exact": 1}), ("two-launch", {"sls_exact": 0, "din_fused": 0}),
                           ("fused", {"sls_exact": 0, "din_fused": 1})):
            for k, v in opts.items():
                eng.set_option(k, v)
            for b, (idx, lens) in enumerate(sets):
                for bs in (B, 77, 1):
                    got = net.run_staged(b, bs)
                    R = eng.fetch_interaction(bs)
                    exp, R_exp = om.forward(None, idx, lens, bs=bs, want_R=True)
                    assert R.shape == (bs, 4 * D)
                    if mode == "exact":
                        assert np.array_equal(R, R_exp), (mode, b, bs, np.abs(R - R_exp).max())
                        assert H.close(got, exp, rtol=1e-6, atol=1e-7)
                    else:
                        assert H.close(R, R_exp, rtol=1e-5, atol_scale=2e-6), (mode, b, bs, np.abs(R - R_exp).max())
                        assert H.close(got, exp, rtol=H.RTOL_OUT), (mode, b, bs)
                    # the pass-through features are pooled in index order by every form: bitwise
                    for lo in (0, 2 * D, 3 * D):
                        if mode == "exact" or (mode == "fused" and fused_instance):
                            assert np.array_equal(R[:, lo:lo + D], R_exp[:, lo:lo + D]), (mode, lo)
                    ref[(mode, b, bs)] = got
            # a query's bits do not depend on what it was coalesced with, nor on how many samples
            # share a workgroup
            if mode == "fused":
                piped = fused_instance and h == 1 and not ragged
                for S_ in (1, 2, 4):
                    eng.set_option("din_s", S_)
                    assert np.array_equal(net.run_staged(1, B), ref[(mode, 1, B)]), S_
                    assert ("din_pipe_kernel" in " ".join(eng.last_dispatch())) == piped, eng.last_dispatch()
                    if piped:
                        eng.set_option("din_pipe", 0)
                        for bs in (B, 77, 1):
                            assert np.array_equal(net.run_staged(1, bs), ref[(mode, 1, bs)]), (S_, bs)
                        assert "din_fused_kernel" in " ".join(eng.last_dispatch())
                        eng.set_option("din_pipe", 1)
                        assert np.array_equal(net.run_staged(1, 77), ref[(mode, 1, 77)]), S_
                eng.set_option("din_s", 0)
            jobs = [(0, B), (1, 77), (0, 1), (1, B), (0, 77), (1, 1), (0, B), (1, B)]
            outs = net.run_staged_multi([b for b, _ in jobs], [n for _, n in jobs])
            for (b, bs), o in zip(jobs, outs):
                assert np.array_equal(o, ref[(mode, b, bs)]), (mode, b, bs)
        # Caffe2's ENFORCE on an index past the table (checked on the host at hand-over; the
        # kernels' own flag is the backstop for device-resident inputs)
        bad = [i.copy() for i in sets[0][0]]
        bad[2][0] = rows[2]
        with pytest.raises(N.DrsError) as e:
            net.run_queued(bad, sets[0][1], None, B)
        assert e.value.code == N.ERR_INDEX_RANGE
        assert net.run_staged(0, B).shape == (B, 2)
    finally:
        eng.close()


@pytest.mark.parametrize("D,Hs,U,init", [(32, 64, 40, "xavier"), (16, 8, 5, "fed"), (64, 32, 9, "xavier"), (32, 16, 3, "xavier")])
def test_dien_recurrent_layers_match_oracle(D, Hs, U, init):
    """DIEN's two BasicRNN layers (dien.hip) against the oracle: the pass-through features bitwise,
    the recurrent state within the tanhf tolerance; query sizes 1 .. B (the reference's Reshape makes
    a sample's sequence depend on its query's batch size), ragged bags, 8 coalesced queries of
    different sizes equal to the same queries served alone."""
    rng = np.random.RandomState(D + Hs + U)
    rows = [500] + [300] * U + [700, 400]
    T, B, Lmax = len(rows), 70, 3
    args = H.args_from({}, arch_sparse_feature_size=D, arch_embedding_size="-".join(map(str, rows)),
                       arch_mlp_top="24-2", hidden_size=Hs, arch_interaction_op="cat",
                       num_indices_per_lookup=Lmax, num_batches=2, max_mini_batch_size=B,
                       mini_batch_size=B, numpy_rand_seed=3, model_type="dien", accel_slots=2)
    args.dien_rnn_init = init
    np.random.seed(3)
    net = H.M.DIEN_Net(args)
    om = H.oracle_model(net)
    sets = []
    for b in range(2):
        lens = [rng.randint(0, Lmax + 1, size=B).astype(np.int32) for _ in range(T)]
        idx = [rng.randint(0, rows[t], size=int(lens[t].sum())).astype(np.int64) for t in range(T)]
        sets.append((idx, lens))
    net.create(None, sets[0][1], sets[0][0], None)
    eng = net.engine
    # randn weights (the values models/dien.py feeds) make the recurrence chaotic: looser bar
    rtol, atol = (1e-3, 1e-4) if init == "fed" else (2e-5, 2e-6)
    try:
        for b, (idx, lens) in enumerate(sets):
            eng.stage_batch(b, None, idx, lens)
        eng.set_option("sls_exact", 1)
        ref = {}
        for b, (idx, lens) in enumerate(sets):
            for bs in (B, 33, 2, 1):
                got = net.run_staged(b, bs)
                R = eng.fetch_interaction(bs)
                exp, R_exp = om.forward(None, idx, lens, bs=bs, want_R=True)
                assert R.shape == (bs, Hs + 3 * D)
                assert np.array_equal(R[:, Hs:], R_exp[:, Hs:]), (b, bs)
                assert H.close(R, R_exp, rtol=rtol, atol=atol), (b, bs, np.abs(R - R_exp).max())
                assert H.close(got, exp, rtol=max(rtol, H.RTOL_OUT), atol=atol), (b, bs, np.abs(got - exp).max())
                ref[(b, bs)] = got
        jobs = [(0, B), (1, 33), (0, 1), (1, B), (0, 33), (1, 2), (0, 2), (1, 1)]
        assert eng.get_option("dien_fuse_top") == 1
        for mfma, fuse in ((1, 1), (2, 0), (2, 1), (1, 0), (0, 1), (3, 1), (3, 0)):
            # the matrix-core form (16 samples per workgroup; hidden sizes that are multiples of 16),
            # the one-wave-per-sample form and the any-shape form (3: one workgroup per sample, din_any.hip)
            # run the same fma chains: the same bits -- with the top MLP inside the recurrence's launch
            # (its default when it fits) or in a launch of its own behind it
            eng.set_option("dien_mfma", mfma)
            eng.set_option("dien_fuse_top", fuse)
            outs = net.run_staged_multi([b for b, _ in jobs], [n for _, n in jobs])
            for (b, bs), o in zip(jobs, outs):
                assert np.array_equal(o, ref[(b, bs)]), (mfma, fuse, b, bs)
            assert any("dien_rnn_any_kernel" in d for d in eng.last_dispatch()) == (mfma == 3), eng.last_dispatch()
    finally:
        eng.close()


@pytest.mark.parametrize("D,bot,U", [(32, "8-4", 5),        # two hidden layers
                                     (32, "100", 4),         # one hidden layer, wider than din.hip's 64
                                     (10, "3", 6),           # rows that are not 16-byte pieces
                                     (300, "5-7-9", 3),      # rows wider than 256 columns, three hidden layers
                                     (16, "600", 8),         # (T - 3) * h beyond the two-launch kernel's LDS
                                     (6, "2-300-1", 3)])     # a hidden layer wider than a workgroup
def test_din_attention_units_of_any_shape_match_oracle(D, bot, U):
    """An attention unit is create_mlp over 3*D - <arch_mlp_bot> - D, any depth and widths (models/din.py:255-277);
    din.hip serves one hidden layer of <= 64 units over 16-byte row pieces, everything else takes
    din_attention_any_kernel (din_any.hip: each output its own k-ordered fmaf chain, the oracle's order).  The top
    MLP's input row bit-exact after the sequential-order gather, outputs to 1e-6; ragged bags (empty ones included),
    query sizes 1 .. B, coalesced queries equal to the same queries alone."""
    rng = np.random.RandomState(D + U)
    rows = [500] + [300] * U + [700, 400]
    T, B, Lmax = len(rows), 70, 4
    args = H.args_from({}, arch_sparse_feature_size=D, arch_embedding_size="-".join(map(str, rows)),
                       arch_mlp_bot=bot, arch_mlp_top="24-2", arch_interaction_op="cat",
                       num_indices_per_lookup=Lmax, num_batches=2, max_mini_batch_size=B,
                       mini_batch_size=B, numpy_rand_seed=3, model_type="din", accel_slots=2)
    np.random.seed(3)
    net = H.M.DIN_Net(args)
    om = H.oracle_model(net)
    sets = []
    for b in range(2):
        lens = [rng.randint(0, Lmax + 1, size=B).astype(np.int32) for _ in range(T)]
        lens[T - 2][:3] = 0
        idx = [rng.randint(0, rows[t], size=int(lens[t].sum())).astype(np.int64) for t in range(T)]
        sets.append((idx, lens))
    net.create(None, sets[0][1], sets[0][0], None)
    eng = net.engine
    try:
        for b, (idx, lens) in enumerate(sets):
            eng.stage_batch(b, None, idx, lens)
        sequential_anyway = D % 4 != 0 or D > 256          # sls_any_kernel sums in index order in either mode
        ref = {}
        for exact in (1, 0):
            eng.set_option("sls_exact", exact)
            for b, (idx, lens) in enumerate(sets):
                for bs in (B, 33, 1):
                    got = net.run_staged(b, bs)
                    assert any("din_attention_any_kernel" in d for d in eng.last_dispatch()), eng.last_dispatch()
                    R = eng.fetch_interaction(bs)
                    exp, R_exp = om.forward(None, idx, lens, bs=bs, want_R=True)
                    assert R.shape == (bs, 4 * D)
                    if exact or sequential_anyway:
                        assert np.array_equal(R, R_exp), (exact, b, bs, np.abs(R - R_exp).max())
                        assert H.close(got, exp, rtol=1e-6, atol=1e-7), (exact, b, bs)
                    else:
                        assert H.close(R, R_exp, rtol=1e-5, atol_scale=2e-6), (b, bs, np.abs(R - R_exp).max())
                        # (an output a ReLU holds near zero is a cancellation: the floor of the R check)
                        assert H.close(got, exp, rtol=H.RTOL_OUT, atol_scale=2e-6), (b, bs, np.abs(got - exp).max())
                    ref[(exact, b, bs)] = got
            jobs = [(0, B), (1, 33), (0, 1), (1, B), (0, 33), (1, 1), (0, 1), (1, 33), (0, B), (1, 1), (0, 33)]
            outs = net.run_staged_multi([b for b, _ in jobs], [n for _, n in jobs])
            for (b, bs), o in zip(jobs, outs):
                assert np.array_equal(o, ref[(exact, b, bs)]), (exact, b, bs)
        # per-call inputs take the same path
        idx, lens = sets[1]
        assert np.array_equal(eng.forward_inputs(None, idx, lens, B), ref[(0, 1, B)])
    finally:
        eng.close()


@pytest.mark.parametrize("D,Hs,U", [(32, 100, 7),      # hidden size beyond dien.hip's 64
                                    (24, 40, 5),        # neither is one of dien.hip's instances
                                    (10, 7, 4),         # rows that are not 16-byte pieces, odd hidden size
                                    (64, 128, 6),       # a multiple of 16 the matrix-core form has no instance for
                                    (300, 20, 3),       # rows wider than 256 columns
                                    (16, 600, 3)])      # more hidden units than a workgroup has threads
def test_dien_recurrence_of_any_shape_matches_oracle(D, Hs, U):
    """rnn_cell.BasicRNN(arch_sparse_feature_size -> hidden_size) for any two integers (models/dien.py:308-380): the
    pairs dien.hip has no instance for take dien_rnn_any_kernel (din_any.hip).  Pass-through features bitwise, the
    recurrent state within the tanh tolerance of test_dien_recurrent_layers_match_oracle; query sizes 1 .. B (the
    Reshape makes a sample's sequence depend on its query's size), ragged bags, coalesced = alone."""
    rng = np.random.RandomState(D + Hs + U)
    rows = [500] + [300] * U + [700, 400]
    T, B, Lmax = len(rows), 50, 3
    args = H.args_from({}, arch_sparse_feature_size=D, arch_embedding_size="-".join(map(str, rows)),
                       arch_mlp_top="24-2", hidden_size=Hs, arch_interaction_op="cat",
                       num_indices_per_lookup=Lmax, num_batches=2, max_mini_batch_size=B,
                       mini_batch_size=B, numpy_rand_seed=3, model_type="dien", accel_slots=2)
    args.dien_rnn_init = "xavier"
    np.random.seed(3)
    net = H.M.DIEN_Net(args)
    om = H.oracle_model(net)
    sets = []
    for b in range(2):
        lens = [rng.randint(0, Lmax + 1, size=B).astype(np.int32) for _ in range(T)]
        idx = [rng.randint(0, rows[t], size=int(lens[t].sum())).astype(np.int64) for t in range(T)]
        sets.append((idx, lens))
    net.create(None, sets[0][1], sets[0][0], None)
    eng = net.engine
    try:
        for b, (idx, lens) in enumerate(sets):
            eng.stage_batch(b, None, idx, lens)
        eng.set_option("sls_exact", 1)
        ref = {}
        for b, (idx, lens) in enumerate(sets):
            for bs in (B, 33, 2, 1):
                got = net.run_staged(b, bs)
                assert any("dien_rnn_any_kernel" in d for d in eng.last_dispatch()), eng.last_dispatch()
                R = eng.fetch_interaction(bs)
                exp, R_exp = om.forward(None, idx, lens, bs=bs, want_R=True)
                assert R.shape == (bs, Hs + 3 * D)
                assert np.array_equal(R[:, Hs:], R_exp[:, Hs:]), (b, bs)
                assert H.close(R, R_exp, rtol=2e-5, atol=2e-6), (b, bs, np.abs(R - R_exp).max())
                assert H.close(got, exp, rtol=max(2e-5, H.RTOL_OUT), atol=2e-6), (b, bs, np.abs(got - exp).max())
                ref[(b, bs)] = got
        # (12 queries: the upper half of the kernels' per-query argument tables)
        jobs = [(0, B), (1, 33), (0, 1), (1, B), (0, 33), (1, 2), (0, 2), (1, 1), (0, B), (1, 2), (0, 33), (1, 33)]
        outs = net.run_staged_multi([b for b, _ in jobs], [n for _, n in jobs])
        for (b, bs), o in zip(jobs, outs):
            assert np.array_equal(o, ref[(b, bs)]), (b, bs)
    finally:
        eng.close()


@pytest.mark.parametrize("kind,D,width", [("din", 4096, 3000), ("dien", 64, 5000)])
def test_any_shape_forms_with_more_than_64_kb_of_lds(kind, D, width):
    """The any-shape kernels keep a sample's activations in LDS, up to the CU's 160 KB (drs_create refuses what does not
    fit): a DIN unit 12288 -> 3000 -> 4096 (88 KB) and a DIEN recurrence 64 -> 5000 (78 KB) against the oracle."""
    U = 1 if kind == "din" else 2
    rows = [50] + [40] * U + [60, 30]
    T, B = len(rows), 6
    over = dict(arch_mlp_bot=str(width)) if kind == "din" else dict(hidden_size=width)
    args = H.args_from({}, arch_sparse_feature_size=D, arch_embedding_size="-".join(map(str, rows)),
                       arch_mlp_top="16-2", arch_interaction_op="cat", num_indices_per_lookup=2, num_batches=1,
                       max_mini_batch_size=B, mini_batch_size=B, numpy_rand_seed=3, model_type=kind, accel_slots=1, **over)
    np.random.seed(3)
    net = (H.M.DIN_Net if kind == "din" else H.M.DIEN_Net)(args)
    om = H.oracle_model(net)
    rng = np.random.RandomState(1)
    lens = [np.full(B, 2, dtype=np.int32) for _ in range(T)]
    idx = [rng.randint(0, rows[t], size=2 * B).astype(np.int64) for t in range(T)]
    net.create(None, lens, idx, None)
    eng = net.engine
    try:
        eng.stage_batch(0, None, idx, lens)
        eng.set_option("sls_exact", 1)
        for bs in (B, 1):
            got = net.run_staged(0, bs)
            assert any(("%s_" % kind) in d and "any_kernel" in d for d in eng.last_dispatch()), eng.last_dispatch()
            R = eng.fetch_interaction(bs)
            exp, R_exp = om.forward(None, idx, lens, bs=bs, want_R=True)
            if kind == "din":
                assert np.array_equal(R, R_exp), np.abs(R - R_exp).max()
                assert H.close(got, exp, rtol=1e-6, atol=1e-7)
            else:
                assert np.array_equal(R[:, width:], R_exp[:, width:])
                assert H.close(R, R_exp, rtol=2e-5, atol=2e-6), np.abs(R - R_exp).max()
                assert H.close(got, exp, rtol=H.RTOL_OUT, atol=2e-6)
    finally:
        eng.close()


@pytest.mark.parametrize("kind", ["dlrm_dot", "wnd", "ncf"])
def test_coalesced_queries_equal_individual_queries(kind):
    """drs_forward_multi_async: several queries in one set of launches return exactly the
    bits of the same queries run one by one (rows never mix)."""
    case = {"dlrm_dot": "dlrm_rm1_mini", "wnd": "wnd_mini", "ncf": "ncf_mini"}[kind]
    meta, z = H.load_fixture(case)
    over = dict(arch_interaction_op="dot", arch_mlp_top="128-1") if kind == "dlrm_dot" else {}
    args = H.args_from(meta["args"], num_batches=2 if kind == "dlrm_dot" else 1, accel_slots=2, **over)
    net, lX, lS_l, lS_i, lT = H.materialize(args)
    net.create(lX[0], lS_l[0], lS_i[0], lT[0])
    try:
        net.stage_batches(None if kind == "ncf" else lX, lS_l, lS_i)
        eng = net.engine
        n, nb = len(lS_l[0][0]), len(lS_l)
        for exact in (1, 0):
            eng.set_option("sls_exact", exact)
            jobs = [(0, n), (nb - 1, 1), (0, 0), (nb - 1, n - 3), (0, 5), (nb - 1, n), (0, 2), (0, n)]
            singles = [eng.forward(b, bs) for b, bs in jobs]
            for fuse, split in ((1, 1), (0, 1), (0, 0)):   # launch structure must not change a bit
                eng.set_option("mlp_fuse", fuse)
                eng.set_option("mlp_split", split)
                eng.forward_multi_async(1, [b for b, _ in jobs], [bs for _, bs in jobs])
                got = eng.wait(1, sum(bs for _, bs in jobs))
                # same k-ordered chains whatever the tiling: bit-identical
                assert np.array_equal(got, np.concatenate(singles, axis=0)), (exact, fuse, split)
            eng.set_option("mlp_fuse", 1)
            eng.set_option("mlp_split", 1)
        with pytest.raises(N.DrsError):
            eng.forward_multi_async(0, [0] * 17, [1] * 17)
    finally:
        net.engine.close()


# ------------------------------------------------------------------------------------
# MLP launch structures: weight-tile stream kernel vs per-layer chain kernel vs one launch
# per MLP, single stream vs pipelined gather/MLP streams -- every one the same k-ordered
# fma chains, so the same bits
@pytest.mark.parametrize("op", ["cat", "dot"])
@pytest.mark.parametrize("D,T,bot,top", [
    (8, 3, "20-36-8", "100-200-1"),        # K tails (20, 36, 100), N not a multiple of 16, 2 passes (200)
    (64, 8, "128-64-64", "256-64-1"),      # BASELINE RMC1 widths
    (32, 8, "128-64-32", "256-64-1"),      # reference dlrm_rm1.json widths
    (16, 2, "64-16", "300-4-1"),           # 3 passes, a 4-wide layer, fewer tiles than the prefetch ring
    (4, 1, "4-4", "4-1"),                  # smallest legal widths: 3 tiles in total
    (16, 20, "32-16", "64-1"),             # 21 features: the dot interaction's pairs in three 16 x 16 blocks (226-wide top input)
    (8, 32, "16-8", "96-1"),               # 33 features (RM2's count in dot mode): six blocks
])
def test_mlp_launch_structures_are_bit_identical(D, T, bot, top, op):
    rows, L, B = 5000, 3, 100
    args, net, lX, lS_l, lS_i = _big_case(rows, D, T, L, bot, top, B, nb=2, seed=7, op=op)
    net.create(lX[0], lS_l[0], lS_i[0], None)
    try:
        net.stage_batches(lX, lS_l, lS_i)
        eng = net.engine
        eng.set_option("sls_exact", 1)
        lo, hi = -float(np.sqrt(1 / rows)), float(np.sqrt(1 / rows))
        net.emb_w = [orc.fill_table_uniform(rows, D, t, lo, hi, args.numpy_rand_seed, nthreads=0)
                     for t in range(T)]
        om = H.oracle_model(net)
        jobs = [(0, B), (1, 1), (0, 37), (1, 64), (0, 17)]      # row tails: 100, 1, 37, 17
        exp = np.concatenate([om.forward(lX[b], lS_i[b], lS_l[b], bs=bs, nthreads=0) for b, bs in jobs])
        results = {}
        for name, opts in {
            "stream": dict(mlp_stream=1, mlp_fuse=1, shared_stream=1),
            "chain": dict(mlp_stream=0, mlp_fuse=1, shared_stream=1),
            "stream_packed": dict(mlp_stream=2, mlp_fuse=1, shared_stream=1),       # weights from the packed twins, no LDS staging
            "unfused_stream_packed": dict(mlp_stream=2, mlp_fuse=0, shared_stream=1),
            "pipelined_packed": dict(mlp_stream=2, mlp_fuse=1, shared_stream=2),
            "packed_ring3_2_per_cu": dict(mlp_stream=2, mlp_fuse=1, shared_stream=1, mlp_stream_2cu=1),   # 128 VGPRs: two workgroups per CU
            "stream4": dict(mlp_stream=4, mlp_fuse=1, shared_stream=1),               # 4 waves, one asm statement per (layer, pass)
            "unfused_stream4": dict(mlp_stream=4, mlp_fuse=0, shared_stream=1),
            "stream4_2_per_cu": dict(mlp_stream=4, mlp_fuse=1, shared_stream=1, mlp_stream_2cu=1),
            "stream4_32_rows": dict(mlp_stream=4, mlp_fuse=1, shared_stream=1, mlp_rows32=1),         # 32 rows per workgroup: two halves share the weight operands
            "unfused_stream4_32_rows": dict(mlp_stream=4, mlp_fuse=0, shared_stream=1, mlp_rows32=1),
            "pipelined_stream4_32_rows": dict(mlp_stream=4, mlp_fuse=1, shared_stream=2, mlp_rows32=1),
            "pipelined_stream4": dict(mlp_stream=4, mlp_fuse=1, shared_stream=2),
            # column-split form: the first top layer's columns over 4 / 2 workgroups per slab of rows, the pieces exchanged
            # through L2, the last arriver runs the remaining layers (taken when that layer is 128 ... 1024 wide in 64s)
            "stream4_nsplit4": dict(mlp_stream=4, mlp_fuse=1, shared_stream=1, mlp_nsplit=4, mlp_nsplit_rows=1 << 20),
            "stream4_nsplit2": dict(mlp_stream=4, mlp_fuse=1, shared_stream=1, mlp_nsplit=2, mlp_nsplit_rows=1 << 20),
            "stream4_32_rows_nsplit2": dict(mlp_stream=4, mlp_fuse=1, shared_stream=1, mlp_rows32=1, mlp_nsplit=2, mlp_nsplit_rows=1 << 20),
            "stream4_32_rows_nsplit4": dict(mlp_stream=4, mlp_fuse=1, shared_stream=1, mlp_rows32=1, mlp_nsplit=4, mlp_nsplit_rows=1 << 20),
            "pipelined_stream4_nsplit4": dict(mlp_stream=4, mlp_fuse=1, shared_stream=2, mlp_nsplit=4, mlp_nsplit_rows=1 << 20),
            # early start: the launch runs its prologue and the bottom chain beside the gather and polls the slot's flag
            # before it fetches the pooled rows (Done::wait_flag)
            "early_stream4": dict(mlp_stream=4, mlp_fuse=1, shared_stream=2, mlp_early=1),
            "unfused_stream": dict(mlp_stream=1, mlp_fuse=0, shared_stream=1),
            "unfused_chain": dict(mlp_stream=0, mlp_fuse=0, shared_stream=1),
            "standalone_layers": dict(mlp_stream=1, mlp_fuse=0, shared_stream=1, mlp_wide_kn=1),
            "pipelined": dict(mlp_stream=1, mlp_fuse=1, shared_stream=2),
            "per_slot_streams": dict(mlp_stream=1, mlp_fuse=1, shared_stream=0),
        }.items():
            if not H.runs_here(opts):
                continue                                    # (a lab option: DRS_TEST_LAB=1 runs it)
            for k, v in opts.items():
                eng.set_option(k, v)
            for slot in (0, 1, 2):      # keep several launch sets in flight
                eng.forward_multi_async(slot, [b for b, _ in jobs], [bs for _, bs in jobs])
            outs = [eng.wait(slot, sum(bs for _, bs in jobs)) for slot in (0, 1, 2)]
            assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2]), name
            results[name] = outs[0]
            # (the early start is taken when the set is ONE plain stream4_kernel launch: the RMC1-class widths)
            took_early = "early" in eng.last_dispatch(0)
            assert not took_early or name == "early_stream4", (name, eng.last_dispatch(0))
            if name == "early_stream4" and (D, T, op) == (64, 8, "cat"):
                assert took_early, eng.last_dispatch(0)
            took_split = any("nsplit" in d for d in eng.last_dispatch(0))
            assert took_split == ("nsplit" in name and top.startswith("256-")), (name, eng.last_dispatch(0))
            eng.set_option("mlp_nsplit", 0)
            if H.LAB:
                eng.set_option("mlp_early", 0)
            eng.set_option("mlp_wide_kn", 512 * 1024)
            eng.set_option("mlp_stream_2cu", 0)
            eng.set_option("mlp_rows32", 0)
        for name, got in results.items():
            assert np.array_equal(got, results["stream_packed"]), name
        assert H.close(results["stream_packed"], exp, rtol=1e-6, atol=1e-7)
        # the interaction tensor the top MLP saw (cat layout / dot triangle), default structure
        for k, v in dict(mlp_stream=2, mlp_fuse=1, shared_stream=2).items():
            eng.set_option(k, v)
        eng.forward(1, 37)
        _, R_exp = om.forward(lX[1], lS_i[1], lS_l[1], bs=37, want_R=True, nthreads=0)
        assert np.array_equal(eng.fetch_interaction(37), R_exp)
    finally:
        net.engine.close()


# ------------------------------------------------------------------------------------
# BASELINE.json config 3 at full size (12 tables x 10M rows x 32 = 15.36 GB of tables, batch
# 512, L = 20): no CPU oracle at this size -- size-independent properties instead
def test_rmc3_baseline_size_counting_property():
    """Tables filled with ones: every pooled column must equal the bag length EXACTLY (a sum
    of L ones is exact in any fp32 order), for both gather variants, including bags that
    touch row 0 and the last row of a 10M-row table; and the Caffe2 index ENFORCE must fire
    for row N at that size."""
    T, rows, D, L, B = 12, 10_000_000, 32, 20, 512
    # the REAL config-3 graph (bench.py --workload rmc3): bottom 2560-1024-256-32, top 416-512-256-1
    ln_bot, ln_top = [2560, 1024, 256, 32], [D * (T + 1), 512, 256, 1]
    eng = N.Engine(N.MODEL_DLRM, [rows] * T, D, ln_bot, ln_top, N.INTERACT_CAT,
                   sigmoid_top=3, max_batch=B, max_lookups=L, num_staged_batches=1, num_slots=3)
    try:
        for t in range(T):
            eng.fill_table_uniform(t, 1.0, 1.0, 5)
        rng = np.random.RandomState(3)
        for mlp, ln in ((N.MLP_BOT, ln_bot), (N.MLP_TOP, ln_top)):
            for i in range(len(ln) - 1):
                # (pooled columns are all L = 20 here: the first top layer is scaled down so the sigmoid stays inside (0, 1))
                scale = np.sqrt(2.0 / (ln[i] + ln[i + 1])) * (0.02 if (mlp == N.MLP_TOP and i == 0) else 1.0)
                eng.set_fc(mlp, i, (rng.randn(ln[i + 1], ln[i]) * scale).astype(np.float32),
                           (rng.randn(ln[i + 1]) * np.sqrt(1.0 / ln[i + 1]) * 0.1).astype(np.float32))
        idx = [np.sort(rng.randint(0, rows, size=(B, L)), axis=1).astype(np.int64) for _ in range(T)]
        for t in range(T):
            idx[t][0, 0] = 0
            idx[t][B - 1, L - 1] = rows - 1          # the very last row of the table
        lens = [np.full(B, L, dtype=np.int32) for _ in range(T)]
        dense = rng.rand(B, ln_bot[0]).astype(np.float32)
        eng.stage_batch(0, dense, [i.reshape(-1) for i in idx], lens)
        outs = {}
        for exact in (1, 0):
            eng.set_option("sls_exact", exact)
            for bs in (B, 165, 1):
                out = eng.forward(0, bs)
                R = eng.fetch_interaction(bs)
                assert R.shape == (bs, D * (T + 1))
                assert np.array_equal(R[:, D:], np.full((bs, D * T), float(L), np.float32)), (exact, bs)
                assert np.all(np.isfinite(out)) and np.all((out > 0) & (out < 1))
                outs[(exact, bs)] = out
        # pooled sums identical -> the whole forward identical between the two gather variants
        for bs in (B, 165, 1):
            assert np.array_equal(outs[(1, bs)], outs[(0, bs)])
        # the launch sets bench.py --workload rmc3 times: 16 queries of batch 512 (8 192 rows: 32-row
        # stream4 chains, GEMM launches on the MLP streams), three sets in flight -- every pooled column
        # still counts L exactly and every query's bits are those of the query served alone
        assert eng.get_option("preferred_coalesce") == 16 and eng.get_option("mlp_rows32") == 8192
        sizes = [B, 165, B, 1] * 4
        for rnd in range(2):
            for s_ in range(3):
                eng.forward_multi_async(s_, [0] * 16, sizes)
            got = [eng.wait(s_, sum(sizes)) for s_ in range(3)]
        for s_ in range(3):
            Rv = eng.fetch_interaction(B * 16, slot=s_)
            o = v = 0
            for k, n in enumerate(sizes):
                assert np.array_equal(Rv[v:v + n, D:], np.full((n, D * T), float(L), np.float32)), (s_, k)
                assert np.array_equal(got[s_][o:o + n], outs[(0, n)]), (s_, k)
                o += n
                v += (n + 63) // 64 * 64
        assert eng.gather_bytes(0, B) == B * T * (L * D * 4 + L * 4 + 4 + D * 4)
        bad = [i.copy() for i in idx]
        bad[T - 1][7, 3] = rows                       # one past the end
        with pytest.raises(N.DrsError) as ei:
            eng.forward_inputs(dense, [i.reshape(-1) for i in bad], lens, B)
        assert ei.value.code == N.ERR_INDEX_RANGE
    finally:
        eng.close()


def test_rmc3_baseline_graph_pipelined_sets_match_oracle():
    """BASELINE config 3's REAL graph as `bench.py --workload rmc3 --batch 512` runs it (VERDICT r3 #1b) --
    T = 12 tables x 32, L = 20 (two bags per wave in the flat gather), bottom 2560-1024-256-32 (two GEMM
    launches + a chain), top 416-512-256-1, batch 512, 16 queries per launch set (8 192 rows: the 32-row
    stream4 chains), three sets in flight over the gather stream and the MLP streams -- on 1 M-row tables,
    where the oracle can follow: every query of every set against the oracle's forward on the same
    counter-based table fill (R within the flat-gather tolerance, bottom MLP columns bitwise, outputs
    1e-4), and the sequential-order gather bitwise."""
    rows, D, T, L, B = 1_000_000, 32, 12, 20, 512
    args, net, lX, lS_l, lS_i = _big_case(rows, D, T, L, "2560-1024-256-32", "512-256-1", B, nb=2, seed=31)
    net.create(lX[0], lS_l[0], lS_i[0], None)
    eng = net.engine
    try:
        net.stage_batches(lX, lS_l, lS_i)
        lo, hi = -float(np.sqrt(1 / rows)), float(np.sqrt(1 / rows))
        net.emb_w = [orc.fill_table_uniform(rows, D, t, lo, hi, args.numpy_rand_seed, nthreads=0) for t in range(T)]
        om = H.oracle_model(net)
        assert eng.get_option("preferred_coalesce") == 16 and eng.get_option("mlp_streams") == 3
        assert eng.get_option("mlp_rows32") == 8192 and eng.get_option("shared_stream") == 2
        ref = {(bid, bs): om.forward(lX[bid], lS_i[bid], lS_l[bid], bs=bs, want_R=True, nthreads=0)
               for bid in (0, 1) for bs in (B, 165)}
        sets = [[((s + k) % 2, B if (s + k) % 3 else 165) for k in range(16)] for s in range(3)]
        for exact in (0, 1):
            eng.set_option("sls_exact", exact)
            for rnd in range(2):
                for s in range(3):
                    eng.forward_multi_async(s, [b for b, _ in sets[s]], [n for _, n in sets[s]])
                outs = [eng.wait(s, sum(n for _, n in sets[s])) for s in range(3)]
            for s in range(3):
                Rv = eng.fetch_interaction(B * 16, slot=s)
                o = v = 0
                for k, (bid, n) in enumerate(sets[s]):
                    exp, R_exp = ref[(bid, n)]
                    if exact:
                        assert np.array_equal(Rv[v:v + n], R_exp), (s, k)
                        assert H.close(outs[s][o:o + n], exp, rtol=1e-6, atol=1e-7), (s, k)
                    else:
                        assert np.array_equal(Rv[v:v + n, :D], R_exp[:, :D]), (s, k)    # GEMMs + chain: bitwise
                        assert H.close(Rv[v:v + n], R_exp, rtol=1e-5, atol_scale=2e-6), (s, k)
                        assert H.close(outs[s][o:o + n], exp, rtol=H.RTOL_OUT, atol=1e-7), (s, k)
                    o += n
                    v += (n + 63) // 64 * 64
    finally:
        eng.close()


@pytest.mark.parametrize("unique", [True, False])
def test_gather_on_synthetic_locality_traces_matches_oracle(tmp_path, unique):
    """`--data_generation synthetic` end to end: index streams synthesised from a stack-distance profile
    (data_generator/dlrm_data_caffe2.py:34-60,152-222; the reuse-heavy `hot` profile: lines are re-touched
    within and across bags) staged and gathered -- unique=True: the reference's np.unique bags (ragged:
    ring-walk kernels); unique=False: every bag exactly L lookups with duplicates (the flat kernel, what
    `bench.py --trace` times) -- sequential-order gather bitwise, default gather within its tolerance,
    coalesced sets equal to the queries served alone."""
    from deeprecsys_amd.data_generator.dlrm_data import DLRMDataGenerator
    from deeprecsys_amd.data_generator import trace_generator as TG
    z = np.load(os.path.join(H.GOLDEN, "traces.npz"))
    path = str(tmp_path / "dist_emb_j.log".replace("j", "hot"))
    TG.write_dist_to_file(path, z["hot/list_sd"].tolist(), z["hot/cumm_sd"].tolist())
    rows, D, L, B, nb = [40_000, 60_000, 50_000, 30_000], 64, 80, 96, 2
    a = H.args_from({}, arch_sparse_feature_size=D, arch_embedding_size="-".join(map(str, rows)), arch_mlp_bot="16-32-64",
                    arch_mlp_top="64-1", arch_interaction_op="cat", num_indices_per_lookup=L, num_batches=nb,
                    max_mini_batch_size=B, mini_batch_size=B, numpy_rand_seed=4, model_type="dlrm",
                    data_generation="synthetic", data_trace_file=path, accel_slots=2)
    np.random.seed(4)
    _, lX, lS_l, lS_i = DLRMDataGenerator(a).generate_synthetic_input_data(nb, B, False, L, True, 16, np.array(rows), path,
                                                                           False, unique=unique)
    lS_l = [[np.asarray(l, np.int32) for l in per] for per in lS_l]
    lS_i = [[np.asarray(i, np.int64) for i in per] for per in lS_i]
    net = H.M.DLRM_Net(a)
    om = H.oracle_model(net)
    net.create(lX[0], lS_l[0], lS_i[0], None)
    eng = net.engine
    try:
        net.stage_batches(lX, lS_l, lS_i)
        if unique:
            assert min(int(l.min()) for l in lS_l[0]) < L          # ragged
        ref = {}
        for exact in (1, 0):
            eng.set_option("sls_exact", exact)
            for bid in range(nb):
                for bs in (B, 33):
                    got = net.run_staged(bid, bs)
                    R = eng.fetch_interaction(bs)
                    exp, R_exp = om.forward(lX[bid], lS_i[bid], lS_l[bid], bs=bs, want_R=True, nthreads=0)
                    if exact:
                        assert np.array_equal(R, R_exp), (bid, bs)
                        assert H.close(got, exp, rtol=1e-6, atol=1e-7)
                    else:
                        assert H.close(R, R_exp, rtol=1e-5, atol_scale=2e-6), (bid, bs)
                        assert H.close(got, exp, rtol=H.RTOL_OUT, atol=1e-7)
                    ref[(exact, bid, bs)] = got
            jobs = [(0, B), (1, 33), (1, B), (0, 33)]
            outs = net.run_staged_multi([b for b, _ in jobs], [n for _, n in jobs])
            for (bid, bs), o in zip(jobs, outs):
                assert np.array_equal(o, ref[(exact, bid, bs)]), (exact, bid, bs)
    finally:
        eng.close()


# ------------------------------------------------------------------------------------
# flat gather variant (fixed-length bags: what every shipped reference config generates)
@pytest.mark.parametrize("D,T,L", [(64, 8, 80), (32, 8, 80), (32, 12, 20), (32, 10, 20), (64, 4, 20), (128, 4, 7),
                                   (64, 6, 2), (32, 4, 33), (48, 4, 20), (64, 3, 41), (64, 4, 120), (32, 4, 200)])
def test_flat_gather_variants_match_oracle(D, T, L):
    """Every shape of the flat variant (1 / 2 / 4 bags per wave, 5 / 10 / 20 loads per lane, row
    widths 128 / 256 / 512 B, lengths that leave a ragged last load) against the oracle's
    sequential-order pooling: same rows, different fp32 order -> the wave-split tolerance; single
    query (with prefix sizes) and three coalesced queries at their 64-row aligned virtual offsets."""
    rng = np.random.RandomState(D * 1000 + T * 100 + L)
    rows, B = [3001 + 17 * t for t in range(T)], 160
    eng = N.Engine(N.MODEL_DLRM, rows, D, [8, D], [D * (T + 1), 4, 1], N.INTERACT_CAT, sigmoid_top=2,
                   max_batch=B, max_lookups=L, num_staged_batches=2, num_slots=2)
    try:
        tables = [rng.uniform(-1, 1, (r, D)).astype(np.float32) for r in rows]
        for t in range(T):
            eng.set_table(t, tables[t])
        eng.set_fc(N.MLP_BOT, 0, rng.randn(D, 8).astype(np.float32), rng.randn(D).astype(np.float32))
        eng.set_fc(N.MLP_TOP, 0, rng.randn(4, D * (T + 1)).astype(np.float32) * 0.05, np.zeros(4, np.float32))
        eng.set_fc(N.MLP_TOP, 1, rng.randn(1, 4).astype(np.float32), np.zeros(1, np.float32))
        idx = [[rng.randint(0, rows[t], size=(B, L)).astype(np.int64) for t in range(T)] for _ in range(2)]
        for b in range(2):
            for t in range(T):
                idx[b][t][0, 0], idx[b][t][B - 1, L - 1] = 0, rows[t] - 1      # first and last row of every table
            eng.stage_batch(b, rng.rand(B, 8).astype(np.float32), [i.reshape(-1) for i in idx[b]],
                            [np.full(B, L, np.int32) for _ in range(T)])

        def pooled(b, bs):
            return np.concatenate([orc.sls(tables[t], idx[b][t][:bs].reshape(-1), np.full(bs, L, np.int32))
                                   for t in range(T)], axis=1)
        bpws = [w for w in (0, 1, 2, 4) if w == 0 or T % w == 0]
        for bpw in bpws:
            eng.set_option("sls_bpw", bpw)
            for bs in (B, 1, 65):
                eng.forward(0, bs)
                R = eng.fetch_interaction(bs)[:, D:]
                assert H.close(R, pooled(0, bs), rtol=1e-5, atol_scale=2e-6), (bpw, bs)
            jobs = [(1, 64), (0, 130), (1, 0), (0, 3)]
            eng.forward_multi_async(1, [b for b, _ in jobs], [n for _, n in jobs])
            eng.wait(1, sum(n for _, n in jobs))
            R = eng.fetch_interaction(64 + 192 + 64, slot=1)[:, D:]
            for (b, n), v0 in zip(jobs, (0, 64, 256, 256)):
                assert H.close(R[v0:v0 + n], pooled(b, n), rtol=1e-5, atol_scale=2e-6), (bpw, b, n)
        # the same launches with the flat variant off take the ring-walk kernels: same tolerance,
        # and the sequential-order variant stays bit-exact whatever the flat options say
        eng.set_option("sls_bpw", 0)
        eng.set_option("sls_exact", 1)
        eng.forward(0, B)
        assert np.array_equal(eng.fetch_interaction(B)[:, D:], pooled(0, B))
    finally:
        eng.close()


def test_per_call_inputs_2d_arrays_worker_pool_and_enforces():
    """The run_queues signature (models/dlrm_s_caffe2.py:162-174) at RMC1 size: 2-D id / length
    arrays (row pointers only, strided slices of a bigger set like inferenceEngine.py:200-206)
    give the bits of per-table lists and of the staged path, with 0, 1 or 3 conversion workers;
    the Caffe2 ENFORCEs fire from the worker pool and name the first failing table."""
    T, rows, D, L, B = 8, 100_000, 64, 80, 256
    rng = np.random.RandomState(21)
    eng = N.Engine(N.MODEL_DLRM, [rows] * T, D, [16, D], [D * (T + 1), 8, 1], N.INTERACT_CAT, sigmoid_top=2,
                   max_batch=B, max_lookups=L, num_staged_batches=1, num_slots=3)
    try:
        for t in range(T):
            eng.fill_table_uniform(t, -0.1, 0.1, 3)
        eng.set_fc(N.MLP_BOT, 0, rng.randn(D, 16).astype(np.float32), rng.randn(D).astype(np.float32))
        eng.set_fc(N.MLP_TOP, 0, rng.randn(8, D * (T + 1)).astype(np.float32) * 0.05, np.zeros(8, np.float32))
        eng.set_fc(N.MLP_TOP, 1, rng.randn(1, 8).astype(np.float32), np.zeros(1, np.float32))
        big_ids = rng.randint(0, rows, size=(T, 2 * B * L)).astype(np.int64)      # a bigger pre-generated set
        big_len = np.full((T, 2 * B), L, dtype=np.int32)
        dense = rng.rand(B, 16).astype(np.float32)
        for bs in (B, 165, 1):
            ids, lens = big_ids[:, :bs * L], big_len[:, :bs]                      # strided 2-D slices
            assert not ids.flags["C_CONTIGUOUS"] or bs == 2 * B
            eng.stage_batch(0, dense[:bs], [r.copy() for r in ids], [r.copy() for r in lens])
            ref = eng.forward(0, bs)
            for workers, mode, lt in ((0, 3, 1), (1, 1, 0), (3, 2, 1), (-1, 0, 0), (-1, 3, 1), (-1, 1, 1), (-1, 2, 0)):
                if not H.LAB and (mode == 0 or lt == 1):
                    continue                             # (per-array copies and the launcher thread: lab options)
                eng.set_option("host_threads", workers)
                eng.set_option("zero_copy_inputs", mode)
                if H.LAB:
                    eng.set_option("launch_thread", lt)  # launches on the calling thread (0) or handed to the launcher thread (1)
                assert np.array_equal(eng.forward_inputs(dense[:bs], ids, lens, bs), ref), (bs, workers, mode, lt)
                assert np.array_equal(eng.forward_inputs(dense[:bs], list(ids), list(lens), bs), ref)
            if H.LAB:
                eng.set_option("launch_thread", 1)
            # calls handed to the launcher thread (lab build; the calling thread in the product), mixed with staged submits on the other slots (every
            # other entry point first lets that thread finish)
            for rep in range(20):
                eng.forward_inputs_async(dense[:bs], ids, lens, bs, slot=0)
                eng.forward_async(1, 0, bs)
                eng.forward_inputs_async(dense[:bs], ids, lens, bs, slot=2)
                for s_ in (1, 0, 2):
                    assert np.array_equal(eng.wait(s_, bs), ref), (bs, rep, s_)
            # three calls in flight on three slots
            for s_ in range(3):
                eng.forward_inputs_async(dense[:bs], ids, lens, bs, slot=s_)
            for s_ in range(3):
                assert np.array_equal(eng.wait(s_, bs), ref)
            # "sls_uniform" 0: the kernels read the prefix sums even for fixed-length bags, so every
            # copy mode has to ship them (the one-DMA-copy modes used to skip that upload)
            for mode in ((0, 1, 2, 3) if H.LAB else ()):
                eng.set_option("sls_uniform", 0)
                eng.set_option("zero_copy_inputs", mode)
                for s_ in range(3):
                    eng.forward_inputs_async(dense[:bs], ids, lens, bs, slot=s_)
                for s_ in range(3):
                    assert np.array_equal(eng.wait(s_, bs), ref), (bs, mode, "sls_uniform=0")
                eng.set_option("sls_uniform", 1)
        with pytest.raises(ValueError):          # lengths narrower than bs: a Python error, not a host out-of-bounds read
            eng.forward_inputs(dense, big_ids[:, :B * L], big_len[:, :B - 1], B)
        with pytest.raises(ValueError):          # dense rows of the wrong width
            eng.forward_inputs(dense[:, :8].copy(), big_ids[:, :B * L], big_len[:, :B], B)
        bad = big_ids[:, :B * L].copy()
        bad[5, 17] = rows            # table 5 ...
        bad[2, 9000] = -1            # ... and table 2: the lower table reports, like a sequential pass
        with pytest.raises(N.DrsError) as ei:
            eng.forward_inputs(dense, bad, big_len[:, :B], B)
        assert ei.value.code == N.ERR_INDEX_RANGE and "table 2" in ei.value.detail and "position 9000" in ei.value.detail
        short = big_len[:, :B].copy()
        short[6, 3] = L - 1
        with pytest.raises(N.DrsError) as ei:
            eng.forward_inputs(dense, big_ids[:, :B * L], short, B)
        assert ei.value.code == N.ERR_LENGTHS_SUM and "table 6" in ei.value.detail
    finally:
        eng.close()


def test_per_call_inputs_of_a_whole_launch_set():
    """drs_run_queues_multi_async: the arrays of several waiting requests (inferenceEngine.py:195-215:
    slices of the pre-generated sets) as ONE launch set -- every query's bits are those of the same
    query served alone through the staged path, whatever it is coalesced with (1..16 queries, mixed
    prefix sizes, ragged bags, several sets in flight); the ENFORCEs name the failing query's table
    and nothing is launched then."""
    T, rows, D, L, B = 8, 100_000, 64, 80, 256
    rng = np.random.RandomState(33)
    eng = N.Engine(N.MODEL_DLRM, [rows] * T, D, [16, D], [D * (T + 1), 8, 1], N.INTERACT_CAT, sigmoid_top=2,
                   max_batch=B, max_lookups=L, num_staged_batches=4, num_slots=3)
    try:
        for t in range(T):
            eng.fill_table_uniform(t, -0.1, 0.1, 3)
        eng.set_fc(N.MLP_BOT, 0, rng.randn(D, 16).astype(np.float32), rng.randn(D).astype(np.float32))
        eng.set_fc(N.MLP_TOP, 0, rng.randn(8, D * (T + 1)).astype(np.float32) * 0.05, np.zeros(8, np.float32))
        eng.set_fc(N.MLP_TOP, 1, rng.randn(1, 8).astype(np.float32), np.zeros(1, np.float32))
        nb = 4
        sets = []
        for k in range(nb):
            ids = rng.randint(0, rows, size=(T, B * L)).astype(np.int64)
            lens = np.full((T, B), L, dtype=np.int32)
            dense = rng.rand(B, 16).astype(np.float32)
            eng.stage_batch(k, dense, list(ids), list(lens))
            sets.append((dense, ids, lens))
        alone = {}
        def ref(k, bs):
            if (k, bs) not in alone:
                alone[(k, bs)] = eng.forward(k, bs)
            return alone[(k, bs)]
        def query(k, bs):
            dense, ids, lens = sets[k]
            return (dense[:bs], ids[:, :bs * L], lens[:, :bs], bs)       # strided slices, as the feeder makes them
        for n, sizes in ((1, (B,)), (2, (165, B)), (5, (1, 64, 65, B, 17)), (8, (B,) * 8), (12, (B,) * 12), (16, (B, 200) * 8), (3, (0, 7, 0))):
            qs = [query(i % nb, sizes[i % len(sizes)]) for i in range(n)]
            for workers in (-1, 0):
                eng.set_option("host_threads", workers)
                eng.run_queues_multi_async(qs, slot=0)
                out = eng.wait(0, sum(q[3] for q in qs))
                o = 0
                for i, q in enumerate(qs):
                    assert np.array_equal(out[o:o + q[3]], ref(i % nb, q[3])), (n, i, q[3], workers)
                    o += q[3]
        # three sets in flight, mixed with a staged set and a single per-call query
        eng.set_option("host_threads", -1)
        for rep in range(10):
            qa = [query((rep + i) % nb, B) for i in range(8)]
            qb = [query((rep + i + 1) % nb, 165) for i in range(3)]
            eng.run_queues_multi_async(qa, slot=0)
            eng.forward_multi_async(1, [0, 1], [B, 99])
            eng.run_queues_multi_async(qb, slot=2)
            out = eng.wait(0, 8 * B)
            for i in range(8):
                assert np.array_equal(out[i * B:(i + 1) * B], ref((rep + i) % nb, B)), (rep, i)
            out = eng.wait(1, B + 99)
            assert np.array_equal(out[:B], ref(0, B)) and np.array_equal(out[B:], ref(1, 99))
            out = eng.wait(2, 3 * 165)
            for i in range(3):
                assert np.array_equal(out[i * 165:(i + 1) * 165], ref((rep + i + 1) % nb, 165)), (rep, i)
            d, i_, l_, _ = query(rep % nb, B)
            assert np.array_equal(eng.forward_inputs(d, i_, l_, B, slot=0), ref(rep % nb, B))
        # ragged bags: the prefix sums travel with the set (every table: a permutation of the same lengths)
        base = rng.randint(0, L + 1, size=B).astype(np.int32)
        lens_r = np.stack([rng.permutation(base) for _ in range(T)]).astype(np.int32)
        n_r = int(base.sum())
        ids_r = rng.randint(0, rows, size=(T, n_r)).astype(np.int64)
        eng.stage_batch(3, sets[3][0], list(ids_r), list(lens_r))
        want = eng.forward(3, B)
        eng.run_queues_multi_async([(sets[3][0], ids_r, lens_r, B), query(0, B)], slot=1)
        out = eng.wait(1, 2 * B)
        assert np.array_equal(out[:B], want) and np.array_equal(out[B:], ref(0, B))
        # ENFORCEs: query 1 of the set is bad
        bad = sets[1][1].copy()
        bad[4, 123] = rows
        with pytest.raises(N.DrsError) as ei:
            eng.run_queues_multi_async([query(0, B), (sets[1][0], bad, sets[1][2], B), query(2, B)], slot=0)
        assert ei.value.code == N.ERR_INDEX_RANGE and "table 4" in ei.value.detail
        eng.run_queues_multi_async([query(2, B)], slot=0)                         # the slot is usable afterwards
        assert np.array_equal(eng.wait(0, B), ref(2, B))
        with pytest.raises(ValueError):
            eng.run_queues_multi_async([(sets[0][0], sets[0][1], sets[0][2][:, :10], B)], slot=0)
        with pytest.raises(N.DrsError):
            eng.run_queues_multi_async([query(0, B)] * 17, slot=0)
    finally:
        eng.close()


@pytest.mark.parametrize("case", ["din_mini", "dien_mini", "ncf_mini", "wnd_mini"])
def test_per_call_launch_sets_of_the_other_models(case):
    """The same call on DIN / DIEN / NCF (no dense input) and W&D: a set of per-call queries gives
    the bits of each query served alone from staged inputs."""
    meta, z = H.load_fixture(case)
    args = H.args_from(meta["args"], accel_slots=2)
    net, lX, lS_l, lS_i, lT = H.materialize(args)
    net.create(lX[0], lS_l[0], lS_i[0], lT[0])
    eng = net.engine
    try:
        net.stage_batches(lX if eng.m_den else None, lS_l, lS_i)
        n = len(lS_l[0][0])
        L = int(args.num_indices_per_lookup)
        nb = len(lS_l)
        qs, want = [], []
        for k in range(min(nb, 5)):
            ids2 = np.stack([np.asarray(i, dtype=np.int64) for i in lS_i[k]])
            len2 = np.stack([np.asarray(l, dtype=np.int32) for l in lS_l[k]])
            bs = max(1, n - 3 * k)
            dense = np.asarray(lX[k], dtype=np.float32) if eng.m_den else None
            qs.append((None if dense is None else dense[:bs], ids2[:, :bs * L], len2[:, :bs], bs))
            want.append(net.run_staged(k, bs))
        eng.run_queues_multi_async(qs, slot=1)
        out = eng.wait(1, sum(q[3] for q in qs))
        o = 0
        for q, w in zip(qs, want):
            assert np.array_equal(out[o:o + q[3]], w), (case, q[3])
            o += q[3]
    finally:
        eng.close()


@pytest.mark.parametrize("case", H.MODEL_CASES)
def test_stream4_forms_on_every_model_kind(case):
    """stream4_kernel is an option on every model (the default on some): its one- and two-per-CU
    instantiations, the summed-input one NCF takes and the 32-row form give the bits of the model's
    default launch structure, alone and coalesced."""
    meta, z = H.load_fixture(case)
    args = H.args_from(meta["args"], accel_slots=2)
    net, lX, lS_l, lS_i, lT = H.materialize(args)
    net.create(lX[0], lS_l[0], lS_i[0], lT[0])
    eng = net.engine
    try:
        net.stage_batches(lX if eng.m_den else None, lS_l, lS_i)
        n = len(lS_l[0][0])
        nb = len(lS_l)
        ids, sizes = [k % nb for k in range(5)], [n, 1, max(1, n // 2), n, max(1, n - 1)]
        def run():
            outs = [net.run_staged(0, n).copy()]
            outs += [o.copy() for o in net.run_staged_multi(ids, sizes, slot=1)]
            return outs
        eng.set_option("mlp_stream", 2)
        eng.set_option("mlp_stream_2cu", 0)
        want = run()
        for opts in (dict(mlp_stream=4, mlp_stream_2cu=0), dict(mlp_stream=4, mlp_stream_2cu=1),
                     dict(mlp_stream=4, mlp_stream_2cu=0, mlp_rows32=1), dict(mlp_stream=4, mlp_stream_2cu=1, mlp_rows32=1)):
            for k, v in opts.items():
                eng.set_option(k, v)
            got = run()
            assert all(np.array_equal(a_, b_) for a_, b_ in zip(got, want)), (case, opts)
            eng.set_option("mlp_rows32", 0)
    finally:
        eng.close()


def test_conversion_worker_pool_created_and_destroyed_without_work():
    """A small model's per-call inputs never reach the size at which the conversion is spread over the
    worker pool, so a pool is created (first call) and destroyed ("host_threads", close) without ever
    running a job -- 400 times in a row.  (A worker that got its first time slice only after the
    destructor had signalled used to sleep for ever, and the join with it: round 3.)"""
    meta, z = H.load_fixture("ncf_mini")
    args = H.args_from(meta["args"], accel_slots=2)
    net, lX, lS_l, lS_i, lT = H.materialize(args)
    net.create(lX[0], lS_l[0], lS_i[0], lT[0])
    eng = net.engine
    try:
        net.stage_batches(None, lS_l, lS_i)
        n = len(lS_l[0][0])
        L = int(args.num_indices_per_lookup)
        ids = np.stack([np.asarray(i, dtype=np.int64) for i in lS_i[0]])[:, :n * L]
        lens = np.stack([np.asarray(l, dtype=np.int32) for l in lS_l[0]])[:, :n]
        ref = net.run_staged(0, n)
        for k in range(400):
            eng.set_option("host_threads", 1 + k % 7)          # destroys the pool of the call before
            out = eng.forward_inputs(None, ids, lens, n)       # creates one (no job for it)
            if k % 50 == 0:
                assert np.array_equal(out, ref)
    finally:
        eng.close()


@pytest.mark.parametrize("case", ["din_mini", "dien_mini", "ncf_mini"])
def test_per_call_inputs_of_the_sparse_only_models(case):
    """DIN / DIEN / NCF take no dense input: run_queues' id / length arrays alone, as 2-D arrays or
    per-table lists, read in place from pinned memory or copied (modes 0-3), several calls in
    flight, ragged prefix sizes -- the bits of the staged path."""
    meta, z = H.load_fixture(case)
    args = H.args_from(meta["args"], accel_slots=3)
    net, lX, lS_l, lS_i, lT = H.materialize(args)
    net.create(lX[0], lS_l[0], lS_i[0], lT[0])
    eng = net.engine
    try:
        net.stage_batches(None, lS_l, lS_i)
        n = len(lS_l[0][0])
        L = int(args.num_indices_per_lookup)
        ids2 = np.stack([np.asarray(i, dtype=np.int64) for i in lS_i[0]])
        len2 = np.stack([np.asarray(l, dtype=np.int32) for l in lS_l[0]])
        for bs in sorted({n, max(1, n // 2), 1}):
            ref = net.run_staged(0, bs)
            ids, lens = ids2[:, :bs * L], len2[:, :bs]
            for workers, mode in ((0, 3), (1, 1), (3, 2), (-1, 0 if H.LAB else 3)):
                eng.set_option("host_threads", workers)
                eng.set_option("zero_copy_inputs", mode)
                assert np.array_equal(eng.forward_inputs(None, ids, lens, bs), ref), (case, bs, workers, mode)
                assert np.array_equal(eng.forward_inputs(None, list(ids), list(lens), bs), ref), (case, bs, mode)
            for s_ in range(3):
                eng.forward_inputs_async(None, ids, lens, bs, slot=s_)
            for s_ in range(3):
                assert np.array_equal(eng.wait(s_, bs), ref), (case, bs, s_)
    finally:
        eng.close()


def test_enable_profiling_prints_the_per_operator_type_table(capsys):
    """run(..., enable_prof=True) prints what the reference's benchmark_net prints per operator
    type, in the layout experiments/operator_breakdown/sweep_p.py:21-28 parses."""
    meta, z = H.load_fixture("dlrm_rm1_mini")
    args = H.args_from(meta["args"])
    net, lX, lS_l, lS_i, lT = H.materialize(args)
    net.create(lX[0], lS_l[0], lS_i[0], lT[0])
    try:
        net.run(lX[0], lS_l[0], lS_i[0], enable_prof=True)
        ops = {}
        for line in capsys.readouterr().out.splitlines():
            if "ms." in line:                                   # sweep_p.py's own rule
                ops[line.rstrip().split()[3]] = float(line.rstrip().split()[0])
        assert set(ops) == {"SparseLengthsSum", "FC"} and all(0 < v < 50 for v in ops.values()), ops
        assert H.close(net.fetch_output(), z["expected/prob_click"], rtol=H.RTOL_OUT)
    finally:
        net.engine.close()
    # the sparse-only models (NCF / DIN / DIEN) print the table too
    meta, z = H.load_fixture("ncf_mini")
    net, lX, lS_l, lS_i, lT = H.materialize(H.args_from(meta["args"]))
    net.create(lX[0], lS_l[0], lS_i[0], lT[0])
    try:
        net.run(lX[0], lS_l[0], lS_i[0], enable_prof=True)
        lines = [l for l in capsys.readouterr().out.splitlines() if "ms." in l]
        assert {l.rstrip().split()[3] for l in lines} == {"SparseLengthsSum", "FC"}
    finally:
        net.engine.close()


@pytest.mark.parametrize("D,T,L,bot,top,op", [
    (10, 3, 4, "7-12-10", "9-1", "cat"),          # nothing a multiple of 4: rows of 40 bytes, dense 7, top input 40
    (10, 3, 4, "7-12-10", "9-1", "dot"),          # ... and the dot interaction over 10-wide features
    (6, 5, 1, "13-6", "8-3-1", "dot"),            # one lookup per bag
    (50, 2, 7, "16-50", "32-1", "cat"),           # 200-byte rows
    (300, 2, 3, "20-300", "64-1", "cat"),         # wider than the 256 columns the 16-byte forms serve
])
def test_any_embedding_width_is_served_and_matches_oracle(D, T, L, bot, top, op):
    """The reference only requires m_spa == ln_bot[-1] (models/dlrm_s_caffe2.py:435-437); every shipped config has
    D % 4 == 0, which the fast kernels assume.  Other widths take the generic forms (sls_any_kernel: sequential order;
    chain_kernel / fc_kernel / interact_dot_kernel's scalar paths): pooled sums, interaction tensor bit-exact, outputs
    to 1e-6 against the oracle, staged and per-call inputs, single and coalesced, ragged bags included."""
    rows, B = 997, 70
    args, net, lX, lS_l, lS_i = _big_case(rows, D, T, L, bot, top, B, nb=2, seed=11, op=op)
    net.create(lX[0], lS_l[0], lS_i[0], None)
    try:
        net.stage_batches(lX, lS_l, lS_i)
        eng = net.engine
        lo, hi = -float(np.sqrt(1 / rows)), float(np.sqrt(1 / rows))
        net.emb_w = [orc.fill_table_uniform(rows, D, t, lo, hi, args.numpy_rand_seed, nthreads=0) for t in range(T)]
        om = H.oracle_model(net)
        ref = {}
        for bid in (0, 1):
            for bs in (B, 33, 1):
                got = net.run_staged(bid, bs)
                assert any("sls_any_kernel" in d for d in eng.last_dispatch(0)), eng.last_dispatch(0)
                exp, R_exp = om.forward(lX[bid], lS_i[bid], lS_l[bid], bs=bs, want_R=True, nthreads=0)
                assert np.array_equal(eng.fetch_interaction(bs), R_exp), (bid, bs)
                assert H.close(got, exp, rtol=1e-6, atol=1e-7), (bid, bs)
                ref[(bid, bs)] = got
        jobs = [(0, B), (1, 33), (1, 1), (0, 33)]
        for o, (bid, bs) in zip(net.run_staged_multi([b for b, _ in jobs], [n for _, n in jobs]), jobs):
            assert np.array_equal(o, ref[(bid, bs)]), (bid, bs)
        # per-call inputs with RAGGED bags (prefix sums): every second bag loses its last lookup
        rng = np.random.RandomState(3)
        lens = [np.where(np.arange(B) % 2 == 0, L, max(L - 1, 0)).astype(np.int32) for _ in range(T)]
        ids = [rng.randint(0, rows, size=int(l.sum())).astype(np.int64) for l in lens]
        got = eng.forward_inputs(lX[0], ids, lens, B)
        assert H.close(got, om.forward(lX[0], ids, lens, bs=B, nthreads=0), rtol=1e-6, atol=1e-7)
        with pytest.raises(N.DrsError):                  # Caffe2's ENFORCE still fires from the generic kernel
            bad = [i.copy() for i in ids]
            bad[T - 1][0] = rows
            eng.forward_inputs(lX[0], bad, lens, B)
    finally:
        net.engine.close()


@pytest.mark.parametrize("D", [16, 32, 64, 128])
def test_one_lookup_copy_form_equals_the_sequential_form(D):
    """Fixed bags of ONE row (W&D, MT-WnD, NCF, DIEN) take sls_one_kernel -- 64 samples of one table per wave, the
    lookup as an indexed row copy with 8 rows in flight per lane -- instead of the lane-group-per-bag walk: same bits
    ("sls_one" 0 selects the walk), pooled rows bit-exact against the oracle; query sizes that do not fill a 64-sample
    tile, coalesced sets whose tiles straddle queries, more than 8 queries per set, ragged bags (lengths 0 / 1: the
    walk serves them), -0.0 in a table (0.0f + row, like the sequential sum) and Caffe2's index ENFORCE."""
    rows, T, B = 997, 5, 150
    args, net, lX, lS_l, lS_i = _big_case(rows, D, T, 1, "13-%d" % D, "24-1", B, nb=2, seed=7)
    net.create(lX[0], lS_l[0], lS_i[0], None)
    eng = net.engine
    try:
        net.stage_batches(lX, lS_l, lS_i)
        lo, hi = -float(np.sqrt(1 / rows)), float(np.sqrt(1 / rows))
        net.emb_w = [orc.fill_table_uniform(rows, D, t, lo, hi, args.numpy_rand_seed, nthreads=0) for t in range(T)]
        net.emb_w[1][int(lS_i[0][1][0])] = -0.0            # a row of negative zeros: pooled to +0.0 by either form
        eng.set_table(1, net.emb_w[1])
        om = H.oracle_model(net)
        jobs = [(0, B), (1, 33), (1, 1), (0, 70), (1, B), (0, 64), (1, 65), (0, 2), (0, 33), (1, 129)]
        ref = {}
        for one in (1, 0, 64, 16):                        # 1: 64 samples per wave, 16 for small launches; or forced
            eng.set_option("sls_one", one)
            for bid in (0, 1):
                for bs in (B, 65, 64, 1):
                    got = net.run_staged(bid, bs)
                    assert any("sls_one_kernel" in d for d in eng.last_dispatch()) == bool(one), eng.last_dispatch()
                    R = eng.fetch_interaction(bs)
                    if one == 1:
                        exp, R_exp = om.forward(lX[bid], lS_i[bid], lS_l[bid], bs=bs, want_R=True, nthreads=0)
                        assert np.array_equal(R.view(np.uint32), R_exp.view(np.uint32)), (bid, bs)
                        assert H.close(got, exp, rtol=1e-6, atol=1e-7)
                        ref[(bid, bs)] = (got, R)
                    else:
                        assert np.array_equal(got, ref[(bid, bs)][0]) and np.array_equal(R.view(np.uint32), ref[(bid, bs)][1].view(np.uint32))
            outs = net.run_staged_multi([b for b, _ in jobs], [n for _, n in jobs])
            if one == 1:
                ref["multi"] = outs
                for (bid, bs), o in zip(jobs, outs):
                    if (bid, bs) in ref:
                        assert np.array_equal(o, ref[(bid, bs)][0]), (bid, bs)
            else:
                assert all(np.array_equal(x, y) for x, y in zip(outs, ref["multi"]))
        eng.set_option("sls_one", 1)
        # ragged bags (0 or 1 lookups) read the prefix sums: the walk
        rng = np.random.RandomState(3)
        lens = [(rng.rand(B) < 0.7).astype(np.int32) for _ in range(T)]
        ids = [rng.randint(0, rows, size=int(l.sum())).astype(np.int64) for l in lens]
        got = eng.forward_inputs(lX[0], ids, lens, B)
        assert not any("sls_one_kernel" in d for d in eng.last_dispatch())
        assert H.close(got, om.forward(lX[0], ids, lens, bs=B, nthreads=0), rtol=1e-6, atol=1e-7)
        # fixed one-row bags through the per-call path: the copy form again; an index past the table is Caffe2's ENFORCE
        ones = [np.ones(B, dtype=np.int32) for _ in range(T)]
        ids = [rng.randint(0, rows, size=B).astype(np.int64) for _ in range(T)]
        got = eng.forward_inputs(lX[0], ids, ones, B)
        assert any("sls_one_kernel" in d for d in eng.last_dispatch())
        assert H.close(got, om.forward(lX[0], ids, ones, bs=B, nthreads=0), rtol=1e-6, atol=1e-7)
        with pytest.raises(N.DrsError):
            bad = [i.copy() for i in ids]
            bad[T - 1][B - 1] = rows
            eng.forward_inputs(lX[0], bad, ones, B)
    finally:
        eng.close()


def test_wide_and_deep_with_an_odd_dense_width():
    """W&D's Concat(dense, embeddings) with a dense width that is not a multiple of 4 (the reference takes any
    arch_mlp_bot, models/wide_and_deep.py:271-281): scalar row copy + the scalar FC paths."""
    rows, T, D, B = 500, 3, 12, 40
    args = H.args_from({}, arch_sparse_feature_size=D, arch_embedding_size="-".join([str(rows)] * T), arch_mlp_bot="13",
                       arch_mlp_top="20-6-1", arch_interaction_op="cat", num_indices_per_lookup=1, num_batches=2,
                       max_mini_batch_size=B, mini_batch_size=B, numpy_rand_seed=5, model_type="wnd", accel_slots=3)
    net, lX, lS_l, lS_i, lT = H.materialize(args)
    net.create(lX[0], lS_l[0], lS_i[0], None)
    try:
        net.stage_batches(lX, lS_l, lS_i)
        om = H.oracle_model(net)
        for bid in (0, 1):
            for bs in (B, 17, 1):
                n = min(bs, len(lS_l[bid][0]))
                got = net.run_staged(bid, n)
                assert H.close(got, om.forward(lX[bid], lS_i[bid], lS_l[bid], bs=n, nthreads=0), rtol=1e-6, atol=1e-7), (bid, bs)
    finally:
        net.engine.close()


def test_create_rejects_what_the_int32_offsets_cannot_hold():
    """Prefix sums and bag * length products are int32 on the device: a staging capacity at
    2^31 / 8 coalesced queries is refused at drs_create, not left to overflow."""
    with pytest.raises(N.DrsError) as e:
        N.Engine(N.MODEL_DLRM, [16, 16], 8, [4, 8], [24, 4, 1], N.INTERACT_CAT, sigmoid_top=2,
                 max_batch=1 << 16, max_lookups=1 << 12, num_staged_batches=0, num_slots=1)
    assert e.value.code == N.ERR_UNSUPPORTED


@pytest.mark.parametrize("D,L", [(128, 20), (128, 3), (256, 5)])
def test_table_beyond_2_pow_32_floats(D, L):
    """Row offsets travel as 32-bit counts of 16-byte units (round 4): a table of rows*D in [2^32, 2^33)
    floats (17 GB here) gathers the right rows -- bags made of the LAST rows of the table (whose float offsets
    do not fit 32 bits), the first ones and random ones, pooled sums against the fill function the oracle
    shares with the device-side table init (orc_fill_value), in the sequential form (bitwise: the oracle's
    summation order) and the default one (flat kernel for D = 128, ring walk for D = 256)."""
    rows = (1 << 32) // D + 4096
    assert (1 << 32) <= rows * D < (1 << 33)
    B = 8
    args, net, lX, lS_l, lS_i = _big_case(rows, D, 1, L, "16-%d" % D, "8-1", B, nb=1, seed=5)
    idx = lS_i[0][0].reshape(B, L)
    idx[0] = np.arange(rows - L, rows)                 # the table's last rows
    idx[1] = np.arange(L)                              # its first
    idx[2] = np.sort(np.concatenate([[0], np.arange(rows - L + 1, rows)]))[:L] if L > 1 else idx[2]
    idx[3] = (1 << 32) // D + np.arange(L) - L // 2    # around the old limit
    lS_i[0][0] = idx.reshape(-1)
    net.create(lX[0], lS_l[0], lS_i[0], None)
    try:
        net.stage_batches(lX, lS_l, lS_i)
        lo, hi = -float(np.sqrt(1 / rows)), float(np.sqrt(1 / rows))
        seed = args.numpy_rand_seed
        L_ = orc.lib()
        def row(r):
            return np.array([L_.orc_fill_value(seed, 0, int(r) * D + c, lo, hi) for c in range(D)], dtype=np.float32)
        exp = np.zeros((B, D), dtype=np.float32)
        for b in range(B):
            acc = np.zeros(D, dtype=np.float32)
            for r in idx[b]:
                acc = (acc + row(r)).astype(np.float32)      # sequential fp32 sum, the perfkernel's order
            exp[b] = acc
        for exact in (1, 0):
            net.engine.set_option("sls_exact", exact)
            net.run_staged(0, B)
            R = net.engine.fetch_interaction(B)
            pooled = R[:, D:2 * D]                           # cat: [dense_out | table 0]
            if exact:
                assert np.array_equal(pooled, exp)
            else:
                assert H.close(pooled, exp, rtol=1e-5, atol_scale=2e-6)
    finally:
        net.engine.close()


def test_options_are_per_handle_and_engines_coexist():
    """Two engines in one process (the mixed-model accelerator engine does this) keep their own
    tunables: setting an option on one must not leak into the other,
    and both keep producing their own results while interleaved."""
    rng = np.random.RandomState(11)

    def make(D, T, L):
        rows = [500 + t for t in range(T)]
        e = N.Engine(N.MODEL_DLRM, rows, D, [8, D], [D * (T + 1), 1024, 1], N.INTERACT_CAT, sigmoid_top=2,
                     max_batch=64, max_lookups=L, num_staged_batches=1, num_slots=2)
        for t in range(T):
            e.set_table(t, rng.uniform(-1, 1, (rows[t], D)).astype(np.float32))
        e.set_fc(N.MLP_BOT, 0, rng.randn(D, 8).astype(np.float32), rng.randn(D).astype(np.float32))
        e.set_fc(N.MLP_TOP, 0, rng.randn(1024, D * (T + 1)).astype(np.float32) * 0.05, np.zeros(1024, np.float32))
        e.set_fc(N.MLP_TOP, 1, rng.randn(1, 1024).astype(np.float32) * 0.05, np.zeros(1, np.float32))
        e.stage_batch(0, rng.rand(64, 8).astype(np.float32),
                      [rng.randint(0, rows[t], size=64 * L).astype(np.int64) for t in range(T)],
                      [np.full(64, L, np.int32) for _ in range(T)])
        return e
    a, b = make(64, 8, 20), make(32, 4, 20)
    try:
        defaults = {k: a.get_option(k) for k in ("sls_exact", "sls_flat", "sls_bpw", "sls_nt", "mlp_stream", "mlp_gemm_tile") +
                    (("mlp_gemm", "mlp_kc", "mlp_preload") if H.LAB else ())}
        assert defaults == {k: b.get_option(k) for k in defaults}
        ref_a, ref_b = a.forward(0, 64), b.forward(0, 64)
        changed = {"sls_exact": 1, "sls_flat": 0, "sls_bpw": 2, "sls_nt": 0, "mlp_stream": 0 if H.LAB else 2, "mlp_gemm_tile": 11}
        if H.LAB:
            changed.update({"mlp_gemm": 0, "mlp_kc": 64, "mlp_preload": 1})
        for k, v in changed.items():
            a.set_option(k, v)
        assert {k: a.get_option(k) for k in changed} == changed
        assert {k: b.get_option(k) for k in defaults} == defaults          # nothing leaked
        # engine b still runs exactly what it ran before (flat gather, stream kernel, gemm kernel)
        assert np.array_equal(b.forward(0, 64), ref_b)
        # engine a: other kernels, same model -> MLP bits identical by contract, pooling within tolerance
        assert H.close(a.forward(0, 64), ref_a, rtol=H.RTOL_OUT)
        a.forward_async(0, 0, 64)
        b.forward_async(1, 0, 33)
        assert np.array_equal(b.wait(1, 33), ref_b[:33])
        with pytest.raises(N.DrsError):                                    # wait() checks the buffer against the slot
            a.wait(0, 63)
        a.wait(0, 64)
    finally:
        a.close()
        b.close()


# ------------------------------------------------------------------------------------
# race hunt: random launch sets on random slots, pipelined streams, every result bit-identical
# to the same query served alone on an idle engine (tools/stress.py)
@pytest.mark.parametrize("extra", [[], ["--workload", "rmc1_dot"], ["--workload", "ncf", "--batch", "64"],
                                   ["--set", "shared_stream=0"],
                                   # MLP-bound models: one MLP stream per slot, GEMM + chain launches of
                                   # consecutive sets overlap each other
                                   ["--workload", "rmc3_ref", "--batch", "128"], ["--workload", "wnd", "--batch", "128"],
                                   ["--set", "sls_exact=1"],
                                   # small sets start their MLP launch beside the gather (flag poll inside the kernel; lab build)
                                   pytest.param(["--set", "mlp_early=1"], marks=pytest.mark.skipif(not H.LAB, reason="lab option")),
                                   # the LDS-staged form of the stream kernel (the default reads packed twins; lab build)
                                   pytest.param(["--set", "mlp_stream=1"], marks=pytest.mark.skipif(not H.LAB, reason="lab option")),
                                   # DIN: the fused gather + attention launch, 1..8 queries per set (its
                                   # samples-per-workgroup shape changes with the set size, its bits must not)
                                   ["--workload", "din", "--batch", "96"], ["--workload", "dien", "--batch", "64"]])
def test_pipelined_engine_race_hunt(extra):
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "stress.py"), "--seconds", "20"] + extra,
                       capture_output=True, text=True, timeout=400, cwd=root)
    assert r.returncode == 0 and "stress OK" in r.stdout, r.stdout[-500:] + r.stderr[-500:]


# ------------------------------------------------------------------------------------
def test_dispatch_table_of_the_bench_workloads():
    """Which kernel serves which shape: for the eleven bench workloads, a single query, a 4-query set
    and the engine's preferred launch set take exactly the kernel forms DESIGN.md's dispatch table lists
    (tests/golden/dispatch.json, written by tools/dispatch_table.py from drs_last_dispatch; grids left out -- they
    follow from the row count).  Table SIZES do not enter the dispatch: the scalar-row workloads run with small tables."""
    import json
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tools"))
    import dispatch_table as DT
    with open(os.path.join(H.GOLDEN, "dispatch.json")) as f:
        want = json.load(f)
    assert sorted(want) == sorted(DT.WORKLOADS)
    got = DT.table(DT.WORKLOADS, small_rows=True)
    for w in DT.WORKLOADS:
        assert got[w]["preferred_coalesce"] == want[w]["preferred_coalesce"] and got[w]["mlp_streams"] == want[w]["mlp_streams"], w
        for name, r in want[w]["sets"].items():
            assert got[w]["sets"][name]["forms"] == r["forms"], (w, name, got[w]["sets"][name]["forms"], r["forms"])
            streams = lambda t: t[t.index("gather on"):]
            assert streams(got[w]["sets"][name]["set"]) == streams(r["set"]), (w, name)
