"""Model objects of the hot path: host-side mirrors of the reference's graph builders.

    DLRM_Net / DLRM_Wrapper               <- models/dlrm_s_caffe2.py:79-569
    Wide_and_Deep / Wide_and_Deep_Wrapper <- models/wide_and_deep.py:165-477
    NCF / NCF_Wrapper                     <- models/ncf.py:140-523
    MT_Wide_and_Deep / ..._Wrapper        <- models/multi_task_wnd.py:160-420
    DIN_Net / DIN_Wrapper                 <- models/din.py:24-470
    DIEN_Net / DIEN_Wrapper               <- models/dien.py:28-560

Same constructor arguments, the same shape algebra and sys.exit() checks, the same
numpy RNG consumption order for the weights (embeddings, then bottom MLP, then top
MLP: models/dlrm_s_caffe2.py:245-249,297-299,367-386), the same
create()/run()/run_queues() calls.  Where the reference emits Caffe2 operators into
a net, these classes fill a drs_model_cfg and hand the weights to libdrs_hip.so
(include/drs.h); the forward itself is the HIP kernels -- there is no Python or CPU
implementation of the arithmetic in this package.

Differences that are deliberate:
  * run_queues() executes the query synchronously (the reference enqueues blobs for
    a second thread blocked in RunNet; HIP stream order replaces the BlobsQueues);
  * fetch_output() replaces workspace.FetchBlob("prob_click");
  * stage_batches()/run_staged() keep all `num_batches` input sets resident in HBM
    (the reference keeps lX/lS_l/lS_i in process memory, inferenceEngine.py:83) so a
    request is served from (batch_id, batch_size) alone.
"""
import sys
import time

import numpy as np

from . import _native as N


def _ints(s):
    return np.array([int(x) for x in str(s).split("-")], dtype=int)


_TABLE_DTYPES = {"fp32": N.TABLE_FP32, "fp16": N.TABLE_FP16, "bf16": N.TABLE_BF16, "int8_rowwise": N.TABLE_INT8_ROWWISE,
                 "int4_rowwise": N.TABLE_INT4_ROWWISE, "fp8_e4m3": N.TABLE_FP8_E4M3}


def _table_dtype(args):
    """--accel_table_dtype -> the engine's "table_dtype" value (fp32 when the flag is absent)."""
    name = str(getattr(args, "accel_table_dtype", "fp32") or "fp32")
    if name not in _TABLE_DTYPES:
        raise ValueError("--accel_table_dtype %r: one of %s" % (name, ", ".join(_TABLE_DTYPES)))
    return _TABLE_DTYPES[name]


_MLP_DTYPES = {"fp32": N.MLP_FP32, "bf16": N.MLP_BF16}


def _mlp_dtype(args):
    """--accel_mlp_dtype -> the engine's "mlp_dtype" value (fp32 when the flag is absent)."""
    name = str(getattr(args, "accel_mlp_dtype", "fp32") or "fp32")
    if name not in _MLP_DTYPES:
        raise ValueError("--accel_mlp_dtype %r: one of %s" % (name, ", ".join(_MLP_DTYPES)))
    return _MLP_DTYPES[name]


def _mlp_bf16_fuse(args):
    """--accel_mlp_bf16_fuse -> the engine's "mlp_bf16_fuse" value (0 when the flag is absent)."""
    v = int(getattr(args, "accel_mlp_bf16_fuse", 0) or 0)
    if v not in (0, 1):
        raise ValueError("--accel_mlp_bf16_fuse %r: 0 or 1" % (v,))
    return v


def _table_int8_lines(args):
    """--accel_table_int8_lines -> the engine's "table_int8_lines" value (0 when the flag is absent)."""
    v = int(getattr(args, "accel_table_int8_lines", 0) or 0)
    if v not in (0, 1):
        raise ValueError("--accel_table_int8_lines %r: 0 or 1" % (v,))
    return v


def _table_int4_lines(args):
    """--accel_table_int4_lines -> the engine's "table_int4_lines" value (0 when the flag is absent)."""
    v = int(getattr(args, "accel_table_int4_lines", 0) or 0)
    if v not in (0, 1):
        raise ValueError("--accel_table_int4_lines %r: 0 or 1" % (v,))
    return v


_SLS_POOLS = {"sum": N.POOL_SUM, "mean": N.POOL_MEAN}


def _sls_pool(args):
    """--accel_sls_pool -> the engine's "sls_pool" value (sum when the flag is absent)."""
    name = str(getattr(args, "accel_sls_pool", "sum") or "sum")
    if name not in _SLS_POOLS:
        raise ValueError("--accel_sls_pool %r: one of %s" % (name, ", ".join(_SLS_POOLS)))
    return _SLS_POOLS[name]


def _sls_weighted_flat(args):
    """--accel_sls_weighted_flat -> the engine's "sls_weighted_flat" value (0 when the flag is absent)."""
    v = int(getattr(args, "accel_sls_weighted_flat", 0) or 0)
    if v not in (0, 1):
        raise ValueError("--accel_sls_weighted_flat %r: 0 or 1" % (v,))
    return v


_SLS_WEIGHTS = ("none", "uniform")


def sls_weights(args, lS_i):
    """--accel_sls_weights -> per-index weights of the generated input sets, or None ("none", and when the flag is absent).
    "uniform": one fp32 weight in [0, 1) per index (k / 2^24, so never 1.0), drawn from a RandomState of its own seeded
    with numpy_rand_seed: the global stream -- indices, dense inputs, tables -- is what it is without the flag."""
    name = str(getattr(args, "accel_sls_weights", "none") or "none")
    if name not in _SLS_WEIGHTS:
        raise ValueError("--accel_sls_weights %r: one of %s" % (name, ", ".join(_SLS_WEIGHTS)))
    if name == "none":
        return None
    rs = np.random.RandomState(int(getattr(args, "numpy_rand_seed", 0)))
    return [[(rs.randint(0, 1 << 24, size=len(i)) * np.float32(2.0 ** -24)).astype(np.float32) for i in per] for per in lS_i]


def device_request(request, T, m_den, device, i=0):
    """One request of run_queued_device_multi -- (ids, lengths, fc, batch_size[, fixed_len]), torch tensors on GPU `device`
    -- as the tuple Engine.run_queues_device_multi_async takes.  Checks everything the tensors themselves show (dtype,
    shape, layout, then the device) and raises ValueError naming the argument; touches no engine.  m_den == 0: fc is
    ignored, as the models without dense input ignore it."""
    import torch
    if len(request) not in (4, 5):
        raise ValueError("request %d: (ids, lengths, fc, batch_size[, fixed_len])" % i)
    ids, lengths, fc, bs = request[:4]
    fixed_len = int(request[4]) if len(request) == 5 else -1
    bs = int(bs)
    if m_den == 0:
        fc = None

    def check(name, t, dtype, rows, cols):
        if not isinstance(t, torch.Tensor):
            raise ValueError("request %d: %s must be a torch tensor, got %s" % (i, name, type(t).__name__))
        if t.dtype != dtype:
            raise ValueError("request %d: %s must be %s, got %s" % (i, name, dtype, t.dtype))
        if t.dim() != 2 or (rows is not None and t.shape[0] != rows) or (cols is not None and t.shape[1] != cols):
            raise ValueError("request %d: %s must be [%s, %s], got %r" % (i, name, "bs" if rows is None else rows,
                                                                           "n" if cols is None else cols, tuple(t.shape)))
        if t.shape[1] > 1 and t.stride(1) != 1:
            raise ValueError("request %d: the last dimension of %s must be contiguous (stride %d)" % (i, name, t.stride(1)))
        if t.shape[0] > 1 and t.stride(0) < 0:
            raise ValueError("request %d: %s has a negative row stride" % (i, name))

    if bs < 0:
        raise ValueError("request %d: batch_size %d" % (i, bs))
    check("ids", ids, torch.int64, T, None)
    check("lengths", lengths, torch.int32, T, bs)
    if fc is not None:
        check("fc", fc, torch.float32, bs, m_den)
        if bs > 1 and fc.stride(0) != m_den:
            raise ValueError("request %d: the rows of fc must be contiguous (row stride %d, width %d)" % (i, fc.stride(0), m_den))
    for name, t in (("ids", ids), ("lengths", lengths), ("fc", fc)):
        if t is not None and (t.device.type != "cuda" or t.device.index != device):
            raise ValueError("request %d: %s lives on %s, the engine on cuda:%d" % (i, name, t.device, device))
    return (bs, 0 if fc is None else fc.data_ptr(), ids.data_ptr(), ids.stride(0) if T > 1 else ids.shape[1], ids.shape[1],
            lengths.data_ptr(), lengths.stride(0) if T > 1 else bs, fixed_len)


def device_weights(w, T, n, device, i=0):
    """The per-sample weights of one request of run_queued_device_multi -- a torch tensor [T, n] of float32, float16 or
    bfloat16 on GPU `device`, one weight per index of ids, last dimension contiguous, rows any non-negative stride apart (a
    column slice of a wider tensor goes down as it is) -- as the (ptr, row_stride, dtype) entry
    Engine.run_queues_device_multi_async takes; None stays None (the request is unweighted).  Checks what the tensor itself
    shows (dtype, shape, layout, then the device) and raises ValueError naming the argument; touches no engine."""
    import torch
    if w is None:
        return None
    if not isinstance(w, torch.Tensor):
        raise ValueError("request %d: weights must be a torch tensor or None, got %s" % (i, type(w).__name__))
    codes = {torch.float32: N.WEIGHT_FP32, torch.float16: N.WEIGHT_FP16, torch.bfloat16: N.WEIGHT_BF16}
    if w.dtype not in codes:
        raise ValueError("request %d: weights must be torch.float32, torch.float16 or torch.bfloat16, got %s" % (i, w.dtype))
    if w.dim() != 2 or w.shape[0] != T or w.shape[1] != n:
        raise ValueError("request %d: weights must be [%d, %d] (one per index of ids), got %r" % (i, T, n, tuple(w.shape)))
    if w.shape[1] > 1 and w.stride(1) != 1:
        raise ValueError("request %d: the last dimension of weights must be contiguous (stride %d)" % (i, w.stride(1)))
    if w.shape[0] > 1 and w.stride(0) < 0:
        raise ValueError("request %d: weights has a negative row stride" % i)
    if w.device.type != "cuda" or w.device.index != device:
        raise ValueError("request %d: weights lives on %s, the engine on cuda:%d" % (i, w.device, device))
    return (w.data_ptr(), w.stride(0) if T > 1 else n, codes[w.dtype])


def device_out(t, bs, n_out, device, i=0):
    """One output of run_queued_device_io_multi -- a torch fp32 tensor [bs, n_out] on GPU `device`, last dimension contiguous,
    rows any non-negative stride apart (a column block of a wider tensor goes down as it is) -- as the (ptr, row_stride)
    Engine.run_queues_device_io_multi_async takes.  Checks what the tensor itself shows (dtype, shape, layout, then the
    device) and raises ValueError naming the argument; touches no engine."""
    import torch
    if not isinstance(t, torch.Tensor):
        raise ValueError("out %d: must be a torch tensor, got %s" % (i, type(t).__name__))
    if t.dtype != torch.float32:
        raise ValueError("out %d: must be %s, got %s" % (i, torch.float32, t.dtype))
    if t.dim() != 2 or t.shape[0] != bs or t.shape[1] != n_out:
        raise ValueError("out %d: must be [%d, %d], got %r" % (i, bs, n_out, tuple(t.shape)))
    if t.shape[1] > 1 and t.stride(1) != 1:
        raise ValueError("out %d: the last dimension must be contiguous (stride %d)" % (i, t.stride(1)))
    if t.shape[0] > 1 and t.stride(0) < 0:
        raise ValueError("out %d: a negative row stride" % i)
    if t.device.type != "cuda" or t.device.index != device:
        raise ValueError("out %d: lives on %s, the engine on cuda:%d" % (i, t.device, device))
    return (t.data_ptr() if bs > 0 else 0, t.stride(0) if bs > 1 else n_out)


def device_top(pair, k, n_out, device, i=0):
    """One output of run_queued_device_topk_multi -- (idx, scores): torch tensors on GPU `device`, idx int32 [k] and scores
    float32 [k, n_out], both contiguous -- as the (idx_ptr, scores_ptr) Engine.run_queues_device_topk_multi_async takes.
    Checks what the tensors themselves show (dtype, shape, layout, then the device) and raises ValueError naming the
    argument; touches no engine."""
    import torch
    if not isinstance(pair, (tuple, list)) or len(pair) != 2:
        raise ValueError("out %d: must be a pair (idx, scores)" % i)
    for name, t, dtype, shape in (("idx", pair[0], torch.int32, (k,)), ("scores", pair[1], torch.float32, (k, n_out))):
        if not isinstance(t, torch.Tensor):
            raise ValueError("out %d: %s must be a torch tensor, got %s" % (i, name, type(t).__name__))
        if t.dtype != dtype:
            raise ValueError("out %d: %s must be %s, got %s" % (i, name, dtype, t.dtype))
        if tuple(t.shape) != shape:
            raise ValueError("out %d: %s must be %s, got %r" % (i, name, list(shape), tuple(t.shape)))
        if not t.is_contiguous():
            raise ValueError("out %d: %s must be contiguous (strides %r)" % (i, name, tuple(t.stride())))
    for name, t in (("idx", pair[0]), ("scores", pair[1])):
        if t.device.type != "cuda" or t.device.index != device:
            raise ValueError("out %d: %s lives on %s, the engine on cuda:%d" % (i, name, t.device, device))
    return (pair[0].data_ptr() if k > 0 else 0, pair[1].data_ptr() if k > 0 else 0)


def on_device(x, device):
    """is x a torch tensor on GPU `device`?  (what sends update_embedding_rows / embedding_rows down the device route; a
    module that never imported torch holds no such tensor)"""
    torch = sys.modules.get("torch")
    return torch is not None and isinstance(x, torch.Tensor) and x.device.type == "cuda" and x.device.index == device


def device_row_ids(ids, device):
    """The ids of a device row update or read-back -- a torch int64 tensor [n], contiguous, on GPU `device` -- as the (ptr, n)
    Engine.update_rows_device takes.  Checks what the tensor itself shows and raises ValueError naming the rule; touches no
    engine."""
    import torch
    if not isinstance(ids, torch.Tensor):
        raise ValueError("ids: must be a torch tensor, got %s" % type(ids).__name__)
    if ids.dtype != torch.int64:
        raise ValueError("ids: must be torch.int64, got %s" % ids.dtype)
    if ids.dim() != 1:
        raise ValueError("ids: must be [n], got %r" % (tuple(ids.shape),))
    if not ids.is_contiguous():
        raise ValueError("ids: must be contiguous (stride %d)" % ids.stride(0))
    if ids.shape[0] > N.DEVICE_ROWS_MAX:
        raise ValueError("ids: %d rows, one call names at most %d" % (ids.shape[0], N.DEVICE_ROWS_MAX))
    if ids.device.type != "cuda" or ids.device.index != device:
        raise ValueError("ids: lives on %s, the engine on cuda:%d" % (ids.device, device))
    return ids.data_ptr(), int(ids.shape[0])


def device_row_values(v, n, D, device, name="values", dtypes=None):
    """The rows of a device row update -- a torch tensor [n, D] of float32, float16 or bfloat16 on GPU `device`, last
    dimension contiguous, rows at least D elements apart (a column block of a wider tensor goes down as it is) -- as the
    (ptr, row_stride, dtype code) Engine.update_rows_device takes; with dtypes=(torch.float32,) the output of a read-back.
    Checks what the tensor itself shows (dtype, shape, layout, then the device) and raises ValueError naming the rule;
    touches no engine."""
    import torch
    codes = {torch.float32: N.TABLE_FP32, torch.float16: N.TABLE_FP16, torch.bfloat16: N.TABLE_BF16}
    allowed = tuple(codes) if dtypes is None else tuple(dtypes)
    if not isinstance(v, torch.Tensor):
        raise ValueError("%s: must be a torch tensor, got %s" % (name, type(v).__name__))
    if v.dtype not in allowed:
        raise ValueError("%s: must be %s, got %s" % (name, " or ".join(str(d) for d in allowed), v.dtype))
    if v.dim() != 2 or v.shape[0] != n or v.shape[1] != D:
        raise ValueError("%s: must be [%d, %d], got %r" % (name, n, D, tuple(v.shape)))
    if D > 1 and v.stride(1) != 1:
        raise ValueError("%s: the last dimension must be contiguous (stride %d)" % (name, v.stride(1)))
    if n > 1 and v.stride(0) < D:
        raise ValueError("%s: a row stride of %d, below the row width %d (the rows would overlap)" % (name, v.stride(0), D))
    if v.device.type != "cuda" or v.device.index != device:
        raise ValueError("%s: lives on %s, the engine on cuda:%d" % (name, v.device, device))
    return v.data_ptr(), (v.stride(0) if n > 1 else D), codes[v.dtype]


def _stream_handle(stream):
    """None stays None (`ordered` 0); a torch.cuda.Stream or a raw handle becomes the handle (`ordered` 1)"""
    if stream is None:
        return None
    return stream.cuda_stream if hasattr(stream, "cuda_stream") else int(stream)


def _init_table(n, m):
    # models/dlrm_s_caffe2.py:297-299
    return np.random.uniform(low=-np.sqrt(1 / n), high=np.sqrt(1 / n), size=(n, m)).astype(np.float32)


def _init_mlp(ln):
    # models/dlrm_s_caffe2.py:240-249: W ~ N(0, sqrt(2/(m+n))) [m, n]; b ~ N(0, sqrt(1/m)) [m]
    layers = []
    for i in range(1, ln.size):
        n, m = int(ln[i - 1]), int(ln[i])
        W = np.random.normal(0.0, np.sqrt(2 / (m + n)), size=(m, n)).astype(np.float32)
        b = np.random.normal(0.0, np.sqrt(1 / m), size=m).astype(np.float32)
        layers.append((W, b))
    return layers


class _HipNet(object):
    """State shared by the three model mirrors: weights on the host until create(),
    then one Engine (one GPU)."""

    kind = None

    def _common_init(self, cli_args):
        self.args = cli_args
        self.accel_en = getattr(cli_args, "use_accel", False)
        self.engine = None
        self._out = None
        self._device = int(getattr(cli_args, "_drs_device", 0))
        self._table_init = getattr(cli_args, "accel_table_init", "numpy")
        self.tout = "prob_click"

    # -- weights ------------------------------------------------------------------
    def _make_tables(self, m, ln_emb):
        if self._table_init == "device":
            return [None] * ln_emb.size        # filled on the GPU in create()
        return [_init_table(int(n), m) for n in ln_emb]

    # -- device -------------------------------------------------------------------
    def _num_slots(self):
        """--accel_slots n launch sets in flight; 0 (default): what the engine asks for (drs_get_option
        "preferred_slots": 3 -- gather | MLP | enqueue -- for the gather-bound models, 6 for the MLP-bound ones, whose
        sets are chains of MFMA-bound launches that overlap each other; 4 for DIEN, MT-WnD and W&D, two sets at a time).  The engine decides the class from the model's
        shapes at creation: this is the first guess, _build_engine re-creates the (still empty) engine when it differs."""
        req = int(getattr(self.args, "accel_slots", 0) or 0)
        return req if req > 0 else (3 if self.kind in (N.MODEL_DLRM, N.MODEL_DIN) else 4 if self.kind in (N.MODEL_DIEN, N.MODEL_MTWND, N.MODEL_WND) else 6)

    def _build_engine(self, ln_bot_cfg, ln_top_cfg, interaction_op, itself, sigmoid_top, ln_task=None, num_tasks=0):
        a = self.args
        n_stage = max(int(getattr(a, "num_batches", 0)), 1)
        max_batch = max(int(getattr(a, "max_mini_batch_size", 1)), int(getattr(a, "mini_batch_size", 1)), 1)
        dtype = _table_dtype(a)
        mlp_dtype = _mlp_dtype(a)
        bf16_fuse = _mlp_bf16_fuse(a)
        int8_lines = _table_int8_lines(a)
        int4_lines = _table_int4_lines(a)
        pool = _sls_pool(a)
        weighted_flat = _sls_weighted_flat(a)
        def make(n_slots):
            eng = N.Engine(self.kind, self.ln_emb, self.m_spa, ln_bot_cfg, ln_top_cfg,
                           interaction_op=interaction_op, interaction_itself=itself,
                           sigmoid_top=sigmoid_top, max_batch=max_batch,
                           max_lookups=max(int(a.num_indices_per_lookup), 1),
                           num_staged_batches=n_stage,
                           num_slots=n_slots, device=self._device,
                           ln_task=ln_task, num_tasks=num_tasks)
            # --accel_table_int8_lines: ahead of table_dtype, so that the int8 arena is laid out once; only when asked for
            if int8_lines:
                eng.set_option("table_int8_lines", int8_lines)
            # --accel_table_int4_lines: the same for an int4 arena
            if int4_lines:
                eng.set_option("table_int4_lines", int4_lines)
            # --accel_table_dtype: first, while the arena is empty -- the engine then re-derives its by-model launch
            # forms (and "preferred_slots") for the element size, and every table write below is rounded on the device
            if dtype != N.TABLE_FP32:
                eng.set_option("table_dtype", dtype)
            # --accel_mlp_dtype: the layers set below get their bf16 twins as they arrive (only when asked for: an fp32
            # engine is never told)
            if mlp_dtype != N.MLP_FP32:
                eng.set_option("mlp_dtype", mlp_dtype)
            # --accel_mlp_bf16_fuse: behind it, and only when asked for
            if bf16_fuse:
                eng.set_option("mlp_bf16_fuse", bf16_fuse)
            # --accel_sls_pool mean: every bag's pooled vector is its mean (only when asked for: a sum engine is never told)
            if pool != N.POOL_SUM:
                eng.set_option("sls_pool", pool)
            # --accel_sls_weighted_flat 1: weighted launch sets keep the flat and one-lookup forms (only when asked for: the
            # CPU restatement of the ABI does not know the key)
            if weighted_flat:
                eng.set_option("sls_weighted_flat", weighted_flat)
            return eng
        eng = make(self._num_slots())
        if int(getattr(a, "accel_slots", 0) or 0) <= 0 and eng.get_option("preferred_slots") != eng.num_slots:
            # (an MLP-bound DLRM such as RM3: the class follows from the shapes, which the engine has just read)
            want = int(eng.get_option("preferred_slots"))
            eng.close()
            eng = make(want)
            if eng.get_option("preferred_slots") != eng.num_slots:
                raise RuntimeError("accel_slots 0: created %d slots, the engine prefers %d" % (
                    eng.num_slots, eng.get_option("preferred_slots")))
        # A/B aid for runs through the queue harness: DRS_ENGINE_OPTS="key=value,key=value"
        import os
        for kv in filter(None, os.environ.get("DRS_ENGINE_OPTS", "").split(",")):
            k, v = kv.split("=")
            eng.set_option(k.strip(), int(v))
        seed = int(getattr(a, "numpy_rand_seed", 0))
        for t, W in enumerate(self.emb_w):
            if W is None:
                n = int(self.ln_emb[t])
                eng.fill_table_uniform(t, -float(np.sqrt(1 / n)), float(np.sqrt(1 / n)), seed)
            else:
                eng.set_table(t, W)
        return eng

    def create(self, X, S_lengths, S_indices, T, id_qs=None, len_qs=None):
        """Build the device model (reference: create_input + create_model,
        models/dlrm_s_caffe2.py:509-546).  X/S_* are the first input set; they are kept as
        the "current blobs" exactly like the reference's initial FeedBlobs."""
        self._create_engine()
        self._cur_inputs = (X, S_lengths, S_indices)

    def parameters(self):
        return self

    # -- execution ----------------------------------------------------------------
    def run(self, X=None, S_lengths=None, S_indices=None, enable_prof=False, S_weights=None):
        """One forward of a fed batch; returns the time at which input hand-over ended,
        like the reference's run() (models/dlrm_s_caffe2.py:549-569).  S_weights (stand-alone runs only: the resident
        input set carries them, the per-call input path is unweighted): per-index weights, one array or None per table."""
        if X is None and S_indices is None:
            X, S_lengths, S_indices = self._cur_inputs
        else:
            self._cur_inputs = (X, S_lengths, S_indices)
        if S_weights is not None and not getattr(self, "split_load", False):
            raise ValueError("per-index weights travel with staged batches only (stage_batches, or a stand-alone run)")
        bs = len(S_lengths[0])
        if getattr(self, "split_load", False):
            # stand-alone runs (main() below): the reference's run() feeds the blobs, takes the time, then
            # runs the net (models/dlrm_s_caffe2.py:551-568) -- "data loading" vs "computation".  Same split
            # here: narrow + ENFORCE-check + copy the inputs into a resident input set (synchronous), take the
            # time, then the forward on resident inputs.
            self.engine.stage_batch(0, X, S_indices, S_lengths, weights=S_weights)
            load_time = time.time()
            if enable_prof:
                self._run_profiled(None, None, None, bs, staged=0)
            else:
                self._out = self.engine.forward(0, bs)
            return load_time
        load_time = time.time()
        if enable_prof:
            self._run_profiled(X, S_lengths, S_indices, bs)
        else:
            self._out = self.engine.forward_inputs(X, S_indices, S_lengths, bs)
        return load_time

    def _run_profiled(self, X, S_lengths, S_indices, bs, staged=None):
        """--enable_profiling: the reference runs `workspace.C.benchmark_net(net, 0, 1, True)`
        (models/dlrm_s_caffe2.py:565-566), whose per-operator-type table
        experiments/operator_breakdown/sweep_p.py:21-28 parses (`<ms> ms. <pct>%. <OpType>`,
        value = field 0, type = field 3).  Here a query is two kinds of launches, timed with HIP
        events on the streams they run on: the multi-table gather (= every SparseLengthsSum of the
        graph) and the MLP launches (= every FC with its fused Relu / Sigmoid, the Concat /
        BatchMatMul / BatchGather interaction and the Cast, which have no launch of their own)."""
        eng = self.engine
        eng.reset_kernel_time()
        eng.set_profiling(2)
        try:
            self._out = eng.forward_inputs(X, S_indices, S_lengths, bs) if staged is None else eng.forward(staged, bs)
        finally:
            eng.set_profiling(0)
        sls_ms, _ = eng.kernel_time(N.KERNEL_SLS)
        mlp_ms, _ = eng.kernel_time(N.KERNEL_MLP)
        tot = max(sls_ms + mlp_ms, 1e-12)
        print("Time per operator type:")
        for ms, name in sorted(((sls_ms, "SparseLengthsSum"), (mlp_ms, "FC")), reverse=True):
            print("%16.6g ms. %10.5g%%. %s" % (ms, 100.0 * ms / tot, name))
        print("%16.6g ms in Total" % tot)
        sys.stdout.flush()

    def run_queued(self, ids, lengths, fc, batch_size):
        # 2-D arrays (what the reference's feeder passes) go down as they are: row pointers only
        if not (isinstance(ids, np.ndarray) and isinstance(lengths, np.ndarray)):
            ids, lengths = list(ids), list(lengths)
        self._out = self.engine.forward_inputs(fc, ids, lengths, int(batch_size))
        return self._out

    def run_queued_multi(self, requests, slot=0):
        """run_queues for every request an engine found waiting in its queue, as ONE launch set
        (drs_run_queues_multi_async): `requests` is a list of (ids, lengths, fc, batch_size) in
        run_queues' argument order; returns the list of their [bs_i, n_out] outputs."""
        no_dense = self.engine.m_den == 0
        qs = [(None if no_dense else fc, np.asarray(ids) if not isinstance(ids, np.ndarray) else ids,
               np.asarray(lengths) if not isinstance(lengths, np.ndarray) else lengths, int(bs))
              for ids, lengths, fc, bs in requests]
        self.engine.run_queues_multi_async(qs, slot=slot)
        sizes = [q[3] for q in qs]
        out = self.engine.wait(slot, sum(sizes))
        outs = np.split(out, np.cumsum(sizes)[:-1], axis=0)
        self._out = outs[-1]
        return outs

    def run_queued_device_multi(self, requests, slot=0):
        """run_queued_multi for requests whose arrays are torch tensors on the engine's GPU
        (drs_run_queues_device_multi_async): a request is (ids, lengths, fc, batch_size[, fixed_len]) with ids [T, n]
        int64, lengths [T, bs] int32, fc [bs, m_den] float32 or None -- last dimension contiguous, row strides as the
        tensors have them, so slices of wider tensors go down as they are.  fixed_len >= 0 promises that every bag holds
        that many indices (default -1: the lengths are read).  No byte crosses the bus: one kernel launch narrows, scans
        and checks the arrays.  Returns the list of [bs_i, n_out] outputs (numpy, as run_queued_multi).
        A request may carry a sixth element, its per-sample weights (SparseLengthsWeightedSum; device_weights): a [T, n]
        tensor of float32, float16 or bfloat16 on the same GPU, one weight per index of ids, or None -- the same launch
        copies or widens them (drs_run_queues_device_weighted_multi_async); requests with and without weights mix."""
        import torch
        eng = self.engine
        qs, spare, wts = self._device_queries(requests)
        # the engine cannot order itself behind the work that produced the tensors: once per call, torch's stream
        torch.cuda.current_stream(eng.device).synchronize()
        eng.run_queues_device_multi_async(qs, slot=slot, weights=wts)
        sizes = [q[0] for q in qs]
        out = eng.wait(slot, sum(sizes))
        outs = np.split(out, np.cumsum(sizes)[:-1], axis=0)
        self._out = outs[-1]
        return outs

    def _device_queries(self, requests):
        """requests of torch tensors -> (the tuples Engine.run_queues_device_multi_async takes, a tensor to keep alive or None,
        its `weights` argument: None unless a request has a sixth element, the per-sample weights or None)"""
        import torch
        eng = self.engine
        for i, r in enumerate(requests):
            if len(r) not in (4, 5, 6):
                raise ValueError("request %d: (ids, lengths, fc, batch_size[, fixed_len[, weights]])" % i)
        qs = [device_request(r[:5], eng.T, eng.m_den, eng.device, i) for i, r in enumerate(requests)]
        wts = None
        if any(len(r) == 6 for r in requests):
            wts = [device_weights(r[5], eng.T, q[4], eng.device, i) if len(r) == 6 else None
                   for i, (r, q) in enumerate(zip(requests, qs))]
        # (torch gives an empty tensor a null data_ptr; the library takes no null ids with bs > 0, even where none is read)
        spare = None
        for k, q in enumerate(qs):
            if q[0] > 0 and q[2] == 0:
                if spare is None:
                    spare = torch.zeros((eng.T, 1), dtype=torch.int64, device="cuda:%d" % eng.device)
                qs[k] = q[:2] + (spare.data_ptr(), 1) + q[4:]
        return qs, spare, wts

    def run_queued_device_io_multi(self, requests, out=None, stream=None, slot=0):
        """run_queued_device_multi whose results stay on the GPU (drs_run_queues_device_io_multi_async, `ordered` 1): returns
        at once the list of [bs_i, n_out] float32 torch tensors the scores go to -- `out`, one tensor per request (column
        blocks of wider tensors are fine), or freshly allocated ones.  The set runs behind what is enqueued on `stream` (a
        torch.cuda.Stream or a raw handle; default: torch's current stream of the engine's GPU) and work enqueued there
        after this call sees the scores; nothing synchronises on the host.  A set that failed on the device holds NaN in
        every element.  The request and output tensors are kept referenced until the next wait on the slot -- torch's
        caching allocator does not know the engine's streams -- so call finish_device(slot) (the set's completion and its
        status) before tensors handed in here are overwritten by anything not ordered on `stream`."""
        import torch
        eng = self.engine
        n_out, device = eng.n_out, eng.device
        if out is not None and len(out) != len(requests):
            raise ValueError("%d requests, %d output tensors" % (len(requests), len(out)))
        qs, spare, wts = self._device_queries(requests)
        if out is None:
            out = [torch.empty((q[0], n_out), dtype=torch.float32, device="cuda:%d" % device) for q in qs]
        outs_arg = [device_out(t, q[0], n_out, device, i) for i, (t, q) in enumerate(zip(out, qs))]
        if stream is None:
            stream = torch.cuda.current_stream(device)
        handle = stream.cuda_stream if isinstance(stream, torch.cuda.Stream) else int(stream)
        eng.run_queues_device_io_multi_async(qs, outs_arg, stream=handle, slot=slot, weights=wts)     # (waits first for a set still on the slot)
        refs = getattr(self, "_device_refs", None)
        if refs is None:
            refs = self._device_refs = {}
        refs[slot] = (list(requests), list(out), spare)
        return list(out)

    def run_queued_device_topk_multi(self, requests, k, col=0, out=None, stream=None, slot=0):
        """run_queued_device_io_multi that hands back each request's best rows instead of every score
        (drs_run_queues_device_topk_multi_async, `ordered` 1): returns at once a list of (idx, scores) torch tensors, int32
        [k_i] and float32 [k_i, n_out] with k_i = min(k, bs_i) -- the row numbers within request i of the k_i samples that
        rank first by score column `col` (NaN first, equal scores by the lower row) and their full score rows -- `out`, one
        pair per request, or freshly allocated ones.  ONE kernel launch per set ranks every request.  stream, the lifetime of
        the tensors and finish_device(slot): as in run_queued_device_io_multi; a set that failed on the device holds -1 in
        every idx and NaN in every score.  A request's sixth element carries its per-sample weights as before."""
        import torch
        eng = self.engine
        n_out, device = eng.n_out, eng.device
        k = int(k)
        if k < 0 or k > N.TOPK_MAX:
            raise ValueError("k: %d outside 0..%d" % (k, N.TOPK_MAX))
        if not 0 <= int(col) < n_out:
            raise ValueError("col: %d outside [0, %d)" % (int(col), n_out))
        if out is not None and len(out) != len(requests):
            raise ValueError("%d requests, %d output pairs" % (len(requests), len(out)))
        qs, spare, wts = self._device_queries(requests)
        ks = [min(k, q[0]) for q in qs]
        if out is None:
            dev = "cuda:%d" % device
            out = [(torch.empty((ki,), dtype=torch.int32, device=dev), torch.empty((ki, n_out), dtype=torch.float32, device=dev))
                   for ki in ks]
        tops = [device_top(p, ki, n_out, device, i) for i, (p, ki) in enumerate(zip(out, ks))]
        if stream is None:
            stream = torch.cuda.current_stream(device)
        handle = stream.cuda_stream if isinstance(stream, torch.cuda.Stream) else int(stream)
        eng.run_queues_device_topk_multi_async(qs, ks, int(col), tops, stream=handle, slot=slot, weights=wts)   # (waits first for a set still on the slot)
        refs = getattr(self, "_device_refs", None)
        if refs is None:
            refs = self._device_refs = {}
        out = [tuple(p) for p in out]
        refs[slot] = (list(requests), out, spare)
        return list(out)

    def finish_device(self, slot=0):
        """The completion of the set run_queued_device_io_multi put on `slot`: returns once its outputs are written, drops the
        references held for it, and raises DrsError for a set that failed on the device (its outputs are NaN)."""
        try:
            self.engine.wait(slot)
        finally:
            getattr(self, "_device_refs", {}).pop(slot, None)

    def stage_batches(self, lX, lS_l, lS_i, lS_w=None):
        """lS_w: per-index weights of every input set (sls_weights), or None."""
        for j in range(len(lS_l)):
            self.engine.stage_batch(j, None if lX is None else lX[j], lS_i[j], lS_l[j],
                                    weights=None if lS_w is None else lS_w[j])
        self._n_staged = len(lS_l)

    def update_embedding_rows(self, t, ids, values, stream=None):
        """Rows `ids` of embedding table t take `values` ([n, m_spa] fp32) in place, stored in the tables' current type
        (FBGEMM's emb_inplace_update; Engine.update_rows): queries enqueued before the call see the old rows.
        `ids` a torch tensor on the engine's GPU: the device route (drs_update_rows_device) -- ids int64 [n] contiguous,
        values [n, m_spa] float32, float16 or bfloat16 on the same GPU, last dimension contiguous (device_row_ids,
        device_row_values); no byte crosses the bus.  stream None: the tensors are complete; a torch.cuda.Stream or a raw
        handle: the update runs behind what is enqueued there and the caller does not synchronise.  numpy arguments take
        the host route (`stream` is refused there)."""
        eng = self.engine
        if not on_device(ids, eng.device):
            if stream is not None:
                raise ValueError("stream: ordering applies to the device route, ids on cuda:%d" % eng.device)
            return eng.update_rows(t, ids, values)
        ids_ptr, n = device_row_ids(ids, eng.device)
        val_ptr, stride, code = device_row_values(values, n, eng.D, eng.device)
        eng.update_rows_device(t, ids_ptr, n, val_ptr, stride, code, stream=_stream_handle(stream))

    def embedding_rows(self, t, ids, out=None, stream=None):
        """-> [n, m_spa] fp32: rows `ids` of embedding table t as the engine serves them (Engine.get_rows).
        `ids` a torch tensor on the engine's GPU: the device route (drs_get_rows_device) -- returns a float32 tensor on that
        GPU, `out` when given ([n, m_spa] float32, last dimension contiguous; a column block of a wider tensor keeps what
        lies between its rows); stream as in update_embedding_rows.  numpy ids take the host route (`out` and `stream` are
        refused there)."""
        eng = self.engine
        if not on_device(ids, eng.device):
            if out is not None or stream is not None:
                raise ValueError("out / stream: the device route only, ids on cuda:%d" % eng.device)
            return eng.get_rows(t, ids)
        import torch
        ids_ptr, n = device_row_ids(ids, eng.device)
        if out is None:
            out = torch.empty((n, eng.D), dtype=torch.float32, device="cuda:%d" % eng.device)
        out_ptr, stride, _ = device_row_values(out, n, eng.D, eng.device, name="out", dtypes=(torch.float32,))
        eng.get_rows_device(t, ids_ptr, n, out_ptr, stride, stream=_stream_handle(stream))
        return out

    def tune_table_placement(self, candidates=12, sets=128, spacer_gb=None, policies=(1, 0), max_extra_gb=48, sharers=1):
        """Where the tables live in HBM, and with which cache policy their rows are read, moves the many-rows-per-bag
        gather by up to 9 % -- a property of the PHYSICAL memory (it follows the memory through address changes;
        gigabytes-wide regions of HBM are "fast" or "slow", and they are different regions for non-temporal and for
        plain loads) that no synthetic probe sees, only the model's own launch sets (DESIGN.md 5,
        profiles/r05_placement/README.md).  With the input sets staged, this times full launch sets of the engine's
        preferred size (served as they will be: pipelined, the gather beside the previous set's MLP launch) on the arena drs_create made, under each load policy ("sls_nt"
        1 / 0), then on up to `candidates` - 1 further arenas taken from further on in HBM (`spacer_gb` of untouched
        memory between two candidates, default = the arena's size), and keeps the fastest (arena, policy) -- the first
        arena unless another is at least 1 % faster.  It stops as soon as one arena's best reading is 8 % under another's (the
        fast level is reached).  Every other arena and the spacers are released before it returns: one copy of the
        tables, nothing held.  Returns {"gather_us": [[nt, plain], ...], "kept": k, "sls_nt": p, ...} or
        None when the engine has nothing to time.  ~70 ms per candidate.
        While it runs every candidate and spacer stays allocated (a freed loser's pages would be handed out again as the
        next candidate): the search's transient footprint is bounded by `max_extra_gb` / `sharers` (engine processes
        that share the GPU) beside the engine's own guards (a quarter of the free memory per copy, 8 GB left free).
        A load policy the caller set with set_option is kept (only the arena is searched); "table_alloc" is restored."""
        eng = self.engine
        nb = int(getattr(self, "_n_staged", 0))
        if nb < 1 or candidates < 1:
            return None
        # only where it was measured to pay: gather-bound DLRM (incl. the in-between class, e.g. dlrm_rm1.json, whose
        # 128-byte rows read 10 % faster with plain loads when the tables are small) and DIN.  The MLP-bound shapes have
        # nothing to gain (their gather is a tenth of a set), the one-lookup models' tables are cache resident.
        # (round 5: DIN as well -- its fused gather + attention launch is its set's longest kernel; "din_nt" is its policy knob)
        if self.kind not in (N.MODEL_DLRM, N.MODEL_DIN) or not int(eng.get_option("gather_bound")):
            return None
        nt_key = "din_nt" if self.kind == N.MODEL_DIN else "sls_nt"
        co = max(1, min(int(eng.get_option("preferred_coalesce")), 16))
        bs = int(eng.max_batch)
        nt0 = int(eng.get_option(nt_key))
        ta0 = int(eng.get_option("table_alloc"))
        if nt_key in getattr(eng, "user_options", ()):     # the caller pinned the policy: search the arenas only
            policies = (nt0,)
        budget_gb = float(max_extra_gb) / max(1, int(sharers))

        # The sets are timed AS THEY WILL BE SERVED: the engine's stream mode, `preferred_slots` sets in flight, the gather
        # launches stamped by their own workgroups while the previous set's MLP launch runs beside them.  (Until the end of
        # round 5 they ran on one stream, the gather alone -- and an (arena, policy) that read 81.8 us alone took 87.1 us beside
        # the MLP launch where the first arena with plain loads took 82.8: profiles/r05_placement/README.md.)
        n_slots = max(1, min(int(eng.get_option("preferred_slots")), int(getattr(eng, "num_slots", 1))))

        def gather_us():
            busy = [False] * n_slots
            try:
                for phase, n_sets in (("warm", max(8, sets // 4)), ("timed", sets)):
                    if phase == "timed":
                        for s_ in range(n_slots):
                            if busy[s_]:
                                eng.wait(s_)
                                busy[s_] = False
                        eng.reset_kernel_time()
                        eng.set_profiling(1)
                    for g in range(n_sets):
                        s_ = g % n_slots
                        if busy[s_]:
                            eng.wait(s_)
                        eng.forward_multi_async(s_, [(g * co + k) % nb for k in range(co)], [bs] * co)
                        busy[s_] = True
                for s_ in range(n_slots):
                    if busy[s_]:
                        eng.wait(s_)
                        busy[s_] = False
                eng.set_profiling(0)
                ms, n = eng.kernel_time(N.KERNEL_SLS_CLOCK)
            finally:
                eng.set_profiling(0)
            return ms / n * 1e3 if n else None

        def both():
            out = []
            for p in policies:
                eng.set_option(nt_key, p, user=False)
                out.append(gather_us())
            return out

        times, best = [], None          # best = (us, arena index, policy)
        import time as _time
        t_begin = _time.perf_counter()
        try:
            t = both()
            if t[0] is None:
                return None
            times.append(t)
            size_gb = max(1, -(-int(eng.get_option("table_bytes")) // (1 << 30)))
            gap = size_gb if spacer_gb is None else int(spacer_gb)
            eng.set_option("table_alloc", 0, user=False)  # (plain hipMalloc candidates: arenas of the virtual-memory API read as
            for _ in range(1, candidates):              #  fast alone but measured 2 % slower beside two MLP streams, dlrm_rm1.json)
                if len(times) * (size_gb + max(gap, 0)) + size_gb > budget_gb:
                    break                               # the next candidate (and its spacer) would pass the footprint bound
                per_arena = [min(tt) for tt in times]
                if min(per_arena) <= 0.92 * max(per_arena):
                    break                               # an arena 8 % under the slowest one: the fast level has been seen (beside the MLP
                                                        # launch the levels read 90 / 88 / 85-86 / 82 us on RMC1; stopping at 5 % kept an 84.6)
                try:
                    if gap > 0:
                        eng.set_option("table_spacer", gap << 30, user=False)
                    eng.set_option("table_placement", -1, user=False)
                except N.DrsError:
                    break                               # no room for one more copy: the ones so far compete
                t = both()
                if any(u is None for u in t):
                    break                               # (nothing was timed on this one: it does not compete)
                times.append(t)
            flat = [(u, k, policies[i]) for k, tt in enumerate(times) for i, u in enumerate(tt)]
            best = min(flat)
            # the arena drs_create made stays unless another one is at least 1 % faster (timed as served, the readings repeat
            # to +-0.2 %; at 2 % a run kept an 84.6 us arena with 83.5 us ones on the list)
            first = min((u, 0, policies[i]) for i, u in enumerate(times[0]))
            if best[1] != 0 and best[0] > 0.99 * first[0]:
                best = first
            return {"gather_us": [[round(u, 2) for u in tt] for tt in times], "timed": "pipelined, %d sets in flight" % n_slots, "policies": ["nt" if p else "plain" for p in policies],
                    "kept": best[1], "sls_nt": best[2], "candidates": len(times), "losers": "freed",
                    "seconds": round(_time.perf_counter() - t_begin, 2)}
        except N.DrsError:
            return None                                 # (staged sets smaller than a full batch, ...: serve from where it is)
        finally:
            try:
                eng.set_option("table_alloc", ta0, user=False)
                eng.set_option(nt_key, best[2] if best else nt0, user=False)
                if best:
                    eng.set_option("table_placement", best[1], user=False)
                eng.set_option("table_placement", -2, user=False)
            except N.DrsError:
                pass

    def run_staged(self, batch_id, batch_size):
        self._out = self.engine.forward(int(batch_id), int(batch_size))
        return self._out

    def run_staged_multi(self, batch_ids, batch_sizes, slot=0):
        """Several queued queries in one set of launches (drs_forward_multi_async); returns
        the list of their [bs_i, n_out] outputs."""
        sizes = [int(b) for b in batch_sizes]
        self.engine.forward_multi_async(slot, [int(b) for b in batch_ids], sizes)
        out = self.engine.wait(slot, sum(sizes))
        cuts = np.cumsum(sizes)[:-1]
        outs = np.split(out, cuts, axis=0)
        self._out = outs[-1]
        return outs

    def submit_staged_multi(self, batch_ids, batch_sizes, slot):
        """Enqueue one set of launches on `slot` and return at once; collect_staged_multi(slot,
        batch_sizes) hands the outputs over.  With several slots the engine process keeps the
        gather of one set, the MLP of the previous one and the host work of the next in flight
        at the same time."""
        self.engine.forward_multi_async(slot, [int(b) for b in batch_ids], [int(b) for b in batch_sizes])

    def collect_staged_multi(self, batch_sizes, slot):
        sizes = [int(b) for b in batch_sizes]
        out = self.engine.wait(slot, sum(sizes))
        outs = np.split(out, np.cumsum(sizes)[:-1], axis=0)
        self._out = outs[-1]
        return outs

    def fetch_output(self):
        """FetchBlob("prob_click") counterpart: [bs, n_out] float32 of the last run."""
        return self._out


# =====================================================================================
class DLRM_Net(_HipNet):
    kind = N.MODEL_DLRM

    def __init__(self, cli_args, model=None, tag=None, enable_prof=False, id_qs=None, len_qs=None,
                 fc_q=None):
        self._common_init(cli_args)
        # shape algebra + checks of models/dlrm_s_caffe2.py:403-440
        ln_bot = _ints(cli_args.arch_mlp_bot)
        m_den = ln_bot[0]
        m_spa = cli_args.arch_sparse_feature_size
        ln_emb = _ints(cli_args.arch_embedding_size)
        num_fea = ln_emb.size + 1
        m_den_out = ln_bot[ln_bot.size - 1]
        if cli_args.arch_interaction_op == "dot":
            if cli_args.arch_interaction_itself:
                num_int = (num_fea * (num_fea + 1)) // 2 + m_den_out
            else:
                num_int = (num_fea * (num_fea - 1)) // 2 + m_den_out
        elif cli_args.arch_interaction_op == "cat":
            num_int = num_fea * m_den_out
        else:
            sys.exit("ERROR: --arch-interaction-op=" + cli_args.arch_interaction_op
                     + " is not supported")
        ln_top = _ints(str(num_int) + "-" + cli_args.arch_mlp_top)
        if m_spa != m_den_out:
            sys.exit("ERROR: arch-sparse-feature-size " + str(m_spa)
                     + " does not match last dim of bottom mlp " + str(m_den_out))
        if num_int != ln_top[0]:
            sys.exit("ERROR: # of feature interactions " + str(num_int)
                     + " does not match first dim of top mlp " + str(ln_top[0]))
        self.m_spa, self.ln_emb, self.ln_bot, self.ln_top = m_spa, ln_emb, ln_bot, ln_top
        self.arch_interaction_op = cli_args.arch_interaction_op
        self.arch_interaction_itself = cli_args.arch_interaction_itself
        self.sigmoid_bot = -1
        self.sigmoid_top = ln_top.size - 1
        # create_sequential_forward_ops order (:367-386): embeddings, bottom, top
        self.emb_w = self._make_tables(m_spa, ln_emb)
        self.bot_w = _init_mlp(ln_bot)
        self.top_w = _init_mlp(ln_top)

    def _create_engine(self):
        op = N.INTERACT_DOT if self.arch_interaction_op == "dot" else N.INTERACT_CAT
        self.engine = self._build_engine(self.ln_bot, self.ln_top, op, self.arch_interaction_itself,
                                         self.sigmoid_top)
        for i, (W, b) in enumerate(self.bot_w):
            self.engine.set_fc(N.MLP_BOT, i, W, b)
        for i, (W, b) in enumerate(self.top_w):
            self.engine.set_fc(N.MLP_TOP, i, W, b)

    def tril_indices(self):
        """interaction_tril_indices blob (models/dlrm_s_caffe2.py:529-535)."""
        offset = 1 if self.arch_interaction_itself else 0
        num_fea = self.ln_emb.size + 1
        return np.array([j + i * num_fea for i in range(num_fea) for j in range(i + offset)])


class Wide_and_Deep(_HipNet):
    kind = N.MODEL_WND

    def __init__(self, cli_args, model=None, tag=None, enable_prof=False, id_qs=None, len_qs=None,
                 fc_q=None):
        self._common_init(cli_args)
        # models/wide_and_deep.py:307-346
        if cli_args.arch_interaction_op != "cat":
            sys.exit("ERROR: sparse and dense features must be concatenated in wide and deep")
        ln_bot = _ints(cli_args.arch_mlp_bot)
        if ln_bot.size != 1:
            sys.exit("ERROR: wide and deep has no MLP layers for the continuous features")
        m_spa = cli_args.arch_sparse_feature_size
        ln_emb = _ints(cli_args.arch_embedding_size)
        num_fea = ln_emb.size + 1
        num_int = (num_fea - 1) * int(m_spa) + int(ln_bot[0])
        ln_top = _ints(str(num_int) + "-" + cli_args.arch_mlp_top)
        self.m_spa, self.ln_emb, self.ln_bot, self.ln_top = m_spa, ln_emb, ln_bot, ln_top
        self.arch_interaction_op = "cat"
        self.arch_interaction_itself = cli_args.arch_interaction_itself
        self.sigmoid_bot = -1
        self.sigmoid_top = ln_top.size - 1
        self.emb_w = self._make_tables(m_spa, ln_emb)     # :282-287
        self.top_w = _init_mlp(ln_top)                    # :299-302

    def _create_engine(self):
        self.engine = self._build_engine(self.ln_bot, self.ln_top, N.INTERACT_CAT, False, self.sigmoid_top)
        for i, (W, b) in enumerate(self.top_w):
            self.engine.set_fc(N.MLP_TOP, i, W, b)


class MT_Wide_and_Deep(Wide_and_Deep):
    """Multi-task W&D (models/multi_task_wnd.py): the W&D trunk with an all-ReLU shared top MLP
    (:301 passes sigmoid_layer -1), then `num_multi_tasks` task heads of widths arch_mlp_tasks
    over its output, each with Sigmoid on the layer index the reference calls sigmoid_top
    (= ln_top.size - 1, :399,309).  The reference builds and runs every head but keeps only the
    last as `last_output` (:316); here the heads' outputs come back side by side,
    [bs, num_tasks * ln_task[-1]] (the reference's last_output is the last ln_task[-1] columns)."""
    kind = N.MODEL_MTWND

    def __init__(self, cli_args, model=None, tag=None, enable_prof=False, id_qs=None, len_qs=None,
                 fc_q=None):
        # weights in the reference's order: embeddings, shared top, then each head (:286-312)
        Wide_and_Deep.__init__(self, cli_args, model, tag, enable_prof)
        self.ln_task = _ints(cli_args.arch_mlp_tasks)
        if self.ln_top[-1] != self.ln_task[0]:
            sys.exit("ERROR: Shared top layer and task MLP layers must have same input/output dimension")
        self.num_tasks = int(cli_args.num_multi_tasks)
        self.task_w = [_init_mlp(self.ln_task) for _ in range(self.num_tasks)]

    def _create_engine(self):
        self.engine = self._build_engine(self.ln_bot, self.ln_top, N.INTERACT_CAT, False, self.sigmoid_top,
                                         ln_task=self.ln_task, num_tasks=self.num_tasks)
        for i, (W, b) in enumerate(self.top_w):
            self.engine.set_fc(N.MLP_TOP, i, W, b)
        for k, head in enumerate(self.task_w):
            for i, (W, b) in enumerate(head):
                self.engine.set_fc(N.MLP_TASK0 + k, i, W, b)

class _NoDenseNet(_HipNet):
    """Models whose query is sparse features only (NCF, DIN): the dense argument of the
    reference's signatures is accepted and ignored, as the reference ignores it."""

    def run(self, X=None, S_lengths=None, S_indices=None, enable_prof=False, S_weights=None):
        if S_indices is None:
            X, S_lengths, S_indices = self._cur_inputs
        else:
            self._cur_inputs = (X, S_lengths, S_indices)
        if S_weights is not None and not getattr(self, "split_load", False):
            raise ValueError("per-index weights travel with staged batches only (stage_batches, or a stand-alone run)")
        bs = len(S_lengths[0])
        if getattr(self, "split_load", False):      # stand-alone runs: see _HipNet.run
            self.engine.stage_batch(0, None, S_indices, S_lengths, weights=S_weights)
            load_time = time.time()
            if enable_prof:
                self._run_profiled(None, None, None, bs, staged=0)
            else:
                self._out = self.engine.forward(0, bs)
            return load_time
        load_time = time.time()
        if enable_prof:     # the reference runs benchmark_net for these models too (sweep_p.py parses the table)
            self._run_profiled(None, S_lengths, S_indices, bs)
        else:
            self._out = self.engine.forward_inputs(None, S_indices, S_lengths, bs)
        return load_time

    def run_queued(self, ids, lengths, fc, batch_size):
        self._out = self.engine.forward_inputs(None, list(ids), list(lengths), int(batch_size))
        return self._out

    def stage_batches(self, lX, lS_l, lS_i, lS_w=None):
        for j in range(len(lS_l)):
            self.engine.stage_batch(j, None, lS_i[j], lS_l[j], weights=None if lS_w is None else lS_w[j])
        self._n_staged = len(lS_l)


class NCF(_NoDenseNet):
    kind = N.MODEL_NCF

    def __init__(self, cli_args, model=None, tag=None, enable_prof=False, id_qs=None, len_qs=None):
        self._common_init(cli_args)
        # models/ncf.py:348-392
        if cli_args.arch_interaction_op != "cat":
            sys.exit("ERROR: sparse and dense features must be concatenated in NCF")
        ln_emb = _ints(cli_args.arch_embedding_size)
        if ln_emb.size != 4:
            sys.exit("ERROR: NCF only has 4 embedding tables")
        if cli_args.num_indices_per_lookup != 1:
            sys.exit("ERROR: NCF has 1 lookup per table")
        m_spa = cli_args.arch_sparse_feature_size
        num_int = 2 * int(m_spa)
        ln_top = _ints(str(num_int) + "-" + cli_args.arch_mlp_top)
        self.m_spa, self.ln_emb, self.ln_top = m_spa, ln_emb, ln_top
        self.ln_bot = np.array([0], dtype=int)
        self.arch_interaction_op = "cat"
        self.arch_interaction_itself = cli_args.arch_interaction_itself
        # create_emb: MF tables 0,1 then MLP tables 2,3 (:198-299); MLP over ln_top[:-1]
        # (:332-333); predictor [m_spa + ln_top[-2], ln_top[-1]] (:341-345); all Relu
        self.emb_w = self._make_tables(m_spa, ln_emb)
        self.top_w = _init_mlp(ln_top[:-1])
        self.final_w = _init_mlp(np.array([int(m_spa) + int(ln_top[-2]), int(ln_top[-1])]))

    def _create_engine(self):
        self.engine = self._build_engine(np.array([0]), self.ln_top[:-1], N.INTERACT_CAT, False, -1)
        for i, (W, b) in enumerate(self.top_w):
            self.engine.set_fc(N.MLP_TOP, i, W, b)
        W, b = self.final_w[0]
        self.engine.set_fc(N.MLP_FINAL, 0, W, b)


class DIN_Net(_NoDenseNet):
    """Deep Interest Network (models/din.py:247-390).  Tables = [user profile | the behaviour
    tables | candidate ad | context] (utils.cli has already replicated the behaviour table
    `user_behavior_tables` times, utils/utils.py:132-149).  Per behaviour table one attention unit
    with its OWN MLP 3*D -> arch_mlp_bot -> D over Concat(u_i, ad, u_i + ad) (:247-285);
    atten_out = Sum of the units; top MLP over Concat(profile, atten_out, ad, context)
    (:311-323); every activation is ReLU (the reference passes no sigmoid layer, :274,323)."""
    kind = N.MODEL_DIN

    def __init__(self, cli_args, model=None, tag=None, enable_prof=False, id_qs=None, len_qs=None):
        self._common_init(cli_args)
        m_spa = int(cli_args.arch_sparse_feature_size)
        ln_emb = _ints(cli_args.arch_embedding_size)
        if ln_emb.size < 4:                         # the reference asserts (:356)
            sys.exit("ERROR: DIN needs user profile, user behavior, candidate ad and context tables")
        num_int = 4 * m_spa
        ln_top = _ints(str(num_int) + "-" + cli_args.arch_mlp_top)
        self.ln_att = _ints(str(3 * m_spa) + "-" + cli_args.arch_mlp_bot + "-" + str(m_spa))   # :255-260
        self.m_spa, self.ln_emb, self.ln_top = m_spa, ln_emb, ln_top
        self.ln_bot = self.ln_att
        self.arch_interaction_op = "cat"
        self.arch_interaction_itself = cli_args.arch_interaction_itself
        # create order (:288-323): embeddings, each unit's MLP in table order, top MLP
        self.emb_w = self._make_tables(m_spa, ln_emb)
        self.att_w = [_init_mlp(self.ln_att) for _ in range(ln_emb.size - 3)]
        self.top_w = _init_mlp(ln_top)

    def _create_engine(self):
        self.engine = self._build_engine(self.ln_att, self.ln_top, N.INTERACT_CAT, False, -1)
        for u, unit in enumerate(self.att_w):
            for i, (W, b) in enumerate(unit):
                self.engine.set_fc(N.MLP_ATT0 + u, i, W, b)
        for i, (W, b) in enumerate(self.top_w):
            self.engine.set_fc(N.MLP_TOP, i, W, b)


# =====================================================================================
class DIEN_Net(_NoDenseNet):
    """Deep Interest Evolution Network (models/dien.py:308-470).  Tables as DIN.  The behaviour
    embeddings of a query go through two caffe2 rnn_cell.BasicRNN layers (tanh, zero initial state,
    arch_sparse_feature_size -> hidden_size -> hidden_size); the top MLP (all ReLU) reads
    Concat(last state of the second layer, user profile, candidate ad, context) (:411-431).

    Reference behaviour kept as it is: the Reshape of the Concat'ed [bs, U*D] embeddings to
    [U, bs, D] is a row-major reinterpretation (:316-320), so for bs > 1 step t of "sample" b is
    embedding (t*bs + b) % U of sample (t*bs + b) // U; the FC + Softmax between the two RNNs is
    dead (the Sum that follows overwrites its output with a copy of the first RNN's states,
    :336-348) and is not computed.

    Recurrent weights: the reference feeds np.random.randn values (:318-331,350-363) -- drawn here
    in the same order so the numpy stream stays aligned for the top MLP -- and then create() runs
    Caffe2's param_init_net (:528), which re-draws them with XavierFill / zero biases from Caffe2's
    own RNG.  `dien_rnn_init` = "xavier" (default) uses U(+-sqrt(3/fan_in)) weights and zero biases
    from a RandomState of their own (what a live reference run has, up to the unknowable RNG);
    "fed" keeps the randn values (the recorded-graph fixture, tests/golden/dien_mini)."""
    kind = N.MODEL_DIEN

    def __init__(self, cli_args, model=None, tag=None, enable_prof=False, id_qs=None, len_qs=None,
                 seq_q=None, hid_q=None):
        self._common_init(cli_args)
        m_spa = int(cli_args.arch_sparse_feature_size)
        H = int(cli_args.hidden_size)
        ln_emb = _ints(cli_args.arch_embedding_size)
        if ln_emb.size < 4:                         # the reference asserts (:457)
            sys.exit("ERROR: DIEN needs user profile, user behavior, candidate ad and context tables")
        self.m_spa, self.ln_emb, self.hidden_size = m_spa, ln_emb, H
        self.ln_bot = np.array([m_spa, H], dtype=int)
        self.ln_top = _ints(str(H + 3 * m_spa) + "-" + cli_args.arch_mlp_top)      # :426-429
        self.arch_interaction_op = "cat"
        self.arch_interaction_itself = cli_args.arch_interaction_itself
        self.emb_w = self._make_tables(m_spa, ln_emb)

        def fed(din):   # gates_t_w, gates_t_b, i2h_w, i2h_b (:318-321) -> {i2h: (W, b), gates_t: (W, b)}
            gw = np.random.randn(H, H).astype(np.float32)
            gb = np.random.randn(H).astype(np.float32)
            iw = np.random.randn(H, din).astype(np.float32)
            ib = np.random.randn(H).astype(np.float32)
            return [(iw, ib), (gw, gb)]
        self.rnn_w = [fed(m_spa), fed(H)]
        if getattr(cli_args, "dien_rnn_init", "xavier") != "fed":
            rs = np.random.RandomState(int(getattr(cli_args, "numpy_rand_seed", 0)) + 1)
            z = np.zeros(H, dtype=np.float32)
            self.rnn_w = [[(rs.uniform(-np.sqrt(3 / din), np.sqrt(3 / din), (H, din)).astype(np.float32), z),
                           (rs.uniform(-np.sqrt(3 / H), np.sqrt(3 / H), (H, H)).astype(np.float32), z)]
                          for din in (m_spa, H)]
        self.top_w = _init_mlp(self.ln_top)

    def _create_engine(self):
        self.engine = self._build_engine(self.ln_bot, self.ln_top, N.INTERACT_CAT, False, -1)
        for l, mlp in enumerate((N.MLP_RNN0, N.MLP_RNN1)):
            for i, (W, b) in enumerate(self.rnn_w[l]):
                self.engine.set_fc(mlp, i, W, b)
        for i, (W, b) in enumerate(self.top_w):
            self.engine.set_fc(N.MLP_TOP, i, W, b)


class _Wrapper(object):
    """X_Wrapper(args): .create(...), .run_queues(ids, lengths, fc, batch_size)
    (models/dlrm_s_caffe2.py:79-174).  The 2T+1 Caffe2 BlobsQueues the reference
    builds here (:127-139,179-211) have no counterpart: a HIP stream orders the work."""

    net_cls = None
    attr = None

    def __init__(self, cli_args, model=None, tag=None, enable_prof=False):
        self.args = cli_args
        self.accel_en = getattr(cli_args, "use_accel", False)
        setattr(self, self.attr, self.net_cls(cli_args, model, tag, enable_prof))

    @property
    def net(self):
        return getattr(self, self.attr)

    def create(self, X, S_lengths, S_indices, T):
        self.net.create(X, S_lengths, S_indices, T)

    def run_queues(self, ids, lengths, fc, batch_size):
        return self.net.run_queued(ids, lengths, fc, batch_size)

    def run_queues_multi(self, requests, slot=0):
        """Several queued requests, each in run_queues' argument order, as one launch set."""
        return self.net.run_queued_multi(requests, slot=slot)

    def run_queues_device_multi(self, requests, slot=0):
        """run_queues_multi for requests whose arrays are torch tensors on the engine's GPU (_HipNet.run_queued_device_multi);
        a request's optional sixth element is its per-sample weights."""
        return self.net.run_queued_device_multi(requests, slot=slot)

    def run_queues_device_io_multi(self, requests, out=None, stream=None, slot=0):
        """run_queues_device_multi whose results stay on the GPU, ordered on a torch stream: returns the list of [bs_i, n_out]
        device tensors at once (_HipNet.run_queued_device_io_multi); finish_device(slot) is the set's completion."""
        return self.net.run_queued_device_io_multi(requests, out=out, stream=stream, slot=slot)

    def run_queues_device_topk_multi(self, requests, k, col=0, out=None, stream=None, slot=0):
        """run_queues_device_io_multi that keeps each request's k best rows by score column `col`: returns the list of
        (idx, scores) device tensors at once, ranked by one kernel launch per set (_HipNet.run_queued_device_topk_multi);
        finish_device(slot) is the set's completion."""
        return self.net.run_queued_device_topk_multi(requests, k, col=col, out=out, stream=stream, slot=slot)

    def finish_device(self, slot=0):
        return self.net.finish_device(slot=slot)


class DLRM_Wrapper(_Wrapper):
    net_cls, attr = DLRM_Net, "dlrm"


class Wide_and_Deep_Wrapper(_Wrapper):
    net_cls, attr = Wide_and_Deep, "wnd"


class NCF_Wrapper(_Wrapper):
    net_cls, attr = NCF, "ncf"


class MT_Wide_and_Deep_Wrapper(_Wrapper):
    net_cls, attr = MT_Wide_and_Deep, "mtwnd"


class DIN_Wrapper(_Wrapper):
    net_cls, attr = DIN_Net, "din"


class DIEN_Wrapper(_Wrapper):
    net_cls, attr = DIEN_Net, "dien"


WRAPPERS = {"dlrm": DLRM_Wrapper, "wnd": Wide_and_Deep_Wrapper, "ncf": NCF_Wrapper,
            "mtwnd": MT_Wide_and_Deep_Wrapper, "din": DIN_Wrapper, "dien": DIEN_Wrapper}


def main(argv=None):
    """Stand-alone model benchmark: the `__main__` of the reference's model scripts
    (models/dlrm_s_caffe2.py:575-661; wide_and_deep.py, ncf.py, multi_task_wnd.py, din.py, dien.py end the
    same way; models/run.sh:8-57 lists the invocations), with the reference's flags:

        python -m deeprecsys_amd.dlrm_s_hip --inference_only --config_file <models/configs/dlrm_rm1.json> \
            --num_batches 4 --nepochs 100 --mini_batch_size 256 --max_mini_batch_size 256 [--enable_profiling]

    One script for every model family (`--model_type dlrm|wnd|ncf|mtwnd|din|dien`, set by the shipped
    config files); it always runs on the accelerator (`--use_accel` is accepted and implied: this
    package has no CPU forward).  Prints the six `***` lines that
    accelerator/nvidia_gtx_1080_ti/generate_data.py:20 collects into `results_<model>.txt`,
    accelerator/predict_execution.py:10-29 parses and experiments/speedup/sweep_rt.py:158-183 sweeps."""
    from .utils.utils import cli
    return standalone(cli(argv))


def standalone(args):
    """The stand-alone loop itself, on parsed arguments: what the reference's inferenceEngine() runs when it has no
    request queue (inferenceEngine.py:137-173, reached from `DeepRecSys.py` without --queue, :184-185) -- nepochs passes
    over the generated batches, then the six `***` lines."""
    from .data_generator.dlrm_data import DLRMDataGenerator
    np.random.seed(args.numpy_rand_seed)
    np.set_printoptions(precision=args.print_precision)
    print("Using %d Accel(s)..." % max(N.device_count(), 0))
    if args.model_type not in WRAPPERS:
        sys.exit("ERROR: --model_type=" + str(args.model_type) + " is not supported")
    if args.data_generation == "dataset":
        print("Error we have disabled this function currently....")
        sys.exit()
    dc = DLRMDataGenerator(args)
    (nbatches, lX, lS_l, lS_i) = dc.generate_input_data()       # random | synthetic; anything else exits there
    print("Generating output dataset")
    (nbatches, lT) = dc.generate_output_data()
    lS_l = [[np.asarray(l, dtype=np.int32) for l in per] for per in lS_l]
    lS_i = [[np.asarray(i, dtype=np.int64) for i in per] for per in lS_i]
    lS_w = sls_weights(args, lS_i)                              # --accel_sls_weights (None: unweighted bags)
    print("Trying to initialize %s" % args.model_type.upper())
    net_cls = WRAPPERS[args.model_type].net_cls
    resident, args.num_batches = args.num_batches, 1      # one resident input set: run() re-feeds it per batch
    try:
        net = net_cls(args)
        print("Initialized %s Net" % args.model_type.upper())
        net.create(lX[0], lS_l[0], lS_i[0], lT[0])
    finally:
        args.num_batches = resident
    net.split_load = True
    print("Created network")
    no_dense = net.engine.m_den == 0
    total_time = dload_time = 0.0
    net.run(None if no_dense else lX[0], lS_l[0], lS_i[0], S_weights=None if lS_w is None else lS_w[0])   # (first launch: code objects, clocks)
    time_start = time.time()
    print("Running networks")
    for _k in range(args.nepochs):
        for j in range(nbatches):
            time_load_start = time.time()
            time_load_end = net.run(None if no_dense else lX[j], lS_l[j], lS_i[j], args.enable_profiling,
                                    S_weights=None if lS_w is None else lS_w[j])
            dload_time += (time_load_end - time_load_start)
    time_end = time.time()
    dload_time *= 1000.
    total_time += (time_end - time_start) * 1000.
    n_iter = max(args.nepochs * nbatches, 1)
    print("Total data loading time: ***", dload_time, " ms")
    print("Total data loading time: ***", dload_time / n_iter, " ms/iter")
    print("Total computation time: ***", (total_time - dload_time), " ms")
    print("Total computation time: ***", (total_time - dload_time) / n_iter, " ms/iter")
    print("Total execution time: ***", total_time, " ms")
    print("Total execution time: ***", total_time / n_iter, " ms/iter")
    sys.stdout.flush()
    net.engine.close()


if __name__ == "__main__":
    main()
