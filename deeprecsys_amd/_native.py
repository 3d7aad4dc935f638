"""ctypes binding of include/drs.h (libdrs_hip.so) -- the only way into the kernels.

Fails loudly: a missing library raises at first use, and drs_create fails when no
HIP device is visible.  Nothing here (or anywhere in this package) falls back to a
CPU implementation.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libdrs_hip.so")   # the one library this package binds (no override)

# status codes (include/drs.h)
OK, ERR_BAD_ARG, ERR_OOM, ERR_HIP, ERR_INDEX_RANGE, ERR_LENGTHS_SUM, ERR_STATE, ERR_UNSUPPORTED = \
    0, -1, -2, -3, -4, -5, -6, -7
MODEL_DLRM, MODEL_WND, MODEL_NCF, MODEL_MTWND, MODEL_DIN, MODEL_DIEN = 0, 1, 2, 3, 4, 5
INTERACT_DOT, INTERACT_CAT = 0, 1
TABLE_FP32, TABLE_FP16, TABLE_BF16 = 0, 1, 2   # option "table_dtype": element type of the stored tables
TABLE_FP8_E4M3 = 4                              # ... OCP fp8 e4m3 codes (torch's float8_e4m3fn) under one power-of-two scale per table (Engine.table_fp8_exponent)
TABLE_INT8_ROWWISE = 8                          # ... 8-bit codes with an fp32 scale and bias per row (Caffe2's Fused8BitRowwise)
TABLE_INT4_ROWWISE = 9                          # ... 4-bit codes with an fp16 scale and bias per row (torch's embedding_bag_4bit_prepack; even D)
POOL_SUM, POOL_MEAN = 0, 1                      # option "sls_pool": a bag's pooled vector is its sum | its mean (the fp32 sum / length)
MLP_FP32, MLP_BF16 = 0, 2                       # option "mlp_dtype": arithmetic of the FC layers with K, N >= 64 (bf16 operands, fp32 accumulation)
ACT_NONE, ACT_RELU, ACT_SIGMOID = 0, 1, 2
MLP_BOT, MLP_TOP, MLP_FINAL = 0, 1, 2
MLP_TASK0 = 16     # + k: task head k (MT-WnD)
MLP_ATT0 = 1024    # + i: attention unit i (DIN)
MLP_RNN0, MLP_RNN1 = 32, 33   # the two BasicRNN layers (DIEN): layer 0 = i2h, layer 1 = gates_t
KERNEL_SLS, KERNEL_MLP, KERNEL_SLS_CLOCK = 0, 1, 2

_f32p = C.POINTER(C.c_float)
_i32p = C.POINTER(C.c_int32)
_i64p = C.POINTER(C.c_int64)

# every symbol include/drs.h declares: (name, restype, argtypes)
SYMBOLS = [
    ("drs_abi_version", C.c_int32, []),
    ("drs_backend", C.c_char_p, []),
    ("drs_device_count", C.c_int32, [_i32p]),
    ("drs_last_error", C.c_char_p, [C.c_void_p]),
    ("drs_create", C.c_int32, [C.c_void_p, C.c_int32, C.POINTER(C.c_void_p)]),
    ("drs_destroy", C.c_int32, [C.c_void_p]),
    ("drs_set_table", C.c_int32, [C.c_void_p, C.c_int32, _f32p, C.c_int64]),
    ("drs_fill_table_uniform", C.c_int32, [C.c_void_p, C.c_int32, C.c_float, C.c_float, C.c_uint64]),
    ("drs_set_fc", C.c_int32, [C.c_void_p, C.c_int32, C.c_int32, _f32p, _f32p, C.c_int32, C.c_int32]),
    ("drs_stage_batch", C.c_int32, [C.c_void_p, C.c_int32, C.c_int32, _f32p, C.POINTER(_i64p), _i64p,
                                    C.POINTER(_i32p)]),
    ("drs_forward", C.c_int32, [C.c_void_p, C.c_int32, C.c_int32, _f32p]),
    ("drs_forward_async", C.c_int32, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32]),
    ("drs_forward_multi_async", C.c_int32, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    ("drs_wait", C.c_int32, [C.c_void_p, C.c_int32, _f32p, C.c_int64]),
    ("drs_sync", C.c_int32, [C.c_void_p]),
    ("drs_forward_inputs_async", C.c_int32, [C.c_void_p, C.c_int32, C.c_int32, _f32p, C.POINTER(_i64p), _i64p,
                                             C.POINTER(_i32p)]),
    ("drs_forward_inputs", C.c_int32, [C.c_void_p, C.c_int32, C.c_int32, _f32p, C.POINTER(_i64p), _i64p,
                                       C.POINTER(_i32p), _f32p]),
    ("drs_run_queues_async", C.c_int32, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64,
                                         C.c_int64, C.c_void_p, C.c_int64]),
    ("drs_run_queues_multi_async", C.c_int32, [C.c_void_p, C.c_int32, C.c_int32, _i32p, C.POINTER(C.c_void_p),
                                               C.POINTER(C.c_void_p), _i64p, _i64p, C.POINTER(C.c_void_p), _i64p]),
    ("drs_fetch_interaction", C.c_int32, [C.c_void_p, C.c_int32, C.c_int32, _f32p]),
    ("drs_out_width", C.c_int32, [C.c_void_p, _i32p]),
    ("drs_interaction_width", C.c_int32, [C.c_void_p, _i32p]),
    ("drs_sls", C.c_int32, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p,
                            C.c_int64, C.c_int64, C.c_void_p, C.c_int32]),
    ("drs_fc", C.c_int32, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p,
                           C.c_int32, C.c_int32, C.c_void_p]),
    ("drs_interact_dot", C.c_int32, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32,
                                     C.c_int32, C.c_void_p]),
    ("drs_set_option", C.c_int32, [C.c_void_p, C.c_char_p, C.c_int64]),
    ("drs_get_option", C.c_int32, [C.c_void_p, C.c_char_p, _i64p]),
    ("drs_set_profiling", C.c_int32, [C.c_void_p, C.c_int32]),
    ("drs_kernel_time", C.c_int32, [C.c_void_p, C.c_int32, C.POINTER(C.c_double), _i64p]),
    ("drs_reset_kernel_time", C.c_int32, [C.c_void_p]),
    ("drs_kernel_bytes", C.c_int32, [C.c_void_p, C.c_int32, _i64p]),
    ("drs_debug_gather_stamps", C.c_int32, [C.c_void_p, C.c_int32, C.POINTER(C.c_uint64), C.c_int64, _i64p]),
    ("drs_gather_bytes", C.c_int32, [C.c_void_p, C.c_int32, C.c_int32, _i64p]),
    ("drs_last_dispatch", C.c_int32, [C.c_void_p, C.c_int32, C.c_char_p, C.c_int64]),
    ("drs_comm_unique_id", C.c_int32, [C.POINTER(C.c_uint8)]),
    ("drs_comm_create", C.c_int32, [C.POINTER(C.c_uint8), C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]),
    ("drs_comm_destroy", C.c_int32, [C.c_void_p]),
    ("drs_comm_barrier", C.c_int32, [C.c_void_p]),
    ("drs_stats_allreduce", C.c_int32, [C.c_void_p, _i64p, C.c_int32, C.POINTER(C.c_double)]),
    ("drs_comm_last_error", C.c_char_p, []),
]
COMM_ID_BYTES = 128
# per-sample weights (SparseLengthsWeightedSum): symbols of the HIP build alone.  SYMBOLS above stays the list every
# implementation of the ABI exports (the CPU restatement binds it); lib() binds these on top of it.
WEIGHT_SYMBOLS = [
    ("drs_stage_batch_weights", C.c_int32, [C.c_void_p, C.c_int32, C.POINTER(_f32p), _i64p]),
    ("drs_sls_weighted", C.c_int32, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_int64, C.c_int64, C.c_void_p, C.c_int32]),
]


# fp8 e4m3 tables ("table_dtype" 4): the read-back of a table's scale exponent, include/drs_fp8.h -- the HIP build alone, as above
FP8_SYMBOLS = [
    ("drs_table_fp8_exponent", C.c_int32, [C.c_void_p, C.c_int32, _i32p]),
]

# single table rows, written and read back in the stored type (include/drs_rows.h) -- the HIP build alone, as above
ROW_SYMBOLS = [
    ("drs_update_rows", C.c_int32, [C.c_void_p, C.c_int32, C.c_int64, _i64p, _f32p]),
    ("drs_get_rows", C.c_int32, [C.c_void_p, C.c_int32, C.c_int64, _i64p, _f32p]),
]

# launch sets whose per-query arrays are device arrays (include/drs_device_inputs.h) -- the HIP build alone, as above
DEVICE_INPUT_SYMBOLS = [
    ("drs_run_queues_device_multi_async", C.c_int32, [C.c_void_p, C.c_int32, C.c_int32, _i32p, C.POINTER(C.c_void_p),
                                                      C.POINTER(C.c_void_p), _i64p, _i64p, C.POINTER(C.c_void_p), _i64p, _i32p]),
    ("drs_run_queues_device_async", C.c_int32, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64,
                                                C.c_int64, C.c_void_p, C.c_int64, C.c_int32]),
]

# ... and whose results stay on the device, ordered on a stream of the caller's (include/drs_device_outputs.h) -- the HIP build alone
DEVICE_OUTPUT_SYMBOLS = [
    ("drs_run_queues_device_io_multi_async", C.c_int32, DEVICE_INPUT_SYMBOLS[0][2] + [C.POINTER(C.c_void_p), _i64p, C.c_void_p,
                                                                                     C.c_int32]),
    ("drs_run_queues_device_io_async", C.c_int32, DEVICE_INPUT_SYMBOLS[1][2] + [C.c_void_p, C.c_int64, C.c_void_p, C.c_int32]),
]

# ... and both forms with per-sample weights as device arrays (include/drs_device_weights.h) -- the HIP build alone
DEVICE_WEIGHT_SYMBOLS = [
    ("drs_run_queues_device_weighted_multi_async", C.c_int32, DEVICE_INPUT_SYMBOLS[0][2] + [
        C.POINTER(C.c_void_p), _i64p, _i32p, C.POINTER(C.c_void_p), _i64p, C.c_void_p, C.c_int32]),
]
# single table rows updated and read back from device arrays (include/drs_device_rows.h) -- the HIP build alone, as above
DEVICE_ROW_SYMBOLS = [
    ("drs_update_rows_device", C.c_int32, [C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p,
                                           C.c_int32]),
    ("drs_get_rows_device", C.c_int32, [C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32]),
]
DEVICE_ROWS_MAX = 1 << 24      # DRS_DEVICE_ROWS_MAX: the most rows one device call names
# each query's top-k rows by one score column, one launch per set (include/drs_device_topk.h) -- the HIP build alone, as above
DEVICE_TOPK_SYMBOLS = [
    ("drs_topk_rows", C.c_int32, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                  C.c_void_p]),
    ("drs_run_queues_device_topk_multi_async", C.c_int32, DEVICE_INPUT_SYMBOLS[0][2] + [
        C.POINTER(C.c_void_p), _i64p, _i32p, _i32p, C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_void_p, C.c_int32]),
]
TOPK_MAX = 1024                # DRS_TOPK_MAX: the most rows one query hands back

# the codes of a weight array's element type (wgt_dtype: the DRS_TABLE_* codes of the three float types)
WEIGHT_FP32, WEIGHT_FP16, WEIGHT_BF16 = 0, 1, 2


class ModelCfg(C.Structure):
    _fields_ = [
        ("model_kind", C.c_int32), ("num_tables", C.c_int32), ("table_rows", _i64p),
        ("sparse_dim", C.c_int32), ("n_bot", C.c_int32), ("ln_bot", _i32p),
        ("n_top", C.c_int32), ("ln_top", _i32p),
        ("interaction_op", C.c_int32), ("interaction_itself", C.c_int32),
        ("sigmoid_top", C.c_int32), ("max_batch", C.c_int32), ("max_lookups", C.c_int32),
        ("num_staged_batches", C.c_int32), ("num_slots", C.c_int32),
        ("n_task", C.c_int32), ("ln_task", _i32p), ("num_tasks", C.c_int32),
    ]


class DrsError(RuntimeError):
    def __init__(self, code, what, detail=""):
        super().__init__("%s failed with status %d%s" % (what, code, (": " + detail) if detail else ""))
        self.code = code
        self.detail = detail


_lib = None


def is_lab():
    """the lab build of the library (make -C deeprecsys_amd/csrc lab-lib; -DDRS_LAB) is bound: it also takes the lab's
    instruments and the options of the forms that lost their measurement (docs/OPTIONS.md, last section)"""
    return os.path.basename(LIB_PATH).startswith("libdrs_hip_lab")


def lib():
    """Load libdrs_hip.so (built by __graft_entry__.build() / csrc/Makefile)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                "%s is missing: build it with `make -C deeprecsys_amd/csrc` (hipcc, gfx950). "
                "deeprecsys_amd has no CPU fallback." % LIB_PATH)
        L = C.CDLL(LIB_PATH)
        for name, res, args in SYMBOLS:
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        backend = L.drs_backend() or b""
        if not backend.startswith(b"hip:"):
            raise ImportError("%s identifies itself as %r: deeprecsys_amd binds the HIP build only "
                              "(the CPU restatement of the ABI is test infrastructure)" % (LIB_PATH, backend))
        for name, res, args in (WEIGHT_SYMBOLS + FP8_SYMBOLS + ROW_SYMBOLS + DEVICE_INPUT_SYMBOLS + DEVICE_OUTPUT_SYMBOLS +
                                DEVICE_WEIGHT_SYMBOLS + DEVICE_ROW_SYMBOLS + DEVICE_TOPK_SYMBOLS):     # (the HIP build alone exports these)
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def device_count():
    n = C.c_int32(0)
    rc = lib().drs_device_count(C.byref(n))
    return int(n.value) if rc == OK else 0


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


class Engine(object):
    """Thin object wrapper over a drs_handle (one GPU, one process)."""

    def __init__(self, kind, table_rows, sparse_dim, ln_bot, ln_top, interaction_op=INTERACT_CAT,
                 interaction_itself=False, sigmoid_top=-1, max_batch=1, max_lookups=1,
                 num_staged_batches=1, num_slots=1, device=0, ln_task=None, num_tasks=0):
        L = lib()
        self._rows = np.ascontiguousarray(table_rows, dtype=np.int64)
        self._ln_bot = np.ascontiguousarray(ln_bot, dtype=np.int32)
        self._ln_top = np.ascontiguousarray(ln_top, dtype=np.int32)
        cfg = ModelCfg(kind, self._rows.size, self._rows.ctypes.data_as(_i64p), int(sparse_dim),
                       self._ln_bot.size, self._ln_bot.ctypes.data_as(_i32p),
                       self._ln_top.size, self._ln_top.ctypes.data_as(_i32p),
                       int(interaction_op), int(bool(interaction_itself)), int(sigmoid_top),
                       int(max_batch), int(max_lookups), int(num_staged_batches), int(num_slots))
        if ln_task is not None:
            self._ln_task = np.ascontiguousarray(ln_task, dtype=np.int32)
            cfg.n_task, cfg.ln_task, cfg.num_tasks = self._ln_task.size, self._ln_task.ctypes.data_as(_i32p), int(num_tasks)
        h = C.c_void_p()
        rc = L.drs_create(C.byref(cfg), int(device), C.byref(h))
        if rc != OK:
            raise DrsError(rc, "drs_create", (L.drs_last_error(None) or b"").decode())
        self._h = h
        self.kind = kind
        self.T = int(self._rows.size)
        self.D = int(sparse_dim)
        self.max_batch = int(max_batch)
        self.max_lookups = int(max_lookups)
        # width of a query's dense rows (drs_create's shape algebra): DLRM / W&D / MT-WnD feed ln_bot[0]
        self.m_den = int(self._ln_bot[0]) if kind in (MODEL_DLRM, MODEL_WND, MODEL_MTWND) else 0
        self.num_slots = int(num_slots)
        self.device = int(device)
        self._marsh = ((C.c_int32 * 64)(), (C.c_int32 * 64)())
        self.user_options = set()        # option keys the caller set (set_option)
        # the per-slot record of the kernel forms a launch set took (last_dispatch) costs the host ~1 us per set: off
        # unless asked for -- DRS_DISPATCH_LOG=1 (tests/conftest.py sets it) or set_option("dispatch_log", 1)
        if os.environ.get("DRS_DISPATCH_LOG", "0") not in ("", "0"):
            self.set_option("dispatch_log", 1)

    # -- helpers ------------------------------------------------------------------
    def _check(self, rc, what):
        if rc != OK:
            raise DrsError(rc, what, (lib().drs_last_error(self._h) or b"").decode())

    def close(self):
        if getattr(self, "_h", None):
            lib().drs_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def n_out(self):
        n = C.c_int32(0)
        lib().drs_out_width(self._h, C.byref(n))
        return int(n.value)

    @property
    def num_int(self):
        n = C.c_int32(0)
        lib().drs_interaction_width(self._h, C.byref(n))
        return int(n.value)

    # -- parameters ---------------------------------------------------------------
    def set_table(self, t, W):
        W = _f32(W)
        self._check(lib().drs_set_table(self._h, t, W.ctypes.data_as(_f32p), W.shape[0]), "drs_set_table")

    def fill_table_uniform(self, t, lo, hi, seed):
        self._check(lib().drs_fill_table_uniform(self._h, t, lo, hi, seed), "drs_fill_table_uniform")

    def table_fp8_exponent(self, t):
        """k of table t under "table_dtype" 4: its stored codes are e4m3_rne(x * 2**k), served as decode(code) * 2**-k
        (ERR_UNSUPPORTED unless the tables are fp8)."""
        k = C.c_int32(0)
        self._check(lib().drs_table_fp8_exponent(self._h, int(t), C.byref(k)), "drs_table_fp8_exponent")
        return int(k.value)

    def update_rows(self, t, ids, values):
        """Rows `ids` (int64 [n]) of table t become `values` (fp32 [n, D]), stored as set_table would store them in the
        tables' current type and layout (fp8: under the table's existing scale).  A repeated id takes its last row.  Drains
        the engine first."""
        ids = np.ascontiguousarray(ids, dtype=np.int64)
        values = _f32(values)
        if ids.ndim != 1 or values.shape != (ids.size, self.D):
            raise ValueError("ids [n] and values [n, %d]: got %r and %r" % (self.D, ids.shape, values.shape))
        self._check(lib().drs_update_rows(self._h, int(t), ids.size, ids.ctypes.data_as(_i64p), values.ctypes.data_as(_f32p)),
                    "drs_update_rows")

    def get_rows(self, t, ids):
        """-> fp32 [n, D]: what each of rows `ids` (int64 [n], any order, repeats allowed) of table t serves as a one-row bag."""
        ids = np.ascontiguousarray(ids, dtype=np.int64)
        if ids.ndim != 1:
            raise ValueError("ids [n]: got %r" % (ids.shape,))
        out = np.empty((ids.size, self.D), dtype=np.float32)
        self._check(lib().drs_get_rows(self._h, int(t), ids.size, ids.ctypes.data_as(_i64p), out.ctypes.data_as(_f32p)),
                    "drs_get_rows")
        return out

    def update_rows_device(self, t, ids_ptr, n, val_ptr, row_stride, dtype, stream=None):
        """update_rows for ids and values that are DEVICE arrays on the engine's GPU (drs_update_rows_device): ids_ptr -> n
        contiguous int64, val_ptr -> [n, D] elements of `dtype` (TABLE_FP32, TABLE_FP16 or TABLE_BF16), rows `row_stride`
        elements apart.  stream None: the arrays are complete (`ordered` 0); a stream handle (0: HIP's null stream): the
        passes run behind what is enqueued there (`ordered` 1).  Returns when the rows are in the table."""
        self._check(lib().drs_update_rows_device(self._h, int(t), int(n), C.c_void_p(int(ids_ptr)), C.c_void_p(int(val_ptr)), int(row_stride),
                                                 int(dtype), C.c_void_p(0 if stream is None else int(stream)), 0 if stream is None else 1),
                    "drs_update_rows_device")

    def get_rows_device(self, t, ids_ptr, n, out_ptr, row_stride, stream=None):
        """get_rows into a DEVICE array (drs_get_rows_device): out_ptr -> [n, D] float32, rows `row_stride` floats apart;
        ids_ptr and stream as update_rows_device.  Returns when out is written."""
        self._check(lib().drs_get_rows_device(self._h, int(t), int(n), C.c_void_p(int(ids_ptr)), C.c_void_p(int(out_ptr)), int(row_stride),
                                              C.c_void_p(0 if stream is None else int(stream)), 0 if stream is None else 1),
                    "drs_get_rows_device")

    def set_fc(self, mlp, layer, W, b):
        W, b = _f32(W), _f32(b)
        self._check(lib().drs_set_fc(self._h, mlp, layer, W.ctypes.data_as(_f32p),
                                     b.ctypes.data_as(_f32p), W.shape[0], W.shape[1]), "drs_set_fc")

    # -- inputs -------------------------------------------------------------------
    @staticmethod
    def _pack_sparse(idx, lengths):
        """-> (idx, lengths, n_idx, T pointers, T pointers).  Fast path: the reference's feeder
        hands run_queues 2-D arrays (ids [T, bs*L] int64, lengths [T, bs] int32, rows possibly
        strided slices of the pre-generated sets, inferenceEngine.py:200-206); their row pointers
        are base + t * stride -- no per-table Python objects on the per-query path."""
        if (isinstance(idx, np.ndarray) and idx.ndim == 2 and idx.dtype == np.int64 and idx.strides[1] == 8 and
                isinstance(lengths, np.ndarray) and lengths.ndim == 2 and lengths.dtype == np.int32 and
                lengths.strides[1] == 4 and lengths.shape[0] == idx.shape[0]):
            T = idx.shape[0]
            steps = np.arange(T, dtype=np.int64)
            ia = (steps * idx.strides[0] + idx.ctypes.data).astype(np.uint64)
            la = (steps * lengths.strides[0] + lengths.ctypes.data).astype(np.uint64)
            n_idx = np.full(T, idx.shape[1], dtype=np.int64)
            # (idx, ia) / (lengths, la): the caller keeps these alive across the C call
            return (idx, ia), (lengths, la), n_idx, ia.ctypes.data_as(C.POINTER(_i64p)), la.ctypes.data_as(C.POINTER(_i32p))
        idx = [np.ascontiguousarray(i, dtype=np.int64) for i in idx]
        lengths = [np.ascontiguousarray(l, dtype=np.int32) for l in lengths]
        T = len(idx)
        n_idx = np.array([i.size for i in idx], dtype=np.int64)
        ip = (_i64p * T)(*[i.ctypes.data_as(_i64p) for i in idx])
        lp = (_i32p * T)(*[l.ctypes.data_as(_i32p) for l in lengths])
        return idx, lengths, n_idx, ip, lp

    def stage_batch(self, batch_id, dense, idx, lengths, weights=None):
        """weights: None (an unweighted batch), or one entry per table -- an fp32 weight per index of that table, or None
        for a table whose weights are all 1.0 (SparseLengthsWeightedSum; staging a batch again drops its weights)."""
        n = int(np.asarray(lengths[0]).size)
        idx, lengths, n_idx, ip, lp = self._pack_sparse(idx, lengths)
        dp = None
        if dense is not None:
            dense = _f32(dense)
            dp = dense.ctypes.data_as(_f32p)
        self._check(lib().drs_stage_batch(self._h, batch_id, n, dp, ip, n_idx.ctypes.data_as(_i64p), lp),
                    "drs_stage_batch")
        if weights is not None:
            self.stage_batch_weights(batch_id, weights)

    def stage_batch_weights(self, batch_id, weights):
        """Attach per-index weights to a batch already staged: one entry per table, an fp32 array as long as that table's
        staged indices, or None (every weight 1.0)."""
        if len(weights) != self.T:
            raise ValueError("one weight array (or None) per table: %d for %d tables" % (len(weights), self.T))
        w = [None if a is None else _f32(a).reshape(-1) for a in weights]
        wp = (_f32p * self.T)(*[None if a is None else a.ctypes.data_as(_f32p) for a in w])
        n_w = np.array([-1 if a is None else a.size for a in w], dtype=np.int64)
        self._check(lib().drs_stage_batch_weights(self._h, batch_id, wp, n_w.ctypes.data_as(_i64p)),
                    "drs_stage_batch_weights")

    # -- hot path -----------------------------------------------------------------
    def forward(self, batch_id, bs):
        out = np.empty((bs, self.n_out), dtype=np.float32)
        self._check(lib().drs_forward(self._h, batch_id, bs, out.ctypes.data_as(_f32p)), "drs_forward")
        return out

    def forward_async(self, slot, batch_id, bs):
        self._check(lib().drs_forward_async(self._h, slot, batch_id, bs), "drs_forward_async")

    def forward_multi_async(self, slot, batch_ids, bss):
        """Coalesce several queries into one set of launches; wait(slot, sum(bss)) returns
        their outputs back to back."""
        # (two preallocated ctypes arrays: 0.7 us to fill against 6.5 us for two numpy conversions + pointer casts,
        #  on a call an engine process makes ~15 000 times a second)
        n = len(batch_ids)
        if n > 64 or n != len(bss):          # (the library enforces DRS_MAX_COALESCE itself)
            raise ValueError("one size per query, at most 64 entries")
        a = self._marsh
        a[0][:n] = batch_ids
        a[1][:n] = bss
        self._check(lib().drs_forward_multi_async(self._h, slot, n, a[0], a[1]), "drs_forward_multi_async")

    def wait(self, slot, bs=None):
        """bs = total samples submitted on the slot (sum over coalesced queries); the library
        checks the buffer against what is really in flight there."""
        if bs is None:
            self._check(lib().drs_wait(self._h, slot, None, 0), "drs_wait")
            return None
        out = np.empty((bs, self.n_out), dtype=np.float32)
        self._check(lib().drs_wait(self._h, slot, out.ctypes.data_as(_f32p), out.size), "drs_wait")
        return out

    def sync(self):
        self._check(lib().drs_sync(self._h), "drs_sync")

    def forward_inputs(self, dense, idx, lengths, bs, slot=0):
        if type(idx) is np.ndarray and idx.ndim == 2:
            self.forward_inputs_async(dense, idx, lengths, bs, slot=slot)
            return self.wait(slot, bs)
        idx, lengths, n_idx, ip, lp = self._pack_sparse(idx, lengths)
        dp = None
        if dense is not None:
            dense = _f32(dense)
            dp = dense.ctypes.data_as(_f32p)
        out = np.empty((bs, self.n_out), dtype=np.float32)
        self._check(lib().drs_forward_inputs(self._h, slot, bs, dp, ip, n_idx.ctypes.data_as(_i64p), lp,
                                             out.ctypes.data_as(_f32p)), "drs_forward_inputs")
        return out

    def forward_inputs_async(self, dense, idx, lengths, bs, slot=0):
        """Enqueue only; wait(slot, bs) returns the result.  The arrays are consumed (converted
        into the slot's pinned block) before this returns."""
        if (type(idx) is np.ndarray and idx.ndim == 2 and idx.dtype == np.int64 and idx.strides[1] == 8 and
                type(lengths) is np.ndarray and lengths.ndim == 2 and lengths.dtype == np.int32 and
                lengths.strides[1] == 4 and lengths.shape[0] == idx.shape[0] == self.T and
                (dense is None or (type(dense) is np.ndarray and dense.dtype == np.float32 and dense.flags.c_contiguous))):
            # the reference feeder's arrays as they are: two base pointers and two row strides
            # (the C side reads lengths[t][0 .. bs) and bs dense rows: check them here, a short array
            # must be a Python error, not a host out-of-bounds read)
            if bs < 0 or bs > lengths.shape[1]:
                raise ValueError("bs=%d but lengths has %d columns" % (bs, lengths.shape[1]))
            if dense is not None and (dense.ndim != 2 or dense.shape[0] < bs or dense.shape[1] != self.m_den):
                raise ValueError("bs=%d, dense width %d, but dense has shape %r" % (bs, self.m_den, dense.shape))
            self._check(lib().drs_run_queues_async(self._h, slot, bs, None if dense is None else dense.ctypes.data,
                                                   idx.ctypes.data, idx.strides[0] // 8, idx.shape[1],
                                                   lengths.ctypes.data, lengths.strides[0] // 4),
                        "drs_run_queues_async")
            return
        idx, lengths, n_idx, ip, lp = self._pack_sparse(idx, lengths)
        dp = None
        if dense is not None:
            dense = _f32(dense)
            dp = dense.ctypes.data_as(_f32p)
        self._check(lib().drs_forward_inputs_async(self._h, slot, bs, dp, ip, n_idx.ctypes.data_as(_i64p), lp),
                    "drs_forward_inputs_async")

    def run_queues_multi_async(self, queries, slot=0):
        """Several waiting requests as ONE launch set: `queries` is a list of (dense, ids, lengths, bs)
        with the arrays as the reference's feeder holds them (ids [T, n] int64, lengths [T, >= bs]
        int32, dense [>= bs, m_den] float32 or None; row slices of bigger arrays are fine).
        wait(slot, sum(bs)) returns the outputs back to back.  The arrays are consumed before this
        returns."""
        n = len(queries)
        bsa = np.empty(n, dtype=np.int32)
        ids_stride = np.empty(n, dtype=np.int64)
        len_stride = np.empty(n, dtype=np.int64)
        n_idx = np.empty(n, dtype=np.int64)
        dp = (C.c_void_p * n)()
        ip = (C.c_void_p * n)()
        lp = (C.c_void_p * n)()
        keep = []
        for i, (dense, idx, lengths, bs) in enumerate(queries):
            if not (type(idx) is np.ndarray and idx.ndim == 2 and idx.dtype == np.int64 and idx.strides[1] == 8):
                idx = np.ascontiguousarray(idx, dtype=np.int64)
            if not (type(lengths) is np.ndarray and lengths.ndim == 2 and lengths.dtype == np.int32 and lengths.strides[1] == 4):
                lengths = np.ascontiguousarray(lengths, dtype=np.int32)
            if idx.ndim != 2 or lengths.ndim != 2 or idx.shape[0] != self.T or lengths.shape[0] != self.T:
                raise ValueError("query %d: ids / lengths must be [T=%d, ...] arrays" % (i, self.T))
            if bs < 0 or bs > lengths.shape[1]:
                raise ValueError("query %d: bs=%d but lengths has %d columns" % (i, bs, lengths.shape[1]))
            if dense is not None:
                if not (type(dense) is np.ndarray and dense.dtype == np.float32 and dense.flags.c_contiguous):
                    dense = np.ascontiguousarray(dense, dtype=np.float32)
                if dense.ndim != 2 or dense.shape[0] < bs or dense.shape[1] != self.m_den:
                    raise ValueError("query %d: bs=%d, dense width %d, but dense has shape %r" % (i, bs, self.m_den, dense.shape))
            keep.append((dense, idx, lengths))
            bsa[i] = bs
            ids_stride[i] = idx.strides[0] // 8
            len_stride[i] = lengths.strides[0] // 4
            n_idx[i] = idx.shape[1]
            dp[i] = None if dense is None else dense.ctypes.data
            ip[i] = idx.ctypes.data
            lp[i] = lengths.ctypes.data
        self._check(lib().drs_run_queues_multi_async(self._h, slot, n, bsa.ctypes.data_as(_i32p), dp, ip,
                                                     ids_stride.ctypes.data_as(_i64p), n_idx.ctypes.data_as(_i64p),
                                                     lp, len_stride.ctypes.data_as(_i64p)),
                    "drs_run_queues_multi_async")

    def run_queues_device_multi_async(self, queries, slot=0, weights=None):
        """run_queues_multi_async for arrays that live in DEVICE memory (include/drs_device_inputs.h): `queries` is a list
        of (bs, dense_ptr, ids_ptr, ids_row_stride, n_idx_per_table, len_ptr, len_row_stride, fixed_len) -- device
        addresses as integers (0 / None: no dense rows), strides in elements, fixed_len >= 0 the promise that every bag
        holds that many indices or -1.  One kernel launch converts and checks the arrays; wait(slot, sum(bs)) returns the
        outputs back to back.  The arrays must be complete now and stay untouched until wait() has returned.
        weights: None, or one entry per query (include/drs_device_weights.h) -- (ptr, row_stride, dtype): the query's
        per-sample weights [T, n_idx_per_table] at that device address, rows row_stride elements apart, dtype WEIGHT_FP32 /
        WEIGHT_FP16 / WEIGHT_BF16; or None: the query is unweighted."""
        if weights is not None:
            args, keep = self._device_set(queries)
            wargs, wkeep = self._device_weights(len(queries), weights)
            self._check(lib().drs_run_queues_device_weighted_multi_async(self._h, slot, *(args + wargs + [None, None, None, 0])),
                        "drs_run_queues_device_weighted_multi_async")
            del keep, wkeep
            return
        self._check(lib().drs_run_queues_device_multi_async(self._h, slot, *self._device_set(queries)[0]),
                    "drs_run_queues_device_multi_async")

    @staticmethod
    def _device_weights(n, weights):
        """the `weights` of run_queues_device_multi_async -> (d_weights, wgt_row_stride, wgt_dtype of the call, the arrays
        they point into)"""
        if len(weights) != n:
            raise ValueError("%d queries, %d weight entries" % (n, len(weights)))
        wp = (C.c_void_p * max(n, 1))()
        stride = np.zeros(max(n, 1), dtype=np.int64)
        dtype = np.zeros(max(n, 1), dtype=np.int32)
        for i, w in enumerate(weights):
            if w is None:
                continue
            ptr, rs, dt = w
            wp[i] = ptr or None
            stride[i], dtype[i] = rs, dt
        return [wp, stride.ctypes.data_as(_i64p), dtype.ctypes.data_as(_i32p)], (stride, dtype)

    @staticmethod
    def _device_set(queries):
        """the tuples of run_queues_device_multi_async -> (the call's arguments from n on, the arrays they point into)"""
        n = len(queries)
        bsa = np.empty(n, dtype=np.int32)
        ids_stride = np.empty(n, dtype=np.int64)
        len_stride = np.empty(n, dtype=np.int64)
        n_idx = np.empty(n, dtype=np.int64)
        fixed = np.empty(n, dtype=np.int32)
        dp = (C.c_void_p * max(n, 1))()
        ip = (C.c_void_p * max(n, 1))()
        lp = (C.c_void_p * max(n, 1))()
        for i, (bs, dense_ptr, ids_ptr, ids_rs, ni, len_ptr, len_rs, fl) in enumerate(queries):
            bsa[i], ids_stride[i], n_idx[i], len_stride[i], fixed[i] = bs, ids_rs, ni, len_rs, fl
            dp[i] = dense_ptr or None
            ip[i] = ids_ptr or None
            lp[i] = len_ptr or None
        keep = (bsa, ids_stride, n_idx, len_stride, fixed)
        return [n, bsa.ctypes.data_as(_i32p), dp, ip, ids_stride.ctypes.data_as(_i64p), n_idx.ctypes.data_as(_i64p), lp,
                len_stride.ctypes.data_as(_i64p), fixed.ctypes.data_as(_i32p)], keep

    def run_queues_device_io_multi_async(self, queries, outs, stream=None, slot=0, weights=None):
        """run_queues_device_multi_async whose results stay in DEVICE memory (include/drs_device_outputs.h): `outs` is a list
        of (ptr, row_stride), one per query -- query i's [bs, n_out] fp32 scores go to the device address ptr, rows
        row_stride floats apart (0 / None: no output, an empty query's).  stream None: `ordered` 0 -- the inputs are complete
        now and the outputs are when wait(slot) has returned.  stream an integer hipStream_t handle (0 is the null stream):
        `ordered` 1 -- the set runs behind what is enqueued on that stream, and what is enqueued there after this call sees
        the outputs; nothing waits on the host.  Inputs and outputs must stay alive and untouched until wait(slot).
        weights: as in run_queues_device_multi_async."""
        if len(outs) != len(queries):
            raise ValueError("%d queries, %d outputs" % (len(queries), len(outs)))
        args, keep = self._device_set(queries)
        n = len(outs)
        op = (C.c_void_p * max(n, 1))()
        out_stride = np.empty(n, dtype=np.int64)
        for i, (ptr, rs) in enumerate(outs):
            op[i] = ptr or None
            out_stride[i] = rs
        if weights is not None:
            wargs, wkeep = self._device_weights(len(queries), weights)
            self._check(lib().drs_run_queues_device_weighted_multi_async(self._h, slot, *(args + wargs + [
                op, out_stride.ctypes.data_as(_i64p), None if stream is None else (int(stream) or None), 0 if stream is None else 1])),
                "drs_run_queues_device_weighted_multi_async")
            del wkeep
            return
        self._check(lib().drs_run_queues_device_io_multi_async(self._h, slot, *(args + [
            op, out_stride.ctypes.data_as(_i64p), None if stream is None else (int(stream) or None), 0 if stream is None else 1])),
            "drs_run_queues_device_io_multi_async")

    def run_queues_device_topk_multi_async(self, queries, k, col, tops, stream=None, slot=0, weights=None):
        """run_queues_device_io_multi_async that hands back each query's top-k rows instead of every score
        (include/drs_device_topk.h): `k` one count per query (0..min(bs, TOPK_MAX)), `col` the score column the rows rank by,
        `tops` a list of (idx_ptr, scores_ptr), one per query -- the device addresses of query i's int32 [k_i] row numbers
        and float32 [k_i, n_out] score rows (0 / None where k_i is 0).  One kernel launch per set ranks every query; NaN first,
        equal scores by the lower row.  stream, slot, weights and the lifetime rule: as in run_queues_device_io_multi_async."""
        if len(k) != len(queries) or len(tops) != len(queries):
            raise ValueError("%d queries, %d counts, %d outputs" % (len(queries), len(k), len(tops)))
        args, keep = self._device_set(queries)
        n = len(queries)
        ka = np.zeros(max(n, 1), dtype=np.int32)
        ka[:n] = k
        ip = (C.c_void_p * max(n, 1))()
        sp = (C.c_void_p * max(n, 1))()
        for i, (iptr, sptr) in enumerate(tops):
            ip[i] = iptr or None
            sp[i] = sptr or None
        wkeep = None
        wargs = [None, None, None]
        if weights is not None:
            wargs, wkeep = self._device_weights(n, weights)
        self._check(lib().drs_run_queues_device_topk_multi_async(self._h, slot, *(args + wargs + [
            ka.ctypes.data_as(_i32p), int(col), ip, sp, None if stream is None else (int(stream) or None), 0 if stream is None else 1])),
            "drs_run_queues_device_topk_multi_async")
        del keep, wkeep

    def topk_rows(self, scores_ptr, rows, n_out, row_stride, col, k, idx_ptr, top_ptr, stream=None):
        """The top-k pass on a device array of the caller's (drs_topk_rows): scores_ptr -> [rows, n_out] float32, rows
        `row_stride` floats apart; the k rows that rank first by column `col` go to top_ptr as [k, n_out] float32 and their
        row numbers to idx_ptr as int32 [k].  Enqueued on `stream` (an integer hipStream_t handle; None / 0: the null stream);
        returns at once."""
        self._check(lib().drs_topk_rows(self._h, C.c_void_p(int(scores_ptr or 0)), int(rows), int(n_out), int(row_stride), int(col), int(k),
                                        C.c_void_p(int(idx_ptr or 0)), C.c_void_p(int(top_ptr or 0)),
                                        None if not stream else C.c_void_p(int(stream))), "drs_topk_rows")

    def fetch_interaction(self, bs, slot=0):
        R = np.empty((bs, self.num_int), dtype=np.float32)
        self._check(lib().drs_fetch_interaction(self._h, slot, bs, R.ctypes.data_as(_f32p)),
                    "drs_fetch_interaction")
        return R

    # -- operator level (device pointers, e.g. torch.Tensor.data_ptr()) -------------
    def sls(self, d_W, rows, D, d_idx, d_len, n_bags, n_idx, d_out, exact_order=True, wgt_ptr=None):
        """wgt_ptr: device pointer to one fp32 weight per index (SparseLengthsWeightedSum), or None."""
        if wgt_ptr is not None:
            self._check(lib().drs_sls_weighted(self._h, d_W, rows, D, d_idx, wgt_ptr, d_len, n_bags, n_idx, d_out,
                                               int(bool(exact_order))), "drs_sls_weighted")
            return
        self._check(lib().drs_sls(self._h, d_W, rows, D, d_idx, d_len, n_bags, n_idx, d_out,
                                  int(bool(exact_order))), "drs_sls")

    def fc(self, d_x, M, K, d_W, d_b, N, act, d_y):
        self._check(lib().drs_fc(self._h, d_x, M, K, d_W, d_b, N, act, d_y), "drs_fc")

    def interact_dot(self, d_T, B, F, D, itself, d_R):
        self._check(lib().drs_interact_dot(self._h, d_T, B, F, D, int(bool(itself)), d_R),
                    "drs_interact_dot")

    # -- tuning / measurement -------------------------------------------------------
    def set_option(self, key, value, user=True):
        """user=False: a setting the host code makes on its own behalf (DLRM_Net.tune_table_placement) -- keys set with
        user=True are remembered in `user_options`, and the search leaves those alone."""
        self._check(lib().drs_set_option(self._h, key.encode(), int(value)), "drs_set_option")
        if user:
            self.user_options.add(key)

    def get_option(self, key):
        v = C.c_int64(0)
        self._check(lib().drs_get_option(self._h, key.encode(), C.byref(v)), "drs_get_option")
        return int(v.value)

    def kernel_bytes(self, kernel):
        """Algorithmic gather bytes of exactly the launches kernel_time(kernel) has timed."""
        b = C.c_int64(0)
        self._check(lib().drs_kernel_bytes(self._h, kernel, C.byref(b)), "drs_kernel_bytes")
        return int(b.value)

    def set_profiling(self, level):
        """0 off | 1 device clock stamps of the gather launch (free) | 2 also HIP events."""
        self._check(lib().drs_set_profiling(self._h, int(level)), "drs_set_profiling")

    def kernel_time(self, kernel):
        ms, n = C.c_double(0), C.c_int64(0)
        self._check(lib().drs_kernel_time(self._h, kernel, C.byref(ms), C.byref(n)), "drs_kernel_time")
        return float(ms.value), int(n.value)

    def reset_kernel_time(self):
        self._check(lib().drs_reset_kernel_time(self._h), "drs_reset_kernel_time")

    def gather_stamps(self, slot=0, cap=1 << 16):
        buf = np.zeros(2 * cap, dtype=np.uint64)
        n = C.c_int64(0)
        self._check(lib().drs_debug_gather_stamps(self._h, slot, buf.ctypes.data_as(C.POINTER(C.c_uint64)),
                                                  2 * cap, C.byref(n)), "drs_debug_gather_stamps")
        return buf[:2 * n.value].reshape(-1, 2)

    def last_dispatch(self, slot=0):
        """Which kernels served the launch set last enqueued on `slot`: list of "name<form>[...]" tokens."""
        buf = C.create_string_buffer(1024)
        self._check(lib().drs_last_dispatch(self._h, slot, buf, 1024), "drs_last_dispatch")
        import re
        return re.findall(r"[\w]+(?:<[^>]*>)?(?:\[[^\]]*\])?", buf.value.decode())

    def gather_bytes(self, batch_id, bs):
        b = C.c_int64(0)
        self._check(lib().drs_gather_bytes(self._h, batch_id, bs, C.byref(b)), "drs_gather_bytes")
        return int(b.value)


class Comm(object):
    """RCCL communicator behind the C ABI: the run's single collective (drs_stats_allreduce).
    rank 0 creates the id (Comm.unique_id()), the caller ships the 128 bytes to the other
    ranks, every rank then constructs Comm(id, rank, world, device)."""

    @staticmethod
    def unique_id():
        buf = (C.c_uint8 * COMM_ID_BYTES)()
        rc = lib().drs_comm_unique_id(buf)
        if rc != OK:
            raise DrsError(rc, "drs_comm_unique_id", (lib().drs_comm_last_error() or b"").decode())
        return bytes(buf)

    def __init__(self, uid, rank, world, device):
        buf = (C.c_uint8 * COMM_ID_BYTES).from_buffer_copy(uid)
        h = C.c_void_p()
        rc = lib().drs_comm_create(buf, int(rank), int(world), int(device), C.byref(h))
        if rc != OK:
            raise DrsError(rc, "drs_comm_create", (lib().drs_comm_last_error() or b"").decode())
        self._h, self.rank, self.world = h, int(rank), int(world)

    def _check(self, rc, what):
        if rc != OK:
            raise DrsError(rc, what, (lib().drs_comm_last_error() or b"").decode())

    def barrier(self):
        self._check(lib().drs_comm_barrier(self._h), "drs_comm_barrier")

    def stats_allreduce(self, hist, sum_min_max):
        """hist int64[n] SUM; sum_min_max float64[4]: [0],[1] SUM, [2] MIN, [3] MAX.  Returns copies."""
        h = np.ascontiguousarray(hist, dtype=np.int64).copy()
        s = np.ascontiguousarray(sum_min_max, dtype=np.float64).copy()
        assert s.size == 4
        self._check(lib().drs_stats_allreduce(self._h, h.ctypes.data_as(_i64p), h.size,
                                              s.ctypes.data_as(C.POINTER(C.c_double))), "drs_stats_allreduce")
        return h, s

    def close(self):
        if getattr(self, "_h", None):
            lib().drs_comm_destroy(self._h)
            self._h = None
