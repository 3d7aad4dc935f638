"""CPU side of fp8 e4m3 embedding tables (engine option "table_dtype" 4): the checker the GPU tests stand on
(`fp8_decoded`, torch's float8_e4m3fn under the per-table power-of-two scale), the --accel_table_dtype fp8_e4m3 flag and
the order in which the host code sets the option, and the documents."""
import math
import os
import re

import numpy as np
import pytest
import torch

from deeprecsys_amd import _native as N
from deeprecsys_amd import dlrm_s_hip
from deeprecsys_amd.utils.utils import FLAG_CHOICES, cli
from tests import helpers as H
from tests.test_half_tables_cpu import _Recorder

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def fp8_exponent(absmax):
    """The largest k with absmax * 2**k <= 448, clamped to [-64, 64]; 0 for an all-zero table."""
    absmax = float(np.float32(absmax))
    if not absmax > 0.0:
        return 0
    m, e = math.frexp(absmax)                       # absmax = m * 2**e, m in [0.5, 1)
    k = 9 - e if m <= 0.875 else 8 - e
    return max(-64, min(64, k))


def fp8_codes(W):
    """-> (q, k): table W's e4m3 codes as a torch.float8_e4m3fn tensor, and its scale exponent."""
    W = np.ascontiguousarray(W, dtype=np.float32)
    fin = np.abs(W[np.isfinite(W)])
    k = fp8_exponent(fin.max() if fin.size else 0.0)
    with np.errstate(over="ignore", invalid="ignore"):
        scaled = W * np.float32(2.0 ** k)           # (a power of two: exact)
    return torch.from_numpy(np.ascontiguousarray(scaled)).to(torch.float8_e4m3fn), k


def fp8_decoded(W):
    """-> (dec, k): what an fp8 engine serves for table W, decode(e4m3_rne(W * 2**k)) * 2**-k, and k."""
    q, k = fp8_codes(W)
    return q.to(torch.float32).numpy() * np.float32(2.0 ** -k), k


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- 1. the checker ---------------------------------------------------------------------------------------------------
def test_all_256_codes_round_trip():
    codes = torch.arange(256, dtype=torch.int32).to(torch.uint8)
    vals = codes.view(torch.float8_e4m3fn).to(torch.float32)
    back = vals.to(torch.float8_e4m3fn).view(torch.uint8)
    nan = torch.isnan(vals)
    assert nan.nonzero().flatten().tolist() == [0x7F, 0xFF]                    # the OCP encoding: two NaNs, no infinity
    assert torch.equal(back[~nan], codes[~nan]) and torch.isnan(back.view(torch.float8_e4m3fn).to(torch.float32)[nan]).all()
    assert float(vals[0x7E]) == 448.0 and float(vals[0x01]) == 2.0 ** -9 and float(vals[0x08]) == 2.0 ** -6


def test_ties_subnormals_and_nan_as_torch_rounds_them():
    def rt(x):
        return float(torch.tensor([x], dtype=torch.float32).to(torch.float8_e4m3fn).to(torch.float32)[0])
    assert rt(17.0) == 16.0 and rt(19.0) == 20.0                               # ties to even
    assert rt(2.0 ** -10) == 0.0 and rt(1.5 * 2.0 ** -10) == 2.0 ** -9         # ... among the subnormals too
    assert rt(448.0) == 448.0 and rt(464.0) == 448.0 and math.isnan(rt(465.0))
    assert math.isnan(rt(float("inf"))) and math.isnan(rt(float("-inf"))) and math.isnan(rt(float("nan")))
    q = torch.tensor([np.nan, np.inf, -np.inf], dtype=torch.float32).to(torch.float8_e4m3fn).view(torch.uint8).tolist()
    assert q == [0x7F, 0x7F, 0xFF]


def test_the_scale_rule_puts_absmax_into_the_top_binade():
    above448 = float(np.nextafter(np.float32(448.0), np.float32(1e9)))
    for absmax in (1.0, 1e-3, 37.0, 0.05, 447.9, 224.0, 3.0e38, 1e-30, 448.0, above448, 0.875, 0.8750001, 7.0):
        k = fp8_exponent(absmax)
        if -64 < k < 64:
            assert 224.0 < float(np.float32(absmax)) * 2.0 ** k <= 448.0, (absmax, k)
            assert float(np.float32(absmax)) * 2.0 ** (k + 1) > 448.0
    assert fp8_exponent(448.0) == 0 and fp8_exponent(above448) == -1 and fp8_exponent(224.0) == 1
    assert fp8_exponent(0.05) == 13 and fp8_exponent(1.0) == 8 and fp8_exponent(0.0) == 0
    assert fp8_exponent(1e-30) == 64 and fp8_exponent(3.0e38) == -64             # clamped
    dec, k = fp8_decoded(np.zeros((3, 4), np.float32))
    assert k == 0 and not dec.any()
    W = np.array([[1.0, -3.0, np.inf, np.nan]], np.float32)                       # absmax over the finite elements
    dec, k = fp8_decoded(W)
    assert k == fp8_exponent(3.0) == 7 and dec[0, 0] == 1.0 and dec[0, 1] == -3.0 and np.isnan(dec[0, 2:]).all()


@pytest.mark.parametrize("D", [4, 64])
@pytest.mark.parametrize("L", [1, 20, 80])
def test_scaling_the_finished_sum_equals_summing_the_scaled_rows(D, L):
    """What the kernels do (sum the decoded codes, multiply the finished sum by 2**-k) against what the fp32 twin does (sum
    the decoded table's rows): the same bits, in sequential fp32 order."""
    rng = np.random.RandomState(D + L)
    for factor in (1.0, 1e-3, 37.0):
        W = (rng.uniform(-1, 1, (200, D)) * factor).astype(np.float32)
        q, k = fp8_codes(W)
        dec, k2 = fp8_decoded(W)
        assert k == k2
        codes = q.to(torch.float32).numpy()
        ix = rng.randint(0, 200, size=L)
        a = np.zeros(D, np.float32)
        b = np.zeros(D, np.float32)
        for r in ix:
            a = a + codes[r]
            b = b + dec[r]
        assert np.array_equal(_bits(a * np.float32(2.0 ** -k)), _bits(b)), (factor, k)


# ---- 2. flag and helper -----------------------------------------------------------------------------------------------
def test_flag_word_and_constant():
    assert cli(["--accel_table_dtype", "fp8_e4m3"]).accel_table_dtype == "fp8_e4m3"
    assert "fp8_e4m3" in FLAG_CHOICES["accel_table_dtype"]
    args = cli([])
    args.accel_table_dtype = "fp8_e4m3"
    assert dlrm_s_hip._table_dtype(args) == N.TABLE_FP8_E4M3 == 4
    for bad in ("fp8", "int8", "int4", "e4m3"):
        with pytest.raises(SystemExit):
            cli(["--accel_table_dtype", bad])
        args.accel_table_dtype = bad
        with pytest.raises(ValueError):
            dlrm_s_hip._table_dtype(args)
    assert [n for n, _, _ in N.FP8_SYMBOLS] == ["drs_table_fp8_exponent"]
    assert "drs_table_fp8_exponent" not in [n for n, _, _ in N.SYMBOLS]          # the frozen list stays what it is


def _calls(monkeypatch, **flags):
    meta, _ = H.load_fixture("dlrm_dot_small")
    args = H.args_from(meta["args"], **flags)
    np.random.seed(args.numpy_rand_seed)
    net = H.NET_CLS[args.model_type](args)
    monkeypatch.setattr(dlrm_s_hip.N, "Engine", _Recorder)
    _Recorder.log = []
    net._create_engine()
    return list(_Recorder.log), net


@pytest.mark.parametrize("init", ["numpy", "device"])
def test_option_precedes_every_table_and_weight_write(monkeypatch, init):
    log, net = _calls(monkeypatch, accel_table_dtype="fp8_e4m3", accel_table_init=init)
    dtype_calls = [i for i, c in enumerate(log) if c[:2] == ("set_option", "table_dtype")]
    writes = [i for i, c in enumerate(log) if c[0] in ("set_table", "fill_table_uniform", "set_fc")]
    creates = [i for i, c in enumerate(log) if c[0] == "create"]
    assert sum(1 for c in log if c[0] in ("set_table", "fill_table_uniform")) == len(net.ln_emb)
    assert dtype_calls and dtype_calls == [c + 1 for c in creates]
    assert all(log[i] == ("set_option", "table_dtype", 4) for i in dtype_calls)
    assert max(dtype_calls) < min(writes)


def test_default_flags_add_no_call(monkeypatch):
    log, _ = _calls(monkeypatch)
    assert not [c for c in log if c[:2] == ("set_option", "table_dtype")]
    assert log == _calls(monkeypatch, accel_table_dtype="fp32")[0]


# ---- 3. documents -----------------------------------------------------------------------------------------------------
def test_documents_name_the_type_and_the_header_declares_the_symbol():
    def read(*p):
        return open(os.path.join(ROOT, *p)).read()
    hdr = read("include", "drs.h")
    assert re.search(r"DRS_TABLE_FP8_E4M3\s*=\s*4\b", hdr) and "DRS_TABLE_INT4_ROWWISE = 9" in hdr
    assert '"table_dtype" 0|1|2|4|8|9' in hdr and '#include "drs_fp8.h"' in hdr
    assert "#define DRS_ABI_VERSION 5" in hdr
    fp8 = read("include", "drs_fp8.h")
    assert re.search(r"int32_t\s+drs_table_fp8_exponent\s*\(\s*drs_handle\s+\w+,\s*int32_t\s+\w+,\s*int32_t\s*\*\s*\w+\s*\)\s*;", fp8)
    for doc in (read("docs", "OPTIONS.md"), read("README.md")):
        assert "DRS_TABLE_FP8_E4M3" in doc and "fp8_e4m3" in doc
    assert "drs_fill_table_uniform" in read("docs", "OPTIONS.md") and "448" in read("docs", "OPTIONS.md")
