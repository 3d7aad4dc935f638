"""CPU side of the line-packed int8 rowwise layout (engine option "table_int8_lines"): the --accel_table_int8_lines flag
and when the host code sets the option, the layout rule of docs/OPTIONS.md restated in numpy (no row crosses a 128-byte
line), and the multiply-and-shift quotient the gather kernels take for r / n."""
import os

import numpy as np
import pytest

from deeprecsys_amd import _native as N
from deeprecsys_amd import dlrm_s_hip
from deeprecsys_amd.utils.utils import FLAG_CHOICES, cli
from tests import helpers as H
from tests.test_bf16_mlp_cpu import _Recorder

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DS = [4, 8, 12, 16, 24, 28, 32, 40, 48, 56, 64, 100, 120, 128]


# ---- the layout, restated -------------------------------------------------------------------------------------------
def row_bytes(D):
    """S: D codes, zero padding to a multiple of 8, fp32 scale, fp32 bias."""
    return (D + 7) // 8 * 8 + 8


def rows_per_line(D, lines):
    """n rows share a 128-byte line; 0: the plain layout (option off, S divides 128, or S >= 128)."""
    S = row_bytes(D)
    return 128 // S if lines and S < 128 and 128 % S else 0


def row_offsets(rows, D, lines):
    """byte offset of every row inside its table"""
    S, n, r = row_bytes(D), rows_per_line(D, lines), np.arange(rows, dtype=np.int64)
    return r // n * 128 + r % n * S if n else r * S


def table_bytes(rows, D, lines):
    S, n = row_bytes(D), rows_per_line(D, lines)
    used = (rows + n - 1) // n * 128 if n else rows * S
    return (used + 255) // 256 * 256


def quotient_constants(n):
    """(multiplier, shift): r // n == (r * multiplier) >> shift for every 32-bit r; the kernels take the high half of
    the product (v_mul_hi_u32) and shift by shift - 32."""
    lg = int(np.ceil(np.log2(n)))
    return -(-(1 << (31 + lg)) // n), 31 + lg


def piece_offset(r, D, lines):
    """where the kernels find row r, in 4-byte pieces: r * PR + (r / n) * pad"""
    S, n = row_bytes(D), rows_per_line(D, lines)
    PR = S // 4
    if not n:
        return r * PR
    pad = 32 - n * PR
    if n == 1:
        return r * PR + r * pad
    mul, shift = quotient_constants(n)
    return r * PR + ((r * mul) >> shift) * pad


# ---- flag -----------------------------------------------------------------------------------------------------------
def test_flag_defaults_to_off_and_takes_0_or_1():
    assert cli([]).accel_table_int8_lines == 0
    for v in (0, 1):
        assert cli(["--accel_table_int8_lines", str(v)]).accel_table_int8_lines == v
    assert FLAG_CHOICES["accel_table_int8_lines"] == (0, 1)
    for bad in ("2", "-1", "yes"):
        with pytest.raises(SystemExit):
            cli(["--accel_table_int8_lines", bad])
    args = cli([])
    for bad in (2, -1, 8):
        args.accel_table_int8_lines = bad                        # (a JSON config can set anything: refused at engine build)
        with pytest.raises(ValueError):
            dlrm_s_hip._table_int8_lines(args)
    args.accel_table_int8_lines = 1
    assert dlrm_s_hip._table_int8_lines(args) == 1


def _engine_calls(monkeypatch, **flags):
    meta, _ = H.load_fixture("dlrm_dot_small")
    args = H.args_from(meta["args"], **flags)
    np.random.seed(args.numpy_rand_seed)
    net = H.NET_CLS[args.model_type](args)
    monkeypatch.setattr(dlrm_s_hip.N, "Engine", _Recorder)
    _Recorder.log = []
    net._create_engine()
    return list(_Recorder.log)


def test_with_the_flag_the_option_precedes_table_dtype_and_every_table_write(monkeypatch):
    log = _engine_calls(monkeypatch, accel_table_dtype="int8_rowwise", accel_table_int8_lines=1)
    lines = [i for i, c in enumerate(log) if c[:2] == ("set_option", "table_int8_lines")]
    dtype = [i for i, c in enumerate(log) if c[:2] == ("set_option", "table_dtype")]
    creates = [i for i, c in enumerate(log) if c[0] == "create"]
    writes = [i for i, c in enumerate(log) if c[0] in ("set_table", "fill_table_uniform")]
    assert writes and lines and lines == [c + 1 for c in creates] and dtype == [c + 2 for c in creates]
    assert all(log[i] == ("set_option", "table_int8_lines", 1) for i in lines)
    assert all(log[i] == ("set_option", "table_dtype", N.TABLE_INT8_ROWWISE) for i in dtype)
    assert max(dtype) < min(writes)


@pytest.mark.parametrize("flags", [{}, {"accel_table_dtype": "int8_rowwise"}, {"accel_table_dtype": "fp16"},
                                   {"accel_mlp_dtype": "bf16", "accel_mlp_bf16_fuse": 1}])
def test_without_the_flag_the_calls_are_todays(monkeypatch, flags):
    """The CPU restatement of the ABI does not know the key: only a user who asked for it may reach it.  With the flag
    absent or 0 the engine sees exactly the calls it sees with the flag set, but for the one that sets the key."""
    base = _engine_calls(monkeypatch, **flags)
    assert [c for c in base if c[0] == "set_fc"]
    assert [c for c in base if c[:2] == ("set_option", "table_int8_lines")] == []
    assert _engine_calls(monkeypatch, accel_table_int8_lines=0, **flags) == base
    with_flag = _engine_calls(monkeypatch, accel_table_int8_lines=1, **flags)
    assert [c for c in with_flag if c[:2] != ("set_option", "table_int8_lines")] == base


def test_default_flags_set_nothing_on_the_cpu_abi(cpu_abi):
    meta, _ = H.load_fixture("dlrm_dot_small")
    net, lX, lS_l, lS_i, lT = H.materialize(H.args_from(meta["args"]))
    net.create(lX[0], lS_l[0], lS_i[0], lT[0])
    try:
        assert "table_int8_lines" not in net.engine.user_options
    finally:
        net.engine.close()


# ---- layout -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", DS)
def test_no_row_crosses_a_line_rows_do_not_overlap_and_stay_aligned(D):
    S, n = row_bytes(D), rows_per_line(D, 1)
    for rows in (1, 2, 3, 5, 6, 7, 1000, 3001):
        off = row_offsets(rows, D, 1)
        assert np.all(off % 8 == 0)
        assert np.all(np.diff(off) >= S)                                     # ascending, no overlap
        assert off[-1] + S <= table_bytes(rows, D, 1)
        if n:
            assert np.all(off // 128 == (off + S - 1) // 128), "a row crosses a 128-byte line"
            assert np.all(off % 128 + S <= n * S)                            # the last 128 - n S bytes of a line hold no row
            assert table_bytes(rows, D, 1) == ((rows + n - 1) // n * 128 + 255) // 256 * 256
        else:
            assert np.array_equal(off, row_offsets(rows, D, 0)) and table_bytes(rows, D, 1) == table_bytes(rows, D, 0)
        assert table_bytes(rows, D, 0) == (rows * S + 255) // 256 * 256
        assert np.array_equal(row_offsets(rows, D, 0), np.arange(rows) * S)


def test_the_packed_layout_applies_exactly_where_the_rule_says():
    """S < 128 and 128 % S != 0; n = 128 // S.  The issue's table: D 9..16 -> 5 rows a line, 25..32 -> 3, 33..48 -> 2,
    57..120 -> 1; S in {16, 32, 64, 128} and S > 128 keep the plain layout."""
    want = {4: 0, 8: 0, 12: 5, 16: 5, 24: 0, 28: 3, 32: 3, 40: 2, 48: 2, 56: 0, 64: 1, 100: 1, 120: 0, 128: 0}
    assert {D: rows_per_line(D, 1) for D in DS} == want
    assert all(rows_per_line(D, 0) == 0 for D in DS)
    for D in range(1, 300):
        S, n = row_bytes(D), rows_per_line(D, 1)
        assert (n > 0) == (S < 128 and S not in (16, 32, 64))
        assert n in (0, 1, 2, 3, 5)
    # bytes per row: 24 -> 25.6, 40 -> 42.7, 48 / 56 -> 64, 72 .. 120 -> 128
    assert [128 / rows_per_line(D, 1) for D in (16, 32, 40, 48, 64, 100)] == [25.6, 128 / 3, 64, 64, 128, 128]


@pytest.mark.parametrize("D", DS)
def test_piece_offsets_are_the_byte_offsets(D):
    rows = 4099
    got = np.array([piece_offset(int(r), D, 1) for r in range(rows)], dtype=np.int64)
    assert np.array_equal(got * 4, row_offsets(rows, D, 1))


@pytest.mark.parametrize("n", [2, 3, 5])
def test_multiply_and_shift_quotient_is_exact_for_every_32_bit_row(n):
    mul, shift = quotient_constants(n)
    assert 0 < mul < 1 << 32 and shift >= 32
    assert (mul, shift) == {2: (0x80000000, 32), 3: (0xAAAAAAAB, 33), 5: (0xCCCCCCCD, 34)}[n]
    edge = [0, 1, n - 1, n, n + 1, 2 ** 31 - 1, 2 ** 31, 2 ** 31 + 1, 2 ** 32 - 1, 2 ** 32 - n, 2 ** 32 - n - 1]
    r = np.concatenate([np.array(edge, np.uint64), np.random.RandomState(n).randint(0, 2 ** 32, 10 ** 6, dtype=np.uint64)])
    # the kernels' form: the high 32 bits of the 64-bit product, shifted by shift - 32
    hi = (r * np.uint64(mul)) >> np.uint64(32)
    assert np.array_equal(hi >> np.uint64(shift - 32), r // np.uint64(n))
    for x in edge:
        assert (x * mul) >> shift == x // n


def test_host_constants_are_the_restated_ones():
    """drs_internal.h's i8_lines computes ceil(2^(31 + ceil(log2 n)) / n) and the shift behind the high half"""
    src = open(os.path.join(ROOT, "deeprecsys_amd", "csrc", "drs_internal.h")).read()
    assert "(uint64_t)1 << (31 + lg)" in src and "l.shift = (uint32_t)(lg - 1)" in src
    assert "uint32_t ln_mul, ln_shift, ln_pad;\n};" in src           # the three constants close SlsArgs


def test_documents_name_the_key():
    assert "`table_int8_lines`" in open(os.path.join(ROOT, "docs", "OPTIONS.md")).read()
    assert '"table_int8_lines" 0|1' in open(os.path.join(ROOT, "include", "drs.h")).read()
    assert "--accel_table_int8_lines" in open(os.path.join(ROOT, "README.md")).read()
