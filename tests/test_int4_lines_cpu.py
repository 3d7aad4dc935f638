"""CPU side of the line-packed int4 rowwise layout (engine option "table_int4_lines"): the --accel_table_int4_lines flag
and when the host code sets the option, the layout rule of docs/OPTIONS.md restated in numpy (no row crosses a 128-byte
line), the multiply-and-shift quotient the gather kernels take for r / n, and a compile check of the `I4L` kernels."""
import os
import re
import shutil

import numpy as np
import pytest

from deeprecsys_amd import _native as N
from deeprecsys_amd import dlrm_s_hip
from deeprecsys_amd.utils.utils import FLAG_CHOICES, cli
from tests import helpers as H
from tests.test_bf16_mlp_cpu import _Recorder
from tests.test_table_convert_cpu import listing

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEY = "table_int4_lines"
# even D -> rows per line, the issue's table; every other even D keeps the plain layout
RANGES = [((10, 16), 10), ((26, 32), 6), ((34, 40), 5), ((42, 48), 4), ((58, 72), 3), ((74, 112), 2), ((122, 240), 1)]


# ---- the layout, restated -------------------------------------------------------------------------------------------
def row_bytes(D):
    """S: D / 2 code bytes, zero padding to a multiple of 4, fp16 scale, fp16 bias."""
    return (D // 2 + 3) // 4 * 4 + 4


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
    """where the kernels find row r, in 2-byte pieces: r * PR + (r / n) * pad"""
    S, n = row_bytes(D), rows_per_line(D, lines)
    PR = S // 2
    if not n:
        return r * PR
    pad = 64 - n * PR
    if n == 1:
        return r * PR + r * pad
    mul, shift = quotient_constants(n)
    return r * PR + ((r * mul) >> shift) * pad


# ---- 1. flag ----------------------------------------------------------------------------------------------------------
def test_flag_defaults_to_off_and_takes_0_or_1():
    assert cli([]).accel_table_int4_lines == 0
    for v in (0, 1):
        assert cli(["--accel_table_int4_lines", str(v)]).accel_table_int4_lines == v
    assert FLAG_CHOICES["accel_table_int4_lines"] == (0, 1)
    for bad in ("2", "-1", "yes"):
        with pytest.raises(SystemExit):
            cli(["--accel_table_int4_lines", bad])
    args = cli([])
    for bad in (2, -1, 8):
        args.accel_table_int4_lines = bad                        # (a JSON config can set anything: refused at engine build)
        with pytest.raises(ValueError):
            dlrm_s_hip._table_int4_lines(args)
    args.accel_table_int4_lines = 1
    assert dlrm_s_hip._table_int4_lines(args) == 1


def _engine_calls(monkeypatch, **flags):
    meta, _ = H.load_fixture("dlrm_dot_small")
    args = H.args_from(meta["args"], **flags)
    np.random.seed(args.numpy_rand_seed)
    net = H.NET_CLS[args.model_type](args)
    monkeypatch.setattr(dlrm_s_hip.N, "Engine", _Recorder)
    _Recorder.log = []
    net._create_engine()
    return list(_Recorder.log)


# ---- 2. call order ----------------------------------------------------------------------------------------------------
def test_with_the_flag_the_option_precedes_table_dtype_and_every_table_write(monkeypatch):
    log = _engine_calls(monkeypatch, accel_table_dtype="int4_rowwise", accel_table_int4_lines=1)
    lines = [i for i, c in enumerate(log) if c[:2] == ("set_option", KEY)]
    dtype = [i for i, c in enumerate(log) if c[:2] == ("set_option", "table_dtype")]
    creates = [i for i, c in enumerate(log) if c[0] == "create"]
    writes = [i for i, c in enumerate(log) if c[0] in ("set_table", "fill_table_uniform")]
    assert writes and lines and lines == [c + 1 for c in creates] and dtype == [c + 2 for c in creates]
    assert all(log[i] == ("set_option", KEY, 1) for i in lines)
    assert all(log[i] == ("set_option", "table_dtype", N.TABLE_INT4_ROWWISE) for i in dtype)
    assert max(dtype) < min(writes)


# ---- 3. default calls -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [{}, {"accel_table_dtype": "int4_rowwise"},
                                   {"accel_table_dtype": "int8_rowwise", "accel_table_int8_lines": 1},
                                   {"accel_table_dtype": "fp16"}, {"accel_mlp_dtype": "bf16", "accel_mlp_bf16_fuse": 1}])
def test_without_the_flag_the_calls_are_todays(monkeypatch, flags):
    """The CPU restatement of the ABI does not know the key: only a user who asked for it may reach it.  With the flag
    absent or 0 the engine sees exactly the calls it sees with the flag set, but for the one that sets the key."""
    base = _engine_calls(monkeypatch, **flags)
    assert [c for c in base if c[0] == "set_fc"]
    assert [c for c in base if c[:2] == ("set_option", KEY)] == []
    assert _engine_calls(monkeypatch, accel_table_int4_lines=0, **flags) == base
    with_flag = _engine_calls(monkeypatch, accel_table_int4_lines=1, **flags)
    assert [c for c in with_flag if c[:2] != ("set_option", KEY)] == base


def test_default_flags_set_nothing_on_the_cpu_abi(cpu_abi):
    meta, _ = H.load_fixture("dlrm_dot_small")
    net, lX, lS_l, lS_i, lT = H.materialize(H.args_from(meta["args"]))
    net.create(lX[0], lS_l[0], lS_i[0], lT[0])
    try:
        assert KEY not in net.engine.user_options and "table_int8_lines" not in net.engine.user_options
    finally:
        net.engine.close()


# ---- 4. layout --------------------------------------------------------------------------------------------------------
def test_the_layout_keeps_every_row_inside_a_line_for_every_even_width():
    seen = set()
    for D in range(2, 301, 2):
        S, n = row_bytes(D), rows_per_line(D, 1)
        want = [k for (lo, hi), k in RANGES if lo <= D <= hi]
        assert n == (want[0] if want else 0), D                             # exactly the issue's table
        assert (n > 0) == (S < 128 and S not in (4, 8, 16, 32, 64)), D
        assert (128 - n * S) % 4 == 0                                       # the line tail: whole dwords
        seen.add(n)
        for rows in sorted({1, 2, max(n - 1, 1), max(n, 1), n + 1, 1000, 3001}):
            off = row_offsets(rows, D, 1)
            assert np.all(off % 4 == 0)
            assert np.all(np.diff(off) >= S)                                # ascending, no overlap
            assert off[-1] + S <= table_bytes(rows, D, 1)
            if n:
                assert np.all(off // 128 == (off + S - 1) // 128), "a row crosses a 128-byte line"
                assert np.all(off % 128 + S <= n * S)                       # the last 128 - n S bytes of a line hold no row
                assert table_bytes(rows, D, 1) == ((rows + n - 1) // n * 128 + 255) // 256 * 256
            else:
                assert np.array_equal(off, row_offsets(rows, D, 0)) and table_bytes(rows, D, 1) == table_bytes(rows, D, 0)
            assert table_bytes(rows, D, 0) == (rows * S + 255) // 256 * 256
            assert np.array_equal(row_offsets(rows, D, 0), np.arange(rows) * S)
        assert rows_per_line(D, 0) == 0
    assert seen == {0, 1, 2, 3, 4, 5, 6, 10}
    # bytes per row: 12 -> 12.8, 20 -> 21.3, 24 -> 25.6, 28 -> 32, 36 -> 42.7, 52 -> 64, 68 -> 128
    assert [128 / rows_per_line(D, 1) for D in (16, 32, 40, 48, 64, 96, 128)] == [12.8, 128 / 6, 25.6, 32, 128 / 3, 64, 128]


# ---- 5. piece offsets -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [12, 16, 24, 30, 32, 40, 48, 56, 64, 72, 100, 128, 240, 256])
def test_piece_offsets_are_the_byte_offsets(D):
    rows = 4099
    got = np.array([piece_offset(int(r), D, 1) for r in range(rows)], dtype=np.int64)
    assert np.array_equal(got * 2, row_offsets(rows, D, 1))


# ---- 6. quotient constants --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 3, 4, 5, 6, 10])
def test_multiply_and_shift_quotient_is_exact_for_every_32_bit_row(n):
    mul, shift = quotient_constants(n)
    assert 0 < mul < 1 << 32 and shift >= 32
    assert (mul, shift - 32) == {2: (1 << 31, 0), 3: (0xAAAAAAAB, 1), 4: (1 << 31, 1), 5: (0xCCCCCCCD, 2),
                                 6: (0xAAAAAAAB, 2), 10: (0xCCCCCCCD, 3)}[n]
    assert (mul * n - (1 << shift)) * ((1 << 32) - 1) < 1 << shift          # the error term never reaches the next quotient
    edge = [0, 1, n - 1, n, n + 1, 2 ** 31 - 1, 2 ** 31, 2 ** 31 + 1, 2 ** 32 - 1, 2 ** 32 - n, 2 ** 32 - n - 1]
    r = np.concatenate([np.array(edge, np.uint64), np.random.RandomState(n).randint(0, 2 ** 32, 10 ** 6, dtype=np.uint64)])
    # the kernels' form: the high 32 bits of the 64-bit product, shifted by shift - 32
    hi = (r * np.uint64(mul)) >> np.uint64(32)
    assert np.array_equal(hi >> np.uint64(shift - 32), r // np.uint64(n))
    for x in edge:
        assert (x * mul) >> shift == x // n


def test_host_constants_come_from_the_shared_formula():
    """drs_internal.h computes int4's constants with the formula of the int8 layout, in 2-byte pieces"""
    src = open(os.path.join(ROOT, "deeprecsys_amd", "csrc", "drs_internal.h")).read()
    assert "(uint64_t)1 << (31 + lg)" in src and "i4_lines" in src
    assert "uint32_t ln_mul, ln_shift, ln_pad;\n};" in src           # no field is added behind the three constants


# ---- 7. documents -----------------------------------------------------------------------------------------------------
def test_documents_name_the_key():
    doc = open(os.path.join(ROOT, "docs", "OPTIONS.md")).read()
    assert "`table_int4_lines`" in doc and "--accel_table_int4_lines" in doc and "37 settable keys" in doc
    assert '"table_int4_lines" 0|1' in open(os.path.join(ROOT, "include", "drs.h")).read()
    assert "#define DRS_ABI_VERSION 5" in open(os.path.join(ROOT, "include", "drs.h")).read()
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "--accel_table_int4_lines" in readme and "`table_int4_lines`" in readme


# ---- 8. compile check -------------------------------------------------------------------------------------------------
@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_line_packed_int4_kernels_exist_and_use_no_scratch():
    """sls.hip compiled with the Makefile's flags: an I4L instance of each of the five gather families exists and none
    uses scratch.  (The kernel that moves rows between the two layouts: table_convert.hip,
    tests/test_table_convert_cpu.py.)"""
    asm = listing("sls.hip")
    found = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", asm, re.S):
        name, body = m.group(1), m.group(2)
        kind = re.search(r"(sls_kernel|sls_one_kernel|sls_flat_kernel|sls_flatc_kernel|sls_any_kernel)", name)
        if not kind or "3I4LE" not in name:
            continue
        found[kind.group(1)] = found.get(kind.group(1), 0) + 1
        assert int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body).group(1)) == 0, name
    for kind in ("sls_kernel", "sls_one_kernel", "sls_flat_kernel", "sls_flatc_kernel", "sls_any_kernel"):
        assert found.get(kind, 0) > 0, (kind, found)
