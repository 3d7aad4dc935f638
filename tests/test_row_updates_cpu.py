"""CPU side of drs_update_rows / drs_get_rows (include/drs_rows.h): the symbols and the header, the frozen symbol list, and
the properties of tests/row_update_ref.py that the GPU tests (tests/test_row_updates.py) stand on."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from deeprecsys_amd import _native as N
from tests import row_update_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_library_exports_both_symbols():
    """the built library, loaded as the binding loads it (no GPU needed to dlopen it): lib() binds ROW_SYMBOLS and raises when
    one is missing"""
    L = N.lib()
    for name, res, args in N.ROW_SYMBOLS:
        fn = getattr(L, name)
        assert fn.restype is res and fn.argtypes == args, name


def test_the_header_declares_both_calls_and_the_abi_version_stays():
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "a C compiler preprocesses the header"
    text = subprocess.run([cc, "-E", os.path.join(ROOT, "include", "drs.h")], capture_output=True, text=True, check=True).stdout
    flat = re.sub(r"\s+", " ", text)
    for name, last in (("drs_update_rows", r"const float\s*\*"), ("drs_get_rows", r"float\s*\*")):
        assert re.search(r"int32_t %s\s*\(\s*drs_handle \w+\s*, int32_t \w+\s*, int64_t \w+\s*, const int64_t\s*\*\s*\w+\s*, %s\s*\w+\s*\)\s*;" % (name, last), flat), name
    hdr = open(os.path.join(ROOT, "include", "drs.h")).read()
    assert "#define DRS_ABI_VERSION 5" in hdr and '#include "drs_rows.h"' in hdr
    assert "drs_update_rows" not in hdr and "drs_get_rows" not in hdr          # declared in drs_rows.h alone


def test_the_frozen_symbol_list_is_unchanged(cpu_abi):
    names = [n for n, _, _ in N.SYMBOLS]
    assert len(names) == 40 and len(set(names)) == 40
    assert [n for n, _, _ in N.ROW_SYMBOLS] == ["drs_update_rows", "drs_get_rows"]
    assert not set(names) & {"drs_update_rows", "drs_get_rows"}
    # the CPU restatement binds the frozen list (the fixture has just done so) and knows nothing of the new names
    assert cpu_abi.drs_abi_version() == 5
    for name in ("drs_update_rows", "drs_get_rows"):
        assert not hasattr(cpu_abi, name)


def test_the_last_occurrence_of_an_id_wins():
    ids = np.array([5, 1, 5, 3, 1, 5], np.int64)
    V = np.arange(6 * 2, dtype=np.float32).reshape(6, 2)
    u, rows = R.resolve(ids, V)
    assert u.tolist() == [1, 3, 5] and np.array_equal(rows, V[[4, 3, 5]])
    W = np.full((7, 2), -1, np.float32)
    out = R.replaced(W, ids, V)
    assert np.array_equal(out[[1, 3, 5]], V[[4, 3, 5]]) and np.array_equal(out[[0, 2, 4, 6]], W[[0, 2, 4, 6]])
    u, rows = R.resolve(np.zeros(0, np.int64), np.zeros((0, 2), np.float32))
    assert u.size == 0 and rows.shape == (0, 2)
    assert sorted(set(R.IDS.tolist())) == [0, 6, 7, 150, 299, 300] and R.IDS.tolist().count(150) == 3
    assert R.IDS.tolist() != sorted(R.IDS.tolist()) and R.ABSMAX_ROW not in R.IDS


@pytest.mark.parametrize("D", R.DS)
@pytest.mark.parametrize("dtype", R.DTYPES)
def test_storing_replaced_rows_equals_replacing_stored_rows(dtype, D):
    """Every stored type works row by row: prepacking (rounding, encoding) W with rows replaced gives the bytes of prepacking
    W and then replacing those rows' bytes with the bytes of the new rows prepacked on their own.  This is what lets
    update_rows write single rows, and what the twin-engine comparison of the GPU tests rests on."""
    W = R.table(R.ROWS, D, seed=D)
    V = R.update_values(R.IDS.size, D, seed=100 + D)
    W2 = R.replaced(W, R.IDS, V)
    k = R.table_exponent(W) if dtype == R.FP8 else None
    whole = R.stored(W2, dtype, k)
    u, rows = R.resolve(R.IDS, V)
    patched = R.stored(W, dtype, k).copy()
    patched[u] = R.stored(rows, dtype, k)
    assert np.array_equal(whole, patched)
    a, b = R.served(W2, dtype, k), R.served_after_update(W, R.IDS, V, dtype)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    # and the update is visible: every updated row serves something else than before
    before = R.served(W, dtype, k)
    assert all(not np.array_equal(before[r], a[r]) for r in u)
    untouched = np.setdiff1d(np.arange(R.ROWS), u)
    assert np.array_equal(before[untouched].view(np.uint32), a[untouched].view(np.uint32))


@pytest.mark.parametrize("D", R.DS)
def test_the_fp8_update_values_keep_the_scale_exponent(D):
    W = R.table(R.ROWS, D, seed=D)
    V = R.update_values(R.IDS.size, D, seed=100 + D)
    k = R.table_exponent(W)
    assert k == R.fp8_exponent(1.5) == 8                                 # 1.5 * 2^8 = 384 <= 448 < 768
    assert R.table_exponent(R.replaced(W, R.IDS, V)) == k and R.fp8_fits(V, k)
    edge = np.float32(448 * 2.0 ** -k)
    assert R.fp8_fits(np.array([[edge, -edge, np.inf, np.nan]], np.float32), k)
    assert not R.fp8_fits(np.array([[np.nextafter(edge, np.float32(np.inf))]], np.float32), k)
    assert R.served(np.array([[edge, -edge]], np.float32), R.FP8, k).tolist() == [[float(edge), -float(edge)]]


def test_the_fp8_exponent_is_the_one_the_fp8_tests_use():
    from tests.test_fp8_tables_cpu import fp8_exponent
    for x in (0.0, 1e-30, 0.05, 0.875, 1.0, 1.5, 448.0, 449.0, 3e38):
        assert R.fp8_exponent(x) == fp8_exponent(x), x
