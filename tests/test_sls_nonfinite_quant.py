"""Poison rows of the quantized tables in every gather form on the GPU (-m gpu).

tests/test_sls_nonfinite.py's test for the stored types fp8 e4m3, int8 rowwise and int4 rowwise (plain and line-packed),
on tests/test_sls_nonfinite_quant_cpu.py's layouts: the same bags name rows 0 .. 7, and those rows hold each type's own
poison -- for fp8 the two NaN codes every inf and NaN quantizes to, for the rowwise types FINITE fp32 rows whose header
overflows (scale +inf, every code 0: the row decodes to inf * 0 = NaN in every column, as torch's prepack operators write
it and torch's rowwise bags pool it), beside one control row whose outlier stays just inside the header's range.

Two engines per case, `poisoned` and `clean`, loaded through set_table; unweighted sum, mean, and weighted under
"sls_weighted_flat" 0 and 1; "sls_nt" 1, and 0 for the fixed-length shapes; single queries and the coalesced set of 12.
Checked by run_poison_case, no element left out: the class of every pooled element is the reference's; finite elements are
the sequential chain's bits (weighted_ref_rowwise on torch's codes for the rowwise types) where the form sums in index
order and within the split order's tolerance otherwise; every bag that names no poison row has the clean engine's bits;
empty bags are +0.0; the bottom MLP's columns and the outputs of clean samples are the clean engine's; the dispatch token is
the form's with the kind's tag; forward raises nothing.
"""
import numpy as np
import pytest

from deeprecsys_amd import _native as N
from tests.test_half_tables import _load
from tests.test_sls_nonfinite import _bits, run_poison_case
from tests.test_sls_nonfinite_cpu import RAGGED, SHAPES, classes, nf_shape_id
from tests.test_sls_nonfinite_quant_cpu import QTAG, QUANT_KINDS, quant_case, shapes_of
from tests.test_sls_weights import _engine
from tests.test_sls_weights_flat_cpu import B

pytestmark = pytest.mark.gpu

CASES = [(kind, n) for kind in QUANT_KINDS for n in shapes_of(kind)]


def _same_fp8_exponents(po, cl, T):
    """the poison is NaN codes only: no table's scale moved, i.e. the clean rows keep their codes"""
    ks = [[eng.table_fp8_exponent(t) for t in range(T)] for eng in (po, cl)]
    assert ks[0] == ks[1], ks


@pytest.mark.parametrize("kind,n", CASES, ids=["%s-%s" % (kind, nf_shape_id(SHAPES[n])) for kind, n in CASES])
def test_poison_rows_of_quantized_tables_reach_the_bags_that_name_them_and_no_other(kind, n):
    c = quant_case(SHAPES[n], kind)
    T = len(c["rows"])
    run_poison_case(c, n, kind, QTAG[kind], after_load=(lambda po, cl: _same_fp8_exponents(po, cl, T)) if kind == "fp8" else None)


@pytest.mark.parametrize("kind", ["int8", "int4"])
def test_the_arena_conversion_writes_the_overflowed_headers_set_table_writes(kind):
    """fp32 tables converted in place ("table_dtype" 8 / 9 on a loaded engine) against the same tables quantized row by row
    in set_table: the same pooled bits under "sls_exact" 1, NaN positions included"""
    shape = (64, 3, RAGGED, {"sls_exact": 1})
    D, T, L, opts = shape
    c = quant_case(shape, kind)
    Lmax = max(int(ln.max()) for b in range(2) for ln in c["lens"][b])
    dense = np.random.RandomState(7).rand(B, 8).astype(np.float32)
    conv, direct = _engine(c["rows"], D, Lmax, B, "fp32"), _engine(c["rows"], D, Lmax, B, kind)
    try:
        _load(conv, 11, c["poisoned"], D, T)
        conv.set_option("table_dtype", N.TABLE_INT8_ROWWISE if kind == "int8" else N.TABLE_INT4_ROWWISE)
        _load(direct, 11, c["poisoned"], D, T)
        for eng in (conv, direct):
            eng.set_option("dispatch_log", 1)
            eng.set_option("sls_exact", 1)
        for weighted in (False, True):
            for b in range(2):
                got = []
                for eng in (conv, direct):
                    eng.stage_batch(b, dense, c["idx"][b], c["lens"][b], weights=c["wts"][b] if weighted else None)
                    eng.forward(b, B)
                    got.append(eng.fetch_interaction(B)[:, D:])
                    tok = [t for t in eng.last_dispatch(0) if t.startswith("sls_")]
                    assert len(tok) == 1 and tok[0].startswith("sls_kernel<16,sequential,%s%s>[" % (QTAG[kind], ",w" if weighted else "")), tok
                ref = c["seq"]["w" if weighted else "sum"][b]
                assert np.array_equal(classes(got[0]), classes(ref)), (kind, weighted, b)
                assert np.any(classes(ref) == 3) and np.any(classes(ref) == 0)
                fin = classes(ref) == 0
                assert np.array_equal(_bits(got[0])[fin], _bits(ref)[fin]), (kind, weighted, b)
                assert np.array_equal(np.isnan(got[0]), np.isnan(got[1])), (kind, weighted, b)
                assert np.array_equal(_bits(got[0])[fin], _bits(got[1])[fin]), (kind, weighted, b)
    finally:
        conv.close()
        direct.close()
