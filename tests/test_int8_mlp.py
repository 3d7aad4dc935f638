"""The wide FC layers on the int8 matrix cores (-m gpu): engine option "mlp_int8" 1 (csrc/gemm_i8.hip).

The contract (top of gemm_i8.hip) restated in float32 numpy, an int64 matmul for the sum: held BIT FOR BIT under every tile.
Two things numpy cannot state: a NaN's payload (NaN positions must agree, every other bit must) and the device's expf -- the
sigmoid of the reference's pre-activation comes from act_apply itself, a 1 x 1 identity layer on the handle's fp32 path."""
import numpy as np
import pytest

from deeprecsys_amd import _native as N
from tests.test_bf16_mlp import eligible, fc_op, nets

pytestmark = pytest.mark.gpu
f32 = np.float32
TILES = (12, 22, 44)


def quant(v):
    v = np.ascontiguousarray(v, f32)                     # contract steps 1 and 2 on the rows of v: (codes, scales)
    a = (v.view(np.uint32) & 0x7fffffff).max(axis=1).view(f32)
    fin = np.isfinite(a)
    ok = fin & (a >= f32(2.0 ** -119))
    a1 = np.where(ok, a, f32(1))
    scale = np.where(ok, a1 / f32(127), np.where(fin, f32(0), f32(np.nan))).astype(f32)
    with np.errstate(invalid="ignore", over="ignore"):
        q = np.clip(np.rint(v * (f32(127) / a1)[:, None]), -127, 127)
    return np.where(ok[:, None], np.nan_to_num(q), 0).astype(np.int64), scale


def reference(eng, x, W, b, act):
    (qx, sx), (qw, sw) = quant(x), quant(W)
    acc = qx @ qw.T
    with np.errstate(invalid="ignore"):
        y = acc.astype(f32) * (sx[:, None] * sw[None, :]) + (np.zeros(len(W), f32) if b is None else b)[None, :]
    if act == N.ACT_RELU:
        y = np.where(y > 0, y, f32(0))
    if act == N.ACT_SIGMOID:
        y = fc_op(eng, y.reshape(-1, 1), np.ones((1, 1), f32), None, act).reshape(y.shape)
    return y, acc, sx, sw


def same_bits(got, exp):
    nan = np.isnan(exp)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.uint32)[~nan], exp.view(np.uint32)[~nan])


def small(kind=N.MODEL_DLRM, rows=(16, 16), D=8, bot=(4, 8), top=(24, 4, 1)):
    return N.Engine(kind, list(rows), D, list(bot), list(top), max_batch=4, max_lookups=2, num_staged_batches=1, num_slots=1)


@pytest.fixture(scope="module")
def eng():
    e = small()
    e.set_option("mlp_int8", 1)
    yield e
    e.close()


MKN = [(1, 64, 64), (17, 65, 65), (65, 127, 100), (129, 129, 64), (1, 192, 65), (17, 64, 100), (65, 65, 64), (129, 127, 65),
       (1, 129, 100), (17, 192, 64), (65, 64, 65), (129, 192, 100)]


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("i", range(len(MKN)))
def test_one_layer_has_the_contracts_bits(eng, i, tile):
    (M, K, N_), act, rng = MKN[i], i % 3, np.random.RandomState(i)
    x, W = rng.normal(0, 1, (M, K)).astype(f32), rng.normal(0, 0.1, (N_, K)).astype(f32)
    b = rng.normal(0, 0.1, N_).astype(f32) if i % 2 else None
    eng.set_option("mlp_i8_tile", tile)
    assert same_bits(fc_op(eng, x, W, b, act), reference(eng, x, W, b, act)[0]), (M, K, N_, act)


@pytest.mark.parametrize("tile", TILES)
def test_edges_of_the_quantizer_have_the_contracts_bits(eng, tile):
    M, K, N_, rng = 20, 100, 72, np.random.RandomState(7)
    x, W = rng.uniform(-1, 1, (M, K)).astype(f32), rng.uniform(-1, 1, (N_, K)).astype(f32)
    x[0, K - 1], x[1, 0], x[3] = 3.0, -3.0, 0                          # absmax in the last and in the first element; all zero
    x[2] = np.resize(np.array([127, -127, 0.5, 1.5, 2.5, -0.5, -1.5, 126.5, -126.5], f32), K)   # inv = 1: halves, and +-127
    x[4], x[5] = np.resize(np.array([2.0 ** -119, -2.0 ** -120, 2.0 ** -126], f32), K), np.nextafter(f32(2.0 ** -119), f32(0))
    W[5] = np.where(rng.rand(K) < 0.5, f32(-0.75), f32(0.75))
    clean_x, clean_W = x.copy(), W.copy()
    x[6, 9], x[7, K - 1], W[3, 50] = np.nan, np.inf, np.nan
    b = rng.normal(0, 0.1, N_).astype(f32)
    eng.set_option("mlp_i8_tile", tile)
    got, (exp, _, sx, _) = fc_op(eng, x, W, b, N.ACT_NONE), reference(eng, x, W, b, N.ACT_NONE)
    assert sx[4] > 0 and sx[5] == 0 and np.isnan(sx[6]) and np.isnan(sx[7])
    assert same_bits(got, exp)
    bad = np.isin(np.arange(M), (6, 7))[:, None] | (np.arange(N_) == 3)[None, :]
    assert np.array_equal(np.isnan(got), bad) and np.array_equal(got[3, ~bad[3]], b[~bad[3]])
    assert np.array_equal(fc_op(eng, clean_x, clean_W, b, N.ACT_NONE)[~bad], got[~bad])     # untouched rows and columns
    s = np.where(rng.rand(3, 2048) < 0.5, f32(-1.5), f32(1.5))        # |acc| = 2048 * 127^2 > 2^24: the int -> float rounding
    Wb = np.where(rng.rand(64, 2048) < 0.5, f32(-0.75), f32(0.75))
    Wb[0], Wb[1] = s[0] / 2, -s[0] / 2
    exp, acc = reference(eng, s, Wb, None, N.ACT_NONE)[:2]
    assert acc[0, 0] == 2048 * 127 * 127 > 2 ** 24 and acc[0, 1] == -acc[0, 0] and np.abs(quant(Wb)[0]).min() == 127
    assert same_bits(fc_op(eng, s, Wb, None, N.ACT_NONE), exp)


def test_the_quantizer_is_a_quantizer(eng):
    rng = np.random.RandomState(3)
    x, W, b = rng.normal(0, 1, (64, 256)).astype(f32), rng.normal(0, 1, (128, 256)).astype(f32), rng.normal(0, 1, 128).astype(f32)
    eng.set_option("mlp_i8_tile", 0)
    got = fc_op(eng, x, W, b, N.ACT_NONE).astype(np.float64)
    (_, sx), (_, sw) = quant(x), quant(W)
    sx, sw, x64, W64 = sx.astype(np.float64)[:, None], sw.astype(np.float64)[None, :], x.astype(np.float64), W.astype(np.float64)
    y64 = x64 @ W64.T + b
    bound = (np.abs(W64).sum(1)[None, :] * sx / 2 + np.abs(x64).sum(1)[:, None] * sw / 2 + 256 * sx * sw / 4) * (1 + 2.0 ** -20) \
        + 2.0 ** -22 * (np.abs(y64) + np.abs(b)[None, :])
    assert np.all(np.abs(got - y64) <= bound), float((np.abs(got - y64) / bound).max())


def int8_engine(net, option_first):
    e = net.engine(load=not option_first)
    e.set_option("mlp_int8", 1)
    return (net.load(e), e)[1] if option_first else e


@pytest.mark.parametrize("name", ["wnd", "mtwnd", "dlrm_cat"])
def test_whole_models_keep_a_querys_bits_and_log_the_int8_layers(name):
    net = nets()[name]
    first, later, ref = int8_engine(net, True), int8_engine(net, False), net.engine()
    try:
        shapes = sorted("%dx%d]" % (K, N_) for _, _, K, N_ in net.layers() if eligible(K, N_))
        out = first.forward(0, net.B)
        log, fp32 = first.last_dispatch(0), ref.forward(0, net.B)      # (below: the rest are fp32 launches of their own)
        assert sorted(t.split(", ")[-1] for t in log if t.startswith("gemm_i8_kernel")) == shapes, log
        assert len(log) > len(shapes) + 1 and not any("bf16" in t for t in log) and "gemm_i8" not in " ".join(ref.last_dispatch(0))
        assert np.all(np.isfinite(out)) and not np.array_equal(out, fp32), "mlp_int8 1 changed nothing"
        print("%s: largest |int8 - fp32| / largest output: %.3e" % (name, np.abs(out - fp32).max() / np.abs(fp32).max()))
        assert np.array_equal(later.forward(0, net.B), out)                           # layers before the option
        for tile in TILES + (0,):
            first.set_option("mlp_i8_tile", tile)
            assert np.array_equal(first.forward(0, net.B), out), tile
        jobs = [(0, 37), (1, net.B), (0, 1), (1, 65), (0, 128)]
        first.forward_multi_async(1, [b for b, _ in jobs], [n for _, n in jobs])
        both = np.split(first.wait(1, sum(n for _, n in jobs)), np.cumsum([n for _, n in jobs])[:-1])
        assert all(np.array_equal(got, first.forward(b, n)) for got, (b, n) in zip(both, jobs)), name
        later.set_option("mlp_int8", 0)
        assert np.array_equal(later.forward(0, net.B), fp32) and later.last_dispatch(0) == ref.last_dispatch(0)
    finally:
        [e.close() for e in (first, later, ref)]


def test_the_key():
    e, din = small(), small(N.MODEL_DIN, [50] * 5, 8, [24, 4, 8], [32, 8, 1])
    dien = small(N.MODEL_DIEN, [50] * 5, 16, [16, 8], [56, 8, 1])
    try:
        e.set_option("mlp_int8", 1)
        assert e.get_option("mlp_int8") == 1
        for key, bad, code, word in [("mlp_int8", 2, N.ERR_BAD_ARG, ""), ("mlp_int8", -1, N.ERR_BAD_ARG, ""),
                                     ("mlp_dtype", 2, N.ERR_UNSUPPORTED, "mlp_int8")]:
            with pytest.raises(N.DrsError) as err:
                e.set_option(key, bad)
            assert err.value.code == code and word in str(err.value)
            assert e.get_option("mlp_int8") == 1 and e.get_option("mlp_dtype") == 0
        e.set_option("mlp_int8", 0)
        e.set_option("mlp_dtype", 2)
        for eng_, key in [(e, "mlp_dtype"), (din, "mlp_int8"), (dien, "mlp_int8")]:
            with pytest.raises(N.DrsError) as err:
                eng_.set_option("mlp_int8", 1)
            assert err.value.code == N.ERR_UNSUPPORTED and key in str(err.value) and eng_.get_option("mlp_int8") == 0
            eng_.set_option("mlp_int8", 0)          # (the value it has: nothing to refuse)
        assert e.get_option("mlp_dtype") == 2
    finally:
        [x.close() for x in (e, din, dien)]
