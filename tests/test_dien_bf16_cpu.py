"""CPU side of DIEN's bf16 recurrence (engine option "dien_bf16"): the cases, inputs and references tests/test_dien_bf16.py
runs on the GPU, the measurement its tolerance comes from, the documents and the --accel_dien_bf16 flag.

The reference restates DESIGN.md 4.2's contract in float64: per step and layer
  h = tanh((bf16(in) . bf16(W_i2h)^T + bf16(h_prev) . bf16(W_gates)^T) + (b_i2h + b_gates))
operands rounded with torch's .to(torch.bfloat16), the states carried in fp32 and re-rounded where they are operands, through
the reference's Reshape of the behaviour rows; then the top MLP (every layer FC + ReLU) over [last state | profile | ad | context].
"""
import os
import zlib

import numpy as np
import pytest
import torch

from deeprecsys_amd import _native as N
from tests import gather_shapes as S
from tests import helpers as H
from tests.test_din_dien_nonfinite_cpu import mlp64

TOP = (24, 2)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_MAX = 24                     # samples staged per batch
# (D, H, U, sizes): every shape (the smallest, dien.json's, the two padded-K ones) and set size once, shape x U, sizes x U = 5
CASES = [(16, 16, 1, (16,)), (16, 16, 5, (17,)), (32, 64, 2, (16,)), (32, 64, 9, (17,)), (64, 16, 5, (1,)), (64, 16, 9, (16,)),
         (16, 32, 1, (17,)), (16, 32, 2, (1,)), (16, 32, 5, (5, 7, 9)), (32, 64, 5, (1,)), (32, 64, 5, (16,)), (32, 64, 5, (17,)),
         (32, 64, 5, (5, 7, 9))]
IDS = ["%d_%d_U%d_%s" % (D, Hh, U, "_".join(map(str, sz))) for D, Hh, U, sz in CASES]
# The largest |float32 restatement - float64 reference| over CASES' last states and scores (test_tolerance_is_its_measurement
# prints it): MEASURED -- one flipped bf16 re-rounding of a state; without a flip the distance is 2e-7.  TOL = 8 x that, rounded up to one digit -- tanh_rnn is within ~8 ulp of libm where numpy is within 1,
# and the instruction's summation order is its own.
MEASURED = 4.03e-4
TOL = 4e-3


def key_of(D, Hh, U):
    return ("dien", D, U + 3, (Hh,), TOP)


def model(key):
    """-> (tables, weights): tests/gather_shapes.py's, the recurrent layers' weights halved (a flipped bf16 re-rounding of a
    state then moves a later state by ~1e-3, and TOL stays under 1e-2) and given biases (its own are zero)"""
    tab, w = S.Tables(key), S.Weights(key)
    rng = np.random.RandomState(zlib.crc32(("b" + repr(key)).encode()) % (1 << 31))
    w.rnn = [[(0.5 * W, rng.normal(0, 0.1, W.shape[0]).astype(np.float32)) for W, _ in layer] for layer in w.rnn]
    return tab, w


def batches(key, tab):
    """3 staged batches of N_MAX samples, one row per bag: [(idx per table, lengths per table)]"""
    rng = np.random.RandomState(zlib.crc32(("i" + repr(key)).encode()) % (1 << 31))
    return [([rng.randint(0, r, N_MAX).astype(np.int64) for r in tab.rows], [np.ones(N_MAX, np.int32) for _ in tab.rows]) for _ in range(3)]


def bf16(a, dt):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(torch.bfloat16).to(torch.float32).numpy().astype(dt)


def reference(tab, w, idx, n, dt=np.float64):
    """one query of n samples -> (last state [n, H], scores [n, 2]); dt float32: the same contract in fp32 arithmetic"""
    E = [np.asarray(W[i[:n]], dt) for W, i in zip(tab.W, idx)]              # pooled rows (one row per bag), table by table
    U, D = len(E) - 3, E[0].shape[1]
    X = np.stack(E[1:1 + U], axis=1).reshape(n * U, D).reshape(U, n, D)     # step t of sample b: flat row t n + b
    (Wi0, bi0), (Wg0, bg0) = w.rnn[0]
    (Wi1, bi1), (Wg1, bg1) = w.rnn[1]
    h0 = h1 = np.zeros((n, Wg0.shape[0]), dt)
    for t in range(U):
        h0 = np.tanh((bf16(X[t], dt) @ bf16(Wi0, dt).T + bf16(h0, dt) @ bf16(Wg0, dt).T) + (bi0.astype(dt) + bg0.astype(dt)))
        h1 = np.tanh((bf16(h0, dt) @ bf16(Wi1, dt).T + bf16(h1, dt) @ bf16(Wg1, dt).T) + (bi1.astype(dt) + bg1.astype(dt)))
    h1 = h1.astype(np.float32)                                               # the state the kernel hands on is fp32
    return h1, mlp64(np.concatenate([h1, E[0], E[U + 1], E[U + 2]], axis=1).astype(np.float64), w.top)[0]


def test_tolerance_is_its_measurement():
    worst = 0.0
    for D, Hh, U, sizes in CASES:
        key = key_of(D, Hh, U)
        tab, w = model(key)
        # the GPU test's own queries, and every staged batch whole: over the queries alone (~65 k re-roundings) no rounding
        # happens to flip and the distance is 1e-7, which says nothing about the flips the GPU's other summation order meets
        for idx, _ in batches(key, tab):
            for n in set(sizes) | {N_MAX}:
                (h64, o64), (h32, o32) = reference(tab, w, idx, n), reference(tab, w, idx, n, np.float32)
                worst = max(worst, float(np.abs(h32 - h64).max()), float(np.abs(o32 - o64).max()))
    print("largest |float32 restatement - float64 reference|: %.3g (MEASURED %.3g, TOL %.3g)" % (worst, MEASURED, TOL))
    assert worst <= TOL / 8 and TOL <= 1e-2


def test_the_documents_name_the_key():
    assert "`dien_bf16`" in open(os.path.join(ROOT, "docs", "OPTIONS.md")).read()
    assert '"dien_bf16"' in open(os.path.join(ROOT, "include", "drs.h")).read()


def test_another_model_refuses_the_flag_at_construction():
    meta, _ = H.load_fixture("dlrm_dot_small")
    np.random.seed(0)
    H.NET_CLS[meta["args"]["model_type"]](H.args_from(meta["args"], accel_dien_bf16=0))
    with pytest.raises(ValueError, match="accel_dien_bf16"):
        H.NET_CLS[meta["args"]["model_type"]](H.args_from(meta["args"], accel_dien_bf16=1))
    meta, _ = H.load_fixture("dien_mini")
    H.NET_CLS[meta["args"]["model_type"]](H.args_from(meta["args"], accel_dien_bf16=1))
