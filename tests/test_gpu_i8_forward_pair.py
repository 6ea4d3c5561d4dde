"""GPU: the 8-wave form of the sliced int8-product forward (csrc/qn_fused_i8.hip, PAIR: tanh networks of up to 3 hidden layers;
one staged weight image per workgroup for two row splits, the tanh(n / 512) table, a one-column first layer for d = 1)
against the float64-MFMA fused kernel (QN_PATH_FUSED_DP) and the oracle, with the tolerances of test_gpu_i8_forward.py.
The sizes walk the row plan: one split (N <= 64), two, an odd number (N = 129: three, the upper half of the last workgroup
has no rows), sixteen (N = 1000), with and without a ragged last group of 16 rows."""
import numpy as np
import pytest
import torch

from oracle import mlp_ref
from quinn_amd import _lib
from quinn_amd.ops import BatchedMLP, MLPArch, neg_log_post_from_sse

pytestmark = pytest.mark.gpu


def _data(N, d, o, seed=0):
    rs = np.random.RandomState(seed)
    x = rs.rand(N, d) * 2 * np.pi - np.pi
    y = np.sin(x).sum(axis=1, keepdims=True) * np.ones((1, o)) + 0.02 * rs.randn(N, o)
    return x, y


def _dims(d, o, layers):
    return (d,) + (64,) * layers + (o,)


def _on(op, path, fn):
    old = op.set_path(path)
    try:
        return fn()
    finally:
        op.set_path(old)


def _pair(op, W, row_idx=None):
    f = lambda: tuple(t.cpu().numpy() for t in op.sse_pred(W, row_idx=row_idx))
    return _on(op, _lib.PATH_FUSED, f), _on(op, _lib.PATH_FUSED_DP, f)


@pytest.mark.parametrize("layers", [2, 3])
@pytest.mark.parametrize("o", [1, 4])
@pytest.mark.parametrize("d", [1, 2])
@pytest.mark.parametrize("N", [1, 16, 17, 64, 65, 129, 1000])
@pytest.mark.parametrize("B", [1, 3, 5])
def test_matches_float64_kernel_and_oracle(B, N, d, o, layers):
    dims = _dims(d, o, layers)
    x, y = _data(N, d, o, seed=N + d)
    arch = MLPArch(dims, "tanh")
    W = 0.3 * np.random.RandomState(7 * B + N + o + layers).randn(B, arch.nparams)
    op = BatchedMLP(arch, x, y)
    assert op.path(B, N, False) == _lib.PATH_FUSED and op.arith(B, N, False) == _lib.ARITH_I8_FUSED
    (s8, p8), (sd, pd) = _pair(op, W)
    np.testing.assert_allclose(s8, sd, rtol=1e-11)
    assert np.abs(p8 - pd).max() <= 1e-11 * np.abs(pd).max()
    parts = op.sse_parts(W).cpu().numpy()
    assert parts.shape[1] == min(-(-N // 64), -(-512 // B))              # the row plan the sizes above were chosen for
    np.testing.assert_allclose(parts.sum(axis=1), s8, rtol=1e-13)
    mod = mlp_ref.build_module(mlp_ref.MLPSpec(dims, "tanh"))
    yd = [v for v in y]
    for b in range(B):
        ref = mlp_ref.logpost(mod, W[b], x, yd, 0.02)
        got = -neg_log_post_from_sse(s8[b], N, 0.02)
        assert abs(got - ref) <= 1e-11 * abs(ref), (b, got, ref)


@pytest.mark.parametrize("d,o", [(1, 1), (2, 4)])
def test_row_subset_and_identical_launches(d, o):
    dims = _dims(d, o, 3)
    x, y = _data(777, d, o, seed=3)
    arch = MLPArch(dims, "tanh")
    rs = np.random.RandomState(5)
    W = 0.2 * rs.randn(6, arch.nparams)
    idx = rs.randint(0, 777, size=(6, 403))                             # 7 splits: odd
    op = BatchedMLP(arch, x, y)
    (s8, p8), (sd, pd) = _pair(op, W, row_idx=idx)
    np.testing.assert_allclose(s8, sd, rtol=1e-11)
    assert np.abs(p8 - pd).max() <= 1e-11 * np.abs(pd).max()
    s8b, p8b = (t.cpu().numpy() for t in op.sse_pred(W, row_idx=idx))
    assert np.array_equal(s8b, s8) and np.array_equal(p8b, p8)          # two identical launches: the same bits
    assert np.array_equal(op.sse(W, row_idx=idx).cpu().numpy(), s8)


@pytest.mark.parametrize("N", [40, 129, 200])                           # one split, three, four
@pytest.mark.parametrize("where", ["weight_nan", "weight_inf", "bias_nan"])
def test_one_chain_with_a_weight_that_is_not_finite(N, where):
    """The chain leaves the fast path (its workgroups evaluate their rows in plain float64); the clean chains beside it -- other
    workgroups, and with three splits also a half-empty one -- are untouched."""
    dims = _dims(1, 1, 3)
    arch = MLPArch(dims, "tanh")
    x, y = _data(N, 1, 1, seed=1)
    W = 0.2 * np.random.RandomState(2).randn(3, arch.nparams)
    clean = W.copy()
    if where == "weight_nan": W[1, 64 + 64 + 5 * 64 + 7] = np.nan
    if where == "weight_inf": W[1, 64 + 64 + 5 * 64 + 7] = np.inf
    if where == "bias_nan": W[1, 64 + 3] = np.nan
    op = BatchedMLP(arch, x, y)
    (s8, p8), (sd, pd) = _pair(op, W)
    sg, pg = _on(op, _lib.PATH_GENERIC, lambda: tuple(t.cpu().numpy() for t in op.sse_pred(W)))
    assert np.array_equal(np.isnan(s8), np.isnan(sg)) and np.array_equal(np.isnan(p8), np.isnan(pg))
    assert np.array_equal(np.isinf(s8), np.isinf(sg))
    fin = np.isfinite(pg)
    np.testing.assert_allclose(p8[fin], pg[fin], rtol=1e-10, atol=1e-11)
    s0 = op.sse(clean).cpu().numpy()
    assert s8[0] == s0[0] and s8[2] == s0[2]                             # the clean chains: bit for bit what they give alone
    np.testing.assert_allclose(s8[[0, 2]], sd[[0, 2]], rtol=1e-11)


@pytest.mark.parametrize("N", [50, 129])
def test_chain_with_tiny_activations_takes_the_redo_path(N):
    """Every activation of a chain below ~2^-4.7 (tiny weights, no help from the biases): the fixed activation scale would lose
    relative accuracy, the waves redo their rows in plain float64 -- the result still agrees to 1e-11 RELATIVE."""
    dims = _dims(1, 1, 3)
    arch = MLPArch(dims, "tanh")
    x, y = _data(N, 1, 1, seed=4)
    W = 0.2 * np.random.RandomState(8).randn(3, arch.nparams)
    W[1] *= 1e-4
    op = BatchedMLP(arch, x, y)
    (s8, p8), (sd, pd) = _pair(op, W)
    np.testing.assert_allclose(s8, sd, rtol=1e-11)
    for b in range(3):                                                   # (per chain: the tiny chain against its own scale)
        assert np.abs(p8[b] - pd[b]).max() <= 1e-11 * np.abs(pd[b]).max(), b
    np.testing.assert_allclose(op.sse_parts(W).cpu().numpy().sum(axis=1), s8, rtol=1e-13)


def test_deep_and_relu_networks_keep_the_four_wave_form():
    """4 hidden layers (image + large table exceed the CU's LDS) and relu still run as sliced int8 products."""
    for dims, act in (((1, 64, 64, 64, 64, 1), "tanh"), ((1, 64, 64, 64, 1), "relu")):
        x, y = _data(129, 1, 1, seed=6)
        arch = MLPArch(dims, act)
        W = 0.2 * np.random.RandomState(9).randn(3, arch.nparams)
        op = BatchedMLP(arch, x, y)
        assert op.arith(3, 129, False) == _lib.ARITH_I8_FUSED
        (s8, p8), (sd, pd) = _pair(op, W)
        np.testing.assert_allclose(s8, sd, rtol=1e-11)
        assert np.abs(p8 - pd).max() <= 1e-11 * np.abs(pd).max()
