"""CPU: the multi-chain diagnostics (quinn_amd/mcmc/diagnostics.py) against a direct numpy restatement, their statistical
sanity on AR(1) chains, the batch plan, the argument checks of qn_chain_stats (no device needed) and the row selection of
the pooled predictive ensemble."""
import ctypes

import numpy as np
import pytest

from quinn_amd import _lib
from quinn_amd.mcmc import diagnostics as diag


def window_np(chain, nburn):
    """(x [2C, nbatch, blen, K] float64, t0, nbatch, blen): the rows the diagnostics use, split into halves and batches."""
    chain = np.asarray(chain)
    C, T, K = chain.shape
    half = (T - nburn) // 2
    blen = int(np.floor(np.sqrt(half)))
    nbatch = half // blen
    t0 = T - 2 * nbatch * blen
    return chain[:, t0:].astype(np.float64).reshape(2 * C, nbatch, blen, K), t0, nbatch, blen


def stats_np(chain, nburn):
    """The [C, 6, K] numbers of qn_chain_stats by numpy (two-pass)."""
    x, t0, nbatch, blen = window_np(chain, nburn)
    m, K = x.shape[0], x.shape[3]
    flat = x.reshape(m, nbatch * blen, K)
    mean = flat.mean(axis=1)
    M2 = ((flat - mean[:, None]) ** 2).sum(axis=1)
    Sb = ((x.mean(axis=2) - mean[:, None]) ** 2).sum(axis=1)
    return np.concatenate([a.reshape(m // 2, 2, K) for a in (mean, M2, Sb)], axis=1)


def diagnostics_np(chain, nburn):
    """Split-R-hat, batch-means ESS and pooled moments of chain [C, T, K], straight from their definitions."""
    x, t0, nbatch, blen = window_np(chain, nburn)
    m, K = x.shape[0], x.shape[3]
    n = nbatch * blen
    flat = x.reshape(m, n, K)
    means = flat.mean(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        W = flat.var(axis=1, ddof=1).mean(axis=0)
        B = n * means.var(axis=0, ddof=1)
        var = (n - 1) / n * W + B / n
        sigma2 = (blen * x.mean(axis=2).var(axis=1, ddof=1)).mean(axis=0)
        both = flat.reshape(m // 2, 2 * n, K)
        return {"rhat": np.sqrt(var / W), "ess": m * n * var / sigma2, "mean": means.mean(axis=0), "var": var,
                "chain_mean": both.mean(axis=1), "chain_var": both.var(axis=1, ddof=1), "n_draws": m * n, "nbatch": nbatch,
                "blen": blen, "t0": t0}


def ar1(seed, C, T, K, rho, dtype=np.float64):
    """x_t = rho x_{t-1} + sqrt(1 - rho^2) e_t from the stationary law, [C, T, K]."""
    rs = np.random.RandomState(seed)
    e = rs.randn(C, T, K)
    x = np.empty((C, T, K))
    x[:, 0] = e[:, 0]
    s = np.sqrt(1.0 - rho * rho)
    for t in range(1, T):
        x[:, t] = rho * x[:, t - 1] + s * e[:, t]
    return x.astype(dtype)


def assert_same_diagnostics(got, ref, rtol):
    for k in ("rhat", "ess", "mean", "var", "chain_mean", "chain_var"):
        scale = np.max(np.abs(ref[k]))
        assert got[k].shape == ref[k].shape, k
        assert np.max(np.abs(got[k] - ref[k])) <= rtol * scale, (k, np.max(np.abs(got[k] - ref[k])) / scale)
    for k in ("n_draws", "nbatch", "blen", "t0"):
        assert got[k] == ref[k], k


@pytest.mark.parametrize("shape,nburn", [((4, 2001, 5), 0), ((1, 100, 3), 17), ((3, 1001, 1), 333)])
def test_combine_equals_numpy_restatement(shape, nburn):
    x = ar1(3, *shape, rho=0.6) * 2.5 + 0.7
    t0, nbatch, blen = diag.batch_plan(shape[1], nburn)
    got = diag.combine(stats_np(x, nburn), nbatch, blen, t0)
    assert_same_diagnostics(got, diagnostics_np(x, nburn), 1e-12)
    assert got["rhat"].shape == (shape[2],) and got["chain_mean"].shape == (shape[0], shape[2])


def test_combine_constant_entry_is_nan_without_warning():
    x = ar1(0, 2, 400, 3, rho=0.3)
    x[:, :, 1] = 4.0                                       # a parameter no chain ever moved
    t0, nbatch, blen = diag.batch_plan(400, 0)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        d = diag.combine(stats_np(x, 0), nbatch, blen)
    assert np.isnan(d["rhat"][1]) and np.isnan(d["ess"][1]) and d["mean"][1] == 4.0
    assert np.isfinite(d["rhat"][[0, 2]]).all() and np.isfinite(d["ess"][[0, 2]]).all()
    assert d["t0"] is None


@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("rho", [0.0, 0.5])
def test_ar1_ess_and_rhat(seed, rho):
    """ess / n_draws against the theoretical (1 - rho) / (1 + rho) of an AR(1) chain; R-hat of agreeing chains near 1."""
    x = ar1(seed, 4, 20001, 8, rho)
    t0, nbatch, blen = diag.batch_plan(20001, 1000)
    d = diag.combine(stats_np(x, 1000), nbatch, blen, t0)
    ratio = d["ess"] / d["n_draws"] / ((1 - rho) / (1 + rho))
    assert ratio.min() >= 0.75 and ratio.max() <= 1.35, (ratio.min(), ratio.max())
    assert d["rhat"].max() < 1.01
    x[2] += 2.0                                            # one chain of four somewhere else
    d = diag.combine(stats_np(x, 1000), nbatch, blen, t0)
    assert d["rhat"].min() > 1.2, d["rhat"]


def test_batch_plan():
    assert diag.batch_plan(10001, 5000) == (5001, 50, 50)   # half = 2500
    assert diag.batch_plan(10001, 0) == (61, 71, 70)        # half = 5000: blen = 70, 71 batches, the first 61 rows unused
    assert diag.batch_plan(8, 0) == (0, 2, 2)
    assert diag.batch_plan(9, 1) == (1, 2, 2)
    assert diag.batch_plan(9, 0) == (1, 2, 2)               # an odd row count: the first row is left out
    assert diag.batch_plan(50, 0) == (0, 5, 5)
    for T, nburn in [(7, 0), (8, 1), (100, 93), (1, 0)]:
        with pytest.raises(ValueError):
            diag.batch_plan(T, nburn)
    for T, nburn in [(100, 100), (100, -1), (100, 250)]:
        with pytest.raises(ValueError):
            diag.batch_plan(T, nburn)
    for T in (8, 9, 50, 777, 4097, 10001):
        for nburn in (0, 1, T // 3):
            if T - nburn < 8:
                continue
            t0, nb, bl = diag.batch_plan(T, nburn)
            assert t0 >= nburn and nb >= 2 and bl >= 1 and t0 + 2 * nb * bl == T


def test_abi_argument_checks_need_no_device():
    _lib.build()
    L = _lib.lib()
    assert L.qn_chain_stats_workspace_bytes(64, 10001, 8513, 70, 70) == 64 * 140 * 2 * 8513 * 8
    assert L.qn_chain_stats_workspace_bytes(1, 8, 1, 2, 2) > 0
    for args in [(0, 100, 4, 2, 10), (2, 100, 0, 2, 10), (2, 100, 4, 1, 10), (2, 100, 4, 2, 0), (2, 100, 4, 5, 11),
                 (2, 0, 4, 2, 2), (2, 100, 4, 2, 2 ** 62)]:
        assert L.qn_chain_stats_workspace_bytes(*args) == 0, args
        assert b"qn_chain_stats_workspace_bytes" in L.qn_last_error()
    # refused before any pointer is touched: the pointers here are not addresses of anything
    bogus = ctypes.c_void_p(8)
    for dtype, C, T, K, t0, nbatch, blen in [(0, 2, 100, 4, 1, 5, 10), (0, 2, 100, 4, -1, 2, 10), (0, 2, 100, 4, 0, 1, 10),
                                             (0, 2, 100, 4, 0, 2, 0), (7, 2, 100, 4, 0, 2, 10), (0, 0, 100, 4, 0, 2, 10)]:
        rc = L.qn_chain_stats(bogus, dtype, C, T, K, t0, nbatch, blen, bogus, bogus, 1 << 40, None)
        assert rc == -1, (dtype, C, T, K, t0, nbatch, blen)
        assert b"qn_chain_stats" in L.qn_last_error()
    assert L.qn_chain_stats(None, 0, 2, 100, 4, 0, 5, 10, bogus, bogus, 1 << 40, None) == -1
    assert L.qn_chain_stats(bogus, 0, 2, 100, 4, 0, 5, 10, bogus, bogus, 16, None) == -2      # QN_EWORKSPACE


def test_pooled_rows():
    """predict_ens(chain='all'): chain c gives nens // C + (c < nens % C) draws by the reference's thinning rule."""
    assert diag.thinned_rows(6001, 10, 1000) == [1000 + 500 * j for j in range(10)]
    got = diag.pooled_rows(4, 2001, 10, 1000)
    assert [c for c, _ in got] == [0, 1, 2, 3]
    assert [len(r) for _, r in got] == [3, 3, 2, 2]
    for c, rows in got:
        assert rows == diag.thinned_rows(2001, len(rows), 1000)
    assert got[0][1] == [1000, 1333, 1666] and got[3][1] == [1000, 1500]
    assert diag.pooled_rows(1, 2001, 10, 1000) == [(0, diag.thinned_rows(2001, 10, 1000))]
    assert [(c, len(r)) for c, r in diag.pooled_rows(4, 500, 2, 100)] == [(0, 1), (1, 1)]      # fewer draws than chains
    assert sum(len(r) for _, r in diag.pooled_rows(7, 3001, 100, 1000)) == 100
