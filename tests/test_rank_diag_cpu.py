"""CPU: the numpy contract of the rank diagnostics (`quinn_amd/mcmc/rankdiag.py`, the authority of `qn_rank_diag`) against brute
force, closed forms and known statistical behaviour; the header and its binding; and the refusals of the C entry points that
need no device.  `rank_inputs` builds the inputs of tests/test_gpu_rank_diag.py."""
import ctypes
import os
import re

import numpy as np
import pytest

from quinn_amd import _lib
from quinn_amd.mcmc import diagnostics as diag
from quinn_amd.mcmc import rankdiag as rd


def rank_inputs(kind, C, nh, K, seed=0):
    """(chain [C, T, K], t0, stride) of one input kind of the device tests.  'cont': iid normal; 'ties': a Metropolis-like
    series in which about half the rows repeat their predecessor, rounded to one decimal; 'offset': 1e8 + N(0, 1); 'f32':
    float32; 'window': t0 = 5, stride = 3, and every row outside the window NaN."""
    rs = np.random.RandomState(1000 * C + nh + 7 * K + seed)
    T = 2 * nh
    x = rs.randn(C, T, K) + 0.3 * rs.randn(C, 1, K)
    if kind == "ties":
        keep = rs.rand(C, T, K) < 0.5
        keep[:, 0] = True
        idx = np.maximum.accumulate(np.where(keep, np.arange(T)[None, :, None], 0), axis=1)
        x = np.round(np.take_along_axis(x, idx, axis=1), 1)
    elif kind == "offset":
        x = 1e8 + x
    elif kind == "f32":
        x = x.astype(np.float32)
    elif kind == "window":
        full = np.full((C, 5 + 3 * (T - 1) + 1 + 4, K), np.nan)
        full[:, 5:5 + 3 * (T - 1) + 1:3] = x
        return full, 5, 3
    return x, 0, 1


# ------------------------------------------------------------------------------------------ the header and the ABI
def test_rank_header_is_bound_and_exported():
    _lib.build()
    L = _lib.lib()
    hdr = open(_lib.RANK_HEADER).read()
    assert set(re.findall(r"\b(qn_[a-z_0-9]+)\s*\(", hdr)) == set(_lib.RANK_FUNCTIONS) | {"qn_last_error"}
    assert list(_lib.RANK_FUNCTIONS) == ["qn_rank_diag_workspace_bytes", "qn_rank_diag"]
    others = set(_lib.FUNCTIONS) | set(_lib.PSIS_FUNCTIONS) | set(_lib.STACK_FUNCTIONS)
    assert not set(_lib.RANK_FUNCTIONS) & others and "qn_rank.hip" in _lib.SOURCES
    vp, i32, i64, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_size_t
    assert _lib.RANK_FUNCTIONS["qn_rank_diag_workspace_bytes"] == (sz, [i32, i64, i64, i64, i64])
    assert _lib.RANK_FUNCTIONS["qn_rank_diag"] == (i32, [vp, i32, i32, i64, i64, i64, i64, i64, vp, vp, sz, vp])
    for name, (restype, argtypes) in _lib.RANK_FUNCTIONS.items():
        fn = getattr(L, name)
        assert (fn.restype, list(fn.argtypes)) == (restype, argtypes), name
    assert (_lib.RANK_MAX_S, _lib.RANK_NOUT) == (16384, 6) and rd.QN_RANK_MAX_S == 16384
    assert [_lib.RANK_RHAT_BULK, _lib.RANK_RHAT_TAIL, _lib.RANK_ESS_BULK, _lib.RANK_ESS_TAIL, _lib.RANK_ESS_MEAN,
            _lib.RANK_MCSE_MEAN] == list(range(6)) and len(rd.KEYS) == 6


def test_refusals_need_no_device():
    _lib.build()
    L = _lib.lib()
    assert L.qn_rank_diag_workspace_bytes(4, 1000, 7, 100, 2) > 0
    half = _lib.RANK_MAX_S // 2 + 1
    for args, word in (((4, 1000, 7, 3, 1), b"nh >= 4"), ((1, 100000, 7, half, 1), b"at most"), ((4, 1000, 7, 100, 0), b"stride >= 1"),
                       ((4, 1000, 7, 100, 6), b"past T"), ((0, 1000, 7, 100, 1), b"C >= 1")):
        assert L.qn_rank_diag_workspace_bytes(*args) == 0, args
        assert word in L.qn_last_error(), (args, L.qn_last_error())
    # the call itself, refused before any pointer is touched (the pointers are NULL)
    for args in ((4, 1000, 7, 0, 3, 1), (1, 100000, 7, 0, half, 1), (4, 1000, 7, 0, 100, 0), (4, 1000, 7, 802, 100, 1),
                 (4, 1000, 7, -1, 100, 1)):
        C, T, K, t0, nh, stride = args
        assert L.qn_rank_diag(None, _lib.QN_F64, C, T, K, t0, nh, stride, None, None, 0, None) == _lib.CONSTANTS["QN_EINVAL"], args
    assert L.qn_rank_diag(None, 77, 4, 1000, 7, 0, 100, 1, None, None, 0, None) == _lib.CONSTANTS["QN_EINVAL"]
    assert L.qn_rank_diag(None, _lib.QN_F64, 4, 1000, 7, 0, 100, 1, None, None, 0, None) == _lib.CONSTANTS["QN_EINVAL"]
    assert b"NULL" in L.qn_last_error()


# ------------------------------------------------------------------------------------------ the plan
def test_rank_plan():
    assert rd.rank_plan(4, 1000) == (0, 500, 1)                       # everything fits: stride 1, all rows
    assert rd.rank_plan(4, 1001, nburn=1) == (1, 500, 1)
    t0, nh, stride = rd.rank_plan(64, 2000, nburn=300)
    assert (nh, stride) == (128, 6) and t0 + (2 * nh - 1) * stride == 1999 and t0 >= 300
    for C, T, nburn, md in ((1, 100000, 0, None), (3, 777, 100, 500), (8, 50, 7, None), (2, 9, 1, None)):
        t0, nh, stride = rd.rank_plan(C, T, nburn, md)
        assert t0 >= nburn and t0 + (2 * nh - 1) * stride == T - 1 and 2 * C * nh <= (md or rd.QN_RANK_MAX_S) and nh >= 4
    with pytest.raises(ValueError):
        rd.rank_plan(2, 7)
    with pytest.raises(ValueError):
        rd.rank_plan(4, 1000, max_draws=31)
    with pytest.raises(ValueError):
        rd.rank_plan(4, 10, nburn=10)


# ------------------------------------------------------------------------------------------ ranks, median, quantile
def test_ranks_with_ties_are_the_brute_force_count():
    x, _, _ = rank_inputs("ties", 3, 20, 4)
    x = x.reshape(-1, 4)
    assert len(np.unique(x[:, 0])) < x.shape[0] // 2                  # it does have ties
    r2, s = rd.twice_ranks(x)
    brute = (x[None, :, :] < x[:, None, :]).sum(axis=1) + (x[None, :, :] <= x[:, None, :]).sum(axis=1) + 1
    assert np.array_equal(r2, brute) and np.array_equal(s, np.sort(x, axis=0))
    z, _ = rd.rank_normalise(x)
    vals, cnt = np.unique(x[:, 0], return_counts=True)
    same = x[:, 0] == vals[np.argmax(cnt)]
    assert same.sum() > 1 and len(set(z[same, 0])) == 1              # tied draws share a z


def test_median_quantile_and_indicators_closed_form():
    s = np.arange(1.0, 12.0)[:, None]                                  # 1 .. 11, S = 11
    assert rd.sorted_quantile(s, 0.05)[0] == 1.5 and rd.sorted_quantile(s, 0.5)[0] == 6.0
    assert abs(rd.sorted_quantile(s, 0.95)[0] - 10.5) < 1e-14
    chain = np.array([[3.0, 1.0, 4.0, 1.5, 9.0, 2.0, 6.0, 5.0]]).T[None]          # C = 1, T = 8
    xs = np.sort(chain[0, :, 0])
    assert 0.5 * (xs[3] + xs[4]) == 3.5                                # the pooled median of an even S
    assert rd.sorted_quantile(xs[:, None], 1.0)[0] == 9.0 and rd.sorted_quantile(xs[:, None], 0.0)[0] == 1.0
    q05 = rd.sorted_quantile(xs[:, None], 0.05)[0]
    assert abs(q05 - (1.0 + 0.35 * 0.5)) < 1e-15
    assert np.array_equal(chain[0, :, 0] <= q05, [False, True, False, False, False, False, False, False])
    # split-R-hat by hand on m = 2 sequences of 4: z of the ranks, W, B, var+
    w = rd.window(chain, 0, 4, 1)
    assert w.shape == (2, 4, 1) and np.array_equal(w[1, :, 0], [9.0, 2.0, 6.0, 5.0])
    z, _ = rd.rank_normalise(w.reshape(8, 1))
    zz = z.reshape(2, 4)
    W = zz.var(axis=1, ddof=1).mean()
    B = 4 * zz.mean(axis=1).var(ddof=1)
    assert abs(rd.split_rhat(z.reshape(2, 4, 1))[0] - np.sqrt((0.75 * W + B / 4) / W)) < 1e-14
    assert np.allclose(rd.rank_rows(chain, 0, 4, 1)[0, 0], np.sqrt((0.75 * W + B / 4) / W), rtol=1e-14)


def test_ess_steps_by_hand():
    """The Geyer sum written as a plain loop over one entry."""
    rs = np.random.RandomState(3)
    m, n = 4, 200
    w = np.zeros((m, n + 60))
    e = rs.randn(m, n + 60)
    for i in range(1, n + 60):
        w[:, i] = 0.7 * w[:, i - 1] + e[:, i]
    v = np.ascontiguousarray(w[:, 60:, None])
    c = v[:, :, 0] - v[:, :, 0].mean(axis=1, keepdims=True)
    W = (c ** 2).sum(axis=1).mean() / (n - 1)
    varp = (n - 1) / n * W + v[:, :, 0].mean(axis=1).var(ddof=1)
    rho = [1.0] + [1 - (W - np.mean([(c[j, :n - t] * c[j, t:]).sum() / n for j in range(m)])) / varp for t in range(1, n)]
    tau, prev, k = rho[0] + rho[1], rho[0] + rho[1], 1
    tau *= 2
    trail = 0.0
    while k < n // 2:
        P = rho[2 * k] + rho[2 * k + 1]
        if not P > 0:
            trail = max(rho[2 * k], 0.0)
            break
        prev = min(prev, P)
        tau += 2 * prev
        k += 1
    tau = max(tau - 1 + trail, 1 / np.log10(m * n))
    assert 1 < k < n // 2
    assert abs(rd.ess(v)[0] - m * n / tau) < 1e-10 * m * n / tau


def test_scaling_by_four_changes_no_rank_figure():
    for kind in ("cont", "ties"):
        x, t0, stride = rank_inputs(kind, 3, 12, 5)
        a, b = rd.rank_rows(x, t0, 12, stride), rd.rank_rows(4.0 * x, t0, 12, stride)
        assert np.array_equal(a[:4], b[:4]) and np.all(np.isfinite(a))
        assert np.allclose(b[5], 4 * a[5], rtol=1e-12) and np.allclose(b[4], a[4], rtol=1e-12)


def test_nan_and_constant_entries():
    x, _, _ = rank_inputs("cont", 2, 8, 4)
    ref = rd.rank_rows(x, 0, 8, 1)
    y = x.copy()
    y[1, 5, 2] = np.inf
    y[:, :, 0] = 3.0
    got = rd.rank_rows(y, 0, 8, 1)
    assert np.all(np.isnan(got[:, 2])) and np.all(np.isnan(got[:, 0]))
    assert np.array_equal(got[:, [1, 3]], ref[:, [1, 3]])


# ------------------------------------------------------------------------------------------ statistical behaviour, fixed seeds
C8, NH, K64 = 8, 256, 64


def _stats(x):
    return rd.rank_stats_host(x)


def test_iid_normal():
    s = _stats(np.random.RandomState(11).randn(C8, 2 * NH, K64))
    S = s["n_draws"]
    assert (S, s["nh"], s["stride"], s["t0"]) == (4096, NH, 1, 0)
    r = np.median(s["ess_mean"] / S)
    print(f"iid: median ess_mean / S {r:.3f}  bulk {np.median(s['ess_bulk'] / S):.3f}  tail {np.median(s['ess_tail'] / S):.3f}  "
          f"spread of ess_mean / S {np.std(s['ess_mean'] / S):.3f}  max rhat_rank {s['rhat_rank'].max():.4f}")
    assert abs(r - 1) < 0.25
    assert np.all(s["rhat_rank"] < 1.05)
    assert np.allclose(s["mcse_mean"], np.sqrt(1.0 / s["ess_mean"]), rtol=0.1)


def test_ar1():
    rs = np.random.RandomState(12)
    rho = 0.5
    e = rs.randn(C8, 2 * NH + 100, K64)
    x = np.zeros_like(e)
    for i in range(1, e.shape[1]):
        x[:, i] = rho * x[:, i - 1] + e[:, i]
    s = _stats(x[:, 100:])
    r = np.median(s["ess_mean"] / s["n_draws"])
    print(f"AR(1) 0.5: median ess_mean / S {r:.3f} (1/3)  spread {np.std(s['ess_mean'] / s['n_draws']):.3f}")
    assert abs(r - 1 / 3) < 0.25 / 3


def test_scale_difference_is_seen_by_the_folded_rhat_only():
    rs = np.random.RandomState(13)
    x = rs.randn(C8, 2 * NH, K64)
    x[4:] *= 3.0
    classic = diag.combine(_classic_stats(x), *diag.batch_plan(2 * NH)[1:])["rhat"]
    s = _stats(x)
    print(f"scale: classic rhat max {classic.max():.4f}  rhat_tail min {s['rhat_tail'].min():.4f}  rhat_bulk max {s['rhat_bulk'].max():.4f}")
    assert np.all(classic < 1.05)
    assert np.all(s["rhat_tail"] > 1.05)
    assert np.array_equal(s["rhat_rank"], np.maximum(s["rhat_bulk"], s["rhat_tail"]))


def _classic_stats(x):
    """[C, 6, K] chain statistics of qn_chain_stats in numpy (the two half-window means, M2 and batch sums), for `combine`."""
    C, T, K = x.shape
    t0, nbatch, blen = diag.batch_plan(T)
    n = nbatch * blen
    h = x[:, t0:].reshape(C, 2, n, K)
    mean = h.mean(axis=2)
    M2 = ((h - mean[:, :, None]) ** 2).sum(axis=2)
    bm = h.reshape(C, 2, nbatch, blen, K).mean(axis=3)
    Sb = ((bm - mean[:, :, None]) ** 2).sum(axis=2)
    return np.concatenate([mean, M2, Sb], axis=1)


def test_iid_cauchy():
    s = _stats(np.random.RandomState(14).standard_cauchy((C8, 2 * NH, K64)))
    for k in rd.KEYS:
        assert np.all(np.isfinite(s[k])), k
    print(f"Cauchy: rhat_bulk max {s['rhat_bulk'].max():.4f}  median ess_bulk / S {np.median(s['ess_bulk']) / s['n_draws']:.3f}")
    assert np.all(s["rhat_bulk"] < 1.05)
