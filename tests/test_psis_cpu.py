"""CPU: the numpy contract of PSIS-LOO (`quinn_amd/psis.py`, the authority of `qn_psis_loo`) against an analytic
leave-one-out, exact generalised Pareto draws and its own structure; `summarise_loo`; and the refusals of the C entry points
that need no device.  `loo_data` and `loo_reference` are the inputs and the np.longdouble yardstick of
tests/test_gpu_psis.py."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from quinn_amd import _lib, psis, scoring

LD = np.longdouble
KMAX = 257
HEAVY = slice(3, None, 8)                     # the entries whose target lies 6 predictive standard deviations out


def loo_data(M, dtype, sigma, with_v, seed=0):
    """(F, V or None, y) at K = KMAX.  The members spread by half the predictive standard deviation s, the targets by s, so
    the log ratios of an entry span tens, not hundreds: no exp underflows in float64, and the float64 and longdouble
    authorities decide every branch alike.  The HEAVY entries have their target 6 s above the ensemble."""
    rs = np.random.RandomState(1000 * M + seed)
    mu = rs.randn(KMAX) * 2.0
    V = rs.uniform(0.1, 0.5, size=(M, KMAX)).astype(dtype) if with_v else None
    s = math.sqrt(sigma * sigma + (0.3 if with_v else 0.0))
    F = (mu + 0.5 * s * rs.randn(M, KMAX)).astype(dtype)
    y = mu + s * rs.randn(KMAX)
    y[HEAVY] = mu[HEAVY] + 6.0 * s
    return F, V, y


_REF = {}


def loo_reference(M, dtype, sigma, with_v):
    """(F, V, y, the [4, KMAX] rows of the authority in np.longdouble), once per combination: an entry's numbers do not
    depend on K, so the smaller K take the first columns."""
    key = (M, np.dtype(dtype).name, sigma, with_v)
    if key not in _REF:
        F, V, y = loo_data(M, dtype, sigma, with_v)
        _REF[key] = (F, V, y, psis.psis_loo_rows(F, y, sigma, V, dtype=LD))
    return _REF[key]


# ------------------------------------------------------------------------------------------ against known answers
def test_analytic_leave_one_out():
    """y_i ~ N(theta, s^2), flat prior, s = 0.5, n = 20 (y[0] moved out by 2), M = 4000 exact posterior draws; the exact
    elpd_loo_i is log N(y_i; mean(y_-i), s^2 + s^2 / (n - 1)).  Measured with this file's recipe (the M = 1000 draws are
    taken from the stream first): max_i |error| = 0.022, |sum error| = 0.054, khat in 0.13 .. 0.46; at M = 1000: 0.029, 0.060,
    khat in -0.07 .. 0.39.  The error is the Monte-Carlo error of 4000 draws, not the smoothing's."""
    s, n = 0.5, 20
    rs = np.random.RandomState(0)
    y = 1 + 0.5 * rs.randn(n)
    y[0] += 2
    rs.randn(1000)
    theta = y.mean() + s / math.sqrt(n) * rs.randn(4000)
    rows = psis.psis_loo_rows(np.tile(theta[:, None], (1, n)), y, s)
    loo_mean = (y.sum() - y) / (n - 1)
    var = s * s + s * s / (n - 1)
    exact = -0.5 * (y - loo_mean) ** 2 / var - 0.5 * math.log(2 * math.pi * var)
    err = rows[0] - exact
    print(f"max |error| {np.abs(err).max():.4f}  |sum error| {abs(err.sum()):.4f}  khat {rows[1].min():.3f} .. {rows[1].max():.3f}")
    assert np.abs(err).max() < 0.05
    assert np.all(rows[1] < 0.7)
    assert np.all(rows[2] > 100) and np.all((rows[3] > 0) & (rows[3] < 1))
    assert rows[3][0] > 0.99                                  # the moved target is far in the upper tail of its LOO predictive


def _gpd_draws(k, seed):
    u = np.random.RandomState(seed).rand(50, 200)
    return np.sort(((1 - u) ** (-k) - 1) / k, axis=1)          # exact quantile transform, sigma = 1


def test_pareto_fit_recovers_the_shape():
    """50 sorted samples of 200 exact GPD draws.  Measured: k = 0.5: mean khat 0.488, sd of single fits 0.087, mean sigma 1.00;
    k = -0.3: mean khat -0.275 (the prior of PSIS shrinks towards 0.5)."""
    kh, sg = psis.gpd_fit(_gpd_draws(0.5, 1))
    print(f"k = 0.5: mean khat {kh.mean():.3f} sd {kh.std():.3f} mean sigma {sg.mean():.3f}")
    assert abs(kh.mean() - 0.5) < 0.06
    assert abs(sg.mean() - 1.0) < 0.1
    kh, _ = psis.gpd_fit(_gpd_draws(-0.3, 2))
    print(f"k = -0.3: mean khat {kh.mean():.3f}")
    assert kh.mean() < 0


# ------------------------------------------------------------------------------------------ structure
def test_member_permutation_changes_nothing():
    """Measured on these inputs: elpd_loo_k 8.9e-16, khat 0, ess_k / M 3.3e-16 -- the tail is the same set of values at the
    same ranks, only the order of the remaining sums changes."""
    F, V, y = loo_data(257, np.float64, 1.0, True)
    rows = psis.psis_loo_rows(F[:, :40], y[:40], 1.0, V[:, :40])
    perm = np.random.RandomState(3).permutation(257)
    prow = psis.psis_loo_rows(F[perm, :40], y[:40], 1.0, V[perm, :40])
    assert np.isfinite(rows).all()
    dev = [np.max(np.abs(rows[0] - prow[0])), np.max(np.abs(rows[1] - prow[1])), np.max(np.abs(rows[2] - prow[2])) / 257]
    print("permuted members: elpd_loo_k %.1e khat %.1e ess_k / M %.1e" % tuple(dev))
    assert max(dev) < 1e-13


def _raw_rows(F, y, s):
    """The rows with lw = lr: plain truncated importance sampling."""
    ll = -0.5 * ((y - F) / s) ** 2 - 0.5 * math.log(2 * math.pi * s * s)
    lr = -ll - (-ll).max(axis=0)
    w = np.exp(lr) / np.exp(lr).sum(axis=0)
    return np.log((w * np.exp(ll)).sum(axis=0)), 1.0 / (w * w).sum(axis=0)


def test_twenty_members_are_not_smoothed():
    F, _, y = loo_data(20, np.float64, 1.0, False)
    rows = psis.psis_loo_rows(F, y, 1.0)
    assert psis.tail_size(20) == 4 and psis.tail_size(21) == 5
    assert np.all(np.isposinf(rows[1]))
    elpd, ess = _raw_rows(F, y, 1.0)
    assert np.max(np.abs(rows[0] - elpd)) < 1e-13 and np.max(np.abs(rows[2] - ess)) < 1e-12
    assert np.all(np.isfinite(psis.psis_loo_rows(loo_data(21, np.float64, 1.0, False)[0], y, 1.0)[1]))


def test_identical_members():
    rs = np.random.RandomState(4)
    f, y, s = rs.randn(30), rs.randn(30), 0.3
    rows = psis.psis_loo_rows(np.tile(f, (64, 1)), y, s)
    ll = -0.5 * ((y - f) / s) ** 2 - 0.5 * math.log(2 * math.pi * s * s)
    assert np.all(np.isposinf(rows[1]))                       # every excess is 0: x_q <= 0
    assert np.max(np.abs(rows[0] - ll)) < 1e-13 * np.max(np.abs(ll))
    assert np.max(np.abs(rows[2] - 64)) < 1e-11


def test_bad_entry_stays_alone():
    F, V, y = loo_data(64, np.float64, 0.05, True)
    F, V, y = F[:, :6].copy(), V[:, :6].copy(), y[:6].copy()
    clean = psis.psis_loo_rows(F, y, 0.05, V)
    assert np.isfinite(clean[[0, 2, 3]]).all()
    F[5, 0], y[1], V[7, 2], V[9, 3] = np.nan, np.inf, -1.0, -0.05 ** 2          # NaN, Inf, s^2 < 0, s^2 = 0
    rows = psis.psis_loo_rows(F, y, 0.05, V)
    assert np.isnan(rows[:, :4]).all()
    assert np.array_equal(rows[:, 4:], clean[:, 4:])


def test_float64_authority_against_longdouble():
    """Largest |float64 - longdouble| of the authority on the GPU test's inputs, measured: elpd_loo_k 5.3e-14, khat 5.9e-14,
    ess_k / M 2.4e-14, pit_loo 1.2e-15 (M = 1025 and 64, every variant)."""
    worst = np.zeros(4)
    for M in (64, 1025):
        for dtype, sigma, with_v in ((np.float64, 1.0, False), (np.float32, 0.05, True), (np.float64, 0.05, False)):
            F, V, y, ref = loo_reference(M, dtype, sigma, with_v)
            rows = psis.psis_loo_rows(F, y, sigma, V)
            assert np.array_equal(np.isinf(rows), np.isinf(ref.astype(np.float64)))
            fin = np.isfinite(rows)
            d = np.where(fin, np.abs(np.where(fin, rows, 0) - np.where(fin, ref, 0)), 0).astype(np.float64)
            d[2] /= M
            worst = np.maximum(worst, d.max(axis=1))
            print(M, np.dtype(dtype).name, sigma, with_v, "median khat: heavy rows", np.median(rows[1, HEAVY]), "all", np.median(rows[1]))
            assert np.median(rows[1, HEAVY]) > 0.7                  # the heavy rows are flagged
    print("float64 against longdouble, rows", psis.ROWS, ":", " ".join(f"{w:.2e}" for w in worst))
    assert worst.max() < 1e-10


# ------------------------------------------------------------------------------------------ the host combine
def test_summarise_loo_keys_threshold_and_shapes():
    assert psis.khat_threshold(100) == 0.5 and psis.khat_threshold(4000) == 0.7
    assert scoring.summarise_loo is psis.summarise_loo
    y = np.arange(6.0).reshape(3, 2)
    rows = np.array([[-1.0, -2.0, -3.0, -1.5, -0.5, -2.5],
                     [0.1, 0.6, np.inf, 0.45, -0.2, 0.71],
                     [90.0, 50.0, 3.0, 60.0, 99.0, 20.0],
                     [0.5, 0.04, 0.26, 0.98, 0.6, 0.4]])
    r = psis.summarise_loo(rows, y, 100, lppd=-9.0)
    assert set(r) == {"elpd_loo_k", "khat", "ess_k", "pit_loo", "elpd_loo", "looic", "se_elpd_loo", "khat_threshold",
                      "n_khat_bad", "khat_bad", "coverage_loo", "pit_loo_hist", "p_loo"}
    assert r["elpd_loo"] == -10.5 and r["looic"] == 21.0 and r["p_loo"] == 1.5 and r["khat_threshold"] == 0.5
    assert abs(r["se_elpd_loo"] - math.sqrt(6 * rows[0].var(ddof=1))) < 1e-14
    assert r["n_khat_bad"] == 3 and list(r["khat_bad"]) == [1, 2, 5]
    assert all(r[k].shape == y.shape for k in psis.ROWS)
    assert r["coverage_loo"] == {0.5: 4 / 6, 0.9: 4 / 6, 0.95: 5 / 6} and r["pit_loo_hist"].sum() == 6
    r = psis.summarise_loo(rows, y, 4000)
    assert r["n_khat_bad"] == 2 and "p_loo" not in r
    with pytest.raises(ValueError):
        psis.summarise_loo(rows[:, :5], y, 100)


# ------------------------------------------------------------------------------------------ the ABI without a device
def test_psis_header_is_bound_and_exported():
    """include/quinn_amd_psis.h declares the two entry points; the binding follows from it and the library exports them."""
    _lib.build()
    L = _lib.lib()
    hdr = open(_lib.PSIS_HEADER).read()
    assert set(re.findall(r"\b(qn_[a-z_0-9]+)\s*\(", hdr)) == set(_lib.PSIS_FUNCTIONS) | {"qn_last_error"}
    assert list(_lib.PSIS_FUNCTIONS) == ["qn_psis_loo_workspace_bytes", "qn_psis_loo"]
    assert not set(_lib.PSIS_FUNCTIONS) & set(_lib.FUNCTIONS) and os.path.exists(os.path.join(_lib.CSRC, "qn_psis.hip"))
    vp, i32, i64, f64, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_double, ctypes.c_size_t
    assert _lib.PSIS_FUNCTIONS["qn_psis_loo"] == (i32, [vp, vp, i32, vp, i64, i64, f64, vp, vp, sz, vp])
    assert _lib.PSIS_FUNCTIONS["qn_psis_loo_workspace_bytes"] == (sz, [i64, i64])
    for name, (restype, argtypes) in _lib.PSIS_FUNCTIONS.items():
        fn = getattr(L, name)
        assert (fn.restype, list(fn.argtypes)) == (restype, argtypes), name


def test_abi_needs_no_device():
    _lib.build()
    L = _lib.lib()
    EINVAL, EWORKSPACE = -1, -2
    assert _lib.LOO_NOUT == 4 and _lib.PSIS_MAX_M >= 16384
    need = L.qn_psis_loo_workspace_bytes(64, 7)
    assert need > 0
    for args, word in (((1, 7), b"M >= 2"), ((64, 0), b"K >= 1"), ((_lib.PSIS_MAX_M + 1, 7), b"at most"),
                       ((64, 2 ** 31 + 1), b"too large")):
        assert L.qn_psis_loo_workspace_bytes(*args) == 0, args
        assert word in L.qn_last_error(), (args, L.qn_last_error())
    buf = (ctypes.c_double * 8)()
    p = ctypes.addressof(buf)                        # never dereferenced: every call below is refused first

    def call(F=p, V=None, dtype=0, Y=p, M=64, K=7, sigma=0.1, out=p, ws=p, nbytes=need):
        return L.qn_psis_loo(F, V, dtype, Y, M, K, sigma, out, ws, nbytes, None)

    for kw, word in (({"M": 1}, b"M >= 2"), ({"M": _lib.PSIS_MAX_M + 1}, b"at most"), ({"K": 0}, b"K >= 1"),
                     ({"K": 2 ** 31 + 1}, b"too large"), ({"dtype": 2}, b"dtype"), ({"sigma": -0.1}, b"sigma"), ({"sigma": float("nan")}, b"sigma"),
                     ({"sigma": float("inf")}, b"sigma"), ({"sigma": 0.0}, b"variance"), ({"F": None}, b"NULL"),
                     ({"Y": None}, b"NULL"), ({"out": None}, b"NULL"), ({"ws": None}, b"NULL")):
        assert call(**kw) == EINVAL, kw
        assert word in L.qn_last_error(), (kw, L.qn_last_error())
    assert call(nbytes=need - 1) == EWORKSPACE and b"workspace" in L.qn_last_error()
