"""CPU: the numpy restatement of `qn_pred_score` (include/quinn_amd.h) that the GPU tests compare against, checked
against closed forms; the host combine `scoring.summarise`; the calibration of an exactly calibrated synthetic ensemble;
and every argument refusal of the C entry points, which need no device.

`score_np` restates lppd, p_waic, mean and var in np.longdouble (80-bit on x86, eps 1.1e-19) with two-pass variances, and
pit and crps in float64 with scipy's erf / erfc.  `score_bars` gives the per-entry bars of the GPU parity tests (their
derivation is in tests/test_gpu_pred_score.py)."""
import ctypes
import math

import numpy as np
import pytest
from scipy.special import erf, erfc

from quinn_amd import _lib, scoring

EPS = 2.0 ** -53
LD = np.longdouble


def _a(mu, var):
    """A(mu, s^2) = 2 s phi(mu / s) + mu (2 Phi(mu / s) - 1), A(mu, 0) = |mu| (float64)."""
    with np.errstate(all="ignore"):
        sd = np.sqrt(var)
        z = mu / sd
        g = sd * (2.0 / math.sqrt(2.0 * math.pi)) * np.exp(-0.5 * z * z) + mu * erf(z / math.sqrt(2.0))
    return np.where(var == 0.0, np.abs(mu), g)


def _ll(F, s2, y):
    """ll_mk in longdouble from float64 inputs."""
    with np.errstate(all="ignore"):
        r = y.astype(LD)[None] - F.astype(LD)
        return -LD(0.5) * r * r / s2 - LD(0.5) * np.log(2 * LD(np.pi) * s2)


def _s2(F, V, sigma):
    v = np.zeros_like(F) if V is None else np.asarray(V, dtype=np.float64)
    return LD(sigma) * LD(sigma) + v.astype(LD), v


def score_np(F, V, y, sigma, crps=True):
    """[6, K] float64: the rows of qn_pred_score for F [M, K], V [M, K] or None, y [K], all read as float64."""
    F = np.asarray(F, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    M, K = F.shape
    s2, v = _s2(F, V, sigma)
    s2d = s2.astype(np.float64)
    out = np.full((6, K), np.nan)
    with np.errstate(all="ignore"):
        bad = ~np.isfinite(y) | np.any(~np.isfinite(F) | ~np.isfinite(v) | ~(s2 >= 0), axis=0)
        zero_s = np.any(s2 == 0, axis=0)
        ll = _ll(F, s2, y)
        mx = ll.max(axis=0)
        out[0] = (mx + np.log(np.exp(ll - mx).sum(axis=0)) - np.log(LD(M))).astype(np.float64)
        dl = ll - ll[0]                                       # shifted by the first member: identical members give exactly 0
        out[1] = (((dl - dl.mean(axis=0)) ** 2).sum(axis=0) / (M - 1)).astype(np.float64)
        out[:2, zero_s] = np.nan
        r = y[None] - F
        sd = np.sqrt(s2d)
        term = np.where(s2d == 0.0, np.where(r > 0, 1.0, np.where(r == 0, 0.5, 0.0)), 0.5 * erfc(-(r / sd) / math.sqrt(2.0)))
        out[2] = term.mean(axis=0)
        if crps:
            first = _a(r, s2d).mean(axis=0)
            pair = np.empty(K)
            ii, jj = np.tril_indices(M, -1)                   # A is even in mu: pairs j < i twice, the diagonal once
            step = max(1, 3_000_000 // (M * M))               # entries per chunk: the [M (M - 1) / 2, step] temporaries stay small
            for lo in range(0, K, step):
                f, t = F[:, lo:lo + step], s2d[:, lo:lo + step]
                pair[lo:lo + step] = 2.0 * _a(f[ii] - f[jj], t[ii] + t[jj]).sum(axis=0) + _a(0.0 * f, 2.0 * t).sum(axis=0)
            out[3] = first - pair / (2.0 * M * M)
        fl = F.astype(LD)
        df = fl - fl[0]
        out[4] = (fl[0] + df.mean(axis=0)).astype(np.float64)
        out[5] = (((df - df.mean(axis=0)) ** 2).sum(axis=0) / (M - 1)).astype(np.float64)
    out[:, bad] = np.nan
    if not crps:
        out[3] = np.nan
    return out


def score_bars(F, V, y, sigma):
    """[6, K] per-entry absolute bars of the device result against `score_np` (tests/test_gpu_pred_score.py, docstring)."""
    F = np.asarray(F, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    M, K = F.shape
    s2, _ = _s2(F, V, sigma)
    with np.errstate(all="ignore"):
        ll = _ll(F, s2, y).astype(np.float64)
        lmax = np.abs(ll).max(axis=0)
        bars = np.empty((6, K))
        bars[0] = 32 * EPS * (lmax + M + 1)
        bars[1] = 64 * EPS * (lmax * ll.std(axis=0, ddof=1) + ll.var(axis=0, ddof=1))
        bars[2] = 1e-14
        bars[3] = 8 * EPS * M * (np.abs(y[None] - F).max(axis=0) + np.sqrt(s2.astype(np.float64)).max(axis=0))
        bars[4] = 8 * EPS * M * np.abs(F).max(axis=0)
        bars[5] = bars[4] * np.abs(F - F.mean(axis=0)).max(axis=0)
    return bars


# ------------------------------------------------------------------------------------------ the restatement itself
def test_restatement_single_gaussian_crps_closed_form():
    rng = np.random.default_rng(0)
    K, s = 50, 0.7
    f, y = rng.normal(size=K), rng.normal(size=K)
    rows = score_np(np.tile(f, (5, 1)), None, y, s)
    z = (y - f) / s
    Phi, phi = 0.5 * erfc(-z / math.sqrt(2)), np.exp(-0.5 * z * z) / math.sqrt(2 * math.pi)
    closed = s * (z * (2 * Phi - 1) + 2 * phi - 1 / math.sqrt(math.pi))            # Gneiting & Raftery 2007, eq. (21)
    assert np.max(np.abs(rows[3] - closed)) < 1e-14
    assert np.max(np.abs(rows[2] - Phi)) < 1e-15


def test_restatement_sigma_zero_is_ensemble_crps():
    rng = np.random.default_rng(1)
    M, K = 7, 40
    F, y = rng.normal(size=(M, K)), rng.normal(size=K)
    rows = score_np(F, None, y, 0.0)
    direct = np.abs(F - y).mean(axis=0) - np.abs(F[:, None] - F[None]).mean(axis=(0, 1)) / 2
    assert np.max(np.abs(rows[3] - direct)) < 1e-15
    assert np.isnan(rows[:2]).all()                              # no predictive variance: no log density
    assert set(np.unique(rows[2] * M * 2)) <= set(range(2 * M + 1))      # pit: a count of members below y


def test_restatement_identical_members():
    rng = np.random.default_rng(2)
    K, s = 30, 0.3
    f, y = rng.normal(size=K) + 1e3, rng.normal(size=K) + 1e3
    rows = score_np(np.tile(f, (9, 1)), None, y, s)
    ll = -0.5 * ((y - f) / s) ** 2 - 0.5 * np.log(2 * np.pi * s * s)
    assert np.all(rows[1] == 0.0) and np.all(rows[5] == 0.0)
    assert np.max(np.abs(rows[0] - ll)) < 1e-14 * np.max(np.abs(ll))
    assert np.array_equal(rows[4], f)


def test_restatement_bad_entries_and_zero_variance():
    rng = np.random.default_rng(3)
    M, K = 4, 6
    F, y, V = rng.normal(size=(M, K)), rng.normal(size=K), rng.uniform(0.1, 1.0, size=(M, K))
    clean = score_np(F, V, y, 0.0)
    assert np.isfinite(clean).all()
    F2, V2 = F.copy(), V.copy()
    F2[1, 0], V2[2, 1], V2[0, 2] = np.nan, -5.0, 0.0
    rows = score_np(F2, V2, y, 0.0)
    assert np.isnan(rows[:, :2]).all()
    assert np.isnan(rows[:2, 2]).all() and np.isfinite(rows[2:, 2]).all()
    assert np.array_equal(rows[:, 3:], clean[:, 3:])


# ------------------------------------------------------------------------------------------ the host combine
def test_summarise_hand_made_rows():
    y = np.array([[0.0, 1.0], [2.0, 3.0]])
    rows = np.array([[-1.0, -2.0, -3.0, -4.0],
                     [0.1, 0.2, 0.3, 0.4],
                     [0.5, 0.04, 0.26, 0.98],
                     [0.2, 0.4, 0.6, 0.8],
                     [0.0, 1.0, 2.0, 5.0],
                     [1.0, 1.0, 1.0, 1.0]])
    r = scoring.summarise(rows, y)
    assert r["n"] == 4 and r["lppd"] == -10.0 and abs(r["p_waic"] - 1.0) < 1e-15
    assert abs(r["elpd_waic"] + 11.0) < 1e-14 and abs(r["waic"] - 22.0) < 1e-14 and r["nlpd"] == 2.5
    elpd_k = rows[0] - rows[1]
    assert abs(r["se_elpd"] - math.sqrt(4 * elpd_k.var(ddof=1))) < 1e-14
    assert abs(r["crps"] - 0.5) < 1e-15 and abs(r["rmse"] - 1.0) < 1e-15
    assert r["coverage"] == {0.5: 0.5, 0.9: 0.5, 0.95: 0.75}
    assert list(r["pit_hist"]) == [1, 0, 1, 0, 0, 1, 0, 0, 0, 1] and r["pit_hist"].sum() == 4
    assert r["pit"].shape == y.shape and np.array_equal(r["mean"], [[0.0, 1.0], [2.0, 5.0]])
    assert scoring.summarise(rows, y, levels=(0.2,))["coverage"] == {0.2: 0.25}
    with pytest.raises(ValueError):
        scoring.summarise(rows[:, :3], y)


def test_calibrated_ensemble_covers():
    """f_mk ~ N(mu_k, tau^2), y_k ~ N(mu_k, tau^2 + sigma^2): the mixture of infinitely many members is the law of y, so the
    PIT is uniform and coverage(0.9) is 0.9 up to the binomial error of K entries, 4 sqrt(0.9 * 0.1 / K) = 0.019.  With
    M = 256 members the mixture's variance exceeds the true one by tau^2 / M (0.2 % here), a bias of coverage below 1e-3."""
    rng = np.random.default_rng(12345)
    M, K, tau, sigma = 256, 4000, 0.7, 0.4
    mu = rng.normal(size=K)
    F = mu + tau * rng.normal(size=(M, K))
    y = mu + math.sqrt(tau ** 2 + sigma ** 2) * rng.normal(size=K)
    r = scoring.summarise(score_np(F, None, y, sigma, crps=False), y)
    assert abs(r["coverage"][0.9] - 0.9) <= 4 * math.sqrt(0.9 * 0.1 / K)
    assert abs(r["coverage"][0.5] - 0.5) <= 4 * math.sqrt(0.5 * 0.5 / K)
    assert r["pit_hist"].sum() == K and r["pit_hist"].min() > 0.1 * K - 4 * math.sqrt(0.1 * 0.9 * K)


# ------------------------------------------------------------------------------------------ refusals (no device)
@pytest.fixture(scope="module")
def L():
    _lib.build()
    return _lib.lib()


def test_argument_refusals_need_no_device(L):
    EINVAL, EWORKSPACE = -1, -2
    buf = (ctypes.c_double * 8)()
    p = ctypes.addressof(buf)                        # never dereferenced: every call below is refused first
    ALL = scoring.WHAT_ALL
    need = L.qn_pred_score_workspace_bytes(4, 10, ALL)
    assert need >= 10 * 8 and L.qn_pred_score_workspace_bytes(4, 10, _lib.SCORE_MOMENTS) > 0

    def call(F=p, V=None, dtype=0, Y=p, M=4, K=10, sigma=0.1, what=ALL, out=p, ws=p, nbytes=need):
        return L.qn_pred_score(F, V, dtype, Y, M, K, sigma, what, out, ws, nbytes, None)

    for kw, word in (({"M": 1}, b"M >= 2"), ({"K": 0}, b"K >= 1"), ({"dtype": 2}, b"dtype"), ({"what": 0}, b"what"),
                     ({"what": 32}, b"what"), ({"what": ALL | 64}, b"what"), ({"sigma": -0.1}, b"sigma"),
                     ({"sigma": float("nan")}, b"sigma"), ({"sigma": float("inf")}, b"sigma"),
                     ({"sigma": 0.0, "what": _lib.SCORE_LPPD}, b"variance"), ({"sigma": 0.0, "what": _lib.SCORE_PWAIC}, b"variance"),
                     ({"sigma": 0.0, "what": _lib.SCORE_PIT | _lib.SCORE_CRPS}, b"variance"),
                     ({"F": None}, b"NULL"), ({"Y": None}, b"NULL"), ({"out": None}, b"NULL"), ({"ws": None}, b"NULL")):
        assert call(**kw) == EINVAL, kw
        assert word in L.qn_last_error(), (kw, L.qn_last_error())
    assert call(nbytes=need - 1) == EWORKSPACE and b"workspace" in L.qn_last_error()
    for args, word in (((1, 10, ALL), b"M >= 2"), ((4, 0, ALL), b"K >= 1"), ((4, 10, 0), b"what"), ((4, 10, 32), b"what"),
                       ((1 << 40, 1 << 30, ALL), b"too large")):
        assert L.qn_pred_score_workspace_bytes(*args) == 0, args
        assert word in L.qn_last_error(), (args, L.qn_last_error())
