"""Pareto-smoothed importance-sampling leave-one-out (PSIS-LOO) in numpy: the contract of `qn_psis_loo`.

Float64 numpy and the authority for the device kernel (csrc/qn_psis.hip), as mcmc/hyper.py is for the Gibbs draw; every
function takes `dtype=` and runs in np.longdouble too, which is what the GPU tests compare against.  Vehtari, Gelman &
Gabry (Stat. Comput. 27, 2017) and Vehtari, Simpson, Gelman, Yao & Gabry (JMLR 25, 2024); the generalised Pareto fit is
Zhang & Stephens (Technometrics 51, 2009) with the weakly informative prior of PSIS.  The reference has no counterpart.

Per entry k, with ll_m the log density of y_k under member m (N(f_mk, noise^2 + V_mk), as in `qn_pred_score`):

  lr_m = -ll_m - max_m(-ll_m), the log importance ratios of leaving y_k out; T = ceil(min(M / 5, 3 sqrt(M))).
  The tail is the T largest members in the total order (lr_m, m), the cutoff c the (T+1)-th largest lr; the ascending tail
  excesses x_j = exp(lr_(j)) - exp(c) get a generalised Pareto fit (`gpd_fit`: khat, sigma) and are replaced by its
  quantiles, lw = log(exp(c) + sigma expm1(-khat log1p(-p_j)) / khat), p_j = (j - 0.5) / T; every lw is cut at 0, the
  largest raw ratio.  T < 5 or x_q <= 0 (q = floor(T / 4 + 0.5): a tied or underflowed tail) or a non-finite fit leaves the
  raw ratios (truncated importance sampling) and khat = +Inf.
  Rows: elpd_loo_k = logsumexp(ll + lw) - logsumexp(lw), khat, ess_k = 1 / sum w^2 and pit_loo = sum w Phi((y - f) / s),
  w = softmax(lw).  A non-finite f, V or y or a variance noise^2 + V <= 0 makes the entry's four rows NaN.
"""
import numpy as np
from scipy.special import erfc

ROWS = ("elpd_loo_k", "khat", "ess_k", "pit_loo")                 # the rows of qn_psis_loo's output, in order
DEFAULT_LEVELS = (0.5, 0.9, 0.95)


def tail_size(M):
    """T = ceil(min(M / 5, 3 sqrt(M)))."""
    return int(np.ceil(min(M / 5.0, 3.0 * np.sqrt(float(M)))))


def gpd_fit(x, dtype=np.float64):
    """(khat, sigma) of the generalised Pareto fit to the ascending excesses x `[..., n]` (n >= 5, x[q] > 0), one fit per
    leading index: the posterior mean of Zhang & Stephens over m = 30 + floor(sqrt(n)) grid points b_i, no weight dropped,
    and khat = (n k' + 5) / (n + 10), the shrinkage of PSIS towards 0.5."""
    x = np.asarray(x, dtype=dtype)
    n = x.shape[-1]
    q = int(np.floor(n / 4.0 + 0.5))
    m = 30 + int(np.floor(np.sqrt(float(n))))
    one, half = dtype(1), dtype(0.5)
    i = np.arange(1, m + 1).astype(dtype)
    with np.errstate(all="ignore"):
        b = one / x[..., -1:] + (one - np.sqrt(dtype(m) / (i - half))) / (dtype(3) * x[..., q - 1:q])          # [..., m]
        k = np.log1p(-b[..., :, None] * x[..., None, :]).sum(axis=-1) / dtype(n)                               # [..., m]
        L = dtype(n) * (np.log(-b / k) - k - one)
        w = one / np.exp(L[..., None, :] - L[..., :, None]).sum(axis=-1)
        bb = (w * b).sum(axis=-1)
        kp = np.log1p(-bb[..., None] * x).sum(axis=-1) / dtype(n)
        sigma = -kp / bb
        khat = (dtype(n) * kp + dtype(5)) / dtype(n + 10)
    return khat, sigma


def psis_log_weights(lr, dtype=np.float64):
    """(lw `[B, M]`, khat `[B]`): the smoothed, truncated log weights of the log ratios lr `[B, M]` (max 0 per row)."""
    lr = np.asarray(lr, dtype=dtype)
    B, M = lr.shape
    T = tail_size(M)
    khat = np.full(B, np.inf, dtype=dtype)
    lw = lr.copy()
    if B == 0:
        return lw, khat
    order = np.lexsort((np.broadcast_to(np.arange(M), lr.shape), lr), axis=-1)           # ascending in (lr, m)
    rowi = np.arange(B)[:, None]
    tail = order[:, M - T:]                                                               # ascending: j = 1 .. T
    c = lr[np.arange(B), order[:, M - T - 1]]
    if T >= 5:
        q = int(np.floor(T / 4.0 + 0.5))
        with np.errstate(all="ignore"):
            x = np.exp(lr[rowi, tail]) - np.exp(c)[:, None]
            fit = x[:, q - 1] > 0
            xs = np.where(fit[:, None], x, np.arange(1, T + 1).astype(dtype))             # a harmless tail where none is fitted
            kh, sg = gpd_fit(xs, dtype)
            fit &= np.isfinite(kh) & np.isfinite(sg)
            p = (np.arange(1, T + 1).astype(dtype) - dtype(0.5)) / dtype(T)
            l1p = np.log1p(-p)
            quant = np.where((kh == 0)[:, None], -sg[:, None] * l1p, sg[:, None] * np.expm1(-kh[:, None] * l1p) / kh[:, None])
            sm = np.log(np.exp(c)[:, None] + quant)
        r = np.nonzero(fit)[0]
        lw[r[:, None], tail[r]] = sm[r]
        khat[r] = kh[r]
    return np.minimum(lw, dtype(0)), khat


def psis_loo_rows(F, y, noise, V=None, dtype=np.float64):
    """`[4, K]` (elpd_loo_k, khat, ess_k, pit_loo; in `dtype`) of the ensemble F `[M, K]`, optional member variances V
    `[M, K]`, targets y `[K]` and the noise level `noise`: the module docstring, entry by entry.  Phi is float64."""
    f = np.asarray(F).astype(dtype)
    M, K = f.shape
    yy = np.asarray(y).astype(dtype).reshape(K)
    v = np.zeros_like(f) if V is None else np.asarray(V).astype(dtype)
    out = np.full((4, K), np.nan, dtype=dtype)
    with np.errstate(all="ignore"):
        s2 = dtype(noise) * dtype(noise) + v
        good = np.isfinite(yy) & np.all(np.isfinite(f) & np.isfinite(v) & (s2 > 0), axis=0)
        g = np.nonzero(good)[0]
        f, s2, yy = f[:, g].T, s2[:, g].T, yy[g][:, None]                                 # [Kg, M]
        r = yy - f
        two_pi = dtype(8) * np.arctan(dtype(1))
        ll = -dtype(0.5) * r * r / s2 - dtype(0.5) * np.log(two_pi * s2)
        nl = -ll
        lw, khat = psis_log_weights(nl - nl.max(axis=1, keepdims=True), dtype)
        a = ll + lw
        ma, mb = a.max(axis=1), lw.max(axis=1)
        w = np.exp(lw - mb[:, None])
        sb = w.sum(axis=1)
        Phi = (0.5 * erfc(-(r / np.sqrt(s2)).astype(np.float64) / np.sqrt(2.0))).astype(dtype)
        out[0, g] = ma + np.log(np.exp(a - ma[:, None]).sum(axis=1)) - (mb + np.log(sb))
        out[1, g] = khat
        out[2, g] = sb * sb / (w * w).sum(axis=1)
        out[3, g] = (w * Phi).sum(axis=1) / sb
    return out


def khat_threshold(M):
    """min(1 - 1 / log10(M), 0.7): the khat above which M draws do not give a reliable estimate (Vehtari et al. 2024)."""
    return float(min(1.0 - 1.0 / np.log10(float(M)), 0.7))


def summarise_loo(rows, y, M, lppd=None, levels=DEFAULT_LEVELS):
    """The LOO dict from the `[4, K]` rows of `psis_loo_rows` / `qn_psis_loo`, the targets `y` (K values in any shape; the
    per-entry arrays come back in that shape) and the number of members M.

    Per entry: `elpd_loo_k`, `khat`, `ess_k`, `pit_loo`.  Scalars: `elpd_loo` = sum elpd_loo_k, `looic` = -2 elpd_loo,
    `se_elpd_loo` = sqrt(K var_k(elpd_loo_k)) (ddof = 1; NaN for K = 1), `khat_threshold`, `n_khat_bad` and `khat_bad`, the
    count and the flat indices of the entries whose khat exceeds it (+Inf, an unsmoothed entry, does), `coverage_loo[level]`
    and `pit_loo_hist`, formed from pit_loo as `scoring.summarise` forms `coverage` and `pit_hist` from the in-sample PIT, and,
    with the lppd given, `p_loo` = lppd - elpd_loo."""
    y = np.asarray(y, dtype=np.float64)
    rows = np.asarray(rows, dtype=np.float64)
    K = y.size
    if rows.shape != (len(ROWS), K) or K < 1:
        raise ValueError(f"rows of shape {rows.shape}; expected ({len(ROWS)}, {K}) for y of shape {y.shape}")
    res = {name: rows[i].reshape(y.shape).copy() for i, name in enumerate(ROWS)}
    elpd_k, khat, pit = rows[0], rows[1], rows[3]
    res["elpd_loo"] = float(elpd_k.sum())
    res["looic"] = -2.0 * res["elpd_loo"]
    res["se_elpd_loo"] = float(np.sqrt(K * elpd_k.var(ddof=1))) if K > 1 else float("nan")
    res["khat_threshold"] = khat_threshold(M)
    with np.errstate(invalid="ignore"):
        res["khat_bad"] = np.nonzero(khat > res["khat_threshold"])[0]
        res["coverage_loo"] = {float(lv): float(np.mean(np.abs(pit - 0.5) <= 0.5 * float(lv))) for lv in levels}
    res["n_khat_bad"] = int(res["khat_bad"].size)
    res["pit_loo_hist"] = np.histogram(pit[np.isfinite(pit)], bins=10, range=(0.0, 1.0))[0]
    if lppd is not None:
        res["p_loo"] = float(lppd) - res["elpd_loo"]
    return res
