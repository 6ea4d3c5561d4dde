"""The numpy float64 contract of `qn_pred_quantile` (csrc/qn_quantile.hip; include/quinn_amd_quantile.h is its header): quantiles
of the predictive mixture that `qn_pred_score` scores.  Member m predicts N(f_mk, s_mk^2), s_mk^2 = sigma^2 + V_mk, with weight
w_m (None: 1 / M); `pred_quantiles_ref` is the whole call.

Empirical mode (sigma == 0 and V is None) is the order-statistic quantile of the members, `empirical_quantiles`: with equal
weights numpy's default 'linear' method bit for bit, with weights the same interpolation between the positions
p_i = (S_i - w_(i) / 2 - w_(1) / 2) / (S_n - w_(1) / 2 - w_(n) / 2) of the members sorted by (f, m) (S_n = 1 up to rounding).  Mixture mode,
`mixture_quantiles`, finds the root of G(y) = sum_m w_m Phi((y - f_m) / s_m) = q by safeguarded Newton steps; the kernel takes
the same steps in the same order, so that the two differ only through erfc, exp and the order of the sum over the members
(the contract adds pairwise, the kernel in member order).  `residual_bound` is the bound every returned root satisfies.
"""
from statistics import NormalDist

import numpy as np
from scipy.special import erfc

QN_QUANT_MAX_M = 16384
QN_QUANT_MAX_Q = 16
QN_QUANT_MAX_ITER = 128
BRACKET_PAD = 1e-9                      # each end of the first bracket moves out by BRACKET_PAD (|end| + max s)
INV_SQRT_2PI = 0.39894228040143267794


def inv_normal_cdf(q):
    """Phi^-1 by Wichura's AS241, all three branches (Python's statistics.NormalDist.inv_cdf)."""
    nd = NormalDist()
    return np.array([nd.inv_cdf(float(p)) for p in np.asarray(q, dtype=np.float64).reshape(-1)])


def _lerp(a, b, g):
    """numpy's two-sided interpolation, every product rounded before its sum."""
    d = b - a
    return np.where(g < 0.5, a + d * g, b - d * (1.0 - g))


def check_levels(q, empirical):
    q = np.asarray(q, dtype=np.float64).reshape(-1)
    if not 1 <= q.size <= QN_QUANT_MAX_Q:
        raise ValueError(f"{q.size} levels; 1 .. {QN_QUANT_MAX_Q} are needed")
    ok = (q >= 0.0) & (q <= 1.0) if empirical else (q > 0.0) & (q < 1.0)
    if not np.all(ok):
        raise ValueError(f"levels {q[~ok]} outside " + ("[0, 1]" if empirical else "(0, 1)"))
    return q


def check_weights(wm, M):
    """None, or the `(M,)` float64 weights; (weights, valid): an invalid set (negative, non-finite, none positive) is NaN everywhere."""
    if wm is None:
        return None, True
    wm = np.asarray(wm, dtype=np.float64).reshape(-1)
    if wm.shape != (M,):
        raise ValueError(f"{wm.size} weights for {M} members")
    return wm, bool(np.all(np.isfinite(wm)) and np.all(wm >= 0.0) and np.any(wm > 0.0))


def empirical_quantiles(F, q, wm=None):
    """`[Q, K]` order-statistic quantiles of the members F `(M, K)` at the levels q in [0, 1]."""
    F = np.asarray(F).astype(np.float64)
    q = check_levels(q, True)
    M, K = F.shape
    wm, valid = check_weights(wm, M)
    out = np.full((q.size, K), np.nan)
    if not valid:
        return out
    keep = np.arange(M) if wm is None else np.flatnonzero(wm > 0.0)
    n = keep.size
    for k in range(K):
        f = F[keep, k]
        if not np.all(np.isfinite(f)):
            continue
        order = np.argsort(f, kind="stable")                 # the total order (f, m)
        s = f[order]
        if n == 1:
            out[:, k] = s[0]
            continue
        if wm is None:
            h = q * (n - 1)
            j = np.floor(h).astype(np.int64)
            out[:, k] = _lerp(s[j], s[np.minimum(j + 1, n - 1)], h - j)
            continue
        w = wm[keep][order]
        p = np.cumsum(w) - 0.5 * w - 0.5 * w[0]
        p = p / p[-1]                                        # the 1 of the formula is S_n as the running sum found it: p_n = 1 exactly
        for i, qi in enumerate(q):
            j = int(np.flatnonzero(p[:n - 1] <= qi).max())   # p[0] = 0 exactly: never empty
            dp = p[j + 1] - p[j]
            g = min(max((qi - p[j]) / dp, 0.0), 1.0) if dp > 0.0 else 0.0
            out[i, k] = _lerp(s[j], s[j + 1], np.float64(g))
    return out


def mixture_cdf(y, f, s, w=None):
    """(G, g): the mixture's distribution function and density at y `[...]` for the members f, s `(M, ...)` (broadcast against
    y) and the weights w `(M,)` (None: 1 / M).  Members of weight 0 must have been taken out."""
    inv_s = 1.0 / s
    t = (y - f) * inv_s
    Phi = 0.5 * erfc(-t * np.sqrt(0.5))
    dens = INV_SQRT_2PI * np.exp(-0.5 * t * t) * inv_s
    if w is None:
        return Phi.sum(axis=0) / f.shape[0], dens.sum(axis=0) / f.shape[0]
    w = w.reshape((-1,) + (1,) * (Phi.ndim - 1))
    return (w * Phi).sum(axis=0), (w * dens).sum(axis=0)


def residual_bound(y, g, M):
    """The bound on |G(y) - q| of a returned root: the rounding of an M-term sum of non-negative terms that total at most 1
    and the error of erfc, (M + 16) eps, and two spacings of y times the mixture density g."""
    return (M + 16) * np.finfo(np.float64).eps + 2.0 * np.spacing(np.abs(y)) * g


def mixture_quantiles(F, q, sigma, V=None, wm=None, return_iters=False):
    """`[Q, K]` roots of G(y) = q of the mixture of the members F `(M, K)`, s^2 = sigma^2 + V; with return_iters also the
    `(K,)` int32 largest number of evaluations over the levels (0 for a NaN entry)."""
    F = np.asarray(F).astype(np.float64)
    q = check_levels(q, False)
    M, K = F.shape
    Q = q.size
    wm, valid = check_weights(wm, M)
    out = np.full((Q, K), np.nan)
    iters = np.zeros(K, dtype=np.int32)
    S2 = np.full((M, K), float(sigma) ** 2) + (0.0 if V is None else np.asarray(V).astype(np.float64))
    keep = np.arange(M) if wm is None else np.flatnonzero(wm > 0.0)
    w = None if wm is None else wm[keep]
    with np.errstate(all="ignore"):
        good = valid & np.all(np.isfinite(F[keep]) & np.isfinite(S2[keep]) & (S2[keep] > 0.0), axis=0)
        ks = np.flatnonzero(good)
        if ks.size:
            f = F[keep][:, None, ks]                                  # (n, 1, K')
            s = np.sqrt(S2[keep][:, None, ks])
            qq = q[:, None] + np.zeros((Q, ks.size))
            z = inv_normal_cdf(q)[None, :, None]
            a = f + s * z
            lo, hi, smax = a.min(axis=0), a.max(axis=0), s.max(axis=0)
            y = a.sum(axis=0) / M if w is None else (w[:, None, None] * a).sum(axis=0)
            lo = lo - BRACKET_PAD * (np.abs(lo) + smax)
            hi = hi + BRACKET_PAD * (np.abs(hi) + smax)
            y = np.minimum(np.maximum(y, lo), hi)
            rlo = np.full_like(y, np.inf)
            rhi = np.full_like(y, np.inf)
            e1 = hi - lo
            e2 = e1.copy()
            done = np.zeros(y.shape, dtype=bool)
            res = np.full_like(y, np.nan)
            n = np.zeros(y.shape, dtype=np.int32)
            for it in range(1, QN_QUANT_MAX_ITER + 1):
                G, g = mixture_cdf(y, f, s, w)
                act = ~done
                n[act] = it
                r = G - qq
                hit = act & (r == 0.0)
                res[hit] = y[hit]
                done |= hit
                act = ~done
                below = act & (r < 0.0)
                above = act & ~(r < 0.0)
                lo[below], rlo[below] = y[below], -r[below]
                hi[above], rhi[above] = y[above], r[above]
                stop = act & ((hi - lo <= 2.0 * np.spacing(np.maximum(np.abs(lo), np.abs(hi)))) | (it == QN_QUANT_MAX_ITER))
                res[stop] = np.where(rlo <= rhi, lo, hi)[stop]
                done |= stop
                if done.all():
                    break
                step = -r / g
                sp2 = 2.0 * np.spacing(np.abs(y))
                step = np.where(np.abs(step) < sp2, np.copysign(sp2, -r), step)
                yn = y + step
                ok = np.isfinite(step) & (yn > lo) & (yn < hi) & (np.abs(step) <= 0.5 * e2)
                yn = np.where(ok, yn, lo + 0.5 * (hi - lo))
                e2 = e1
                e1 = np.abs(yn - y)
                y = np.where(done, y, yn)
            out[:, ks] = res
            iters[ks] = n.max(axis=0)
    return (out, iters) if return_iters else out


def pred_quantiles_ref(F, q, sigma, V=None, wm=None, return_iters=False):
    """The whole call: empirical mode for sigma == 0 and V None, else mixture mode; the refusals as ValueError."""
    F = np.asarray(F)
    if F.ndim != 2 or not 1 <= F.shape[0] <= QN_QUANT_MAX_M or F.shape[1] < 1:
        raise ValueError(f"F of shape {F.shape}: (M, K) with 1 <= M <= {QN_QUANT_MAX_M} and K >= 1 is needed")
    if not (np.isfinite(sigma) and sigma >= 0.0):
        raise ValueError(f"sigma = {sigma} (finite and >= 0)")
    if sigma == 0.0 and V is None:
        out = empirical_quantiles(F, q, wm)
        return (out, np.zeros(F.shape[1], dtype=np.int32)) if return_iters else out
    return mixture_quantiles(F, q, sigma, V, wm, return_iters)
