"""Stacking of predictive distributions in numpy: the contract of `qn_group_lpd`, `qn_stack_weights` and `qn_pred_score_w`.

Float64 numpy and the authority for the device kernels (csrc/qn_stack.hip), as psis.py is for `qn_psis_loo`; the row
functions take `dtype=` and run in np.longdouble too.  Yao, Vehtari, Simpson & Gelman (Bayesian Anal. 13, 2018) and Yao,
Vehtari & Gelman (JMLR 23, 2022, "Stacking for non-mixing Bayesian computations").  The reference has no counterpart.

L `[G, K]` holds the log predictive density of entry k under group g alone (a chain, an ensemble member); -Inf is density 0.

  m_k = max_g L_gk over the elements that are neither NaN nor +Inf;  E_gk = exp(L_gk - m_k).  A NaN or +Inf element counts
  as E = 0 and in `n_nonfinite`; an entry whose m_k is -Inf (or that has no other element) is dropped from every sum and
  counted in `n_dropped`; K' entries are kept.
  EM for the mixture weights from w = 1 / G:  mix_k = sum_g w_g E_gk,  grad_g = (1 / K') sum_k E_gk / mix_k,
  obj = sum_k (log mix_k + m_k),  gap = K' (max_g grad_g - 1).  obj is concave in w and grad its gradient / K', so gap
  bounds obj(w*) - obj(w) from above: the stopping certificate, in nats.  Stop at the first iterate with gap <= tol or at
  iterate max_iter; else w_g <- w_g grad_g, renormalised by its sum.  obj never decreases.  K' = 0: w = 1 / G, obj = gap = 0.

The weighted rows are those of `qn_pred_score` for the mixture sum_m wm_m N(f_mk, sigma^2 + V_mk), wm >= 0, sum wm = 1:
lppd = logsumexp_m(ll_mk + log wm_m), p_waic = sum wm (ll - mean_w)^2 / (1 - sum wm^2), pit = sum wm Phi, crps =
sum_i wm_i A(y - f_i, s_i^2) - 0.5 sum_ij wm_i wm_j A(f_i - f_j, s_i^2 + s_j^2), mean = sum wm f, var = sum wm (f - mean)^2
/ (1 - sum wm^2).  A member of weight 0 is skipped, its f and V are never looked at; 1 - sum wm^2 == 0 gives 0 in the two
variance rows; a negative or non-finite weight makes every row NaN.
"""
import numpy as np
from scipy.special import erfc

DEFAULT_TOL = 1e-3                 # nats: far below any se_elpd
DEFAULT_MAX_ITER = 5000
STATUS = ("obj", "gap", "iters", "n_kept", "n_nonfinite", "n_dropped", "obj_equal", "done")      # qn_stack_weights' status block


def _log_lik(f, s2, y, dtype):
    two_pi = dtype(8) * np.arctan(dtype(1))
    r = y - f
    return -dtype(0.5) * r * r / s2 - dtype(0.5) * np.log(two_pi * s2)


def group_lpd(F, y, noise, offsets, V=None, dtype=np.float64):
    """L `[G, K]`: L_gk = logsumexp_{m in g} ll_mk - log M_g for the groups of members offsets[g] .. offsets[g + 1] - 1 of
    F `[M, K]` (V `[M, K]` optional member variances, y `[K]`).  A non-finite f, V or y or a variance noise^2 + V <= 0 in a
    member of the group makes L_gk NaN."""
    f = np.asarray(F).astype(dtype)
    M, K = f.shape
    offsets = np.asarray(offsets, dtype=np.int64)
    if offsets[0] != 0 or offsets[-1] != M or np.any(np.diff(offsets) < 1):
        raise ValueError("offsets must rise strictly from 0 to M")
    yy = np.asarray(y).astype(dtype).reshape(K)
    v = np.zeros_like(f) if V is None else np.asarray(V).astype(dtype)
    out = np.empty((len(offsets) - 1, K), dtype=dtype)
    with np.errstate(all="ignore"):
        s2 = dtype(noise) * dtype(noise) + v
        bad = ~(np.isfinite(f) & np.isfinite(v) & (s2 > 0)) | ~np.isfinite(yy)[None]
        ll = _log_lik(f, np.where(bad, dtype(1), s2), yy[None], dtype)
        for g in range(len(offsets) - 1):
            a = ll[offsets[g]:offsets[g + 1]]
            mx = a.max(axis=0)
            mxs = np.where(np.isfinite(mx), mx, dtype(0))
            out[g] = mx + np.log(np.exp(a - mxs).sum(axis=0)) - np.log(dtype(len(a)))
            out[g, np.isneginf(mx)] = -np.inf
            out[g, bad[offsets[g]:offsets[g + 1]].any(axis=0)] = np.nan
    return out


def prepare(L):
    """(E `[G, K']`, m `[K']`, keep `[K]` bool, n_nonfinite) of L `[G, K]`: the module docstring's preparation."""
    L = np.asarray(L, dtype=np.float64)
    if L.ndim != 2 or L.shape[0] < 1 or L.shape[1] < 1:
        raise ValueError(f"L of shape {L.shape}: [G >= 1, K >= 1] is needed")
    nonfin = np.isnan(L) | np.isposinf(L)
    with np.errstate(all="ignore"):
        m = np.where(nonfin, -np.inf, L).max(axis=0)
        keep = m > -np.inf
        E = np.where(nonfin[:, keep], 0.0, np.exp(np.where(nonfin[:, keep], 0.0, L[:, keep]) - m[keep]))
    return E, m[keep], keep, int(nonfin.sum())


def stack_weights(L, tol=DEFAULT_TOL, max_iter=DEFAULT_MAX_ITER, trace=False):
    """The stacking weights of L `[G, K]`: a dict with `w` `[G]`, `obj`, `gap`, `iters`, `n_kept`, `n_nonfinite`,
    `n_dropped`, `obj_equal` (obj at w = 1 / G) and, with trace=True, `objs` and `gaps` of every iterate."""
    E, m, keep, n_nonfinite = prepare(L)
    G, Kp = E.shape
    w = np.full(G, 1.0 / G)
    res = {"n_kept": Kp, "n_nonfinite": n_nonfinite, "n_dropped": int((~keep).sum())}
    objs, gaps = [], []
    if Kp == 0:
        res.update(w=w, obj=0.0, gap=0.0, iters=0, obj_equal=0.0)
    else:
        msum = m.sum()
        for it in range(max_iter + 1):
            mix = w @ E
            grad = (E / mix).sum(axis=1) / Kp
            obj = float(np.log(mix).sum() + msum)
            gap = float(Kp * (grad.max() - 1.0))
            objs.append(obj)
            gaps.append(gap)
            if gap <= tol or it == max_iter:
                break
            w = w * grad
            w = w / w.sum()
        res.update(w=w, obj=obj, gap=gap, iters=it, obj_equal=objs[0])
    if trace:
        res.update(objs=np.array(objs), gaps=np.array(gaps))
    return res


def _crps_a(mu, s2, dtype):
    """A(mu, s^2) = 2 s phi(mu / s) + mu (2 Phi(mu / s) - 1); |mu| at s = 0.  Phi is float64."""
    s = np.sqrt(s2)
    z = np.where(s > 0, mu / np.where(s > 0, s, dtype(1)), dtype(0))
    two_pi = dtype(8) * np.arctan(dtype(1))
    erf = (1.0 - erfc(z.astype(np.float64) / np.sqrt(2.0))).astype(dtype)
    return np.where(s > 0, dtype(2) * s * np.exp(-dtype(0.5) * z * z) / np.sqrt(two_pi) + mu * erf, np.abs(mu))


def weighted_rows(F, y, noise, wm, V=None, crps=True, dtype=np.float64):
    """`[6, K]` (lppd, p_waic, pit, crps, mean, var; in `dtype`) of the weighted mixture: the module docstring, entry by entry.
    y=None gives the two moment rows only.  crps=False leaves row 3 NaN."""
    f = np.asarray(F).astype(dtype)
    M, K = f.shape
    wm = np.asarray(wm).astype(dtype).reshape(M)
    out = np.full((6, K), np.nan, dtype=dtype)
    if not np.all(np.isfinite(wm) & (wm >= 0)):
        return out
    on = wm > 0
    f, w = f[on], wm[on][:, None]
    v = np.zeros_like(f) if V is None else np.asarray(V).astype(dtype)[on]
    den = dtype(1) - (w * w).sum()
    with np.errstate(all="ignore"):
        s2 = dtype(noise) * dtype(noise) + v
        good = np.all(np.isfinite(f) & np.isfinite(v) & (s2 >= 0), axis=0)
        mean = (w * f).sum(axis=0)
        out[4] = mean
        out[5] = (w * (f - mean) ** 2).sum(axis=0) / den if den != 0 else dtype(0)
        if y is not None:
            yy = np.asarray(y).astype(dtype).reshape(K)
            good &= np.isfinite(yy)
            pos = np.all(s2 > 0, axis=0)
            ll = _log_lik(f, np.where(s2 > 0, s2, dtype(1)), yy[None], dtype)
            a = ll + np.log(w)
            mx = a.max(axis=0)
            out[0] = mx + np.log(np.exp(a - np.where(np.isfinite(mx), mx, dtype(0))).sum(axis=0))
            lmean = (w * ll).sum(axis=0)
            out[1] = (w * (ll - lmean) ** 2).sum(axis=0) / den if den != 0 else dtype(0)
            out[:2, ~pos] = np.nan
            r = yy[None] - f
            sd = np.sqrt(s2)
            z = (r / np.where(sd > 0, sd, dtype(1))).astype(np.float64)
            Phi = np.where(sd > 0, 0.5 * erfc(-z / np.sqrt(2.0)), np.where(r > 0, 1.0, np.where(r == 0, 0.5, 0.0))).astype(dtype)
            out[2] = (w * Phi).sum(axis=0)
            if crps:
                first = (w * _crps_a(r, s2, dtype)).sum(axis=0)
                pair = np.zeros(K, dtype=dtype)
                for i in range(len(f)):
                    pair += w[i] * (w * _crps_a(f[i][None] - f, s2[i][None] + s2, dtype)).sum(axis=0)
                out[3] = first - dtype(0.5) * pair
        out[:, ~good] = np.nan
    if y is None:
        out[:4] = np.nan
    return out


def member_weights(w, offsets):
    """`[M]`: weight w_g / M_g for every member of group g -- the `wm` of the weighted rows for group weights w `[G]`."""
    sizes = np.diff(np.asarray(offsets, dtype=np.int64))
    return np.repeat(np.asarray(w, dtype=np.float64) / sizes, sizes)
